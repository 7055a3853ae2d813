// sweep.hpp — the tile relaxation that geo.hip (geo_sweep), flood.hip (flood_sweep, flood_assign) and shape.hip (rc_sweep) share.
// A plane of one word per pixel is driven to the fixed point of a local update, word(p) <- better(word(p), f(the 4-neighbours)).
//
// One launch.  A workgroup of 256 threads owns a 64 x 64 tile and stages it with a halo of one pixel into LDS; the words past
// the image get a value that offers nothing and never changes.  It relaxes the tile to local convergence: a row phase, in which
// a thread owns 16 consecutive pixels of a row and sweeps them forward (taking the pixel before and the two across) and back in
// registers, then a column phase, the same on 16 consecutive pixels of a column; a word moves along any straight run of the
// tile in one phase.  Within a phase every thread reads, then all wait, then the threads that moved a word store it: no thread
// reads a word another one may be storing.  The loop ends when both phases moved nothing.  Only the owned tile is written, to the
// other plane, and the owned pixels whose word moved are counted into changed[b], one agent-scope add per wave.
//
// Connectivity (the template parameter CONN of the relax-line functions and of the sweep kernels, 4 or 8).  With CONN == 8 the
// forward pass of a line also takes the four diagonal words p[(k +- 1) * ALONG +- ACROSS].  All of them lie in the staged square,
// the four halo corners included, for k = 0, for k = SW_SEG - 1 and across a tile corner: nothing more is staged and nothing is
// bounds-checked.  The loop ends only when neither phase moved a word, so "moved nothing" has to mean "stable against all eight
// neighbours": each phase takes all eight offers (before, after, two across, four diagonal).  The row phase alone would be enough
// for that; the column phase takes the diagonals as well because it is faster so, a diagonal run of words then moving in either
// phase (DESIGN.md section 4t has both timings).  The phase discipline above is untouched: the diagonal reads come before the
// phase's barrier like every other read.
//
// Coherence (label.hip's rule): a sweep reads plane A, which an earlier kernel wrote, and writes plane B, which no workgroup of
// the launch reads: a neighbour's halo read never sees this launch's stores, and the hand-off between tiles is the kernel
// boundary.  The counters are only touched by agent-scope adds.  No word is handed from one workgroup to another inside a
// kernel, no loop waits on a load.
//
// Termination and exactness: the update must be monotone (a word only ever moves in the direction of `better`) and bounded (over
// a finite set of values).  Then the loop in a tile ends, the launches end at one that changed nothing, and, the fixed point
// being unique, any order of relaxation reaches it.  Each .hip file states why its update is monotone and bounded.
//
// The launches an op needs are about the tile borders its longest chain of updates crosses, not the chain's length.  The host
// enqueues n_launches of them, ping-pong between the two planes, each counting into a slot row of its own; the caller reads
// the slots back in one copy and stops at the first launch that changed nothing.
#pragma once
#include "elem.hpp"

namespace unet {

static constexpr int SW_TILE = 64;                             // owned pixels per side of a workgroup's tile
static constexpr int SW_SEG = 16;                              // pixels of a row / column one thread owns: 64 lines x 4 segments
static constexpr int SW_STAGED = SW_TILE + 2;                  // the tile and its halo
static constexpr int SW_PITCH = SW_STAGED + 1;                 // LDS row pitch in words (67): 32 lanes on 32 rows, no bank twice

// the tile of this workgroup: image b, origin (oy, ox), OH x OW owned pixels, img the element offset of the image
struct SweepTile { int b, oy, ox, OH, OW; size_t img; };
__device__ __forceinline__ SweepTile sweep_tile(int H, int W)
{
    const int b = blockIdx.z;
    const int oy = blockIdx.y * SW_TILE, ox = blockIdx.x * SW_TILE;
    return {b, oy, ox, min(H, oy + SW_TILE) - oy, min(W, ox + SW_TILE) - ox, (size_t)b * H * W};
}

// The whole staged square, the halo and what lies past the image included: stage(i, in, e, ly, lx, gy, gx) fills the LDS words i
// = ly * SW_PITCH + lx of the kernel's planes; in: the word is inside the image, at element e, row gy, column gx.  Ends in a barrier.
template <class F>
__device__ __forceinline__ void sweep_stage(const SweepTile tl, int H, int W, F stage)
{
    for (int i = threadIdx.x; i < SW_STAGED * SW_STAGED; i += 256) {
        const int ly = i / SW_STAGED, lx = i - ly * SW_STAGED;
        const int gy = tl.oy - 1 + ly, gx = tl.ox - 1 + lx;
        stage(ly * SW_PITCH + lx, gy >= 0 && gy < H && gx >= 0 && gx < W, tl.img + (size_t)gy * W + gx, ly, lx, gy, gx);
    }
    __syncthreads();
}

template <int ALONG, typename T>
__device__ __forceinline__ void store_line(T *p, unsigned moved, const T (&v)[SW_SEG])
{
#pragma unroll
    for (int k = 0; k < SW_SEG; ++k)
        if (moved >> k & 1) p[k * ALONG] = v[k];
}

// Relaxes the staged plane s to the tile's fixed point.  rows(o, v) and cols(o, v) relax the SW_SEG words of the line that starts
// at LDS offset o, along the row and along the column, into v and return the bits of those that moved.
template <typename T, class R, class C>
__device__ __forceinline__ void sweep_converge(T *s, R rows, C cols)
{
    const int line = threadIdx.x & 63, seg = (threadIdx.x >> 6) * SW_SEG;
    const int ro = (1 + line) * SW_PITCH + 1 + seg, co = (1 + seg) * SW_PITCH + 1 + line;
    T v[SW_SEG];
    for (;;) {                                                                       // monotone and bounded: it ends
        const unsigned in_rows = rows(ro, v);
        __syncthreads();                                                             // every read of the phase is done
        store_line<1>(s + ro, in_rows, v);
        __syncthreads();
        const unsigned in_cols = cols(co, v);
        __syncthreads();
        store_line<SW_PITCH>(s + co, in_cols, v);
        if (!__syncthreads_or((in_rows | in_cols) != 0)) break;                      // the tile is at its fixed point
    }
}

// The owned tile from s to dst; the pixels with better(new word, src's word) are counted into changed[b]
template <typename T, class F>
__device__ __forceinline__ void sweep_write_back(const SweepTile tl, const T *s, const T *__restrict__ src, T *__restrict__ dst, int W,
                                                 unsigned *changed, F better)
{
    unsigned n = 0;
    for (int i = threadIdx.x; i < tl.OH * tl.OW; i += 256) {
        const int y = i / tl.OW, x = i - y * tl.OW;
        const size_t e = tl.img + (size_t)(tl.oy + y) * W + tl.ox + x;
        const T k = s[(1 + y) * SW_PITCH + 1 + x];
        n += better(k, src[e]);
        dst[e] = k;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) __hip_atomic_fetch_add(&changed[tl.b], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n_launches sweeps, launch l from plane[l & 1] to plane[~l & 1] with the counters slots[first_slot + l][B], zeroed here; the
// result ends in plane0.  launch(grid, src, dst, changed) enqueues one sweep.
template <class L>
static inline int sweep_launches(void *plane0, void *plane1, size_t elem_size, int B, int H, int W, int n_launches, void *slots_u32,
                                 int first_slot, hipStream_t st, L launch)
{
    unsigned *changed = (unsigned *)slots_u32 + (size_t)first_slot * B;
    HIP_TRY(hipMemsetAsync(changed, 0, (size_t)n_launches * B * sizeof(unsigned), st));
    void *plane[2] = {plane0, plane1};
    const dim3 grid(cdiv(W, SW_TILE), cdiv(H, SW_TILE), B);
    for (int l = 0; l < n_launches; ++l) launch(grid, plane[l & 1], plane[~l & 1], changed + (size_t)l * B);
    HIP_TRY(hipGetLastError());
    if (n_launches & 1) HIP_TRY(hipMemcpyAsync(plane0, plane1, (size_t)B * H * W * elem_size, hipMemcpyDeviceToDevice, st));
    return 0;
}

#define SW_CONN_CHECK(name) ARG_CHECK(connectivity == 4 || connectivity == 8, name ": connectivity must be 4 or 8, got %d", connectivity)

}  // namespace unet
