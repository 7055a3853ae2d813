// boundary.hip — where the contour of a mask lies against the contour of another: the integers and the one fp64 sum behind the
// Hausdorff distance, its percentile, the average symmetric surface distance and the normalised surface Dice
// (functions.mask_boundary, functions.surface_sums, functions.scores_from_surface), batched, on the device.
//
// Region: mask != 0, with select = k >= 0 mask == k.  Contour dA: the pixels of A with a neighbour (4 or 8) outside A; with edge 1
// ('background') a pixel past the image is outside A, with edge 0 ('ignore') it is nothing.  d2(p), p in dA, is the exact squared
// Euclidean distance to the nearest pixel of dB; both directions P -> G (dir 0) and G -> P (dir 1) are taken in one call.
//   1. bd_mark    reads both masks, one byte per pixel: bit 0 = dP, bit 1 = dG; counts |dP| and |dG| per image
//   2. dm_cols    dm.hpp's column pass (the one unet_distance_map runs), once per contour: the sites are the pixels with the bit
//   3. bd_rows    dm.hpp's scan outwards, only in the threads that sit on the other contour: d2 to its plane (-1 elsewhere);
//                 max d2, the counts d2 <= T2[i] and the fp64 sum of sqrt(d2) are reduced over the wave (butterfly), then over
//                 the four waves in wave order, and written to the workgroup's own 32-byte slot: no atomic, one barrier.  A
//                 workgroup without a contour pixel writes a zero slot and leaves.  (Atomic adds per workgroup were 0.3 ms at
//                 30 x 512^2: a thousand adds met on each word.)  The contour pixels are not compacted first: the planes are
//                 an output anyway, and the passes below read them at HBM speed
//   4. bd_hist / bd_pick, three times: a radix select of the j-th and the min(j + 1, n - 1)-th smallest d2 over the digits
//                 [30:20], [19:10], [9:0].  bd_hist counts, per target, the digit of every d2 whose higher digits equal the
//                 target's prefix: LDS histograms, flushed by integer atomic adds.  bd_pick, one workgroup per image and
//                 direction, scans the bins (a block prefix sum), finds the bin that holds the rank, extends the prefix, lowers
//                 the rank by the count of the bins below, and clears the bins.  j and rem come from n, q_num, q_den in 64-bit
//                 integers in the first bd_pick.  No sort, no read-back
//   5. bd_finish  one workgroup per image and direction reduces the slots in slot order and writes the record
// Every count is an integer atomic or a fixed-order reduce and the fp64 sum has no atomic: the outputs are the same in every run.
//
// Empty contours: n = |dA| always.  If dA or dB is empty, every other word of the record of A -> B is 0 and the d2 plane is -1
// everywhere; bd_rows reads the counts of bd_mark for that, never a sentinel distance.
//
// Coherence (label.hip's rule): a word that atomics of one kernel touch is read plainly only by later kernels of the stream;
// bd_pick re-reads its own stores only after a barrier of its one workgroup.
#include "dm.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {

typedef unsigned long long u64;

// the words per (image, direction) that the kernels keep between them
enum { BS_RANK = 0, BS_PREFIX = 2, BS_REM = 4, BS_WORDS = 5 };
static constexpr int BD_BINS = 2048;                           // bins of a histogram: the 11-bit digit; the 10-bit ones use half
static constexpr int BD_REC = 10;                              // words of a record (unet_hip.h)

struct BdMask { const void *p; int dtype, select; };
struct BdT2 { int n; unsigned v[4]; };
struct BdPart { double sum; unsigned within[4]; unsigned top, pad; };      // what one workgroup of bd_rows leaves: 32 bytes

__device__ __forceinline__ bool bd_in(const BdMask m, size_t e)
{
    if (m.select < 0) return mask_on(m.p, m.dtype, e);
    if (m.dtype == 0) return ((const long long *)m.p)[e] == (long long)m.select;
    if (m.dtype == 1) return ((const float *)m.p)[e] == (float)m.select;
    if (m.dtype == 2) return ((const int *)m.p)[e] == m.select;
    return (int)((const unsigned char *)m.p)[e] == m.select;
}

__device__ __forceinline__ unsigned bd_contour(const BdMask m, size_t img, int y, int x, int H, int W, int conn, int edge)
{
    if (!bd_in(m, img + (size_t)y * W + x)) return 0;
    bool open = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            if ((dy == 0 && dx == 0) || (conn == 4 && dy != 0 && dx != 0)) continue;
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) open |= edge != 0;
            else open |= !bd_in(m, img + (size_t)yy * W + xx);
        }
    return open;
}

// ---- 1. mark ------------------------------------------------------------------------------------------------------------------
// g.p and cnt may be NULL (unet_mask_boundary): bit 0 alone, nothing counted
__global__ __launch_bounds__(256) void bd_mark_kernel(const BdMask p, const BdMask g, int H, int W, int conn, int edge,
                                                      unsigned char *__restrict__ out, u64 *cnt)
{
    const unsigned npx = (unsigned)H * W;                       // below 2^31: 32-bit divisions
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned n[2] = {0, 0};
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += gridDim.x * blockDim.x) {
        const int y = (int)(e / (unsigned)W), x = (int)(e - (unsigned)y * W);
        unsigned bits = bd_contour(p, img, y, x, H, W, conn, edge);
        if (g.p) bits |= bd_contour(g, img, y, x, H, W, conn, edge) << 1;
        out[img + e] = (unsigned char)bits;
        n[0] += bits & 1;
        n[1] += bits >> 1;
    }
    if (cnt) block_counts(cnt + 2 * (size_t)blockIdx.y, n);
}

// dm.hpp's site test: a pixel of the contour with this bit
struct BdSite {
    const unsigned char *bits;
    int bit;
    __device__ __forceinline__ bool operator()(size_t e) const { return (bits[e] & bit) != 0; }
};

// ---- 3. rows ------------------------------------------------------------------------------------------------------------------
// grid (W / 256, 2 H, B): blockIdx.y = 2 y + dir.  g: plane 0 the column distances to dP, plane 1 to dG
__global__ __launch_bounds__(256) void bd_rows_kernel(const unsigned char *__restrict__ bits, const int *__restrict__ g, size_t plane, int H, int W,
                                                      const BdT2 t2, const u64 *__restrict__ cnt, int *__restrict__ d2_pg, int *__restrict__ d2_gp,
                                                      BdPart *__restrict__ part)
{
    __shared__ BdPart of_wave[4];
    const int b = blockIdx.z, y = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const size_t z = 2 * (size_t)b + dir;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const bool live = x < W;
    const size_t row = ((size_t)b * H + y) * W;
    int *D = dir ? d2_gp : d2_pg;
    if (cnt[z ^ 1] == 0) {                                     // the other contour is empty: no distance is defined
        if (live) D[row + x] = -1;
        return;
    }
    const bool on = live && (bits[row + x] >> dir & 1);
    unsigned best = 0;
    if (on) {
        const int *G = g + (size_t)(dir ^ 1) * plane + row;
        const unsigned own = (unsigned)G[x];
        best = dm_row_best(G, x, W, own * own);
    }
    if (live) D[row + x] = on ? (int)best : -1;
    BdPart *out = part + (z * H + y) * gridDim.x + blockIdx.x;
    if (!__syncthreads_or(on)) {                               // most workgroups: no contour pixel in these 256 columns
        if (threadIdx.x == 0) *out = BdPart{0.0, {0, 0, 0, 0}, 0, 0};
        return;
    }
    BdPart p;
    p.sum = wave_sum(on ? sqrt((double)best) : 0.0);           // a butterfly: the same order in every run
#pragma unroll
    for (int i = 0; i < 4; ++i) p.within[i] = wave_sum((unsigned)(on && i < t2.n && best <= t2.v[i]));
    p.top = best;                                              // 0 off the contour
    for (int d = 32; d >= 1; d >>= 1) p.top = max(p.top, (unsigned)__shfl_xor(p.top, d, 64));
    p.pad = 0;
    if ((threadIdx.x & 63) == 0) of_wave[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {                              // in wave order
        p.sum += of_wave[w].sum;
        for (int i = 0; i < 4; ++i) p.within[i] += of_wave[w].within[i];
        p.top = max(p.top, of_wave[w].top);
    }
    *out = p;
}

// ---- 4. radix select ------------------------------------------------------------------------------------------------------------
// grid (blocks, 2, B); digit = (d2 >> shift) & (2^nbits - 1); hist [B][2 dir][2 targets][BD_BINS]
__global__ __launch_bounds__(256) void bd_hist_kernel(const int *__restrict__ d2_pg, const int *__restrict__ d2_gp, size_t npx, int shift, int nbits,
                                                      const u64 *__restrict__ cnt, const u64 *__restrict__ state, unsigned *hist)
{
    __shared__ unsigned h[2 * BD_BINS];
    const size_t z = 2 * (size_t)blockIdx.z + blockIdx.y;
    if (cnt[z] == 0 || cnt[z ^ 1] == 0) return;
    const int *D = (blockIdx.y ? d2_gp : d2_pg) + (size_t)blockIdx.z * npx;
    const unsigned p0 = (unsigned)state[z * BS_WORDS + BS_PREFIX], p1 = (unsigned)state[z * BS_WORDS + BS_PREFIX + 1];
    for (int i = threadIdx.x; i < 2 * BD_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const unsigned digit = (1u << nbits) - 1;
    const int above = shift + nbits;                           // 31 in the first pass: nothing above, both prefixes 0
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int v = D[e];
        if (v < 0) continue;
        const unsigned high = (unsigned)v >> above, bin = ((unsigned)v >> shift) & digit;
        if (high == p0) atomicAdd(&h[bin], 1u);
        if (high == p1) atomicAdd(&h[BD_BINS + bin], 1u);
    }
    __syncthreads();
    unsigned *out = hist + z * 2 * BD_BINS;
    for (int i = threadIdx.x; i < 2 * BD_BINS; i += 256)
        if (h[i]) __hip_atomic_fetch_add(&out[i], h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (2 B): one workgroup per image and direction.  PER bins per thread: 2^nbits = 256 PER
template <int PER>
__global__ __launch_bounds__(256) void bd_pick_kernel(int first, int nbits, u64 q_num, u64 q_den, const u64 *__restrict__ cnt, u64 *state,
                                                      unsigned *hist)
{
    const size_t z = blockIdx.x;
    const u64 n = cnt[z];
    if (n == 0 || cnt[z ^ 1] == 0) return;
    u64 *S = state + z * BS_WORDS;
    u64 rank[2], prefix[2];
    if (first) {
        const u64 t = (n - 1) * q_num;                         // < 2^31 2^20
        rank[0] = t / q_den;
        rank[1] = rank[0] + 1 < n ? rank[0] + 1 : n - 1;
        prefix[0] = prefix[1] = 0;
        if (threadIdx.x == 0) S[BS_REM] = t % q_den;
    } else {
        rank[0] = S[BS_RANK]; rank[1] = S[BS_RANK + 1];
        prefix[0] = S[BS_PREFIX]; prefix[1] = S[BS_PREFIX + 1];
    }
    for (int t = 0; t < 2; ++t) {
        unsigned *bins = hist + (z * 2 + t) * BD_BINS + threadIdx.x * PER;
        unsigned c[PER];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { c[k] = bins[k]; bins[k] = 0; mine += (int)c[k]; }
        int total;
        const u64 below = (u64)block_scan256(mine, total);      // the bins hold the d2 with this prefix: rank[t] < total <= n < 2^31
        if (rank[t] >= below && rank[t] < below + (u64)mine) {  // one thread
            u64 r = rank[t] - below;
            int k = 0;
            while (r >= c[k]) r -= c[k++];
            S[BS_RANK + t] = r;
            S[BS_PREFIX + t] = prefix[t] << nbits | (u64)(threadIdx.x * PER + k);
        }
    }
}

// ---- 5. finish ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bd_finish_kernel(const u64 *__restrict__ cnt, const u64 *__restrict__ state, const BdPart *__restrict__ part,
                                                        size_t slots, long long *__restrict__ record)
{
    const size_t z = blockIdx.x;
    const u64 n = cnt[z];
    const bool defined = n != 0 && cnt[z ^ 1] != 0;
    double s = 0.0;
    u64 within[4] = {0, 0, 0, 0};
    unsigned none = 0, top = 0;
    if (defined)
        for (size_t i = threadIdx.x; i < slots; i += 256) {     // a thread takes its slots in slot order, the tree below is fixed
            const BdPart p = part[z * slots + i];
            s += p.sum;
            for (int k = 0; k < 4; ++k) within[k] += p.within[k];
            top = max(top, p.top);
        }
    s = block_sum256(s);
    for (int k = 0; k < 4; ++k) within[k] = block_sum256(within[k]);
    block_sum_max256(none, top);
    if (threadIdx.x != 0) return;
    const u64 *S = state + z * BS_WORDS;
    long long *R = record + z * BD_REC;
    R[0] = (long long)n;
    R[1] = (long long)top;
    R[2] = defined ? (long long)S[BS_PREFIX] : 0;
    R[3] = defined ? (long long)S[BS_PREFIX + 1] : 0;
    R[4] = defined ? (long long)S[BS_REM] : 0;
    for (int i = 0; i < 4; ++i) R[5 + i] = (long long)within[i];
    R[9] = __builtin_bit_cast(long long, s);
}

} // namespace unet

using namespace unet;

#define BD_SIZE_CHECK(name) ARG_CHECK(sizes_ok(B, H, W, DM_EDGE), name ": image too large (H, W <= 32767, H * W < 2^31, B <= 65535)")
#define BD_MASK_CHECK(name, what, ptr, dtype, select)                                                                                          \
    ARG_CHECK((ptr) && (dtype) >= 0 && (dtype) <= 3 && (select) >= -1,                                                                          \
              name ": " what " must not be NULL, its dtype 0 (int64), 1 (float32), 2 (int32) or 3 (uint8), its select -1 (mask != 0) or a class >= 0")
#define BD_RULE_CHECK(name)                                                                                                                    \
    ARG_CHECK((connectivity == 4 || connectivity == 8) && (edge == 0 || edge == 1),                                                             \
              name ": connectivity must be 4 or 8 and edge 0 (ignore) or 1 (background)")

int unet_mask_boundary(const void *mask, int mask_dtype, int select, int B, int H, int W, int connectivity, int edge, void *out_u8, void *stream)
{
    ARG_CHECK(out_u8 && B > 0 && H > 0 && W > 0, "unet_mask_boundary: bad argument");
    BD_MASK_CHECK("unet_mask_boundary", "mask", mask, mask_dtype, select);
    BD_RULE_CHECK("unet_mask_boundary");
    BD_SIZE_CHECK("unet_mask_boundary");
    hipLaunchKernelGGL(bd_mark_kernel, dim3(grid_for((size_t)H * W, 256, 2048), B), dim3(256), 0, (hipStream_t)stream, BdMask{mask, mask_dtype, select},
                       BdMask{nullptr, 0, -1}, H, W, connectivity, edge, (unsigned char *)out_u8, (u64 *)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// [counts | state | histograms : cleared by the call] [bits] [g: 2 planes] [d2: 2 planes] [the slots of bd_rows]
namespace {
struct BdLayout { size_t state, hist, front, bits, g, d2, partial, total, plane, slots; };
BdLayout bd_layout(int B, int H, int W)
{
    BdLayout l;
    const size_t z = 2 * (size_t)B;
    l.state = align_up(z * sizeof(u64), 256);
    l.hist = l.state + align_up(z * BS_WORDS * sizeof(u64), 256);
    l.front = l.hist + z * 2 * BD_BINS * sizeof(unsigned);
    l.bits = l.front;
    l.plane = plane_bytes(B, H, W, sizeof(int));
    l.g = l.bits + plane_bytes(B, H, W, 1);
    l.d2 = l.g + 2 * l.plane;
    l.partial = l.d2 + 2 * l.plane;
    l.slots = (size_t)H * cdiv(W, 256);
    l.total = l.partial + align_up(z * l.slots * sizeof(BdPart), 256);
    return l;
}
}

size_t unet_surface_sums_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return bd_layout(B, H, W).total;
}

int unet_surface_sums(const void *pred, int pred_dtype, int pred_select, const void *gt, int gt_dtype, int gt_select, int B, int H, int W,
                      int connectivity, int edge, long long q_num, long long q_den, const int *t2_i32, int n_t2, void *record,
                      void *d2_pg_i32, void *d2_gp_i32, void *scratch, void *stream)
{
    ARG_CHECK(record && scratch && B > 0 && H > 0 && W > 0, "unet_surface_sums: bad argument");
    BD_MASK_CHECK("unet_surface_sums", "pred", pred, pred_dtype, pred_select);
    BD_MASK_CHECK("unet_surface_sums", "gt", gt, gt_dtype, gt_select);
    BD_RULE_CHECK("unet_surface_sums");
    ARG_CHECK(q_den >= 1 && q_den < (1 << 20) && q_num >= 0 && q_num <= q_den, "unet_surface_sums: the percentile needs 0 <= q_num <= q_den, 1 <= q_den < 2^20");
    ARG_CHECK(n_t2 >= 0 && n_t2 <= 4 && (n_t2 == 0 || t2_i32), "unet_surface_sums: n_t2 must be in [0, 4], t2_i32 not NULL when it is above 0");
    BdT2 t2 = {n_t2, {0, 0, 0, 0}};
    for (int i = 0; i < n_t2; ++i) {
        ARG_CHECK(t2_i32[i] >= 0, "unet_surface_sums: a squared tolerance must not be negative");
        t2.v[i] = (unsigned)t2_i32[i];
    }
    BD_SIZE_CHECK("unet_surface_sums");
    hipStream_t st = (hipStream_t)stream;
    const BdLayout l = bd_layout(B, H, W);
    const size_t npx = (size_t)H * W;
    char *base = (char *)scratch;
    u64 *cnt = (u64 *)base, *state = (u64 *)(base + l.state);
    unsigned *hist = (unsigned *)(base + l.hist);
    unsigned char *bits = (unsigned char *)(base + l.bits);
    int *g = (int *)(base + l.g);
    int *d2_pg = d2_pg_i32 ? (int *)d2_pg_i32 : (int *)(base + l.d2);
    int *d2_gp = d2_gp_i32 ? (int *)d2_gp_i32 : (int *)(base + l.d2 + l.plane);
    BdPart *partial = (BdPart *)(base + l.partial);
    HIP_TRY(hipMemsetAsync(scratch, 0, l.front, st));
    hipLaunchKernelGGL(bd_mark_kernel, dim3(count_blocks(npx, B), B), dim3(256), 0, st, BdMask{pred, pred_dtype, pred_select},
                       BdMask{gt, gt_dtype, gt_select}, H, W, connectivity, edge, bits, cnt);
    for (int c = 0; c < 2; ++c)                                // nothing lies past the image for a distance to a contour: edge 0
        hipLaunchKernelGGL(dm_cols_kernel<BdSite>, dim3(cdiv(W, 64), B), dim3(256), 0, st, BdSite{bits, 1 << c}, H, W, 0,
                           g + (size_t)c * (l.plane / sizeof(int)));
    hipLaunchKernelGGL(bd_rows_kernel, dim3(cdiv(W, 256), 2 * H, B), dim3(256), 0, st, (const unsigned char *)bits, (const int *)g,
                       l.plane / sizeof(int), H, W, t2, (const u64 *)cnt, d2_pg, d2_gp, partial);
    const dim3 hgrid(grid_for(npx, 2048, 64), 2, B);
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = 20 - 10 * pass, nbits = pass == 0 ? 11 : 10;
        hipLaunchKernelGGL(bd_hist_kernel, hgrid, dim3(256), 0, st, (const int *)d2_pg, (const int *)d2_gp, npx, shift, nbits, (const u64 *)cnt,
                           (const u64 *)state, hist);
        if (pass == 0)
            hipLaunchKernelGGL(bd_pick_kernel<BD_BINS / 256>, dim3(2 * B), dim3(256), 0, st, 1, nbits, (u64)q_num, (u64)q_den, (const u64 *)cnt, state, hist);
        else
            hipLaunchKernelGGL(bd_pick_kernel<BD_BINS / 512>, dim3(2 * B), dim3(256), 0, st, 0, nbits, (u64)q_num, (u64)q_den, (const u64 *)cnt, state, hist);
    }
    hipLaunchKernelGGL(bd_finish_kernel, dim3(2 * B), dim3(256), 0, st, (const u64 *)cnt, (const u64 *)state, (const BdPart *)partial, l.slots,
                       (long long *)record);
    HIP_TRY(hipGetLastError());
    return 0;
}
