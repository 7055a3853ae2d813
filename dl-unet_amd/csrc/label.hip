// label.hip — the connected components of a mask, batched, on the device: the one labelling that the weight map (wmap.hip), the
// cell instances (functions.label_cells) and the mask clean-up (clean.hip) stand on.
//
// A labelling (label_roots, common.hpp) of the pixels with (mask != 0) == phase, 4- or 8-connected:
//   1. label_local    one workgroup per 32x32 tile: union-find in LDS (W, N and for connectivity 8 NW, NE neighbours), every pixel
//                     -> its tile-local root (image index); the tile-local root's word of the attribute plane = the pixels under it
//                     in the tile, bit 31 = one of them lies in the first or last row or column; every other word of the plane = 0.
//                     Without an attribute plane (a template flag) no such counts are kept, and the pixels in the phase can be
//                     counted per image instead (the weight map's count(1))
//   2. label_merge    one thread per tile-border position: union of the roots of the straight pair across the border and, for
//                     connectivity 8, of the two diagonal pairs that start there (only where the straight pair is not both in the
//                     phase: else each diagonal's far end is a neighbour along the border of a pixel already joined).  The diagonals
//                     of a vertical border run over all rows, so the two pairs across a tile corner, (31,31)-(32,32) and
//                     (32,31)-(31,32), are among them.  Connectivity 4 reads the second pixel of a pair only behind a first one in
//                     the phase, connectivity 8 both at once
//   3. label_flatten  label = root (the smallest pixel index of the component); a tile-local root that is not the root adds its
//                     count to the root's word and ors its frame bit into it: one or two atomics per tile-local component, not per
//                     pixel, so the one large background component costs one add per tile it covers
// The root of a component is its smallest index whatever the union order, so every word of the result is fixed by the mask.
//
// The raster numbering (inst_number) of such roots:
//   4. inst_count  one workgroup per 1024 consecutive pixels: how many of them are roots (label[e] == e)
//   5. inst_scan   one workgroup per image: exclusive scan of those counts
//   6. inst_rank   the same 1024 pixels again: a root writes 1 + (roots before it in raster order) into the id plane at its index
//   7. inst_write  labels = id[root], 0 off the phase
// A component's root is its first pixel in raster order, so the ranks of the roots are the raster numbering of
// scipy.ndimage.label / cv.connectedComponents.  Passes 4-7 touch every pixel a fixed number of times: their cost does not depend
// on how many components there are.
//
// unet_label_components: 1-7 for phase 1 and connectivity 4.  unet_label_components_conn: 1-7 for either phase and connectivity.
//
// Every count is an integer sum and the frame bit an or: the results do not depend on the order of the atomics.  An area is
// below 2^31 (H * W < 2^31), so bit 31 of a word is never reached by the adds.
//
// Coherence (MI355X: per-XCD L2s are not coherent, a CU's L1 is never refreshed by other CUs' stores): in label_merge every read
// and update of a parent word is an agent-scope atomic read-modify-write and the phase tests read the mask, never the parent
// words; in label_flatten a root's attribute word is only touched by agent-scope atomics (its own thread does not read it), and
// the word a thread reads plainly is a non-root's, which nothing writes there; the count words only by agent-scope adds.  Every
// other hand-off is a kernel boundary.  No loop waits on a plain load.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int LB_TILE = 32;
static constexpr int IN_CHUNK = 1024;                        // pixels per workgroup of inst_count / inst_rank: 256 threads x 4

// ---- 1. tile-local union-find and the tile-local attributes ----------------------------------------------------------------
// ATTR: the attribute plane is written.  Without it the kernel keeps no counts per root, and fg_counts (or null; uniform over the
// launch) receives the pixels in the phase: fg_counts[b] += the tile's
template <bool ATTR>
__global__ __launch_bounds__(256) void label_local_kernel(const void *__restrict__ mask, int dtype, int H, int W, int phase, int conn8,
                                                          int *__restrict__ parent, unsigned *__restrict__ attr,
                                                          unsigned long long *fg_counts)
{
    __shared__ int lp[LB_TILE * LB_TILE];
    __shared__ unsigned cnt[ATTR ? LB_TILE * LB_TILE : 1];
    const int b = blockIdx.z, x0 = blockIdx.x * LB_TILE, y0 = blockIdx.y * LB_TILE, lane = threadIdx.x & 63;
    const size_t img = (size_t)b * H * W;
    bool in[4];
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 31), y = y0 + (i >> 5);
        in[k] = x < W && y < H && mask_on(mask, dtype, img + (size_t)y * W + x) == phase;
        lp[i] = in[k] ? i : -1;
        if constexpr (ATTR) cnt[i] = 0;
    }
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, tx = i & 31;
        if (!in[k]) continue;
        if (tx && lp[i - 1] >= 0) lds_union(lp, i - 1, i);              // the sign of a word never changes: plain read
        if (i < 32) continue;
        if (lp[i - 32] >= 0) { lds_union(lp, i - 32, i); continue; }    // N joins NW and NE itself, as its own W and E neighbours
        if (conn8 && tx && lp[i - 33] >= 0) lds_union(lp, i - 33, i);
        if (conn8 && tx < 31 && lp[i - 31] >= 0) lds_union(lp, i - 31, i);
    }
    __syncthreads();
    int root[4];
    for (int k = 0; k < 4; ++k) {                                       // wave-uniform: the lanes of a wave hold two tile rows
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 31), y = y0 + (i >> 5);
        const int l = root[k] = in[k] ? lds_find(lp, i) : -1;
        if constexpr (ATTR) {
            const int left = __shfl_up(l, 1, 64);                       // runs of equal roots among the 64: one add per run
            const unsigned long long heads = __ballot(lane == 0 || l != left);
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const unsigned n = above ? (unsigned)__ffsll(above) : (unsigned)(64 - lane);
            if ((heads >> lane & 1) && l >= 0) atomicAdd(&cnt[l], n);
            if (l >= 0 && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) atomicOr(&cnt[l], LB_FRAME);
        }
    }
    if constexpr (ATTR) __syncthreads();
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 31), y = y0 + (i >> 5), l = root[k];
        if (x >= W || y >= H) continue;
        const size_t e = img + (size_t)y * W + x;
        parent[e] = l >= 0 ? (y0 + (l >> 5)) * W + x0 + (l & 31) : -1;
        if constexpr (ATTR) attr[e] = l == i ? cnt[i] : 0u;
    }
    if constexpr (!ATTR) {
        if (fg_counts) {
            const unsigned n[1] = {(unsigned)in[0] + in[1] + in[2] + in[3]};
            block_counts(fg_counts + b, n);
        }
    }
}

// ---- 2. merge across tile borders: agent-scope atomics only (gl_find / gl_union: elem.hpp) -----------------------------------
// per image: (tiles_x - 1) vertical borders of H positions, then (tiles_y - 1) horizontal borders of W positions.  a | c is the
// straight pair at a position, d the step to the next position along the border; connectivity 8 adds a - (c + d) and (a + d) - c
__global__ __launch_bounds__(256) void label_merge_kernel(const void *__restrict__ mask, int dtype, int H, int W, int phase, int conn8,
                                                          int *parent, int nv, int total)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t img = (size_t)blockIdx.y * H * W;
    int a, c, d;
    bool more;
    if (e < nv) {
        const int y = e % H, x = (e / H + 1) * LB_TILE;
        a = y * W + x - 1; c = y * W + x; d = W; more = y + 1 < H;
    } else {
        const int x = (e - nv) % W, y = ((e - nv) / W + 1) * LB_TILE;
        a = (y - 1) * W + x; c = y * W + x; d = 1; more = x + 1 < W;
    }
    const bool pa = mask_on(mask, dtype, img + a) == phase;
    bool pc;
    if (conn8) pc = mask_on(mask, dtype, img + c) == phase;             // the diagonals need either: both reads in flight together
    else pc = pa && mask_on(mask, dtype, img + c) == phase;             // c is read only where it can join
    int *P = parent + img;
    if (pa && pc) gl_union(P, a, c);
    else if (conn8 && more) {               // with a | c joined, a diagonal adds nothing: its far end is a's or c's neighbour along the border
        if (pa && mask_on(mask, dtype, img + c + d) == phase) gl_union(P, a, c + d);
        if (pc && mask_on(mask, dtype, img + a + d) == phase) gl_union(P, a + d, c);
    }
}

// ---- 3. flatten: label = root; the tile-local attributes move to the root ---------------------------------------------------
__global__ __launch_bounds__(256) void label_flatten_kernel(const int *__restrict__ parent, int *__restrict__ label, size_t npx,
                                                            unsigned *attr, int *__restrict__ n_objects)
{
    const int b = blockIdx.y;
    const int *P = parent + (size_t)b * npx;
    unsigned *A = attr ? attr + (size_t)b * npx : nullptr;
    int roots = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        int p = P[e];
        if (p >= 0) {
            while (P[p] != p) p = P[p];
            roots += p == (int)e;
            if (A && p != (int)e) {
                const unsigned v = A[e];                                // a non-root's word: nothing writes it in this kernel
                if (v & LB_AREA) __hip_atomic_fetch_add(&A[p], v & LB_AREA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v & LB_FRAME) __hip_atomic_fetch_or(&A[p], LB_FRAME, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        label[(size_t)b * npx + e] = p;
    }
    if (n_objects) {                                                    // uniform over the launch
        const unsigned n[1] = {(unsigned)roots};
        block_counts(n_objects + b, n);
    }
}

// ---- 4-7. raster numbering of the roots -------------------------------------------------------------------------------------
// roots among this thread's 4 consecutive pixels, as a bit mask
__device__ __forceinline__ int inst_roots(const int *__restrict__ L, size_t npx, size_t e0)
{
    int m = 0;
    for (int k = 0; k < 4; ++k)
        if (e0 + k < npx && L[e0 + k] == (int)(e0 + k)) m |= 1 << k;
    return m;
}

__global__ __launch_bounds__(256) void inst_count_kernel(const int *__restrict__ label, size_t npx, int *__restrict__ chunk_roots)
{
    const size_t e0 = (size_t)blockIdx.x * IN_CHUNK + threadIdx.x * 4;
    int total;
    block_scan256(__popc(inst_roots(label + (size_t)blockIdx.y * npx, npx, e0)), total);
    if (threadIdx.x == 0) chunk_roots[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// in place: chunk_roots[b][c] becomes the number of roots in the chunks before c
__global__ __launch_bounds__(256) void inst_scan_kernel(int *__restrict__ chunk_roots, int nchunk)
{
    int *c = chunk_roots + (size_t)blockIdx.x * nchunk;
    int carry = 0;
    for (int base = 0; base < nchunk; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < nchunk ? c[i] : 0;
        int total;
        const int before = block_scan256(v, total);
        if (i < nchunk) c[i] = carry + before;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void inst_rank_kernel(const int *__restrict__ label, size_t npx, const int *__restrict__ chunk_before,
                                                        int *__restrict__ id)
{
    const size_t img = (size_t)blockIdx.y * npx, e0 = (size_t)blockIdx.x * IN_CHUNK + threadIdx.x * 4;
    const int m = inst_roots(label + img, npx, e0);
    int total;
    int rank = chunk_before[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_scan256(__popc(m), total);
    for (int k = 0; k < 4; ++k)
        if (m >> k & 1) id[img + e0 + k] = ++rank;
}

// label holds the root (or -1) on entry and the component's number (or 0) on return; each thread rewrites only what it read
__global__ __launch_bounds__(256) void inst_write_kernel(int *__restrict__ label, size_t npx, const int *__restrict__ id)
{
    const size_t img = (size_t)blockIdx.y * npx;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int r = label[img + e];
        label[img + e] = r >= 0 ? id[img + r] : 0;
    }
}

// passes 1-3 on st (common.hpp)
int label_roots(const void *mask, int dtype, int B, int H, int W, int phase, int conn8, int *parent, int *label, unsigned *attr,
                int *n_objects, unsigned long long *fg_counts, hipStream_t st)
{
    const size_t npx = (size_t)H * W;
    if (n_objects) HIP_TRY(hipMemsetAsync(n_objects, 0, (size_t)B * sizeof(int), st));
    if (fg_counts) HIP_TRY(hipMemsetAsync(fg_counts, 0, (size_t)B * sizeof(unsigned long long), st));
    const int tx = cdiv(W, LB_TILE), ty = cdiv(H, LB_TILE);
    dispatch_bool(attr != nullptr, [&](auto with_attr) {
        hipLaunchKernelGGL(label_local_kernel<with_attr.value>, dim3(tx, ty, B), dim3(256), 0, st, mask, dtype, H, W, phase, conn8, parent,
                           attr, fg_counts);
    });
    const int nv = (tx - 1) * H, total = nv + (ty - 1) * W;
    if (total > 0)
        hipLaunchKernelGGL(label_merge_kernel, dim3(cdiv(total, 256), B), dim3(256), 0, st, mask, dtype, H, W, phase, conn8, parent, nv,
                           total);
    hipLaunchKernelGGL(label_flatten_kernel, dim3(count_blocks(npx, B), B), dim3(256), 0, st, (const int *)parent, label, npx, attr,
                       n_objects);
    return 0;
}

static size_t in_chunks(int H, int W) { return ((size_t)H * W + IN_CHUNK - 1) / IN_CHUNK; }
static size_t inst_chunk_bytes(int B, int H, int W) { return align_up((size_t)B * in_chunks(H, W) * sizeof(int), 256); }

// passes 4-7 on st: label [B,H,W] holds each pixel's root or -1 and becomes 1..n in raster order of the roots, 0 where it was -1;
// ids is an int plane of scratch, chunk_roots inst_chunk_bytes(B, H, W) bytes of it
static int inst_number(int *label, int *ids, int *chunk_roots, int B, int H, int W, hipStream_t st)
{
    const size_t npx = (size_t)H * W;
    const unsigned nchunk = (unsigned)in_chunks(H, W);
    hipLaunchKernelGGL(inst_count_kernel, dim3(nchunk, B), dim3(256), 0, st, (const int *)label, npx, chunk_roots);
    hipLaunchKernelGGL(inst_scan_kernel, dim3(B), dim3(256), 0, st, chunk_roots, (int)nchunk);
    hipLaunchKernelGGL(inst_rank_kernel, dim3(nchunk, B), dim3(256), 0, st, (const int *)label, npx, (const int *)chunk_roots, ids);
    hipLaunchKernelGGL(inst_write_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, label, npx, (const int *)ids);
    HIP_TRY(hipGetLastError());
    return 0;
}

// passes 1-7: the scratch is one int plane, the parent words and then (they are dead after label_flatten) the ids, and the chunk counts
static size_t label_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return plane_bytes(B, H, W, sizeof(int)) + inst_chunk_bytes(B, H, W);
}
static int label_numbered(const void *mask, int dtype, int B, int H, int W, int phase, int conn8, void *labels_i32, void *n_objects_i32,
                          void *scratch, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    int *plane = (int *)scratch;
    int *chunk_roots = (int *)((char *)scratch + plane_bytes(B, H, W, sizeof(int)));
    if (int rc = label_roots(mask, dtype, B, H, W, phase, conn8, plane, (int *)labels_i32, nullptr, (int *)n_objects_i32, nullptr, st))
        return rc;
    return inst_number((int *)labels_i32, plane, chunk_roots, B, H, W, st);
}

} // namespace unet

using namespace unet;

size_t unet_label_components_scratch_bytes(int B, int H, int W) { return label_scratch_bytes(B, H, W); }

int unet_label_components(const void *mask, int dtype, int B, int H, int W, void *labels_i32, void *n_objects_i32, void *scratch,
                          void *stream)
{
    ARG_CHECK(mask && labels_i32 && n_objects_i32 && scratch && B > 0 && H > 0 && W > 0, "unet_label_components: bad argument");
    ARG_CHECK(dtype == 0 || dtype == 1, "unet_label_components: dtype must be 0 (int64) or 1 (float32)");
    ARG_CHECK(label_sizes_ok(B, H, W), "unet_label_components: image too large");
    return label_numbered(mask, dtype, B, H, W, 1, 0, labels_i32, n_objects_i32, scratch, stream);
}

size_t unet_label_components_conn_scratch_bytes(int B, int H, int W) { return label_scratch_bytes(B, H, W); }

int unet_label_components_conn(const void *mask, int dtype, int B, int H, int W, int connectivity, int phase, void *labels_i32,
                               void *n_objects_i32, void *scratch, void *stream)
{
    ARG_CHECK(mask && labels_i32 && n_objects_i32 && scratch && B > 0 && H > 0 && W > 0, "unet_label_components_conn: bad argument");
    ARG_CHECK(dtype >= 0 && dtype <= 3, "unet_label_components_conn: dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_label_components_conn: connectivity must be 4 or 8");
    ARG_CHECK(phase == 0 || phase == 1, "unet_label_components_conn: phase must be 0 (mask == 0) or 1 (mask != 0)");
    ARG_CHECK(label_sizes_ok(B, H, W), "unet_label_components_conn: image too large");
    return label_numbered(mask, dtype, B, H, W, phase, connectivity == 8, labels_i32, n_objects_i32, scratch, stream);
}
