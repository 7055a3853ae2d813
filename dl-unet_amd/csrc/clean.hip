// clean.hip — cleaning a foreground mask between the argmax and the instance map, batched, on the device: fill holes, drop
// small cells and cells on the frame (scipy.ndimage.binary_fill_holes, skimage's remove_small_holes / remove_small_objects /
// clear_border), and the labelling of either phase of a mask with either connectivity that this needs.
//
// A labelling (cl_roots) of the pixels with (mask != 0) == phase, 4- or 8-connected:
//   1. cl_local    one workgroup per 32x32 tile: union-find in LDS (W, N and for connectivity 8 NW, NE neighbours), every pixel ->
//                  its tile-local root (image index); the tile-local root's word of the attribute plane = the pixels under it in
//                  the tile, bit 31 = one of them lies in the first or last row or column; every other word of the plane = 0
//   2. cl_merge    one thread per tile-border position: union of the roots of the straight pair across the border and, for
//                  connectivity 8, of the two diagonal pairs that start there (only where the straight pair is not both in the
//                  phase: else each diagonal's far end is a neighbour along the border of a pixel already joined).  The diagonals
//                  of a vertical border run over all rows, so the two pairs across a tile corner, (31,31)-(32,32) and
//                  (32,31)-(31,32), are among them
//   3. cl_flatten  label = root (the smallest pixel index of the component); a tile-local root that is not the root adds its
//                  count to the root's word and ors its frame bit into it: one or two atomics per tile-local component, not per
//                  pixel, so the one large background component costs one add per tile it covers
// unet_label_components_conn: 1-3, then inst_number (instances.hip passes 4-7).  For phase 1 and connectivity 4 every word is
// what ccl_labels (wmap.hip) and the same passes give: the root of a component is its smallest index whatever the union order.
//
// unet_clean_mask:
//   holes  1-3 on the background with the dual connectivity, then
//   4. cl_fill     filled plane (uint8) = 1 on foreground, 2 on a background pixel whose component has no frame bit and an area
//                  <= max_hole_area, else 0; counts the holes (their roots) and their pixels
//   cells  1-3 on the filled plane's foreground with the connectivity given, then
//   5. cl_select   per pixel the action from the root's word (area < min_area: 3; frame bit and drop_border: 4; else 1 or,
//                  where cl_fill wrote 2, 2), the output mask and the counts
// A fixed list of launches for given arguments, every pixel a fixed number of times: the cost does not depend on how many holes
// or cells there are.  Every count is an integer sum and the frame bit an or: the results do not depend on the order of the
// atomics.  An area is below 2^31 (H * W < 2^31), so bit 31 of a word is never reached by the adds.
//
// Coherence (wmap.hip's rule): in cl_merge every read and update of a parent word is an agent-scope atomic read-modify-write
// and the phase tests read the mask, never the parent words; in cl_flatten a root's attribute word is only touched by agent-scope
// atomics (its own thread does not read it), and the word a thread reads plainly is a non-root's, which nothing writes there;
// the info words only by agent-scope adds.  Every other hand-off is a kernel boundary.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int CL_TILE = 32;
static constexpr unsigned CL_FRAME = 0x80000000u, CL_AREA = 0x7fffffffu;
enum { CI_HOLES = 0, CI_HOLE_PX = 1, CI_SMALL = 2, CI_SMALL_PX = 3, CI_BORDER = 4, CI_BORDER_PX = 5, CI_KEPT = 6, CI_WORDS = 7 };

// n[k], summed over the workgroup, is added to words[k] by one agent-scope add per workgroup and word (none where the sum is 0):
// the adds of a launch meet on a few words per image, so they are reduced in the wave and in LDS first.  Every thread calls it.
template <int N, typename W>
__device__ __forceinline__ void cl_counts(W *words, const unsigned (&n)[N])
{
    __shared__ unsigned tot[N];
    if (threadIdx.x < N) tot[threadIdx.x] = 0;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        const unsigned v = wave_sum(n[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], v);
    }
    __syncthreads();
    if (threadIdx.x < N && tot[threadIdx.x])
        __hip_atomic_fetch_add(&words[threadIdx.x], (W)tot[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 1. tile-local union-find and the tile-local attributes ----------------------------------------------------------------
__global__ __launch_bounds__(256) void cl_local_kernel(const void *__restrict__ mask, int dtype, int H, int W, int phase, int conn8,
                                                       int *__restrict__ parent, unsigned *__restrict__ attr)
{
    __shared__ int lp[CL_TILE * CL_TILE];
    __shared__ unsigned cnt[CL_TILE * CL_TILE];
    const int b = blockIdx.z, x0 = blockIdx.x * CL_TILE, y0 = blockIdx.y * CL_TILE, lane = threadIdx.x & 63;
    const size_t img = (size_t)b * H * W;
    bool in[4];
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 31), y = y0 + (i >> 5);
        in[k] = x < W && y < H && mask_on(mask, dtype, img + (size_t)y * W + x) == phase;
        lp[i] = in[k] ? i : -1;
        cnt[i] = 0;
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
        const int left = __shfl_up(l, 1, 64);                           // runs of equal roots among the 64: one add per run
        const unsigned long long heads = __ballot(lane == 0 || l != left);
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const unsigned n = above ? (unsigned)__ffsll(above) : (unsigned)(64 - lane);
        if ((heads >> lane & 1) && l >= 0) atomicAdd(&cnt[l], n);
        if (l >= 0 && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) atomicOr(&cnt[l], CL_FRAME);
    }
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 31), y = y0 + (i >> 5), l = root[k];
        if (x >= W || y >= H) continue;
        const size_t e = img + (size_t)y * W + x;
        parent[e] = l >= 0 ? (y0 + (l >> 5)) * W + x0 + (l & 31) : -1;
        if (attr) attr[e] = l == i ? cnt[i] : 0u;
    }
}

// ---- 2. merge across tile borders: agent-scope atomics only ------------------------------------------------------------------
// per image: (tiles_x - 1) vertical borders of H positions, then (tiles_y - 1) horizontal borders of W positions.  a | c is the
// straight pair at a position, d the step to the next position along the border; connectivity 8 adds a - (c + d) and (a + d) - c
__global__ __launch_bounds__(256) void cl_merge_kernel(const void *__restrict__ mask, int dtype, int H, int W, int phase, int conn8,
                                                       int *parent, int nv, int total)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t img = (size_t)blockIdx.y * H * W;
    int a, c, d;
    bool more;
    if (e < nv) {
        const int y = e % H, x = (e / H + 1) * CL_TILE;
        a = y * W + x - 1; c = y * W + x; d = W; more = y + 1 < H;
    } else {
        const int x = (e - nv) % W, y = ((e - nv) / W + 1) * CL_TILE;
        a = (y - 1) * W + x; c = y * W + x; d = 1; more = x + 1 < W;
    }
    const bool pa = mask_on(mask, dtype, img + a) == phase, pc = mask_on(mask, dtype, img + c) == phase;
    int *P = parent + img;
    if (pa && pc) gl_union(P, a, c);
    else if (conn8 && more) {               // with a | c joined, a diagonal adds nothing: its far end is a's or c's neighbour along the border
        if (pa && mask_on(mask, dtype, img + c + d) == phase) gl_union(P, a, c + d);
        if (pc && mask_on(mask, dtype, img + a + d) == phase) gl_union(P, a + d, c);
    }
}

// ---- 3. flatten: label = root; the tile-local attributes move to the root ---------------------------------------------------
__global__ __launch_bounds__(256) void cl_flatten_kernel(const int *__restrict__ parent, int *__restrict__ label, size_t npx,
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
                if (v & CL_AREA) __hip_atomic_fetch_add(&A[p], v & CL_AREA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v & CL_FRAME) __hip_atomic_fetch_or(&A[p], CL_FRAME, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        label[(size_t)b * npx + e] = p;
    }
    if (n_objects) {                                                    // uniform over the launch
        const unsigned n[1] = {(unsigned)roots};
        cl_counts(n_objects + b, n);
    }
}

// ---- 4. fill: the holes of the background labelling ---------------------------------------------------------------------------
// label == nullptr: no labelling was made (fill_holes off), filled = the foreground
__global__ __launch_bounds__(256) void cl_fill_kernel(const void *__restrict__ mask, int dtype, size_t npx, const int *__restrict__ label,
                                                      const unsigned *__restrict__ attr, long long max_hole,
                                                      unsigned char *__restrict__ filled, unsigned long long *info)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned holes = 0, px = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        unsigned char v = mask_on(mask, dtype, img + e) ? 1 : 0;
        if (!v && label) {
            const int r = label[img + e];
            const unsigned a = attr[img + r];
            if (!(a & CL_FRAME) && (max_hole < 0 || (long long)(a & CL_AREA) <= max_hole)) {
                v = 2;
                ++px;
                holes += r == (int)e;
            }
        }
        filled[img + e] = v;
    }
    const unsigned n[2] = {holes, px};
    cl_counts(info + blockIdx.y * CI_WORDS + CI_HOLES, n);
}

// ---- 5. select: the action of every pixel from its cell's area and frame bit, the output mask, the counts -------------------
template <typename T>
__global__ __launch_bounds__(256) void cl_select_kernel(const T *__restrict__ mask, const unsigned char *__restrict__ filled,
                                                        const int *__restrict__ label, const unsigned *__restrict__ attr, size_t npx,
                                                        long long min_area, int drop_border, T *__restrict__ out,
                                                        unsigned char *__restrict__ action, unsigned long long *info)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned n[CI_WORDS - CI_SMALL] = {0, 0, 0, 0, 0};
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned char f = filled[img + e];
        unsigned char act = 0;
        if (f) {
            const int r = label[img + e];
            const unsigned a = attr[img + r], first = r == (int)e;
            if ((long long)(a & CL_AREA) < min_area) { act = 3; n[CI_SMALL - CI_SMALL] += first; ++n[CI_SMALL_PX - CI_SMALL]; }
            else if (drop_border && (a & CL_FRAME)) { act = 4; n[CI_BORDER - CI_SMALL] += first; ++n[CI_BORDER_PX - CI_SMALL]; }
            else { act = f; n[CI_KEPT - CI_SMALL] += first; }
        }
        out[img + e] = act == 1 ? mask[img + e] : act == 2 ? T(1) : T(0);
        if (action) action[img + e] = act;
    }
    cl_counts(info + blockIdx.y * CI_WORDS + CI_SMALL, n);
}

// workgroups per image of the grid-stride passes: about 4096 in all, so that the adds of cl_counts stay few per word
static int cl_blocks(size_t npx, int B) { return grid_for(npx, 256, 4096 / B > 1 ? 4096 / B : 1); }

// passes 1-3 on st: parent and label are int planes [B,H,W], attr an unsigned one or null (no attributes); label = the root or -1
// off the phase; with attr, attr[root] = the component's area, bit 31 = it touches the frame; n_objects [B] (or null) is zeroed
// here and receives the component counts.  The parent words are dead afterwards.  The caller has checked the sizes.
static int cl_roots(const void *mask, int dtype, int B, int H, int W, int phase, int conn8, int *parent, int *label, unsigned *attr,
                    int *n_objects, hipStream_t st)
{
    const size_t npx = (size_t)H * W;
    if (n_objects) HIP_TRY(hipMemsetAsync(n_objects, 0, (size_t)B * sizeof(int), st));
    const int tx = cdiv(W, CL_TILE), ty = cdiv(H, CL_TILE);
    hipLaunchKernelGGL(cl_local_kernel, dim3(tx, ty, B), dim3(256), 0, st, mask, dtype, H, W, phase, conn8, parent, attr);
    const int nv = (tx - 1) * H, total = nv + (ty - 1) * W;
    if (total > 0)
        hipLaunchKernelGGL(cl_merge_kernel, dim3(cdiv(total, 256), B), dim3(256), 0, st, mask, dtype, H, W, phase, conn8, parent, nv,
                           total);
    hipLaunchKernelGGL(cl_flatten_kernel, dim3(cl_blocks(npx, B), B), dim3(256), 0, st, (const int *)parent, label, npx, attr,
                       n_objects);
    return 0;
}

} // namespace unet

using namespace unet;

static bool cl_sizes_ok(int B, int H, int W) { return (size_t)H * W < (1u << 31) && H <= 65535 && B <= 65535; }

size_t unet_label_components_conn_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return plane_bytes(B, H, W, sizeof(int)) + inst_chunk_bytes(B, H, W);
}

int unet_label_components_conn(const void *mask, int dtype, int B, int H, int W, int connectivity, int phase, void *labels_i32,
                               void *n_objects_i32, void *scratch, void *stream)
{
    ARG_CHECK(mask && labels_i32 && n_objects_i32 && scratch && B > 0 && H > 0 && W > 0, "unet_label_components_conn: bad argument");
    ARG_CHECK(dtype >= 0 && dtype <= 3, "unet_label_components_conn: dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_label_components_conn: connectivity must be 4 or 8");
    ARG_CHECK(phase == 0 || phase == 1, "unet_label_components_conn: phase must be 0 (mask == 0) or 1 (mask != 0)");
    ARG_CHECK(cl_sizes_ok(B, H, W), "unet_label_components_conn: image too large");
    hipStream_t st = (hipStream_t)stream;
    int *plane = (int *)scratch;                                  // the parent words, then (they are dead after cl_flatten) the ids
    int *chunk_roots = (int *)((char *)scratch + plane_bytes(B, H, W, sizeof(int)));
    if (int rc = cl_roots(mask, dtype, B, H, W, phase, connectivity == 8, plane, (int *)labels_i32, nullptr, (int *)n_objects_i32, st))
        return rc;
    return inst_number((int *)labels_i32, plane, chunk_roots, B, H, W, st);
}

size_t unet_clean_mask_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * plane_bytes(B, H, W, sizeof(int)) + plane_bytes(B, H, W, sizeof(unsigned)) + plane_bytes(B, H, W, 1);
}

int unet_clean_mask(const void *mask, int dtype, int B, int H, int W, int connectivity, int fill, long long max_hole_area,
                    long long min_area, int drop_border, void *out, void *action_u8, void *info_i64, void *scratch, void *stream)
{
    ARG_CHECK(mask && out && info_i64 && scratch && B > 0 && H > 0 && W > 0, "unet_clean_mask: bad argument");
    ARG_CHECK(dtype >= 0 && dtype <= 3, "unet_clean_mask: dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_clean_mask: connectivity must be 4 or 8");
    ARG_CHECK(max_hole_area >= -1 && min_area >= 0, "unet_clean_mask: max_hole_area must be >= -1 (no limit) and min_area >= 0");
    ARG_CHECK(cl_sizes_ok(B, H, W), "unet_clean_mask: image too large");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W, ib = plane_bytes(B, H, W, sizeof(int));
    char *s = (char *)scratch;
    int *parent = (int *)s, *label = (int *)(s + ib);
    unsigned *attr = (unsigned *)(s + 2 * ib);
    unsigned char *filled = (unsigned char *)(s + 3 * ib);
    unsigned long long *info = (unsigned long long *)info_i64;
    const int conn8 = connectivity == 8;
    const dim3 grid(cl_blocks(npx, B), B);
    HIP_TRY(hipMemsetAsync(info, 0, (size_t)B * CI_WORDS * sizeof(unsigned long long), st));
    if (fill) {                                                   // the background takes the dual connectivity
        if (int rc = cl_roots(mask, dtype, B, H, W, 0, !conn8, parent, label, attr, nullptr, st)) return rc;
    }
    hipLaunchKernelGGL(cl_fill_kernel, grid, dim3(256), 0, st, mask, dtype, npx, fill ? (const int *)label : (const int *)nullptr,
                       (const unsigned *)attr, max_hole_area, filled, info);
    if (int rc = cl_roots(filled, 3, B, H, W, 1, conn8, parent, label, attr, nullptr, st)) return rc;
    auto select = [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(cl_select_kernel<T>, grid, dim3(256), 0, st, (const T *)mask, (const unsigned char *)filled, (const int *)label,
                           (const unsigned *)attr, npx, min_area, drop_border, (T *)out, (unsigned char *)action_u8, info);
    };
    if (dtype == 0) select((long long)0);
    else if (dtype == 1) select(0.0f);
    else if (dtype == 2) select((int)0);
    else select((unsigned char)0);
    HIP_TRY(hipGetLastError());
    return 0;
}
