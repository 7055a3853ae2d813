// hull.hip — the convex hull of every cell of an instance map and what is measured on it (area, largest and smallest calliper
// width), batched, on the device: what a loop over cells with scipy.spatial.ConvexHull gives one cell at a time
// (functions.cell_hulls, functions.hull_props).
//
// A pixel (y, x) is the closed unit square [x, x+1] x [y, y+1]; the hull K of id i >= 1 is the convex hull of the union of its
// pixels' squares, that is, of their integer corner points.  A cell whose box spans the rows [y0, y1) has h = y1 - y0 rows and
// h + 1 horizontal levels y0 .. y1; every corner point lies on one of them, and on a level only the leftmost and the rightmost
// corner can be a vertex of K.  So K is the hull of at most 2 (h + 1) points, two per level:
//   lo_k = the smallest x, hi_k = the largest x + 1, over the pixels of the (at most two) rows next to level k.
// The caller gives the boxes (unet_cell_sums's bbox) and the exclusive prefix sum of the level counts of the rows (b, i), which
// places every cell's levels in two flat 32-bit tables (lo kept as the maximum of ~x, so that one memset initialises both) and
// its vertices in a slice of the vertex output.
//
//   1. hull_fill    a wave reads 64 consecutive pixels, one ballot marks where the id changes or a row begins, and the head lane of
//                   a run of n equal ids at (y, x) raises ~x and x + n in the words k = y - y0 and k + 1 of its id (agent-scope
//                   32-bit atomic max).  A pixel with an id outside [0, n_max] is counted in status word 0; one outside its id's
//                   box, or whose id's level count does not fit its box or the tables, in status word 1; neither writes anything
//   2. hull_finish  one thread per (b, i): Andrew's monotone chain with strict turns down the left points, then up the right
//                   points, the cell's slice of the vertex output being the stack; then twice the area (shoelace), the largest
//                   squared distance between two vertices and the smallest width over the edges, by brute force over the k
//                   vertices (a lattice polygon in an h x w box has O((h w)^(1/3)) of them).  Levels next to no pixel of the
//                   cell (an id need not be connected) are skipped
// Everything is an integer and a maximum or a sum of integers: the outputs are the same in every run.
//
// The width of edge (p, q) is c / sqrt(l2), c = max over the vertices v of |cross(q - p, v - p)|, l2 = |q - p|^2.  The edge with
// the smallest c^2 / l2 wins, the smaller l2 on equal ratios.  c reaches 2^31 and l2 2^31 at H, W = 32768: the comparison
// c_a^2 l2_b < c_b^2 l2_a needs products of 93 bits and is made in unsigned __int128; nothing is divided.
//
// Coherence (label.hip's rule): during hull_fill a level word and a status word are touched only by agent-scope atomic
// read-modify-writes; hull_finish is a later kernel of the same stream and reads them plainly.  A thread of hull_finish reads back
// only vertices it stored itself.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

// where the levels of row r = b * (n_max + 1) + i lie: false for id 0, an empty or impossible box, and a level count that is
// not y1 - y0 + 1 or does not fit the tables [0, L)
struct HullRow { int y0, x0, y1, x1; long long base; };
__device__ __forceinline__ bool hull_row(const int *__restrict__ bbox, const long long *__restrict__ off, size_t r, int i, int H, int W,
                                         long long L, HullRow &o)
{
    if (i < 1) return false;
    o.y0 = bbox[r * 4 + 0]; o.x0 = bbox[r * 4 + 1]; o.y1 = bbox[r * 4 + 2]; o.x1 = bbox[r * 4 + 3];
    if (o.y0 < 0 || o.x0 < 0 || o.y1 > H || o.x1 > W || o.y0 >= o.y1 || o.x0 >= o.x1) return false;
    o.base = off[r];
    const long long end = off[r + 1], levels = (long long)(o.y1 - o.y0) + 1;
    return o.base >= 0 && o.base <= L && end - o.base == levels && levels <= L - o.base;
}

// ---- 1. fill ------------------------------------------------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void hull_fill_kernel(const LT *__restrict__ labels, int H, int W, int n_max, const int *__restrict__ bbox,
                                                        const long long *__restrict__ off, long long L, unsigned *lo_tab, unsigned *hi_tab,
                                                        u64 *status)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const size_t npx = (size_t)H * W, N = (size_t)n_max + 1;
    const LT *M = labels + (size_t)b * npx;
    u64 bad = 0, outside = 0;                                    // this lane's share of status[b][0..1]
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npx; base += stride) {   // wave-uniform
        const size_t e = base + lane;
        const bool in = e < npx;
        const int y = in ? (int)(e / W) : 0, x = in ? (int)(e - (size_t)y * W) : 0;
        int id = -2;                                             // the tail past the image
        if (in) {
            const LT v = M[e];
            id = (v < 0 || v > (LT)n_max) ? -1 : (int)v;         // refused ids form runs of their own
        }
        const int left = __shfl_up(id, 1, 64);
        const bool head = lane == 0 || id != left || x == 0;
        const u64 heads = __ballot(head);
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int n = above ? __ffsll(above) : 64 - lane;        // run length: up to the next head
        if (!head || !in || id == 0) continue;                   // no shuffle or ballot follows in this iteration
        if (id < 0) { bad += n; continue; }
        HullRow r;
        if (!hull_row(bbox, off, (size_t)b * N + id, id, H, W, L, r) || y < r.y0 || y >= r.y1) {
            outside += n;
            continue;
        }
        const int xa = max(x, r.x0), xb = min(x + n, r.x1);      // the part of the run inside the box
        if (xa >= xb) { outside += n; continue; }
        outside += n - (xb - xa);
        const long long k = r.base + (y - r.y0);                 // k + 1 <= base + (y1 - y0) < base + levels <= L
        const unsigned lo = ~(unsigned)xa, hi = (unsigned)xb;
        __hip_atomic_fetch_max(&lo_tab[k], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&lo_tab[k + 1], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&hi_tab[k], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&hi_tab[k + 1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bad = wave_sum(bad); outside = wave_sum(outside);
    if (lane == 0) {
        if (bad) __hip_atomic_fetch_add(&status[2 * b], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (outside) __hip_atomic_fetch_add(&status[2 * b + 1], outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- 2. finish ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long hull_cross(int2 o, int2 a, int2 c)
{
    return (long long)(a.x - o.x) * (c.y - o.y) - (long long)(a.y - o.y) * (c.x - o.x);
}

// pushes p on the chain that starts at vtx[first]: points that make no strict turn with p are dropped first
__device__ __forceinline__ void hull_push(int2 *vtx, long long first, long long &k, long long &top, int2 p)
{
    while (k - first >= 2 && hull_cross(vtx[k - 2], vtx[k - 1], p) >= 0) --k;
    vtx[k++] = p;
    top = max(top, k);                                           // how far the stack ever reached: dropped points lie below it
}

__global__ __launch_bounds__(256) void hull_finish_kernel(const int *__restrict__ bbox, const long long *__restrict__ off, long long L, size_t rows,
                                                          int n_max, int H, int W, const unsigned *__restrict__ lo_tab,
                                                          const unsigned *__restrict__ hi_tab, int *__restrict__ n_vertices,
                                                          long long *__restrict__ area2, long long *__restrict__ feret_max2,
                                                          long long *__restrict__ width, int2 *vertices)
{
    const size_t N = (size_t)n_max + 1;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
        HullRow o;
        long long k = 0, top = 0, a2 = 0, f2 = 0, wc = 0, wl = 0;
        if (hull_row(bbox, off, r, (int)(r % N), H, W, L, o)) {
            const int h = o.y1 - o.y0;
            int2 *vtx = vertices + 2 * o.base;                   // the slice [2 base, 2 (base + h + 1)): at most two points per level
            for (int l = 0; l <= h; ++l)                         // the left chain, downwards
                if (hi_tab[o.base + l]) hull_push(vtx, 0, k, top, make_int2((int)~lo_tab[o.base + l], o.y0 + l));
            const long long first = k;
            for (int l = h; l >= 0; --l)                         // the right chain, upwards
                if (hi_tab[o.base + l]) hull_push(vtx, first, k, top, make_int2((int)hi_tab[o.base + l], o.y0 + l));
            for (long long j = k; j < top; ++j) vtx[j] = make_int2(0, 0);      // the rest of the slice is 0 from the memset
            u128 best_num = 0;                                   // c^2 of the best edge so far
            for (long long e = 0; e < k; ++e) {
                const int2 p = vtx[e], q = vtx[e + 1 == k ? 0 : e + 1];
                a2 += (long long)p.x * q.y - (long long)q.x * p.y;
                long long c = 0;
                for (long long v = 0; v < k; ++v) {
                    const int2 t = vtx[v];
                    const long long cr = hull_cross(p, q, t), dx = t.x - p.x, dy = t.y - p.y;
                    c = max(c, cr < 0 ? -cr : cr);
                    f2 = max(f2, dx * dx + dy * dy);
                }
                const long long ex = q.x - p.x, ey = q.y - p.y, l2 = ex * ex + ey * ey;
                const u128 num = (u128)(u64)c * (u64)c;
                const u128 lhs = num * (u64)wl, rhs = best_num * (u64)l2;      // c^2 / l2 < best c^2 / best l2, cross-multiplied
                if (e == 0 || lhs < rhs || (lhs == rhs && l2 < wl)) { best_num = num; wc = c; wl = l2; }
            }
            if (a2 < 0) a2 = -a2;
        }
        n_vertices[r] = (int)k;
        area2[r] = a2;
        feret_max2[r] = f2;
        width[r * 2 + 0] = wc;
        width[r * 2 + 1] = wl;
    }
}

} // namespace unet

using namespace unet;

size_t unet_cell_hulls_scratch_bytes(long long n_levels)
{
    return n_levels <= 0 ? 0 : (size_t)n_levels * 2 * sizeof(unsigned);
}

int unet_cell_hulls(const void *labels, int label_dtype, int B, int H, int W, int n_max, const void *bbox_i32, const void *level_offset_i64,
                    long long n_levels, void *n_vertices_i32, void *area2_i64, void *feret_max2_i64, void *width_i64, void *vertices_i32,
                    void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(labels && bbox_i32 && level_offset_i64 && n_vertices_i32 && area2_i64 && feret_max2_i64 && width_i64 && status_u64 && B > 0 &&
              H > 0 && W > 0 && n_levels >= 0, "unet_cell_hulls: bad argument");
    ARG_CHECK(n_levels == 0 || (vertices_i32 && scratch), "unet_cell_hulls: n_levels > 0 needs vertices_i32 and scratch");
    ARG_CHECK(label_dtype == 0 || label_dtype == 2, "unet_cell_hulls: label dtype must be 0 (int64) or 2 (int32)");
    ARG_CHECK(measure_sizes_ok(B, H, W, n_max), "unet_cell_hulls: H, W must be <= 32768, B <= 65535 and n_max in [0, 2^24)");
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)B * ((size_t)n_max + 1), L = (size_t)n_levels;
    unsigned *lo_tab = (unsigned *)scratch, *hi_tab = lo_tab + L;
    if (L) {
        HIP_TRY(hipMemsetAsync(scratch, 0, L * 2 * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(vertices_i32, 0, L * 2 * sizeof(int2), st));      // the unused tail of every slice stays 0
    }
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * 2 * sizeof(u64), st));
    const dim3 grid(grid_for((size_t)H * W, 256, 2048), B);
    if (label_dtype == 0)
        hipLaunchKernelGGL(hull_fill_kernel<long long>, grid, dim3(256), 0, st, (const long long *)labels, H, W, n_max, (const int *)bbox_i32,
                           (const long long *)level_offset_i64, n_levels, lo_tab, hi_tab, (u64 *)status_u64);
    else
        hipLaunchKernelGGL(hull_fill_kernel<int>, grid, dim3(256), 0, st, (const int *)labels, H, W, n_max, (const int *)bbox_i32,
                           (const long long *)level_offset_i64, n_levels, lo_tab, hi_tab, (u64 *)status_u64);
    hipLaunchKernelGGL(hull_finish_kernel, dim3(grid_for(rows, 256, 4096)), dim3(256), 0, st, (const int *)bbox_i32,
                       (const long long *)level_offset_i64, n_levels, rows, n_max, H, W, (const unsigned *)lo_tab, (const unsigned *)hi_tab,
                       (int *)n_vertices_i32, (long long *)area2_i64, (long long *)feret_max2_i64, (long long *)width_i64, (int2 *)vertices_i32);
    HIP_TRY(hipGetLastError());
    return 0;
}
