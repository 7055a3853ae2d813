// shape.hip — seeds from the shape of a mask alone (functions.distance_map, functions.reconstruct, functions.shape_seeds: the
// distance map of the region, its h-maxima, and the domes that are left as seeds for functions.split_cells), batched, on the
// device.  Integers throughout.  DESIGN.md section 4o has the definitions in full.
//
// The distance map.  d2(p) is the exact squared Euclidean distance from a region pixel (mask != 0) to the nearest pixel outside
// the region, 0 outside it.  edge 0 ('ignore'): there is nothing past the image, and an image without a pixel outside the region
// gets H^2 + W^2 everywhere; edge 1 ('background'): every pixel past the image is outside the region.
//   1. dm_cols   dm.hpp's column pass (grow.hip's without ids; boundary.hip runs the same code on contours), the sites being the
//                pixels outside the region: g is the row distance to the nearest of them in the column (DM_FAR when the column
//                has none; with edge 1 the pixels above row 0 and below row H - 1 count)
//   2. dm_rows   one thread per pixel: d2 = min over x' of g(x')^2 + (x - x')^2, by dm.hpp's scan outwards from x' = x.  The
//                minimum starts at g(x)^2, with edge 1 at min(g(x)^2, (x + 1)^2, (W - x)^2), so a pixel at distance d looks at
//                about 2 d columns.  There is no id and no tie rule here, which is what grow_rows' brute force is for.
//
// Grey reconstruction by dilation, 4-connected: R is the least function on the region with R >= min(marker, under), R <= under and
// R(p) >= min(under(p), R(n)) for every region 4-neighbour n, i.e. the fixed point of
//      R(p) <- min(under(p), max(R(p), max over the 4-neighbours n of R(n)))        started at R = min(marker, under).
// Values only rise, every value ever held is a lower bound of the result (it is min(marker(q), under along a real path from q)),
// and a state that nothing raises satisfies the three conditions, so it is the least such function: any order of relaxation is
// exact.  Pixels outside the region and past the image hold -1 in both planes: they offer nothing (every region value is >= 0)
// and take nothing (min(-1, .) = -1), so the relaxation has no case distinction and the mask is read once.  Monotone and
// bounded, as sweep.hpp asks: values only rise, and under is a ceiling.  With connectivity 8 (unet_reconstruct_sweeps_conn) "4-"
// reads "8-" in all of the above, a diagonal neighbour counting whatever the two pixels beside the step are; the argument never
// uses which pixels are neighbours, only that the path behind a value is real.
//   1. rc_init    R = base = min(marker, under) and under, -1 outside the region; counts the values outside [0, 2^30]
//   2. rc_sweep   sweep.hpp's tile relaxation over R (geo.hip's sweep with a max in place of its min), under staged beside it
//   3. rc_finish  R with 0 outside the region, and the pixels with R > base per image
//
// The element-wise steps of shape_seeds: sh_heights (q = floor(16 sqrt(d2)) exactly, and q + hq), sh_lower (max(v - c, 0)),
// sh_maxima (1.0 where r2 < r1 and r1 >= a floor, else 0.0: a mask unet_label_components takes).
//
// Coherence (label.hip's rule): every kernel reads what an earlier kernel wrote (rc_sweep: sweep.hpp); in dm_cols a thread re-reads
// only its own column.  The counters are only touched by agent-scope adds.
#include "sweep.hpp"
#include "dm.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int RC_TOP = 1 << 30;                         // values are in [0, RC_TOP]

// dm.hpp's site test of the distance map: a pixel outside the region
template <typename T>
struct DmOutside {
    const T *mask;
    __device__ __forceinline__ bool operator()(size_t e) const { return mask[e] == 0; }
};

__global__ __launch_bounds__(256) void dm_rows_kernel(const int *__restrict__ g, int H, int W, int edge, int *__restrict__ d2)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const size_t row = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    const int *G = g + row;
    const unsigned own = (unsigned)G[x];
    unsigned best = own * own;
    if (edge) {                                                // the columns -1 and W
        const unsigned l = (unsigned)(x + 1), r = (unsigned)(W - x);
        best = min(best, min(l * l, r * r));
    }
    best = dm_row_best(G, x, W, best);
    d2[row + x] = best >= DM_FAR2 ? H * H + W * W : (int)best; // no pixel outside the region in the whole image
}

__device__ __forceinline__ long long rc_value(const void *p, int dtype, size_t e)
{
    return dtype == 0 ? ((const long long *)p)[e] : (long long)((const int *)p)[e];
}

__global__ __launch_bounds__(256) void rc_init_kernel(const void *__restrict__ marker, int marker_dtype, const void *__restrict__ under,
                                                      int under_dtype, const void *__restrict__ mask, int mask_dtype, size_t npx,
                                                      int *__restrict__ r, int *__restrict__ u, int *__restrict__ base,
                                                      unsigned long long *status)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned bad = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        long long m = rc_value(marker, marker_dtype, img + e), v = rc_value(under, under_dtype, img + e);
        const bool m_bad = m < 0 || m > RC_TOP, v_bad = v < 0 || v > RC_TOP;
        bad += m_bad || v_bad;
        m = m_bad ? 0 : m;                                     // such a value counts as 0
        v = v_bad ? 0 : v;
        const bool region = !mask || mask_on(mask, mask_dtype, img + e);
        const int start = region ? (int)(m < v ? m : v) : -1;
        r[img + e] = start;
        base[img + e] = start;
        u[img + e] = region ? (int)v : -1;
    }
    bad = block_sum256(bad);
    if (threadIdx.x == 0 && bad)
        __hip_atomic_fetch_add(&status[blockIdx.y], (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the SW_SEG pixels p[k * ALONG] of one line under the ceilings u[k * ALONG], relaxed forward (from the pixel before and the two
// ACROSS; with CONN == 8 from the four diagonal ones too) and backward (from the pixel after) in registers: v[k] is the value
// after both, bit k of the result says that it rose
template <int ALONG, int ACROSS, int CONN>
__device__ __forceinline__ unsigned rc_relax_line(const int *p, const int *u, int (&v)[SW_SEG])
{
    unsigned rose = 0;
    int top[SW_SEG];
    int run = p[-ALONG];
#pragma unroll
    for (int k = 0; k < SW_SEG; ++k) {
        const int own = p[k * ALONG], a = p[k * ALONG - ACROSS], b = p[k * ALONG + ACROSS];
        top[k] = u[k * ALONG];
        int n = max(a, b);
        if constexpr (CONN == 8)
            n = max(max(n, max(p[(k - 1) * ALONG - ACROSS], p[(k - 1) * ALONG + ACROSS])),
                    max(p[(k + 1) * ALONG - ACROSS], p[(k + 1) * ALONG + ACROSS]));
        const int c = min(top[k], max(n, run));
        rose |= (unsigned)(c > own) << k;
        run = v[k] = max(own, c);
    }
    run = p[SW_SEG * ALONG];
#pragma unroll
    for (int k = SW_SEG - 1; k >= 0; --k) {
        const int c = min(top[k], run);
        rose |= (unsigned)(c > v[k]) << k;
        run = v[k] = max(v[k], c);
    }
    return rose;
}

template <int CONN>
__global__ __launch_bounds__(256) void rc_sweep_kernel(const int *__restrict__ src, const int *__restrict__ under, int *__restrict__ dst,
                                                       int H, int W, unsigned *changed)
{
    __shared__ int s[SW_STAGED * SW_PITCH], su[SW_STAGED * SW_PITCH];                // 2 x 17.3 KiB
    const SweepTile tl = sweep_tile(H, W);
    sweep_stage(tl, H, W, [&](int i, bool in, size_t e, int, int, int, int) {       // past the image -1, which never changes
        s[i] = in ? src[e] : -1;
        su[i] = in ? under[e] : -1;
    });
    sweep_converge(s, [&](int o, int (&v)[SW_SEG]) { return rc_relax_line<1, SW_PITCH, CONN>(s + o, su + o, v); },
                   [&](int o, int (&v)[SW_SEG]) { return rc_relax_line<SW_PITCH, 1, CONN>(s + o, su + o, v); });
    sweep_write_back(tl, s, src, dst, W, changed, [](int k, int was) { return k > was; });
}

__global__ __launch_bounds__(256) void rc_finish_kernel(const int *__restrict__ r, const int *__restrict__ base, size_t npx,
                                                        int *__restrict__ out, unsigned *raised)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned n = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int v = r[img + e];
        n += v > base[img + e];
        out[img + e] = max(v, 0);
    }
    n = block_sum256(n);
    if (threadIdx.x == 0 && n) __hip_atomic_fetch_add(&raised[blockIdx.y], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// floor(sqrt(256 d2)) = floor(16 sqrt(d2)): 256 d2 < 2^39 is exact in fp64, whose square root is at most one off
__device__ __forceinline__ int sh_isqrt256(int d2)
{
    const long long v = 256ll * d2;
    long long q = (long long)sqrt((double)v);
    q -= q * q > v;
    q += (q + 1) * (q + 1) <= v;
    return (int)q;
}

__global__ __launch_bounds__(256) void sh_heights_kernel(const int *__restrict__ d2, size_t n, int hq, int *__restrict__ q,
                                                         int *__restrict__ lifted)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int v = sh_isqrt256(max(d2[e], 0));
        q[e] = v;
        if (lifted) lifted[e] = v + hq;
    }
}

__global__ __launch_bounds__(256) void sh_lower_kernel(const int *__restrict__ in, size_t n, int c, int *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
        out[e] = max(in[e] - c, 0);
}

__global__ __launch_bounds__(256) void sh_maxima_kernel(const int *__restrict__ r1, const int *__restrict__ r2, size_t n, int floor_q,
                                                        float *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int v = r1[e];
        out[e] = r2[e] < v && v >= floor_q ? 1.0f : 0.0f;
    }
}

} // namespace unet

using namespace unet;

static size_t sh_plane(int B, int H, int W) { return plane_bytes(B, H, W, sizeof(int)); }
#define SH_SIZE_CHECK(name) ARG_CHECK(sizes_ok(B, H, W, DM_EDGE), name ": image too large (H, W <= 32767, H * W < 2^31, B <= 65535)")

// [g, the column distances]
size_t unet_distance_map_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return sh_plane(B, H, W);
}

int unet_distance_map(const void *mask, int mask_dtype, int B, int H, int W, int edge, void *d2_i32, void *scratch, void *stream)
{
    ARG_CHECK(mask && d2_i32 && scratch && B > 0 && H > 0 && W > 0, "unet_distance_map: bad argument");
    ARG_CHECK(mask_dtype >= 0 && mask_dtype <= 3, "unet_distance_map: mask_dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(edge == 0 || edge == 1, "unet_distance_map: edge must be 0 (ignore) or 1 (background)");
    SH_SIZE_CHECK("unet_distance_map");
    hipStream_t st = (hipStream_t)stream;
    const dim3 cols(cdiv(W, 64), B);
    if (mask_dtype == 0) hipLaunchKernelGGL(dm_cols_kernel<DmOutside<long long>>, cols, dim3(256), 0, st, DmOutside<long long>{(const long long *)mask}, H, W, edge, (int *)scratch);
    else if (mask_dtype == 1) hipLaunchKernelGGL(dm_cols_kernel<DmOutside<float>>, cols, dim3(256), 0, st, DmOutside<float>{(const float *)mask}, H, W, edge, (int *)scratch);
    else if (mask_dtype == 2) hipLaunchKernelGGL(dm_cols_kernel<DmOutside<int>>, cols, dim3(256), 0, st, DmOutside<int>{(const int *)mask}, H, W, edge, (int *)scratch);
    else hipLaunchKernelGGL(dm_cols_kernel<DmOutside<unsigned char>>, cols, dim3(256), 0, st, DmOutside<unsigned char>{(const unsigned char *)mask}, H, W, edge, (int *)scratch);
    hipLaunchKernelGGL(dm_rows_kernel, dim3(cdiv(W, 256), H, B), dim3(256), 0, st, (const int *)scratch, H, W, edge, (int *)d2_i32);
    HIP_TRY(hipGetLastError());
    return 0;
}

// [R plane 0, the current one between calls | R plane 1 | under | base = min(marker, under)]
size_t unet_reconstruct_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 4 * sh_plane(B, H, W);
}

int unet_reconstruct_init(const void *marker, int marker_dtype, const void *under, int under_dtype, const void *mask, int mask_dtype, int B,
                          int H, int W, void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(marker && under && status_u64 && scratch && B > 0 && H > 0 && W > 0, "unet_reconstruct_init: bad argument");
    ARG_CHECK((marker_dtype == 0 || marker_dtype == 2) && (under_dtype == 0 || under_dtype == 2),
              "unet_reconstruct_init: marker_dtype and under_dtype must be 0 (int64) or 2 (int32)");
    ARG_CHECK(!mask || (mask_dtype >= 0 && mask_dtype <= 3),
              "unet_reconstruct_init: mask_dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    SH_SIZE_CHECK("unet_reconstruct_init");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W, plane = sh_plane(B, H, W);
    char *base = (char *)scratch;
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(rc_init_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, marker, marker_dtype, under, under_dtype, mask,
                       mask_dtype, npx, (int *)base, (int *)(base + 2 * plane), (int *)(base + 3 * plane), (unsigned long long *)status_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_reconstruct_sweeps_conn(int B, int H, int W, int connectivity, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                                 void *stream)
{
    ARG_CHECK(changed_out_u32 && scratch && B > 0 && H > 0 && W > 0 && n_launches > 0 && first_slot >= 0, "unet_reconstruct_sweeps: bad argument");
    SW_CONN_CHECK("unet_reconstruct_sweeps_conn");
    SH_SIZE_CHECK("unet_reconstruct_sweeps");
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sh_plane(B, H, W);
    const int *under = (const int *)((char *)scratch + 2 * bytes);
    const auto kernel = connectivity == 8 ? rc_sweep_kernel<8> : rc_sweep_kernel<4>;
    return sweep_launches(scratch, (char *)scratch + bytes, sizeof(int), B, H, W, n_launches, changed_out_u32, first_slot, st,
                          [&](dim3 grid, void *src, void *dst, unsigned *changed) {
                              hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const int *)src, under, (int *)dst, H, W, changed);
                          });
}

int unet_reconstruct_sweeps(int B, int H, int W, int n_launches, void *changed_out_u32, int first_slot, void *scratch, void *stream)
{
    return unet_reconstruct_sweeps_conn(B, H, W, 4, n_launches, changed_out_u32, first_slot, scratch, stream);
}

int unet_reconstruct_finish(int B, int H, int W, void *out_i32, void *raised_u32, void *scratch, void *stream)
{
    ARG_CHECK(out_i32 && raised_u32 && scratch && B > 0 && H > 0 && W > 0, "unet_reconstruct_finish: bad argument");
    SH_SIZE_CHECK("unet_reconstruct_finish");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(raised_u32, 0, (size_t)B * sizeof(unsigned), st));
    hipLaunchKernelGGL(rc_finish_kernel, dim3(grid_for(npx, 1024, 512), B), dim3(256), 0, st, (const int *)scratch,
                       (const int *)((char *)scratch + 3 * sh_plane(B, H, W)), npx, (int *)out_i32, (unsigned *)raised_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_shape_heights(const void *d2_i32, int B, int H, int W, int hq, void *q_i32, void *lifted_i32, void *stream)
{
    ARG_CHECK(d2_i32 && q_i32 && B > 0 && H > 0 && W > 0, "unet_shape_heights: bad argument");
    ARG_CHECK(hq >= 0 && hq <= 1 << 28, "unet_shape_heights: hq must be in [0, 2^28]");
    SH_SIZE_CHECK("unet_shape_heights");
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(sh_heights_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, (hipStream_t)stream, (const int *)d2_i32, n, hq, (int *)q_i32,
                       (int *)lifted_i32);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_shape_lower(const void *in_i32, int B, int H, int W, int c, void *out_i32, void *stream)
{
    ARG_CHECK(in_i32 && out_i32 && B > 0 && H > 0 && W > 0 && c >= 0, "unet_shape_lower: bad argument");
    SH_SIZE_CHECK("unet_shape_lower");
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(sh_lower_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, (hipStream_t)stream, (const int *)in_i32, n, c, (int *)out_i32);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_shape_maxima(const void *r1_i32, const void *r2_i32, int B, int H, int W, int floor_q, void *out_f32, void *stream)
{
    ARG_CHECK(r1_i32 && r2_i32 && out_f32 && B > 0 && H > 0 && W > 0, "unet_shape_maxima: bad argument");
    SH_SIZE_CHECK("unet_shape_maxima");
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(sh_maxima_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, (hipStream_t)stream, (const int *)r1_i32, (const int *)r2_i32, n,
                       floor_q, (float *)out_f32);
    HIP_TRY(hipGetLastError());
    return 0;
}
