// elastic.hip — the paper's elastic deformation (Ronneberger et al. §3.1): random displacements on a coarse
// G x G grid, brought to every pixel with Keys' cubic convolution, and the bilinear warp with them, in one launch.  No
// displacement field is stored: a workgroup keeps the sample's 2 G^2 nodes and the per-axis taps of its tile in LDS.
//   unet_elastic_grid        : P planes of B samples warped with the sample's grid (float out)
//   unet_elastic_grid_sample : image + mask of a training sample: integer rounding, the mask only inside the label window and
//                              thresholded at 127, per-sample min / max of the image
//   unet_normalise01         : (x - min) / (max - min) in place
// Displacement, coordinate and bilinear combination are fp64 (in fp32 some 1e-3 of the pixels of a 700^2 sample
// land on the other side of floor(v + 0.5)); the kernels are gathers bound by memory latency, the fp64 FMAs do not show.
#include "common.hpp"
#include "elem.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {

constexpr int EG_MAX = UNET_ELASTIC_MAX_GRID;
constexpr int EG_TX = 64, EG_TY = 16, EG_ROWS = EG_TY / 4;       // tile of a 256-thread workgroup: 64 x 4 threads, 4 rows each

// Keys' cubic convolution kernel of parameter a at distance d >= 0
__device__ __forceinline__ double keys_weight(double d, double a)
{
    if (d <= 1.0) return ((a + 2.0) * d - (a + 3.0)) * d * d + 1.0;
    if (d < 2.0) return ((a * d - 5.0 * a) * d + 8.0 * a) * d - 4.0 * a;
    return 0.0;
}

// the four taps of pixel p of an axis of n pixels on a corner-aligned grid of G nodes: node indices (clamped) and weights
__device__ __forceinline__ void axis_taps(int p, int n, int G, double a, int *idx, double *w)
{
    const double u = (double)p * (double)(G - 1) / (double)(n - 1);
    int i0 = (int)floor(u);
    if (i0 > G - 1) i0 = G - 1;
    for (int k = 0; k < 4; ++k) {
        const int node = i0 - 1 + k;
        w[k] = keys_weight(fabs(u - (double)node), a);
        idx[k] = node < 0 ? 0 : (node > G - 1 ? G - 1 : node);
    }
}

// What a workgroup keeps in LDS: the nodes of its sample and the taps of its tile's columns and rows
struct EgShared {
    double g[2 * EG_MAX * EG_MAX];
    double wx[EG_TX][4], wy[EG_TY][4];
    int ix[EG_TX][4], iy[EG_TY][4];
};

// prologue of a tile at (y0, x0) of sample b: every thread calls it; ends with a barrier
__device__ __forceinline__ void eg_prologue(EgShared &s, const double *__restrict__ grid, int b, int G, double a, int H, int W, int y0, int x0)
{
    const int t = threadIdx.x;
    for (int i = t; i < 2 * G * G; i += 256) s.g[i] = grid[(size_t)b * 2 * G * G + i];
    if (t < EG_TX) {
        const int x = x0 + t < W ? x0 + t : W - 1;
        axis_taps(x, W, G, a, s.ix[t], s.wx[t]);
    } else if (t < EG_TX + EG_TY) {
        const int r = t - EG_TX;
        const int y = y0 + r < H ? y0 + r : H - 1;
        axis_taps(y, H, G, a, s.iy[r], s.wy[r]);
    }
    __syncthreads();
}

struct ColTaps { int i[4]; double w[4]; };

// displacement of one plane of the grid at (row r of the tile, the thread's column).  Written around the node at i0 (tap 1,
// never clamped away): d = g1 + sum w (g - g1), the same sum as sum w g because the weights add up to 1, and exact for a
// constant grid, so a grid of whole pixels shifts by whole pixels.
__device__ __forceinline__ double eg_displacement(const double *gp, int G, const int *iy, const double *wy, const ColTaps &c)
{
    const double base = gp[iy[1] * G + c.i[1]];
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double *row = gp + iy[k] * G;
        double r = 0.0;
#pragma unroll
        for (int l = 0; l < 4; ++l) r += c.w[l] * (row[c.i[l]] - base);
        d += wy[k] * r;
    }
    return base + d;
}

// scipy.ndimage.map_coordinates(order=1, mode='constant', cval=0) at (cy, cx): where to read and with what weights
struct Bilin { bool inside; int y0, x0; double fy, fx; };
__device__ __forceinline__ Bilin bilin_at(double cy, double cx, int H, int W)
{
    Bilin s;
    s.inside = cy >= 0.0 && cy <= (double)(H - 1) && cx >= 0.0 && cx <= (double)(W - 1);      // false for NaN too
    s.y0 = s.x0 = 0; s.fy = s.fx = 0.0;
    if (s.inside) {
        s.y0 = (int)floor(cy); s.x0 = (int)floor(cx);
        if (s.y0 > H - 2) s.y0 = H - 2;                     // H, W >= 2: rows y0, y0 + 1 and columns x0, x0 + 1 exist
        if (s.x0 > W - 2) s.x0 = W - 2;
        s.fy = cy - (double)s.y0; s.fx = cx - (double)s.x0;
    }
    return s;
}
__device__ __forceinline__ double bilin_read(const float *__restrict__ img, int W, const Bilin &s)
{
    if (!s.inside) return 0.0;
    const float *p = img + (size_t)s.y0 * W + s.x0;
    const double v00 = p[0], v01 = p[1], v10 = p[W], v11 = p[W + 1];
    return (1.0 - s.fy) * ((1.0 - s.fx) * v00 + s.fx * v01) + s.fy * ((1.0 - s.fx) * v10 + s.fx * v11);
}

__device__ __forceinline__ double round_levels(double v, double levels)
{
    if (levels <= 0.0) return v;
    v = floor(v + 0.5);
    return v < 0.0 ? 0.0 : (v > levels ? levels : v);
}

// planes [P,B,H,W] -> out [P,B,H,W]; grid (tiles of W, tiles of H, B)
__global__ __launch_bounds__(256) void elastic_grid_kernel(const float *__restrict__ planes, float *__restrict__ out, const double *__restrict__ grid,
                                                           int P, int B, int H, int W, int G, double a)
{
    __shared__ EgShared s;
    const int b = blockIdx.z, x0 = blockIdx.x * EG_TX, y0 = blockIdx.y * EG_TY;
    eg_prologue(s, grid, b, G, a, H, W, y0, x0);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx;
    if (x >= W) return;
    ColTaps c;
#pragma unroll
    for (int l = 0; l < 4; ++l) { c.i[l] = s.ix[tx][l]; c.w[l] = s.wx[tx][l]; }
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int j = 0; j < EG_ROWS; ++j) {
        const int r = ty + 4 * j, y = y0 + r;
        if (y >= H) break;
        const double cy = (double)y + eg_displacement(s.g, G, s.iy[r], s.wy[r], c);
        const double cx = (double)x + eg_displacement(s.g + G * G, G, s.iy[r], s.wy[r], c);
        const Bilin at = bilin_at(cy, cx, H, W);
        for (int p = 0; p < P; ++p) {
            const size_t base = ((size_t)p * B + b) * plane;
            out[base + (size_t)y * W + x] = (float)bilin_read(planes + base, W, at);
        }
    }
}

// float min / max as integer atomics: non-negative floats order like their bits as signed integers, negative ones the other way
// round as unsigned integers (which also places them above every non-negative one).  -0 is stored as +0; a NaN is left out.
__device__ __forceinline__ void atomic_min_f32(float *addr, float v)
{
    v += 0.f;
    if (v >= 0.f) atomicMin((int *)addr, __float_as_int(v));
    else if (v < 0.f) atomicMax((unsigned *)addr, __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float *addr, float v)
{
    v += 0.f;
    if (v >= 0.f) atomicMax((int *)addr, __float_as_int(v));
    else if (v < 0.f) atomicMin((unsigned *)addr, __float_as_uint(v));
}

__global__ void minmax_init_kernel(float *__restrict__ minmax, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) minmax[i] = (i & 1) ? -INFINITY : INFINITY;
}

// img, mask [B,S,S] -> out_img [B,S,S] (rounded), out_gt [B,crop,crop] = (rounded warped mask > 127) for the window
// [pad, pad + crop)^2, minmax[b] = {min, max} of out_img[b] (initialised by minmax_init_kernel); grid (tiles, tiles, B)
__global__ __launch_bounds__(256) void elastic_sample_kernel(const float *__restrict__ img, const float *__restrict__ mask, const double *__restrict__ grid,
                                                             int S, int G, double a, double levels, int pad, int crop,
                                                             float *__restrict__ out_img, long long *__restrict__ out_gt, float *__restrict__ minmax)
{
    __shared__ EgShared s;
    const int b = blockIdx.z, x0 = blockIdx.x * EG_TX, y0 = blockIdx.y * EG_TY;
    eg_prologue(s, grid, b, G, a, S, S, y0, x0);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx;
    float lo = INFINITY, hi = -INFINITY;
    if (x < S) {
        ColTaps c;
#pragma unroll
        for (int l = 0; l < 4; ++l) { c.i[l] = s.ix[tx][l]; c.w[l] = s.wx[tx][l]; }
        const size_t base = (size_t)b * S * S;
        const bool xin = x >= pad && x < pad + crop;
#pragma unroll
        for (int j = 0; j < EG_ROWS; ++j) {
            const int r = ty + 4 * j, y = y0 + r;
            if (y >= S) break;
            const double cy = (double)y + eg_displacement(s.g, G, s.iy[r], s.wy[r], c);
            const double cx = (double)x + eg_displacement(s.g + G * G, G, s.iy[r], s.wy[r], c);
            const Bilin at = bilin_at(cy, cx, S, S);
            const float v = (float)round_levels(bilin_read(img + base, S, at), levels);
            out_img[base + (size_t)y * S + x] = v;
            lo = fminf(lo, v); hi = fmaxf(hi, v);
            if (xin && y >= pad && y < pad + crop) {
                const double m = round_levels(bilin_read(mask + base, S, at), levels);
                out_gt[((size_t)b * crop + (y - pad)) * crop + (x - pad)] = m > 127.0 ? 1 : 0;
            }
        }
    }
    const MinMax m = block_minmax<4>(lo, hi);
    if (threadIdx.x == 0) {
        atomic_min_f32(minmax + 2 * b, m.lo);
        atomic_max_f32(minmax + 2 * b + 1, m.hi);
    }
}

// x [B][n] in place; grid (chunks of n, B)
__global__ __launch_bounds__(256) void normalise01_kernel(float *__restrict__ x, size_t n, const float *__restrict__ minmax)
{
    const int b = blockIdx.y;
    const float lo = minmax[2 * b], hi = minmax[2 * b + 1];
    const float range = hi - lo;
    float *p = x + (size_t)b * n;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) p[e] = (p[e] - lo) / range;
}

static bool eg_shape_ok(int B, int H, int W, int G, double a, const char *who)
{
    if (B < 1 || B > 65535) { set_error("%s: B = %d, need 1 <= B <= 65535", who, B); return false; }
    if (H < 2 || W < 2) { set_error("%s: a sample of %d x %d, need H, W >= 2 (the grid is corner-aligned)", who, H, W); return false; }
    if (G < 2 || G > EG_MAX) { set_error("%s: a grid of %d x %d nodes, need 2 <= G <= %d", who, G, G, EG_MAX); return false; }
    if (!(a == a) || std::isinf(a)) { set_error("%s: the cubic parameter a is not finite", who); return false; }
    if (cdiv(H, EG_TY) > 65535) { set_error("%s: H = %d is more than the launch holds", who, H); return false; }
    return true;
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_elastic_grid(const void *planes, int P, int B, int H, int W, const void *grid_f64, int G, double a, void *out, void *stream)
{
    ARG_CHECK(planes && grid_f64 && out, "unet_elastic_grid: null argument");
    ARG_CHECK(P >= 1, "unet_elastic_grid: P = %d, need at least one plane", P);
    if (!eg_shape_ok(B, H, W, G, a, "unet_elastic_grid")) return -2;
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)P * B * H * W;
    ProfScope ps("N1.elastic_grid");
    return profiled(PK_ELEMWISE, "elastic_grid", st, 0.0, 0.0, 8.0 * px, [&] {
        hipLaunchKernelGGL(elastic_grid_kernel, dim3(cdiv(W, EG_TX), cdiv(H, EG_TY), B), dim3(256), 0, st, (const float *)planes, (float *)out,
                           (const double *)grid_f64, P, B, H, W, G, a);
    });
}

int unet_elastic_grid_sample(const void *img, const void *mask, int B, int S, const void *grid_f64, int G, double a, int levels,
                             int pad, int crop, void *out_img, void *out_gt_i64, void *minmax, void *stream)
{
    ARG_CHECK(img && mask && grid_f64 && out_img && out_gt_i64 && minmax, "unet_elastic_grid_sample: null argument");
    if (!eg_shape_ok(B, S, S, G, a, "unet_elastic_grid_sample")) return -2;
    ARG_CHECK(levels == 0 || levels == 255 || levels == 65535, "unet_elastic_grid_sample: levels must be 0 (float), 255 or 65535");
    ARG_CHECK(pad >= 0 && crop >= 1 && (long)pad + crop <= S, "unet_elastic_grid_sample: the window [%d, %d + %d) does not lie in a sample of %d (pad + crop > S)",
              pad, pad, crop, S);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)B * S * S, win = (double)B * crop * crop;
    ProfScope ps("N1.elastic_grid");
    return profiled(PK_ELEMWISE, "elastic_grid_sample", st, 0.0, 0.0, 8.0 * px + 12.0 * win, [&] {
        hipLaunchKernelGGL(minmax_init_kernel, dim3(cdiv(2 * B, 256)), dim3(256), 0, st, (float *)minmax, B);
        hipLaunchKernelGGL(elastic_sample_kernel, dim3(cdiv(S, EG_TX), cdiv(S, EG_TY), B), dim3(256), 0, st, (const float *)img, (const float *)mask,
                           (const double *)grid_f64, S, G, a, (double)levels, pad, crop, (float *)out_img, (long long *)out_gt_i64, (float *)minmax);
    });
}

int unet_normalise01(void *x, int B, size_t n, const void *minmax, void *stream)
{
    ARG_CHECK(x && minmax, "unet_normalise01: null argument");
    ARG_CHECK(B >= 1 && B <= 65535 && n >= 1, "unet_normalise01: bad shape (1 <= B <= 65535, n >= 1)");
    hipLaunchKernelGGL(normalise01_kernel, dim3(grid_for(n, 256, 4096), B), dim3(256), 0, (hipStream_t)stream, (float *)x, n, (const float *)minmax);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
