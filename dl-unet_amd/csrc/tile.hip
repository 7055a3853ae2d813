// tile.hip — overlap-tile segmentation of images of any size (Ronneberger et al. 2015, Fig. 2), both HBM-bound:
//   gather : tiles [nt,1,S,S] of a [B,H,W] image batch, numpy 'reflect' outside the image, optional (x-min)/(max-min)
//   stitch : logits [nt,2,So,So] of those tiles -> argmax mask int64 [B,H,W] (+ foreground probability fp32); stitch_k: [nt,K,So,So]
//            -> the K-way argmax (+ the softmax of all K classes)
// Geometry (tester.tile_grid): So = S - 184, margin m = 92; the ny x nx output grid is centred on the image, top-left corner
// (oy0, ox0) <= 0.  Tile t = (b*ny + i)*nx + j reads rows [oy0 + i*So - m, +S), columns [ox0 + j*So - m, +S) and covers
// output rows [oy0 + i*So, +So), columns [ox0 + j*So, +So), clipped to the image; the output rectangles partition it.
#include "common.hpp"
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

constexpr int TILE_MARGIN = 92;

// numpy.pad(mode='reflect'): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; repeats with period 2(n-1) for pads wider than n (n >= 2)
__device__ __forceinline__ int tile_reflect(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// one lane = 4 consecutive columns of one tile row (S % 4 == 0): scalar reads (the mirror bands run backwards and the
// window's column origin has any alignment), one 16-byte store when `out` is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax,
                                                          int S, int oy0, int ox0, int ny, int nx, long long t0,
                                                          float *__restrict__ out, size_t quads)
{
    const int So = S - 2 * TILE_MARGIN, S4 = S >> 2;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(q % S4);
        const size_t r = q / S4;
        const int Y = (int)(r % S);
        const long long t = t0 + (long long)(r / S);
        const int j = (int)(t % nx);
        const long long ti = t / nx;
        const int i = (int)(ti % ny);
        const size_t b = (size_t)(ti / ny);
        const int row = tile_reflect(oy0 + i * So - TILE_MARGIN + Y, H);
        const int c0 = ox0 + j * So - TILE_MARGIN + 4 * xq;
        const float *src = img + (b * H + row) * (size_t)W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[tile_reflect(c0 + k, W)];
        if (minmax) {
            const float lo = minmax[2 * b], hi = minmax[2 * b + 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (v[k] - lo) / (hi - lo);        // true division: torch's (x - min) / ptp in fp32
        }
        float *o = out + 4 * q;
        if (VEC) {
            f32x4 w = {v[0], v[1], v[2], v[3]};
            *(f32x4 *)o = w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = v[k];
        }
    }
}

// one lane = 4 consecutive columns of one tile's output row (So % 4 == 0); rows and columns outside the image are skipped,
// so every image pixel is written by exactly one lane of exactly one tile
template <bool VEC>
__global__ __launch_bounds__(256) void tile_stitch_kernel(const float *__restrict__ logits, int So, int oy0, int ox0, int ny, int nx,
                                                          long long t0, int H, int W, long long *__restrict__ mask,
                                                          float *__restrict__ prob, size_t quads)
{
    const int S4 = So >> 2;
    const size_t plane = (size_t)So * So;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(q % S4);
        const size_t r = q / S4;
        const int y = (int)(r % So);
        const size_t tl = r / So;
        const long long t = t0 + (long long)tl;
        const int j = (int)(t % nx);
        const long long ti = t / nx;
        const int i = (int)(ti % ny);
        const size_t b = (size_t)(ti / ny);
        const int row = oy0 + i * So + y;
        if ((unsigned)row >= (unsigned)H) continue;
        const int c0 = ox0 + j * So + 4 * xq;
        const float *p0 = logits + 2 * tl * plane + (size_t)y * So + 4 * xq, *p1 = p0 + plane;
        float l0[4], l1[4];
        if (VEC) {
            const f32x4 a = *(const f32x4 *)p0, c = *(const f32x4 *)p1;
#pragma unroll
            for (int k = 0; k < 4; ++k) { l0[k] = a[k]; l1[k] = c[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { l0[k] = p0[k]; l1[k] = p1[k]; }
        }
        const size_t o = (b * H + row) * (size_t)W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = c0 + k;
            if ((unsigned)col >= (unsigned)W) continue;
            mask[o + col] = l1[k] > l0[k] ? 1 : 0;                             // unet_argmax2's rule: ties -> class 0
            if (prob) prob[o + col] = 1.f / (1.f + expf(l0[k] - l1[k]));   // softmax of the two logits, class 1
        }
    }
}

// K classes (2 <= K <= KP): the same lanes as tile_stitch_kernel; argmax with ties -> the lowest class (torch.argmax), and
// optionally the softmax of all K classes, prob [B,K,H,W], as exp(l_k - max) / sum_j exp(l_j - max)
template <int KP>
__global__ __launch_bounds__(256) void tile_stitch_k_kernel(const float *__restrict__ logits, int So, int K, int oy0, int ox0, int ny, int nx,
                                                            long long t0, int B, int H, int W, long long *__restrict__ mask,
                                                            float *__restrict__ prob, size_t quads)
{
    const int S4 = So >> 2;
    const size_t plane = (size_t)So * So, iplane = (size_t)H * W;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(q % S4);
        const size_t r = q / S4;
        const int y = (int)(r % So);
        const size_t tl = r / So;
        const long long t = t0 + (long long)tl;
        const int j = (int)(t % nx);
        const long long ti = t / nx;
        const int i = (int)(ti % ny);
        const size_t b = (size_t)(ti / ny);
        const int row = oy0 + i * So + y;
        if ((unsigned)row >= (unsigned)H) continue;
        const int c0 = ox0 + j * So + 4 * xq;
        const float *p0 = logits + (size_t)K * tl * plane + (size_t)y * So + 4 * xq;
        float l[KP][4];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k < K) {
                const f32x4 a = *(const f32x4 *)(p0 + k * plane);       // So % 4 == 0 and 16-byte aligned logits (checked)
#pragma unroll
                for (int c = 0; c < 4; ++c) l[k][c] = a[c];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) l[k][c] = 0.f;
            }
        }
        const size_t o = (b * H + row) * (size_t)W;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = c0 + c;
            if ((unsigned)col >= (unsigned)W) continue;
            float m = l[0][c];
            int am = 0;
#pragma unroll
            for (int k = 1; k < KP; ++k) if (k < K && l[k][c] > m) { m = l[k][c]; am = k; }
            mask[o + col] = am;
            if (prob) {
                float ex[KP], se = 0.f;
#pragma unroll
                for (int k = 0; k < KP; ++k) { ex[k] = k < K ? expf(l[k][c] - m) : 0.f; se += ex[k]; }
#pragma unroll
                for (int k = 0; k < KP; ++k) if (k < K) prob[(b * K + k) * iplane + (size_t)row * W + col] = ex[k] / se;
            }
        }
    }
}

// checks shared by both entry points: the grid covers the image and is centred as tester.tile_grid makes it
static int check_tile_grid(const char *who, int B, int H, int W, int So, int oy0, int ox0, int ny, int nx, long long t0, int nt)
{
    ARG_CHECK(B > 0 && H >= 2 && W >= 2 && H < (1 << 30) && W < (1 << 30), "%s: bad image shape [%d,%d,%d] (H, W >= 2)", who, B, H, W);
    ARG_CHECK(So > 0 && So % 4 == 0, "%s: output tile size %d is not a positive multiple of 4", who, So);
    ARG_CHECK(ny > 0 && nx > 0 && (long long)ny * So >= H && (long long)(ny - 1) * So < H && (long long)nx * So >= W &&
              (long long)(nx - 1) * So < W, "%s: a %dx%d grid of %d-pixel tiles does not cover %dx%d exactly", who, ny, nx, So, H, W);
    ARG_CHECK(oy0 <= 0 && ox0 <= 0 && oy0 + (long long)ny * So >= H && ox0 + (long long)nx * So >= W,
              "%s: grid origin (%d,%d) does not cover the image", who, oy0, ox0);
    ARG_CHECK(nt > 0 && t0 >= 0 && t0 + nt <= (long long)B * ny * nx, "%s: tiles [%lld, %lld) outside [0, %lld)", who, t0, t0 + nt,
              (long long)B * ny * nx);
    return 0;
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_tile_gather(const void *img, int B, int H, int W, const void *minmax, int S, int oy0, int ox0, int ny, int nx, long t0, int nt,
                     void *tiles_out, void *stream)
{
    ARG_CHECK(img && tiles_out, "unet_tile_gather: null argument");
    ARG_CHECK(S > 2 * TILE_MARGIN, "unet_tile_gather: tile size %d has no output (S must exceed 184)", S);
    int rc = check_tile_grid("unet_tile_gather", B, H, W, S - 2 * TILE_MARGIN, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t quads = (size_t)nt * S * (S / 4);
    ProfScope ps("N2.tile_gather");
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_gather", st, 0.0, 0.0, 8.0 * quads * 4, [&] {
        if (((uintptr_t)tiles_out & 15) == 0)
            hipLaunchKernelGGL(tile_gather_kernel<true>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W, (const float *)minmax,
                               S, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
        else
            hipLaunchKernelGGL(tile_gather_kernel<false>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W, (const float *)minmax,
                               S, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
    });
}

int unet_tile_stitch(const void *logits, int So, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W, void *mask_i64,
                     void *prob_f32, void *stream)
{
    ARG_CHECK(logits && mask_i64, "unet_tile_stitch: null argument");
    int rc = check_tile_grid("unet_tile_stitch", B, H, W, So, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t quads = (size_t)nt * So * (So / 4);
    ProfScope ps("N2.tile_stitch");
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_stitch", st, 0.0, 0.0, (8.0 + 8.0 + (prob_f32 ? 4.0 : 0.0)) * quads * 4, [&] {
        if (((uintptr_t)logits & 15) == 0)
            hipLaunchKernelGGL(tile_stitch_kernel<true>, dim3(grid), dim3(256), 0, st, (const float *)logits, So, oy0, ox0, ny, nx,
                               (long long)t0, H, W, (long long *)mask_i64, (float *)prob_f32, quads);
        else
            hipLaunchKernelGGL(tile_stitch_kernel<false>, dim3(grid), dim3(256), 0, st, (const float *)logits, So, oy0, ox0, ny, nx,
                               (long long)t0, H, W, (long long *)mask_i64, (float *)prob_f32, quads);
    });
}

int unet_tile_stitch_k(const void *logits, int So, int K, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W,
                       void *mask_i64, void *prob_f32, void *stream)
{
    ARG_CHECK(logits && mask_i64, "unet_tile_stitch_k: null argument");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_tile_stitch_k: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK(((uintptr_t)logits & 15) == 0, "unet_tile_stitch_k: logits must be 16-byte aligned");
    int rc = check_tile_grid("unet_tile_stitch_k", B, H, W, So, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t quads = (size_t)nt * So * (So / 4);
    ProfScope ps("N2.tile_stitch");
    return profiled(PK_ELEMWISE, "tile_stitch_k", st, 0.0, 0.0, (4.0 * K + 8.0 + (prob_f32 ? 4.0 * K : 0.0)) * quads * 4, [&] {
        CLASS_DISPATCH(K, hipLaunchKernelGGL(tile_stitch_k_kernel<KP_>, dim3(grid_for(quads, 256, 16384)), dim3(256), 0, st, (const float *)logits,
                                             So, K, oy0, ox0, ny, nx, (long long)t0, B, H, W, (long long *)mask_i64, (float *)prob_f32, quads));
    });
}

}  // extern "C"
