// tile.hip — overlap-tile segmentation of images of any size (Ronneberger et al. 2015, Fig. 2), both HBM-bound:
//   gather : tiles [nt,1,S,S] of a [B,H,W] image batch, numpy 'reflect' outside the image, optional (x-min)/(max-min)
//   stitch : logits [nt,2,So,So] of those tiles -> argmax mask int64 [B,H,W] (+ foreground probability fp32); stitch_k: [nt,K,So,So]
//            -> the K-way argmax (+ the softmax of all K classes)
//   gather_view / stitch_view : the same two for one of the 8 dihedral views of the image (tester.apply_view), without the view
//            being materialised; stitch_view stores, adds and finally averages the views' probabilities in the image's frame
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

// ---- dihedral views (tester.apply_view): code v, t = v & 1 (transpose), fy = (v >> 1) & 1, fx = (v >> 2) & 1.  View pixel (y, x)
// of the (Hv, Wv) = t ? (W, H) : (H, W) view is image pixel t ? (x', y') : (y', x') with y' = fy ? Hv-1-y : y, x' = fx ? Wv-1-x : x.
// The tile grid, the reflection and the tile index are those of the view; H, W stay the image's.

constexpr int VIEW_BLOCK = 32;                     // transposed views move 32 x 32 blocks through LDS rows of 33 floats

// t = 0: tile_gather_kernel's lanes with the flips folded into the row and column index
template <bool VEC>
__global__ __launch_bounds__(256) void tile_gather_view_kernel(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax,
                                                               int S, int fy, int fx, int oy0, int ox0, int ny, int nx, long long t0,
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
        int row = tile_reflect(oy0 + i * So - TILE_MARGIN + Y, H);
        if (fy) row = H - 1 - row;
        const int c0 = ox0 + j * So - TILE_MARGIN + 4 * xq;
        const float *src = img + (b * H + row) * (size_t)W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = tile_reflect(c0 + k, W);
            v[k] = src[fx ? W - 1 - c : c];
        }
        if (minmax) {
            const float lo = minmax[2 * b], hi = minmax[2 * b + 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (v[k] - lo) / (hi - lo);        // true division, as tile_gather_kernel
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

// t = 1: tile row Y runs along the image's columns.  One workgroup moves 32 x 32 blocks of a tile: the loads run lanes along
// Y (unit stride in the image, apart from the mirror bands), the stores along X (unit stride in the tile); the LDS tile is
// written [X][Y] and read [X][Y] with the lane on X, 33 floats apart, so neither side has a bank conflict
__global__ __launch_bounds__(256) void tile_gather_view_t_kernel(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax,
                                                                 int S, int fy, int fx, int oy0, int ox0, int ny, int nx, long long t0,
                                                                 float *__restrict__ out, size_t tasks)
{
    __shared__ float lds[VIEW_BLOCK][VIEW_BLOCK + 1];
    const int So = S - 2 * TILE_MARGIN, nbs = (S + VIEW_BLOCK - 1) / VIEW_BLOCK;
    const int Hv = W, Wv = H;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (size_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const int bx = (int)(task % nbs);
        const size_t r = task / nbs;
        const int by = (int)(r % nbs);
        const size_t tl = r / nbs;
        const long long t = t0 + (long long)tl;
        const int j = (int)(t % nx);
        const long long ti = t / nx;
        const int i = (int)(ti % ny);
        const size_t b = (size_t)(ti / ny);
        float lo = 0.f, hi = 1.f;
        if (minmax) { lo = minmax[2 * b]; hi = minmax[2 * b + 1]; }
        const int Y = by * VIEW_BLOCK + tx;
        int col = tile_reflect(oy0 + i * So - TILE_MARGIN + Y, Hv);             // view row -> image column
        if (fy) col = Hv - 1 - col;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int Xl = ty + 8 * e, X = bx * VIEW_BLOCK + Xl;
            if (X < S && Y < S) {
                int row = tile_reflect(ox0 + j * So - TILE_MARGIN + X, Wv);     // view column -> image row
                if (fx) row = Wv - 1 - row;
                float v = img[(b * H + row) * (size_t)W + col];
                if (minmax) v = (v - lo) / (hi - lo);
                lds[Xl][tx] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int Yl = ty + 8 * e, Yo = by * VIEW_BLOCK + Yl, X = bx * VIEW_BLOCK + tx;
            if (X < S && Yo < S) out[(tl * S + Yo) * (size_t)S + X] = lds[tx][Yl];
        }
        __syncthreads();                                                        // the next block overwrites the tile
    }
}

// one pixel's class probabilities, by the expressions of tile_stitch_kernel (BIN: K = 2, one plane, class 1) and of
// tile_stitch_k_kernel (the softmax of all K classes)
template <int KP, bool BIN>
__device__ __forceinline__ void view_probs(const float (&l)[KP], int K, float (&p)[KP])
{
    if (BIN) {
        p[0] = 1.f / (1.f + expf(l[0] - l[1]));
        return;
    }
    float m = l[0];
#pragma unroll
    for (int k = 1; k < KP; ++k) if (k < K && l[k] > m) m = l[k];
    float ex[KP], se = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) { ex[k] = k < K ? expf(l[k] - m) : 0.f; se += ex[k]; }
#pragma unroll
    for (int k = 0; k < KP; ++k) p[k] = ex[k] / se;
}

// phase bit 0 (FIRST): the probability is stored, else added to what is there; bit 1 (LAST): the sum is then divided by the
// number of views and the mask written: BIN prob > 0.5, else the argmax of the sums, ties -> the lowest class
enum { VIEW_FIRST = 1, VIEW_LAST = 2 };

// t = 0: tile_stitch_kernel's lanes (4 consecutive columns of one tile output row), flips folded into the image index
template <int KP, bool BIN, bool VEC>
__global__ __launch_bounds__(256) void tile_stitch_view_kernel(const float *__restrict__ logits, int So, int K, int fy, int fx, int oy0, int ox0,
                                                               int ny, int nx, long long t0, int H, int W, int phase, float nf,
                                                               float *__restrict__ prob, long long *__restrict__ mask, size_t quads)
{
    const int S4 = So >> 2, np = BIN ? 1 : K;
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
        const int vy = oy0 + i * So + y;
        if ((unsigned)vy >= (unsigned)H) continue;
        const int row = fy ? H - 1 - vy : vy;
        const int c0 = ox0 + j * So + 4 * xq;
        const float *p0 = logits + (size_t)K * tl * plane + (size_t)y * So + 4 * xq;
        float l[KP][4];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k < K) {
                if (VEC) {
                    const f32x4 a = *(const f32x4 *)(p0 + k * plane);
#pragma unroll
                    for (int c = 0; c < 4; ++c) l[k][c] = a[c];
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) l[k][c] = p0[k * plane + c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) l[k][c] = 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int vx = c0 + c;
            if ((unsigned)vx >= (unsigned)W) continue;
            const size_t o = (size_t)row * W + (fx ? W - 1 - vx : vx);
            float lc[KP], p[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) lc[k] = l[k][c];
            view_probs<KP, BIN>(lc, K, p);
            float best = 0.f;
            int am = 0;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (k >= np) continue;
                float *a = prob + (b * np + k) * iplane + o;
                float s = p[k];
                if (!(phase & VIEW_FIRST)) s += *a;
                if (phase & VIEW_LAST) {
                    if (!BIN && (k == 0 || s > best)) { best = s; am = k; }
                    s = s / nf;
                    if (BIN) am = s > 0.5f ? 1 : 0;
                }
                *a = s;
            }
            if (phase & VIEW_LAST) mask[b * iplane + o] = am;
        }
    }
}

// t = 1: tile output row y runs along the image's columns.  32 x 32 blocks: each lane computes the probabilities of 4 pixels
// with lanes along x (unit-stride logit loads), then one class plane at a time goes through LDS ([y][x], rows of 33 floats, two
// buffers so that one barrier per class is enough) and is accumulated with lanes along y: unit stride on prob and mask
template <int KP, bool BIN>
__global__ __launch_bounds__(256) void tile_stitch_view_t_kernel(const float *__restrict__ logits, int So, int K, int fy, int fx, int oy0, int ox0,
                                                                 int ny, int nx, long long t0, int H, int W, int phase, float nf,
                                                                 float *__restrict__ prob, long long *__restrict__ mask, size_t tasks)
{
    __shared__ float lds[2][VIEW_BLOCK][VIEW_BLOCK + 1];
    const int nbs = (So + VIEW_BLOCK - 1) / VIEW_BLOCK, np = BIN ? 1 : K;
    const int Hv = W, Wv = H;
    const size_t plane = (size_t)So * So, iplane = (size_t)H * W;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (size_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const int bx = (int)(task % nbs);
        const size_t r = task / nbs;
        const int by = (int)(r % nbs);
        const size_t tl = r / nbs;
        const long long t = t0 + (long long)tl;
        const int j = (int)(t % nx);
        const long long ti = t / nx;
        const int i = (int)(ti % ny);
        const size_t b = (size_t)(ti / ny);
        float p[4][KP];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int y = by * VIEW_BLOCK + ty + 8 * e, x = bx * VIEW_BLOCK + tx;
#pragma unroll
            for (int k = 0; k < KP; ++k) p[e][k] = 0.f;
            if (y < So && x < So) {
                const float *p0 = logits + (size_t)K * tl * plane + (size_t)y * So + x;
                float l[KP];
#pragma unroll
                for (int k = 0; k < KP; ++k) l[k] = k < K ? p0[k * plane] : 0.f;
                view_probs<KP, BIN>(l, K, p[e]);
            }
        }
        // the pixels this lane accumulates: block column ty + 8e, block row tx
        size_t o[4];
        bool ok[4];
        const int y = by * VIEW_BLOCK + tx, vy = oy0 + i * So + y;
        const int col = fy ? Hv - 1 - vy : vy;                                  // view row -> image column
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = bx * VIEW_BLOCK + ty + 8 * e, vx = ox0 + j * So + x;
            ok[e] = y < So && x < So && (unsigned)vy < (unsigned)Hv && (unsigned)vx < (unsigned)Wv;
            const int row = fx ? Wv - 1 - vx : vx;                              // view column -> image row
            o[e] = ok[e] ? (size_t)row * W + col : 0;
        }
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int am[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (c < np) {                                                       // np is the same for the whole grid
                float (*buf)[VIEW_BLOCK + 1] = lds[c & 1];
#pragma unroll
                for (int e = 0; e < 4; ++e) buf[ty + 8 * e][tx] = p[e][c];
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!ok[e]) continue;
                    float *a = prob + (b * np + c) * iplane + o[e];
                    float s = buf[tx][ty + 8 * e];
                    if (!(phase & VIEW_FIRST)) s += *a;
                    if (phase & VIEW_LAST) {
                        if (!BIN && (c == 0 || s > best[e])) { best[e] = s; am[e] = c; }
                        s = s / nf;
                        if (BIN) am[e] = s > 0.5f ? 1 : 0;
                    }
                    *a = s;
                }
            }
        }
        if (phase & VIEW_LAST) {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (ok[e]) mask[b * iplane + o[e]] = am[e];
        }
        __syncthreads();                                                        // the next block's first plane reuses lds[0]
    }
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

int unet_tile_gather_view(const void *img, int B, int H, int W, const void *minmax, int S, int view, int oy0, int ox0, int ny, int nx,
                          long t0, int nt, void *tiles_out, void *stream)
{
    ARG_CHECK(img && tiles_out, "unet_tile_gather_view: null argument");
    ARG_CHECK(view >= 0 && view <= 7, "unet_tile_gather_view: view %d is not a code 0..7", view);
    ARG_CHECK(S > 2 * TILE_MARGIN, "unet_tile_gather_view: tile size %d has no output (S must exceed 184)", S);
    ARG_CHECK(((uintptr_t)img & 3) == 0 && ((uintptr_t)tiles_out & 3) == 0 && ((uintptr_t)minmax & 3) == 0,
              "unet_tile_gather_view: pointers must be 4-byte aligned");
    const int tr = view & 1, fy = (view >> 1) & 1, fx = (view >> 2) & 1;
    int rc = check_tile_grid("unet_tile_gather_view", B, tr ? W : H, tr ? H : W, S - 2 * TILE_MARGIN, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("N2.tile_gather");
    const double bytes = 8.0 * nt * S * S;
    if (tr) {
        const size_t nbs = (S + VIEW_BLOCK - 1) / VIEW_BLOCK, tasks = (size_t)nt * nbs * nbs;
        return profiled(PK_ELEMWISE, "tile_gather_view_t", st, 0.0, 0.0, bytes, [&] {
            hipLaunchKernelGGL(tile_gather_view_t_kernel, dim3(grid_for(tasks, 1, 16384)), dim3(256), 0, st, (const float *)img, H, W,
                               (const float *)minmax, S, fy, fx, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, tasks);
        });
    }
    const size_t quads = (size_t)nt * S * (S / 4);
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_gather_view", st, 0.0, 0.0, bytes, [&] {
        if (((uintptr_t)tiles_out & 15) == 0)
            hipLaunchKernelGGL(tile_gather_view_kernel<true>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W, (const float *)minmax,
                               S, fy, fx, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
        else
            hipLaunchKernelGGL(tile_gather_view_kernel<false>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W, (const float *)minmax,
                               S, fy, fx, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
    });
}

int unet_tile_stitch_view(const void *logits, int So, int K, int view, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W,
                          int phase, int n_views, void *prob_f32, void *mask_i64, void *stream)
{
    ARG_CHECK(logits && prob_f32, "unet_tile_stitch_view: null argument");
    ARG_CHECK(view >= 0 && view <= 7, "unet_tile_stitch_view: view %d is not a code 0..7", view);
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_tile_stitch_view: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK(phase >= 0 && phase <= 3, "unet_tile_stitch_view: phase %d is not a combination of FIRST (1) and LAST (2)", phase);
    ARG_CHECK(n_views >= 1, "unet_tile_stitch_view: n_views=%d must be at least 1", n_views);
    ARG_CHECK(mask_i64 || !(phase & VIEW_LAST), "unet_tile_stitch_view: the LAST phase writes the mask, which is null");
    ARG_CHECK(((uintptr_t)logits & 3) == 0 && ((uintptr_t)prob_f32 & 3) == 0 && ((uintptr_t)mask_i64 & 7) == 0,
              "unet_tile_stitch_view: logits and prob must be 4-byte aligned, mask 8-byte aligned");
    ARG_CHECK(K == 2 || ((uintptr_t)logits & 15) == 0, "unet_tile_stitch_view: logits of K > 2 classes must be 16-byte aligned");
    const int tr = view & 1, fy = (view >> 1) & 1, fx = (view >> 2) & 1;
    int rc = check_tile_grid("unet_tile_stitch_view", B, tr ? W : H, tr ? H : W, So, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float nf = (float)n_views;
    const int np = K == 2 ? 1 : K;
    ProfScope ps("N2.tile_stitch");
    const double bytes = (4.0 * K + (phase & VIEW_FIRST ? 4.0 : 8.0) * np + (phase & VIEW_LAST ? 8.0 : 0.0)) * nt * So * So;
    if (tr) {
        const size_t nbs = (So + VIEW_BLOCK - 1) / VIEW_BLOCK, tasks = (size_t)nt * nbs * nbs;
        const int grid = grid_for(tasks, 1, 16384);
        return profiled(PK_ELEMWISE, "tile_stitch_view_t", st, 0.0, 0.0, bytes, [&] {
            if (K == 2)
                hipLaunchKernelGGL((tile_stitch_view_t_kernel<2, true>), dim3(grid), dim3(256), 0, st, (const float *)logits, So, K, fy, fx, oy0,
                                   ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32, (long long *)mask_i64, tasks);
            else
                CLASS_DISPATCH(K, hipLaunchKernelGGL((tile_stitch_view_t_kernel<KP_, false>), dim3(grid), dim3(256), 0, st, (const float *)logits,
                                                     So, K, fy, fx, oy0, ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32,
                                                     (long long *)mask_i64, tasks));
        });
    }
    const size_t quads = (size_t)nt * So * (So / 4);
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_stitch_view", st, 0.0, 0.0, bytes, [&] {
        if (K == 2 && ((uintptr_t)logits & 15) == 0)
            hipLaunchKernelGGL((tile_stitch_view_kernel<2, true, true>), dim3(grid), dim3(256), 0, st, (const float *)logits, So, K, fy, fx, oy0,
                               ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32, (long long *)mask_i64, quads);
        else if (K == 2)
            hipLaunchKernelGGL((tile_stitch_view_kernel<2, true, false>), dim3(grid), dim3(256), 0, st, (const float *)logits, So, K, fy, fx, oy0,
                               ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32, (long long *)mask_i64, quads);
        else
            CLASS_DISPATCH(K, hipLaunchKernelGGL((tile_stitch_view_kernel<KP_, false, true>), dim3(grid), dim3(256), 0, st, (const float *)logits,
                                                 So, K, fy, fx, oy0, ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32,
                                                 (long long *)mask_i64, quads));
    });
}

}  // extern "C"
