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
#include "softmax.hpp"
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

// where a lane's task lies: column group x (of S4) of row y (of `rows`) of local tile tl, which is tile t0 + tl = (b*ny + i)*nx + j
struct TilePos { int x, y, j, i; size_t tl, b; };
__device__ __forceinline__ TilePos tile_quad(size_t q, int S4, int rows, long long t0, int ny, int nx)
{
    TilePos p;
    p.x = (int)(q % S4);
    const size_t r = q / S4;
    p.y = (int)(r % rows);
    p.tl = r / rows;
    const long long t = t0 + (long long)p.tl;
    p.j = (int)(t % nx);
    const long long ti = t / nx;
    p.i = (int)(ti % ny);
    p.b = (size_t)(ti / ny);
    return p;
}
// the same for the 32 x 32 blocks of the transposed views: block column x and block row y of the nbs x nbs blocks of a tile
__device__ __forceinline__ TilePos tile_block(size_t task, int nbs, long long t0, int ny, int nx) { return tile_quad(task, nbs, nbs, t0, ny, nx); }

// one lane = 4 consecutive columns of one tile row (S % 4 == 0): scalar reads (the mirror bands run backwards and the
// window's column origin has any alignment), one 16-byte store when `out` is 16-byte aligned.  VIEW: the untransposed dihedral
// views (below), the flips folded into the row and column index; H, W, the grid and the reflection are then the view's = the image's
template <bool VEC, bool VIEW>
__device__ __forceinline__ void tile_gather_body(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax, int S, int fy,
                                                 int fx, int oy0, int ox0, int ny, int nx, long long t0, float *__restrict__ out,
                                                 size_t quads, size_t first, size_t stride)
{
    const int So = S - 2 * TILE_MARGIN, S4 = S >> 2;
    for (size_t q = first; q < quads; q += stride) {
        const TilePos p = tile_quad(q, S4, S, t0, ny, nx);
        int row = tile_reflect(oy0 + p.i * So - TILE_MARGIN + p.y, H);
        if (VIEW && fy) row = H - 1 - row;
        const int c0 = ox0 + p.j * So - TILE_MARGIN + 4 * p.x;
        const float *src = img + (p.b * H + row) * (size_t)W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = tile_reflect(c0 + k, W);
            v[k] = src[VIEW && fx ? W - 1 - c : c];
        }
        if (minmax) {
            const float lo = minmax[2 * p.b], hi = minmax[2 * p.b + 1];
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
template <bool VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax,
                                                          int S, int oy0, int ox0, int ny, int nx, long long t0,
                                                          float *__restrict__ out, size_t quads)
{
    tile_gather_body<VEC, false>(img, H, W, minmax, S, 0, 0, oy0, ox0, ny, nx, t0, out, quads, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                                 (size_t)gridDim.x * blockDim.x);
}

// 4 consecutive columns of one row of one logit plane at p, or zeros for a plane above K (on = false): one 16-byte load when
// the logits are 16-byte aligned (So % 4 == 0).  The loop over the planes stays in the kernels: inside this function it changed
// their code
template <bool VEC>
__device__ __forceinline__ void load_logits4(const float *p, bool on, float (&l)[4])
{
    if (on) {
        if (VEC) {
            const f32x4 a = *(const f32x4 *)p;
#pragma unroll
            for (int c = 0; c < 4; ++c) l[c] = a[c];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) l[c] = p[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) l[c] = 0.f;
    }
}

// one pixel's class probabilities.  BIN (K = 2): one plane, class 1 of the softmax of the two logits, p[0] = 1 / (1 + e^(l0 - l1));
// else the softmax of all K classes as exp(l_k - max) / sum_j exp(l_j - max), the sum in increasing j (softmax.hpp, as the losses)
template <int KP, bool BIN>
__device__ __forceinline__ void class_probs(const float (&l)[KP], int K, float (&p)[KP])
{
    if (BIN) {
        p[0] = 1.f / (1.f + expf(l[0] - l[1]));
        return;
    }
    int am;
    float ex[KP];
    const float se = class_exps<KP>(l, K, first_max<KP>([&](int k) { return l[k]; }, K, am), ex);
#pragma unroll
    for (int k = 0; k < KP; ++k) p[k] = ex[k] / se;         // true division (the loss kernels multiply by 1.f / se)
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
        const TilePos t = tile_quad(q, S4, So, t0, ny, nx);
        const int row = oy0 + t.i * So + t.y;
        if ((unsigned)row >= (unsigned)H) continue;
        const int c0 = ox0 + t.j * So + 4 * t.x;
        const float *p0 = logits + 2 * t.tl * plane + (size_t)t.y * So + 4 * t.x;
        float l[2][4];
#pragma unroll
        for (int k = 0; k < 2; ++k) load_logits4<VEC>(p0 + k * plane, true, l[k]);
        const size_t o = (t.b * H + row) * (size_t)W;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = c0 + c;
            if ((unsigned)col >= (unsigned)W) continue;
            mask[o + col] = l[1][c] > l[0][c] ? 1 : 0;                         // unet_argmax2's rule: ties -> class 0
            if (prob) {
                const float lc[2] = {l[0][c], l[1][c]};
                float p[2];
                class_probs<2, true>(lc, 2, p);
                prob[o + col] = p[0];
            }
        }
    }
}

// K classes (2 <= K <= KP): the same lanes as tile_stitch_kernel; argmax with ties -> the lowest class (torch.argmax), and
// optionally the softmax of all K classes, prob [B,K,H,W]
template <int KP>
__global__ __launch_bounds__(256) void tile_stitch_k_kernel(const float *__restrict__ logits, int So, int K, int oy0, int ox0, int ny, int nx,
                                                            long long t0, int B, int H, int W, long long *__restrict__ mask,
                                                            float *__restrict__ prob, size_t quads)
{
    const int S4 = So >> 2;
    const size_t plane = (size_t)So * So, iplane = (size_t)H * W;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const TilePos t = tile_quad(q, S4, So, t0, ny, nx);
        const int row = oy0 + t.i * So + t.y;
        if ((unsigned)row >= (unsigned)H) continue;
        const int c0 = ox0 + t.j * So + 4 * t.x;
        const float *p0 = logits + (size_t)K * t.tl * plane + (size_t)t.y * So + 4 * t.x;
        float l[KP][4];
#pragma unroll
        for (int k = 0; k < KP; ++k) load_logits4<true>(p0 + k * plane, k < K, l[k]);        // 16-byte aligned logits (checked)
        const size_t o = (t.b * H + row) * (size_t)W;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = c0 + c;
            if ((unsigned)col >= (unsigned)W) continue;
            float lc[KP], p[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) lc[k] = l[k][c];
            float m = lc[0];
            int am = 0;
#pragma unroll
            for (int k = 1; k < KP; ++k) if (k < K && lc[k] > m) { m = lc[k]; am = k; }
            mask[o + col] = am;
            if (prob) {
                class_probs<KP, false>(lc, K, p);
#pragma unroll
                for (int k = 0; k < KP; ++k) if (k < K) prob[(t.b * K + k) * iplane + (size_t)row * W + col] = p[k];
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

// t = 0: tile_gather_body with the flips
template <bool VEC>
__global__ __launch_bounds__(256) void tile_gather_view_kernel(const float *__restrict__ img, int H, int W, const float *__restrict__ minmax,
                                                               int S, int fy, int fx, int oy0, int ox0, int ny, int nx, long long t0,
                                                               float *__restrict__ out, size_t quads)
{
    tile_gather_body<VEC, true>(img, H, W, minmax, S, fy, fx, oy0, ox0, ny, nx, t0, out, quads, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                                (size_t)gridDim.x * blockDim.x);
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
        const TilePos t = tile_block(task, nbs, t0, ny, nx);
        const int bx = t.x, by = t.y, j = t.j, i = t.i;
        const size_t tl = t.tl, b = t.b;
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

// phase bit 0 (FIRST): the probability is stored, else added to what is there; bit 1 (LAST): the sum is then divided by the
// number of views and the mask written: BIN prob > 0.5, else the argmax of the sums, ties -> the lowest class
enum { VIEW_FIRST = 1, VIEW_LAST = 2 };

// one class plane k of one pixel: a holds the plane's sum so far, s the view's probability; best / am follow the argmax
template <bool BIN>
__device__ __forceinline__ void view_accumulate(float *a, float s, int k, int phase, float nf, float &best, int &am)
{
    if (!(phase & VIEW_FIRST)) s += *a;
    if (phase & VIEW_LAST) {
        if (!BIN && (k == 0 || s > best)) { best = s; am = k; }
        s = s / nf;
        if (BIN) am = s > 0.5f ? 1 : 0;
    }
    *a = s;
}

// t = 0: tile_stitch_kernel's lanes (4 consecutive columns of one tile output row), flips folded into the image index
template <int KP, bool BIN, bool VEC>
__global__ __launch_bounds__(256) void tile_stitch_view_kernel(const float *__restrict__ logits, int So, int K, int fy, int fx, int oy0, int ox0,
                                                               int ny, int nx, long long t0, int H, int W, int phase, float nf,
                                                               float *__restrict__ prob, long long *__restrict__ mask, size_t quads)
{
    const int S4 = So >> 2, np = BIN ? 1 : K;
    const size_t plane = (size_t)So * So, iplane = (size_t)H * W;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const TilePos t = tile_quad(q, S4, So, t0, ny, nx);
        const int vy = oy0 + t.i * So + t.y;
        if ((unsigned)vy >= (unsigned)H) continue;
        const int row = fy ? H - 1 - vy : vy;
        const int c0 = ox0 + t.j * So + 4 * t.x;
        const float *p0 = logits + (size_t)K * t.tl * plane + (size_t)t.y * So + 4 * t.x;
        float l[KP][4];
#pragma unroll
        for (int k = 0; k < KP; ++k) load_logits4<VEC>(p0 + k * plane, k < K, l[k]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int vx = c0 + c;
            if ((unsigned)vx >= (unsigned)W) continue;
            const size_t o = (size_t)row * W + (fx ? W - 1 - vx : vx);
            float lc[KP], p[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) lc[k] = l[k][c];
            class_probs<KP, BIN>(lc, K, p);
            float best = 0.f;
            int am = 0;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < np) view_accumulate<BIN>(prob + (t.b * np + k) * iplane + o, p[k], k, phase, nf, best, am);
            if (phase & VIEW_LAST) mask[t.b * iplane + o] = am;
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
        const TilePos t = tile_block(task, nbs, t0, ny, nx);
        const int bx = t.x, by = t.y, j = t.j, i = t.i;
        const size_t tl = t.tl, b = t.b;
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
                class_probs<KP, BIN>(l, K, p[e]);
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
                for (int e = 0; e < 4; ++e)
                    if (ok[e]) view_accumulate<BIN>(prob + (b * np + c) * iplane + o[e], buf[tx][ty + 8 * e], c, phase, nf, best[e], am[e]);
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

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// view code -> transpose, flip of the view's rows, flip of its columns (tester.apply_view)
struct ViewCode { int tr, fy, fx; };
static ViewCode split_view(int view) { return {view & 1, (view >> 1) & 1, (view >> 2) & 1}; }
// check_tile_grid on the view's shape: a transposed view of an H x W image is W x H
static int check_view_grid(const char *who, int B, int H, int W, int tr, int So, int oy0, int ox0, int ny, int nx, long long t0, int nt)
{
    return check_tile_grid(who, B, tr ? W : H, tr ? H : W, So, oy0, ox0, ny, nx, t0, nt);
}

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
        dispatch_bool(aligned16(tiles_out), [&](auto vec) {
            hipLaunchKernelGGL(tile_gather_kernel<decltype(vec)::value>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W,
                               (const float *)minmax, S, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
        });
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
        dispatch_bool(aligned16(logits), [&](auto vec) {
            hipLaunchKernelGGL(tile_stitch_kernel<decltype(vec)::value>, dim3(grid), dim3(256), 0, st, (const float *)logits, So, oy0, ox0,
                               ny, nx, (long long)t0, H, W, (long long *)mask_i64, (float *)prob_f32, quads);
        });
    });
}

int unet_tile_stitch_k(const void *logits, int So, int K, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W,
                       void *mask_i64, void *prob_f32, void *stream)
{
    ARG_CHECK(logits && mask_i64, "unet_tile_stitch_k: null argument");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_tile_stitch_k: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK(aligned16(logits), "unet_tile_stitch_k: logits must be 16-byte aligned");
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
    const ViewCode v = split_view(view);
    int rc = check_view_grid("unet_tile_gather_view", B, H, W, v.tr, S - 2 * TILE_MARGIN, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("N2.tile_gather");
    const double bytes = 8.0 * nt * S * S;
    if (v.tr) {
        const size_t nbs = (S + VIEW_BLOCK - 1) / VIEW_BLOCK, tasks = (size_t)nt * nbs * nbs;
        return profiled(PK_ELEMWISE, "tile_gather_view_t", st, 0.0, 0.0, bytes, [&] {
            hipLaunchKernelGGL(tile_gather_view_t_kernel, dim3(grid_for(tasks, 1, 16384)), dim3(256), 0, st, (const float *)img, H, W,
                               (const float *)minmax, S, v.fy, v.fx, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, tasks);
        });
    }
    const size_t quads = (size_t)nt * S * (S / 4);
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_gather_view", st, 0.0, 0.0, bytes, [&] {
        dispatch_bool(aligned16(tiles_out), [&](auto vec) {
            hipLaunchKernelGGL(tile_gather_view_kernel<decltype(vec)::value>, dim3(grid), dim3(256), 0, st, (const float *)img, H, W,
                               (const float *)minmax, S, v.fy, v.fx, oy0, ox0, ny, nx, (long long)t0, (float *)tiles_out, quads);
        });
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
    ARG_CHECK(K == 2 || aligned16(logits), "unet_tile_stitch_view: logits of K > 2 classes must be 16-byte aligned");
    const ViewCode v = split_view(view);
    int rc = check_view_grid("unet_tile_stitch_view", B, H, W, v.tr, So, oy0, ox0, ny, nx, t0, nt);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float nf = (float)n_views;
    const int np = K == 2 ? 1 : K;
    ProfScope ps("N2.tile_stitch");
    const double bytes = (4.0 * K + (phase & VIEW_FIRST ? 4.0 : 8.0) * np + (phase & VIEW_LAST ? 8.0 : 0.0)) * nt * So * So;
    // KP_ == 2 exactly when K == 2: the one-plane (BIN) kernels; only they have a scalar-load form (K > 2: aligned, checked above)
    if (v.tr) {
        const size_t nbs = (So + VIEW_BLOCK - 1) / VIEW_BLOCK, tasks = (size_t)nt * nbs * nbs;
        const int grid = grid_for(tasks, 1, 16384);
        return profiled(PK_ELEMWISE, "tile_stitch_view_t", st, 0.0, 0.0, bytes, [&] {
            CLASS_DISPATCH(K, hipLaunchKernelGGL((tile_stitch_view_t_kernel<KP_, KP_ == 2>), dim3(grid), dim3(256), 0, st, (const float *)logits,
                                                 So, K, v.fy, v.fx, oy0, ox0, ny, nx, (long long)t0, H, W, phase, nf, (float *)prob_f32,
                                                 (long long *)mask_i64, tasks));
        });
    }
    const size_t quads = (size_t)nt * So * (So / 4);
    const int grid = grid_for(quads, 256, 16384);
    return profiled(PK_ELEMWISE, "tile_stitch_view", st, 0.0, 0.0, bytes, [&] {
        dispatch_bool(aligned16(logits), [&](auto vec) {
            CLASS_DISPATCH(K, hipLaunchKernelGGL((tile_stitch_view_kernel<KP_, KP_ == 2, KP_ != 2 || decltype(vec)::value>), dim3(grid),
                                                 dim3(256), 0, st, (const float *)logits, So, K, v.fy, v.fx, oy0, ox0, ny, nx, (long long)t0,
                                                 H, W, phase, nf, (float *)prob_f32, (long long *)mask_i64, quads));
        });
    });
}

}  // extern "C"
