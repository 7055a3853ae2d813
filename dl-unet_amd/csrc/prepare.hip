// prepare.hip — from a Cell Tracking Challenge instance image to a trainable target and the weights of its crop origins
// (the reference's preprocess_gt, data.py:195-221, and the window loop of ImageDataset.__init__, data.py:67-82), batched, on
// the device.
//
// unet_carve_borders: preprocess_gt dilates every cell twice with a 5 x 5 rectangle and adds 255 on the ring each cell gains.
//   Two iterations of a 5 x 5 rectangle are one 9 x 9 rectangle clipped to the image (the default dilate border adds nothing),
//   so with r = the reach (4) and n(p) = the number of distinct ids c, c != 0 and c != id(p), in the (2r+1)^2 window around p:
//   mask_global = 255 n, gt = max(0, id - 255 n), gt_bin = 255 (gt > 0).  One kernel, carve_kernel: a workgroup owns a 32 x 32
//   tile of outputs and holds the ids of the tile and its r-pixel halo in LDS as int32 (0 outside the image and for ids out of
//   range).  Two separable passes give every window's smallest non-zero id and largest id:
//     no non-zero id           -> n = 0
//     smallest == largest      -> n = (that id != own)
//     else                     -> n = (smallest != own) + (largest != own) + the distinct ids strictly between them: one scan of
//     the window, (2r+1)^2 LDS reads, which near a border of two cells finds nothing more; a value between them (near junctions
//     of three or more ids) is counted at its first occurrence only, found by re-scanning the earlier positions up to the first
//     match: at most (2r+1)^4 / 2 LDS reads per pixel whatever the image holds.  The cost is bounded by r and the image size,
//     never by the number of cells.
//
// unet_crop_counts: c[b][i][j] = non-zero pixels of rows [skip i, skip i + crop) x columns [skip j, skip j + crop), exact:
//   1. crop_prefix   one workgroup per image row: P[x] = non-zero pixels left of x, 1024 pixels per pass with a carry
//   2. crop_rowsum   rowsum[y][j] = P[skip j + crop] - P[skip j]
//   3. crop_colsum   one thread per (b, i, j) sums rowsum[skip i .. skip i + crop)[j]
//   Every pixel is read once, every prefix word twice at the most: nothing is read once per window.
//
// Coherence (label.hip's rule): status words are only touched by agent-scope adds; every other word a kernel reads was written
// by an earlier kernel of the same stream (or by the caller).  No word is handed from one workgroup to another inside a kernel.
#include "elem.hpp"
#include <algorithm>
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int CV_TILE = 32;                           // outputs per side of a workgroup's tile
static constexpr int CV_RMAX = 8;
static constexpr int CV_PITCH = CV_TILE + 2 * CV_RMAX;       // LDS row pitch of the id tile (48)
static constexpr int CV_ID_LIMIT = 1 << 24;                  // valid ids lie below: every output is then exact in fp32
static constexpr int CP_PASS = 1024;                         // pixels per pass of crop_prefix: 256 threads x 4

// the id at element e as an int in [0, 2^24), or -1 when it is outside that range (dtype 0: int64, 1: float32, 2: int32)
__device__ __forceinline__ int carve_id(const void *ids, int dtype, size_t e)
{
    if (dtype == 0) {
        const long long v = ((const long long *)ids)[e];
        return v >= 0 && v < CV_ID_LIMIT ? (int)v : -1;
    }
    if (dtype == 1) {
        const float v = ((const float *)ids)[e];
        return v >= 0.0f && v < (float)CV_ID_LIMIT ? (int)v : -1;          // a NaN fails both comparisons
    }
    const int v = ((const int *)ids)[e];
    return v >= 0 && v < CV_ID_LIMIT ? v : -1;
}

__global__ __launch_bounds__(256) void carve_kernel(const void *__restrict__ ids, int dtype, int H, int W, int r,
                                                    float *__restrict__ gt, float *__restrict__ edges,
                                                    unsigned char *__restrict__ bin, unsigned long long *__restrict__ status)
{
    __shared__ int tile[CV_PITCH * CV_PITCH];                // ids of the tile and its halo: [halo row][halo column]
    __shared__ unsigned hmin[CV_PITCH * CV_TILE];            // per halo row and output column: min of (id - 1) as unsigned over
    __shared__ int hmax[CV_PITCH * CV_TILE];                 // the 2r+1 columns (0 wraps to the largest value), and max of id
    const int b = blockIdx.z, y0 = blockIdx.y * CV_TILE, x0 = blockIdx.x * CV_TILE;
    const int side = CV_TILE + 2 * r, win = 2 * r + 1;
    const size_t img = (size_t)b * H * W;
    unsigned bad = 0;
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int hy = i / side, hx = i - hy * side;
        const int y = y0 + hy - r, x = x0 + hx - r;
        int v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = carve_id(ids, dtype, img + (size_t)y * W + x);
            if (v < 0) {
                v = 0;
                // every pixel is some tile's own exactly once: count it there, not in the halos that also hold it
                if (hy >= r && hy < r + CV_TILE && hx >= r && hx < r + CV_TILE) ++bad;
            }
        }
        tile[hy * CV_PITCH + hx] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < side * CV_TILE; i += 256) {
        const int hy = i / CV_TILE, tx = i - hy * CV_TILE;
        const int *row = tile + hy * CV_PITCH + tx;
        unsigned mn = ~0u;
        int mx = 0;
        for (int k = 0; k < win; ++k) {
            const int v = row[k];
            mn = min(mn, (unsigned)(v - 1));
            mx = max(mx, v);
        }
        hmin[i] = mn;
        hmax[i] = mx;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CV_TILE * CV_TILE; i += 256) {
        const int ty = i / CV_TILE, tx = i - ty * CV_TILE;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        unsigned mn = ~0u;
        int mx = 0;
        for (int k = 0; k < win; ++k) {
            mn = min(mn, hmin[(ty + k) * CV_TILE + tx]);
            mx = max(mx, hmax[(ty + k) * CV_TILE + tx]);
        }
        const int own = tile[(ty + r) * CV_PITCH + tx + r];
        int n = 0;
        if (mx != 0) {
            const int lo = (int)(mn + 1);                    // the smallest non-zero id
            if (lo == mx) n = mx != own;
            else {
                // two or more ids: the smallest and the largest count once each; any value between them (a third id: only near
                // junctions of three or more) counts at its first occurrence
                n = (lo != own) + (mx != own);
                const int *w0 = tile + ty * CV_PITCH + tx;   // top left of the window
                for (int j = 0; j < win * win; ++j) {
                    const int jy = j / win, jx = j - jy * win;
                    const int v = w0[jy * CV_PITCH + jx];
                    if (v == 0 || v == own || v == lo || v == mx) continue;
                    bool first = true;
                    for (int ky = 0; ky <= jy && first; ++ky) {
                        const int kend = ky < jy ? win : jx;
                        for (int kx = 0; kx < kend; ++kx)
                            if (w0[ky * CV_PITCH + kx] == v) { first = false; break; }
                    }
                    n += first;
                }
            }
        }
        const int e = n * 255, g = max(0, own - e);
        const size_t o = img + (size_t)y * W + x;
        if (gt) gt[o] = (float)g;
        if (edges) edges[o] = (float)e;
        if (bin) bin[o] = g > 0 ? 255 : 0;
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad)
        __hip_atomic_fetch_add(&status[b], (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// P[b][y][0..W]: P[x] = non-zero pixels of the row left of x.  One workgroup per row, CP_PASS pixels per pass
__global__ __launch_bounds__(256) void crop_prefix_kernel(const void *__restrict__ mask, int dtype, int H, int W, unsigned *__restrict__ P)
{
    const size_t row = (size_t)blockIdx.y * H + blockIdx.x;
    const size_t in = row * W;
    unsigned *p = P + row * ((size_t)W + 1);
    if (threadIdx.x == 0) p[0] = 0;
    int carry = 0;
    for (int base = 0; base < W; base += CP_PASS) {          // uniform over the workgroup: block_scan256 has barriers
        const int x = base + threadIdx.x * 4;
        int m[4], mine = 0;
        for (int k = 0; k < 4; ++k) {
            m[k] = x + k < W ? mask_on(mask, dtype, in + x + k) : 0;
            mine += m[k];
        }
        int total;
        int run = carry + block_scan256(mine, total);
        for (int k = 0; k < 4; ++k) {
            run += m[k];
            if (x + k < W) p[x + k + 1] = (unsigned)run;
        }
        carry += total;
    }
}

__global__ __launch_bounds__(256) void crop_rowsum_kernel(const unsigned *__restrict__ P, size_t rows, int W, int crop, int skip, int nx,
                                                          unsigned *__restrict__ rowsum)
{
    const size_t total = rows * nx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / nx;
        const int j = (int)(i - row * nx);
        const unsigned *p = P + row * ((size_t)W + 1) + (size_t)skip * j;
        rowsum[i] = p[crop] - p[0];
    }
}

__global__ __launch_bounds__(256) void crop_colsum_kernel(const unsigned *__restrict__ rowsum, int B, int H, int crop, int skip, int ny,
                                                          int nx, unsigned *__restrict__ counts)
{
    const size_t total = (size_t)B * ny * nx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % nx);
        const size_t bi = i / nx;
        const int wi = (int)(bi % ny);
        const size_t b = bi / ny;
        const unsigned *rs = rowsum + (b * H + (size_t)skip * wi) * nx + j;
        unsigned c = 0;
        for (int y = 0; y < crop; ++y) c += rs[(size_t)y * nx];
        counts[i] = c;
    }
}

} // namespace unet

using namespace unet;

int unet_carve_borders(const void *ids, int dtype, int B, int H, int W, int reach, void *gt_f32, void *edges_f32, void *bin_u8,
                       void *status_u64, void *stream)
{
    ARG_CHECK(ids && status_u64 && B > 0 && H > 0 && W > 0, "unet_carve_borders: bad argument");
    ARG_CHECK(gt_f32 || edges_f32 || bin_u8, "unet_carve_borders: at least one of gt_f32, edges_f32 and bin_u8 must be given");
    ARG_CHECK(dtype == 0 || dtype == 1 || dtype == 2, "unet_carve_borders: dtype must be 0 (int64), 1 (float32) or 2 (int32)");
    ARG_CHECK(reach >= 0 && reach <= CV_RMAX, "unet_carve_borders: reach must be in [0, %d]", CV_RMAX);
    ARG_CHECK((size_t)H * W < (1u << 31) && B <= 65535 && cdiv(H, CV_TILE) <= 65535, "unet_carve_borders: image too large");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(carve_kernel, dim3(cdiv(W, CV_TILE), cdiv(H, CV_TILE), B), dim3(256), 0, st, ids, dtype, H, W, reach,
                       (float *)gt_f32, (float *)edges_f32, (unsigned char *)bin_u8, (unsigned long long *)status_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}

// windows along an axis of n pixels: len(range(0, n - crop, skip)); 0 when the arguments allow none
static int crop_windows(int n, int crop, int skip)
{
    if (crop < 1 || skip < 1 || n <= crop) return 0;
    return (int)(((long long)n - crop + skip - 1) / skip);
}
static size_t crop_prefix_bytes(int B, int H, int W) { return align_up((size_t)B * H * ((size_t)W + 1) * sizeof(unsigned), 256); }

size_t unet_crop_counts_scratch_bytes(int B, int H, int W, int crop, int skip)
{
    const int ny = crop_windows(H, crop, skip), nx = crop_windows(W, crop, skip);
    if (B <= 0 || ny == 0 || nx == 0) return 0;
    return crop_prefix_bytes(B, H, W) + align_up((size_t)B * H * nx * sizeof(unsigned), 256);
}

int unet_crop_counts(const void *mask, int dtype, int B, int H, int W, int crop, int skip, void *counts_u32, void *scratch, void *stream)
{
    ARG_CHECK(mask && counts_u32 && scratch && B > 0 && H > 0 && W > 0, "unet_crop_counts: bad argument");
    ARG_CHECK(dtype >= 0 && dtype <= 3, "unet_crop_counts: dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(crop >= 1 && skip >= 1, "unet_crop_counts: crop and skip must be at least 1");
    ARG_CHECK(H > crop && W > crop, "unet_crop_counts: no window: the image (%d x %d) must be larger than the crop (%d) on both axes", H, W,
              crop);
    ARG_CHECK((size_t)H * W < (1u << 31) && B <= 65535, "unet_crop_counts: image too large");
    hipStream_t st = (hipStream_t)stream;
    const int ny = crop_windows(H, crop, skip), nx = crop_windows(W, crop, skip);
    unsigned *P = (unsigned *)scratch;
    unsigned *rowsum = (unsigned *)((char *)scratch + crop_prefix_bytes(B, H, W));
    hipLaunchKernelGGL(crop_prefix_kernel, dim3(H, B), dim3(256), 0, st, mask, dtype, H, W, P);
    hipLaunchKernelGGL(crop_rowsum_kernel, dim3(grid_for((size_t)B * H * nx)), dim3(256), 0, st, (const unsigned *)P, (size_t)B * H, W, crop,
                       skip, nx, rowsum);
    hipLaunchKernelGGL(crop_colsum_kernel, dim3(grid_for((size_t)B * ny * nx)), dim3(256), 0, st, (const unsigned *)rowsum, B, H, crop, skip,
                       ny, nx, (unsigned *)counts_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
