// grow.hip — nearest-cell growth of an instance map (the "expand the labels" step: skimage.segmentation.expand_labels with an
// exact metric and a stated tie rule), batched, on the device.  A labelled pixel keeps its id; a background pixel takes the id of
// the labelled pixel at the smallest exact squared Euclidean distance d^2 (an integer), the smallest id among those at that d^2;
// with a limit only labelled pixels with d^2 <= max_dist2 count, and a pixel with none in reach stays 0.
//
//   1. grow_cols   one thread per column (x, b), coalesced across x: a downward and an upward sweep leave, for every pixel, the
//                  word  g^2 << 24 | id  of the nearest labelled pixel of its column (g = the row distance; above and below at
//                  the same g: the smaller id, which is the smaller word), or GR_NONE when the column has none, or none with
//                  g^2 <= max_dist2
//   2. grow_rows   one workgroup per 256 consecutive pixels of a row: the row's column words go through LDS in chunks, and every
//                  background pixel takes the minimum over x' of the 64-bit key  word(x') + ((x - x')^2 << 24)
//                  = d^2 << 24 | id;  with a limit only |x - x'| <= R = floor(sqrt(max_dist2)) is scanned, and a minimum whose
//                  d^2 > max_dist2 is dropped
//
// Exactness: every nearest labelled pixel q = (x', y') of a pixel (x, y) is the column-nearest labelled pixel of column x' as seen
// from row y, above or below: a labelled pixel of that column nearer in rows would be nearer to (x, y) than q.  Pass 1 keeps, for
// every column and row, the nearer of the two (both ids' minimum at equal g), pass 2 looks at every column in reach: together they
// see every candidate (d^2, id), and the minimum of the packed keys is the lexicographic minimum of (d^2, id), ties included.  A
// parabola-stack lower envelope would find d^2 in O(W) per row but not, for free, the smallest id among equal d^2: the row pass is
// brute force on purpose.
//
// Cost: H * W * min(W, 2 R + 257) key evaluations (one LDS broadcast read, one 64-bit add, one 64-bit minimum each), about
// 1.4e8 for an unlimited 512 x 512 image, plus 2 H steps per column.  Nothing depends on the number of cells or on their ids.
//
// Coherence (label.hip's rule): grow_rows reads what grow_cols, an earlier kernel, wrote; in grow_cols a thread re-reads only the
// words of its own column, which it wrote itself.  No word is handed from one workgroup to another inside a kernel.
#include "elem.hpp"
#include <algorithm>
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int GR_ID_BITS = 24;
static constexpr unsigned GR_ID_MASK = (1u << GR_ID_BITS) - 1;
static constexpr int GR_PX = 256;                              // pixels per workgroup of grow_rows
static constexpr int GR_CHUNK = 1024;                          // column words staged per round (8 KiB of LDS)
static constexpr int GR_EDGE = 65535;                          // H, W <= GR_EDGE: g^2, dx^2 < 2^32, d^2 < 2^33, a key < 2^57
static constexpr unsigned long long GR_NONE = 1ull << 60;      // above every key, and GR_NONE + (dx^2 << 24) does not wrap
static constexpr unsigned long long GR_UNLIMITED = 1ull << 34; // above every d^2, below GR_NONE >> 24

__device__ __forceinline__ bool gr_labelled(int v) { return v > 0 && v <= (int)GR_ID_MASK; }

__global__ __launch_bounds__(64) void grow_cols_kernel(const int *__restrict__ labels, int H, int W, unsigned long long lim,
                                                       unsigned long long *__restrict__ col)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const size_t o = (size_t)blockIdx.y * H * W + x;
    const int *L = labels + o;
    unsigned long long *C = col + o;
    unsigned long long g = 0, id = 0;                          // id 0: no labelled pixel seen yet
#pragma unroll 8
    for (int y = 0; y < H; ++y) {                              // downward: the nearest labelled pixel at or above y
        const int v = L[(size_t)y * W];
        if (gr_labelled(v)) { id = (unsigned)v; g = 0; } else ++g;
        C[(size_t)y * W] = id ? (g * g) << GR_ID_BITS | id : GR_NONE;
    }
    id = 0;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {                         // upward: the nearest at or below y, merged with the word above
        const unsigned long long dn = C[(size_t)y * W];        // this thread's own store
        if (dn >> GR_ID_BITS == 0) { id = dn & GR_ID_MASK; g = 0; } else ++g;
        unsigned long long m = id ? (g * g) << GR_ID_BITS | id : GR_NONE;
        m = dn < m ? dn : m;
        C[(size_t)y * W] = m >> GR_ID_BITS > lim ? GR_NONE : m;
    }
}

__global__ __launch_bounds__(GR_PX) void grow_rows_kernel(const int *__restrict__ labels, const unsigned long long *__restrict__ col,
                                                          int H, int W, int R, unsigned long long lim, int *__restrict__ out)
{
    __shared__ unsigned long long s[GR_CHUNK];
    const int y = blockIdx.y, x0 = blockIdx.x * GR_PX, x = x0 + (int)threadIdx.x;
    const size_t row = ((size_t)blockIdx.z * H + y) * W;
    const int v = x < W ? labels[row + x] : 1;                 // lanes past the row's end ask for nothing
    if (!__syncthreads_or(v == 0)) {                           // no background pixel among the 256
        if (x < W) out[row + x] = v;
        return;
    }
    const int lo = max(0, x0 - R), hi = min(W, x0 + GR_PX + R);                    // R <= GR_EDGE: no overflow
    unsigned long long best = GR_NONE;
    for (int c0 = lo; c0 < hi; c0 += GR_CHUNK) {
        const int n = min(GR_CHUNK, hi - c0);
        __syncthreads();                                       // the previous round's reads of s are done
        for (int i = threadIdx.x; i < n; i += GR_PX) s[i] = col[row + c0 + i];
        __syncthreads();
        if (v != 0) continue;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const unsigned dx = (unsigned)abs(x - c0 - j);
            const unsigned long long key = s[j] + ((unsigned long long)(dx * dx) << GR_ID_BITS);
            best = key < best ? key : best;
        }
    }
    if (x < W) out[row + x] = v != 0 ? v : best >> GR_ID_BITS <= lim ? (int)(best & GR_ID_MASK) : 0;
}

} // namespace unet

using namespace unet;

size_t unet_grow_labels_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return plane_bytes(B, H, W, sizeof(unsigned long long));
}

int unet_grow_labels(const void *labels_i32, int B, int H, int W, long long max_dist2, void *out_i32, void *scratch, void *stream)
{
    ARG_CHECK(labels_i32 && out_i32 && scratch && B > 0 && H > 0 && W > 0, "unet_grow_labels: bad argument");
    ARG_CHECK((size_t)H * W < (1u << 31) && H <= GR_EDGE && B <= 65535, "unet_grow_labels: image too large");
    ARG_CHECK(W <= GR_EDGE, "unet_grow_labels: W is at most %d (a squared distance and an id share one 64-bit key)", GR_EDGE);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long lim = GR_UNLIMITED;
    int R = GR_EDGE;
    if (max_dist2 >= 0 && (unsigned long long)max_dist2 < GR_UNLIMITED) {
        lim = (unsigned long long)max_dist2;
        R = (int)std::min(std::sqrt((double)max_dist2), (double)GR_EDGE);                 // floor(sqrt(max_dist2)), in integers
        while ((long long)R * R > max_dist2) --R;
        while (R < GR_EDGE && (long long)(R + 1) * (R + 1) <= max_dist2) ++R;
    }
    unsigned long long *col = (unsigned long long *)scratch;
    hipLaunchKernelGGL(grow_cols_kernel, dim3(cdiv(W, 64), B), dim3(64), 0, st, (const int *)labels_i32, H, W, lim, col);
    hipLaunchKernelGGL(grow_rows_kernel, dim3(cdiv(W, GR_PX), H, B), dim3(GR_PX), 0, st, (const int *)labels_i32,
                       (const unsigned long long *)col, H, W, R, lim, (int *)out_i32);
    HIP_TRY(hipGetLastError());
    return 0;
}
