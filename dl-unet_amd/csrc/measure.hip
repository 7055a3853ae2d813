// measure.hip — one row of exact integers per cell of an instance map (and optionally of an image under it), batched, on the
// device: what scipy.ndimage's sum_labels / find_objects / center_of_mass / minimum / maximum give one quantity and one cell at
// a time; and the per-id remap of an instance map that drops or renumbers cells by any decision taken on those rows.
//
// The record of (image b, id i) is MS_WORDS = 16 64-bit words = 128 bytes, all zero before the fill:
//   0      area | frame << 32   (area <= 2^30, frame <= 2 (H + W) <= 2^17: the two adds never meet)
//   1-5    sum y, sum x, sum y^2, sum x^2, sum x y
//   6, 7   open, contact edges
//   8, 9   sum v, sum v^2        (integer image: u64; float32 image: fp64 bits)
//   10-13  ~y0, ~x0, y1, x1      (the box, half-open; a minimum is kept as the maximum of the complement, so that zero is the
//                                 neutral word of every field and one memset initialises the table)
//   14, 15 ~key(min v), key(max v)   (key: v itself for an integer image, the order-preserving map of the float bits else)
// Words 0-9 are only ever added to, words 10-15 only ever raised (unsigned max).
//
//   1. ms_fill      one workgroup per 64 x 16 tile: the ids of the tile and of its one-pixel halo go to LDS once (-1 outside the
//                   image, -2 for an id outside [0, n_max], which is counted and indexes nothing).  A wave takes four rows, one
//                   at a time, lane = column.  One ballot marks where the id changes; the head lane of a run of n equal ids at
//                   (y, x0) forms area, box and the five moments in closed form.  The per-pixel terms (the three edge counts, v,
//                   v^2, min, max) are reduced per run by a segmented suffix scan in fixed lane order.  The head adds its run to
//                   the workgroup's table in LDS (MS_SLOTS slots, open addressing on the id, at most MS_PROBES probes, 64-bit
//                   LDS add / max); a run that finds no slot goes straight to the global record.  At the end the workgroup
//                   flushes every occupied slot: 16 consecutive lanes cover the 128 contiguous bytes of one record.
//   2. ms_finish    one thread per (b, id): the record becomes the rows of the output tensors, complements and keys undone, every
//                   field 0 and present = 0 where area == 0.
// ms_remap: out = map[b][labels], ids outside [0, n_max] counted and written as 0.
//
// No loop over ids: the work is per pixel (three LDS reads of neighbours, one image read) plus per run.  Integer sums and maxima
// commute, so every integer field is the same in every run, whichever of the two paths a run took; the fp64 sums of a float
// image are summed in fixed order inside a run and in arrival order across runs.
//
// Coherence (label.hip's rule): during ms_fill a global record word is touched only by agent-scope atomic read-modify-writes,
// never read or stored plainly; ms_finish is a later kernel of the same stream and reads with plain loads.  The status words
// likewise.  The LDS table is workgroup-scope and handed over by barriers.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

typedef unsigned long long u64;

static constexpr int MS_WORDS = 16;
static constexpr int MS_TW = 64, MS_TH = 16;                   // tile: one wave-row wide, four rows per wave
static constexpr int MS_SLOTS = 128, MS_SLOT_BITS = 7;         // 128 records of 128 B = 16 KiB of LDS
static constexpr int MS_PROBES = 8;
static constexpr int MS_OUTSIDE = -1, MS_BAD = -2, MS_EMPTY = -1;
enum { MW_AREA = 0, MW_SY = 1, MW_SX = 2, MW_SYY = 3, MW_SXX = 4, MW_SXY = 5, MW_OPEN = 6, MW_CONTACT = 7, MW_SV = 8, MW_SVV = 9,
       MW_Y0 = 10, MW_X0 = 11, MW_Y1 = 12, MW_X1 = 13, MW_VMIN = 14, MW_VMAX = 15 };
enum { IMG_NONE = 0, IMG_INT = 1, IMG_FLOAT = 2 };

// order-preserving map of finite float bits onto unsigned integers, and back
__device__ __forceinline__ unsigned float_key(float v)
{
    const unsigned b = __builtin_bit_cast(unsigned, v);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ unsigned key_float_bits(unsigned k) { return (k & 0x80000000u) ? k ^ 0x80000000u : ~k; }

// word w of a record takes value v: LDS (workgroup scope) or global (agent scope); fadd: the word is an fp64 sum
template <bool GLOBAL>
__device__ __forceinline__ void ms_word(u64 *rec, int w, u64 v, bool fadd)
{
    constexpr auto scope = GLOBAL ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
    if (v == 0) return;                                        // the neutral word of every field (+0.0 for an fp64 sum)
    if (fadd) __hip_atomic_fetch_add((double *)rec + w, __builtin_bit_cast(double, v), __ATOMIC_RELAXED, scope);
    else if (w < MW_Y0) __hip_atomic_fetch_add(rec + w, v, __ATOMIC_RELAXED, scope);
    else __hip_atomic_fetch_max(rec + w, v, __ATOMIC_RELAXED, scope);
}

template <int IMG> struct ms_sum { typedef u64 type; };
template <> struct ms_sum<IMG_FLOAT> { typedef double type; };

template <typename LT>
__device__ __forceinline__ int ms_id(const LT *lab, size_t e, int n_max)
{
    const LT v = lab[e];
    return (v < 0 || v > (LT)n_max) ? MS_BAD : (int)v;
}

// image value at e as (sum term, sum-of-squares term, key); false: a value the entry refuses
template <int IMG, typename S>
__device__ __forceinline__ bool ms_value(const void *image, int dtype, size_t e, S &v, S &vv, unsigned &key)
{
    if (IMG == IMG_FLOAT) {
        const float f = ((const float *)image)[e];
        if (!(fabsf(f) <= 3.402823466e+38f)) return false;     // NaN and the infinities
        v = (S)f; vv = (S)f * (S)f; key = float_key(f);        // f * f is exact in fp64
        return true;
    }
    const long long i = dtype == 0 ? ((const long long *)image)[e] : dtype == 2 ? (long long)((const int *)image)[e]
                                                                               : (long long)((const unsigned char *)image)[e];
    if (i < 0 || i > 65535) return false;
    v = (S)i; vv = (S)(i * i); key = (unsigned)i;
    return true;
}

// ---- 1. fill ------------------------------------------------------------------------------------------------------------------
template <int IMG, typename LT>
__global__ __launch_bounds__(256) void ms_fill_kernel(const LT *__restrict__ labels, const void *__restrict__ image, int img_dtype, int H, int W,
                                                      int n_max, u64 *records, u64 *status)
{
    typedef typename ms_sum<IMG>::type S;
    __shared__ int lid[MS_TH + 2][MS_TW + 2];
    __shared__ int keys[MS_SLOTS];
    __shared__ u64 tab[MS_SLOTS][MS_WORDS];
    __shared__ unsigned bad[2];
    const int b = blockIdx.z, x0 = blockIdx.x * MS_TW, y0 = blockIdx.y * MS_TH, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)b * H * W;
    u64 *grec = records + (size_t)b * ((size_t)n_max + 1) * MS_WORDS;

    for (int i = threadIdx.x; i < (MS_TH + 2) * (MS_TW + 2); i += 256) {
        const int r = i / (MS_TW + 2), c = i - r * (MS_TW + 2), y = y0 - 1 + r, x = x0 - 1 + c;
        lid[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? ms_id(labels, img + (size_t)y * W + x, n_max) : MS_OUTSIDE;
    }
    for (int i = threadIdx.x; i < MS_SLOTS * MS_WORDS; i += 256) (&tab[0][0])[i] = 0;
    if (threadIdx.x < MS_SLOTS) keys[threadIdx.x] = MS_EMPTY;
    if (threadIdx.x < 2) bad[threadIdx.x] = 0;
    __syncthreads();

    unsigned bad_id = 0, bad_v = 0;
    for (int r = 0; r < MS_TH / 4; ++r) {
        const int ty = wave * (MS_TH / 4) + r, y = y0 + ty, x = x0 + lane;
        if (y >= H) break;                                      // wave-uniform
        const bool inside = x < W;
        const int id = lid[ty + 1][lane + 1];
        const bool valid = inside && id >= 0;
        bad_id += inside && id == MS_BAD;

        unsigned edges = 0;                                     // frame | open << 10 | contact << 20: at most 4 * 64 each per run
        S v = 0, vv = 0;
        unsigned kmin = 0xffffffffu, kmax = 0;
        if (valid) {
            const int nb[4] = {lid[ty][lane + 1], lid[ty + 2][lane + 1], lid[ty + 1][lane], lid[ty + 1][lane + 2]};
            for (int k = 0; k < 4; ++k)
                edges += nb[k] == MS_OUTSIDE ? 1u : nb[k] == id ? 0u : nb[k] == 0 ? 1u << 10 : 1u << 20;
        }
        if (IMG != IMG_NONE && inside) {
            unsigned key = 0;
            S a = 0, aa = 0;
            if (!ms_value<IMG>(image, img_dtype, img + (size_t)y * W + x, a, aa, key)) ++bad_v;
            else if (valid) { v = a; vv = aa; kmin = kmax = key; }
        }

        // runs of equal ids among the 64 lanes (a lane outside the image or with a refused id is a run of its own kind, skipped)
        const int k = valid ? id : MS_OUTSIDE;
        const int left = __shfl_up(k, 1, 64);
        const u64 heads = __ballot(lane == 0 || k != left);
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int rest = above ? __ffsll(above) : 64 - lane;    // lanes from this one to the end of its run
        for (int d = 1; d < 64; d <<= 1) {                      // segmented suffix scan: lane l holds the terms of [l, l + 2d) of its run
            const unsigned e2 = __shfl_down(edges, d, 64);
            const bool in_run = d < rest;
            if (in_run) edges += e2;
            if (IMG != IMG_NONE) {
                const S v2 = __shfl_down(v, d, 64), vv2 = __shfl_down(vv, d, 64);
                const unsigned lo2 = __shfl_down(kmin, d, 64), hi2 = __shfl_down(kmax, d, 64);
                if (in_run) { v += v2; vv += vv2; kmin = min(kmin, lo2); kmax = max(kmax, hi2); }
            }
        }
        if (!(heads >> lane & 1) || !valid) continue;           // heads only from here; the next row's shuffles follow the loop's join

        const u64 n = (u64)rest, xs = (u64)x, yy = (u64)y;
        const u64 sx = n * xs + n * (n - 1) / 2;
        u64 val[MS_WORDS];
        val[MW_AREA] = n | (u64)(edges & 1023u) << 32;
        val[MW_SY] = n * yy;
        val[MW_SX] = sx;
        val[MW_SYY] = n * yy * yy;
        val[MW_SXX] = n * xs * xs + xs * n * (n - 1) + (n - 1) * n * (2 * n - 1) / 6;
        val[MW_SXY] = yy * sx;
        val[MW_OPEN] = edges >> 10 & 1023u;
        val[MW_CONTACT] = edges >> 20 & 1023u;
        val[MW_SV] = IMG == IMG_NONE ? 0 : __builtin_bit_cast(u64, v);
        val[MW_SVV] = IMG == IMG_NONE ? 0 : __builtin_bit_cast(u64, vv);
        val[MW_Y0] = ~yy;
        val[MW_X0] = ~xs;
        val[MW_Y1] = yy + 1;
        val[MW_X1] = xs + n;
        val[MW_VMIN] = IMG == IMG_NONE ? 0 : (u64)(0xffffffffu - kmin);
        val[MW_VMAX] = IMG == IMG_NONE ? 0 : (u64)kmax;

        int slot = (int)(((unsigned)id * 0x9E3779B1u) >> (32 - MS_SLOT_BITS)), found = -1;
        for (int p = 0; p < MS_PROBES && found < 0; ++p) {
            int expect = MS_EMPTY;
            if (__hip_atomic_compare_exchange_strong(&keys[slot], &expect, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ||
                expect == id)
                found = slot;
            slot = (slot + 1) & (MS_SLOTS - 1);
        }
        if (found >= 0) {
            for (int w = 0; w < MS_WORDS; ++w) ms_word<false>(tab[found], w, val[w], IMG == IMG_FLOAT && (w == MW_SV || w == MW_SVV));
        } else {
            u64 *rec = grec + (size_t)id * MS_WORDS;
            for (int w = 0; w < MS_WORDS; ++w) ms_word<true>(rec, w, val[w], IMG == IMG_FLOAT && (w == MW_SV || w == MW_SVV));
        }
    }
    bad_id = wave_sum(bad_id);
    bad_v = wave_sum(bad_v);
    if (lane == 0 && bad_id) atomicAdd(&bad[0], bad_id);
    if (lane == 0 && bad_v) atomicAdd(&bad[1], bad_v);
    __syncthreads();

    const int w = threadIdx.x & (MS_WORDS - 1);
    for (int s = threadIdx.x / MS_WORDS; s < MS_SLOTS; s += 256 / MS_WORDS) {
        const int id = keys[s];
        if (id != MS_EMPTY) ms_word<true>(grec + (size_t)id * MS_WORDS, w, tab[s][w], IMG == IMG_FLOAT && (w == MW_SV || w == MW_SVV));
    }
    if (threadIdx.x < 2 && bad[threadIdx.x])
        __hip_atomic_fetch_add(&status[b * 2 + threadIdx.x], (u64)bad[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 2. finish ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ms_finish_kernel(const u64 *__restrict__ records, size_t rows, int img_kind, long long *__restrict__ area,
                                                        int *__restrict__ bbox, long long *__restrict__ moments, long long *__restrict__ edges,
                                                        u64 *__restrict__ vsum, unsigned *__restrict__ vrange, unsigned char *__restrict__ present)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (size_t)gridDim.x * blockDim.x) {
        u64 r[MS_WORDS];
        for (int w = 0; w < MS_WORDS; ++w) r[w] = records[i * MS_WORDS + w];
        const u64 a = r[MW_AREA] & 0xffffffffull;
        const bool on = a != 0;
        area[i] = (long long)a;
        present[i] = on;
        bbox[i * 4 + 0] = on ? (int)~r[MW_Y0] : 0;
        bbox[i * 4 + 1] = on ? (int)~r[MW_X0] : 0;
        bbox[i * 4 + 2] = (int)r[MW_Y1];
        bbox[i * 4 + 3] = (int)r[MW_X1];
        for (int k = 0; k < 5; ++k) moments[i * 5 + k] = (long long)r[MW_SY + k];
        edges[i * 3 + 0] = (long long)(r[MW_AREA] >> 32);
        edges[i * 3 + 1] = (long long)r[MW_OPEN];
        edges[i * 3 + 2] = (long long)r[MW_CONTACT];
        if (img_kind == IMG_NONE) continue;
        vsum[i * 2 + 0] = r[MW_SV];
        vsum[i * 2 + 1] = r[MW_SVV];
        const unsigned lo = 0xffffffffu - (unsigned)r[MW_VMIN], hi = (unsigned)r[MW_VMAX];
        vrange[i * 2 + 0] = !on ? 0u : img_kind == IMG_FLOAT ? key_float_bits(lo) : lo;
        vrange[i * 2 + 1] = !on ? 0u : img_kind == IMG_FLOAT ? key_float_bits(hi) : hi;
    }
}

// ---- remap --------------------------------------------------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void ms_remap_kernel(const LT *__restrict__ labels, size_t npx, const int *__restrict__ map, int n_max,
                                                       size_t map_stride, int *__restrict__ out, u64 *status)
{
    const int b = blockIdx.y;
    const int *M = map + (size_t)b * map_stride;
    unsigned bad = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int id = ms_id(labels, (size_t)b * npx + e, n_max);
        bad += id < 0;
        out[(size_t)b * npx + e] = id < 0 ? 0 : M[id];
    }
    __shared__ unsigned tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&tot, bad);
    __syncthreads();
    if (threadIdx.x == 0 && tot) __hip_atomic_fetch_add(&status[b], (u64)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace unet

using namespace unet;

size_t unet_cell_sums_scratch_bytes(int B, int n_max)
{
    if (B <= 0 || n_max < 0 || n_max > ID_MAX) return 0;
    return (size_t)B * ((size_t)n_max + 1) * MS_WORDS * sizeof(u64);
}

int unet_cell_sums(const void *labels, int label_dtype, const void *image, int image_dtype, int B, int H, int W, int n_max, void *area_i64,
                   void *bbox_i32, void *moments_i64, void *edges_i64, void *vsum_64, void *vrange_32, void *present_u8, void *status_u64,
                   void *scratch, void *stream)
{
    ARG_CHECK(labels && area_i64 && bbox_i32 && moments_i64 && edges_i64 && present_u8 && status_u64 && scratch && B > 0 && H > 0 && W > 0,
              "unet_cell_sums: bad argument");
    ARG_CHECK(label_dtype == 0 || label_dtype == 2, "unet_cell_sums: label dtype must be 0 (int64) or 2 (int32)");
    ARG_CHECK(!image || (image_dtype >= 0 && image_dtype <= 3), "unet_cell_sums: image dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(!image || (vsum_64 && vrange_32), "unet_cell_sums: an image needs vsum_64 and vrange_32");
    ARG_CHECK(measure_sizes_ok(B, H, W, n_max), "unet_cell_sums: H, W must be <= 32768, B <= 65535 and n_max in [0, 2^24)");
    hipStream_t st = (hipStream_t)stream;
    u64 *records = (u64 *)scratch;
    const int kind = !image ? IMG_NONE : image_dtype == 1 ? IMG_FLOAT : IMG_INT;
    const size_t rows = (size_t)B * ((size_t)n_max + 1);
    HIP_TRY(hipMemsetAsync(records, 0, rows * MS_WORDS * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * 2 * sizeof(u64), st));
    const dim3 grid(cdiv(W, MS_TW), cdiv(H, MS_TH), B);
    auto fill = [&](auto kind_c, auto lt) {
        using LT = decltype(lt);
        hipLaunchKernelGGL((ms_fill_kernel<decltype(kind_c)::value, LT>), grid, dim3(256), 0, st, (const LT *)labels, image, image_dtype, H, W,
                           n_max, records, (u64 *)status_u64);
    };
    auto by_label = [&](auto kind_c) {
        if (label_dtype == 0) fill(kind_c, (long long)0); else fill(kind_c, (int)0);
    };
    if (kind == IMG_NONE) by_label(std::integral_constant<int, IMG_NONE>{});
    else if (kind == IMG_INT) by_label(std::integral_constant<int, IMG_INT>{});
    else by_label(std::integral_constant<int, IMG_FLOAT>{});
    hipLaunchKernelGGL(ms_finish_kernel, dim3(grid_for(rows, 256, 4096)), dim3(256), 0, st, (const u64 *)records, rows, kind, (long long *)area_i64,
                       (int *)bbox_i32, (long long *)moments_i64, (long long *)edges_i64, (u64 *)vsum_64, (unsigned *)vrange_32,
                       (unsigned char *)present_u8);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_remap_labels(const void *labels, int label_dtype, int B, int H, int W, const void *map_i32, int n_max, long long map_stride,
                      void *out_i32, void *status_u64, void *stream)
{
    ARG_CHECK(labels && map_i32 && out_i32 && status_u64 && B > 0 && H > 0 && W > 0, "unet_remap_labels: bad argument");
    ARG_CHECK(label_dtype == 0 || label_dtype == 2, "unet_remap_labels: label dtype must be 0 (int64) or 2 (int32)");
    ARG_CHECK(measure_sizes_ok(B, H, W, n_max), "unet_remap_labels: H, W must be <= 32768, B <= 65535 and n_max in [0, 2^24)");
    ARG_CHECK(map_stride == 0 || map_stride >= (long long)n_max + 1, "unet_remap_labels: map_stride must be 0 (one map for the batch) or >= n_max + 1");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * sizeof(u64), st));
    const dim3 grid(grid_for(npx, 256, 4096 / B > 1 ? 4096 / B : 1), B);
    if (label_dtype == 0)
        hipLaunchKernelGGL(ms_remap_kernel<long long>, grid, dim3(256), 0, st, (const long long *)labels, npx, (const int *)map_i32, n_max,
                           (size_t)map_stride, (int *)out_i32, (u64 *)status_u64);
    else
        hipLaunchKernelGGL(ms_remap_kernel<int>, grid, dim3(256), 0, st, (const int *)labels, npx, (const int *)map_i32, n_max, (size_t)map_stride,
                           (int *)out_i32, (u64 *)status_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}
