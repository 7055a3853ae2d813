// elem.hpp — what the HBM-bound kernels (direct.hip, loss.hip, multiclass.hip, dice.hip, tile.hip, aux.hip) and the data-path files (label.hip, wmap.hip,
// prepare.hip, grow.hip, elastic.hip, clean.hip, warp.hip, measure.hip, hull.hip, through ov_table.hpp instances.hip and track.hip,
// through sweep.hpp geo.hip, shape.hip, flood.hip, and through dm.hpp shape.hip and boundary.hip) share:
//   device : 4 consecutive channels of an activation tensor stored as fp32 (16 B) or bf16 (8 B, arithmetic mode 2), read /
//            written as 4 floats; the sum / min / max of one value per lane over a wave; the min and max of one value per thread
//            over a block; the sum of one value per thread over a 256-thread block, with the max of a second one (the finish
//            kernels of geo.hip and flood.hip), and (label.hip, prepare.hip) the
//            exclusive prefix of one int per thread over it; a few counts per thread summed over the workgroup into one
//            agent-scope add per word (label.hip, clean.hip); whether an element of a mask of any of the four dtypes is set;
//            the union-find of the labelling (label.hip) on LDS words and on global words
//   host   : the grid size of a grid-stride launch, the bytes of a [B,H,W] scratch plane, the size and id limits of the [B,H,W] ops,
//            and the dispatch of a launch on element size, channel width and padded class count (the launch bracket,
//            profiled(), is common.hpp's)
#pragma once
#include "common.hpp"
#include <type_traits>

namespace unet {

typedef unsigned short bf16_t;          // storage type of arithmetic mode 2: bf16 bit patterns

// 4 consecutive channels of a tensor stored as T (float: 16 B, bf16: 8 B), as floats
__device__ __forceinline__ f32x4 load4(const float *p) { return *(const f32x4 *)p; }
__device__ __forceinline__ f32x4 load4(const bf16_t *p)
{
    const uint2 w = *(const uint2 *)p;
    return f32x4{__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
                 __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u)};
}
__device__ __forceinline__ void put1(float *p, float v) { *p = v; }
__device__ __forceinline__ void put1(bf16_t *p, float v) { *p = __builtin_bit_cast(bf16_t, (__bf16)v); }
__device__ __forceinline__ void store4(float *p, f32x4 v) { *(f32x4 *)p = v; }
__device__ __forceinline__ void store4(bf16_t *p, f32x4 v)
{
    uint2 w;
    w.x = (unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[0]) | ((unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[1]) << 16);
    w.y = (unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[2]) | ((unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[3]) << 16);
    *(uint2 *)p = w;
}

// 64-lane butterflies: the result is valid in every lane
template <typename V>
__device__ __forceinline__ V wave_sum(V v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ float wave_min(float v) { for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64)); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64)); return v; }

// min and max of one (lo, hi) pair per thread over a block of NW waves: one wave result per wave through LDS, thread 0 combines
// them: only its return value is the block's
struct MinMax { float lo, hi; };
template <int NW>
__device__ __forceinline__ MinMax block_minmax(float lo, float hi)
{
    __shared__ float slo[NW], shi[NW];
    lo = wave_min(lo); hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < NW; ++w) { lo = fminf(lo, slo[w]); hi = fmaxf(hi, shi[w]); }
    return {lo, hi};
}

// Sum of one value per thread over a 256-thread block: LDS tree in the fixed order 128, 64, ... 1 (deterministic); the total is
// valid in thread 0
template <typename V>
__device__ __forceinline__ V block_sum256(V v)
{
    __shared__ V red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
// Sum of `add` and max of `top`, one of each per thread, over a 256-thread block, in place; both are valid in thread 0 (geo.hip's
// and flood.hip's finish kernels)
__device__ __forceinline__ void block_sum_max256(unsigned &add, unsigned &top)
{
    __shared__ unsigned wave_top[4];
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(top, d, 64);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0) wave_top[threadIdx.x >> 6] = top;
    add = block_sum256(add);                                // its barriers order the four words above, too
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) top = wave_top[w] > top ? wave_top[w] : top;
}
// exclusive prefix of v over the 256 threads of the workgroup, and their sum
__device__ __forceinline__ int block_scan256(int v, int &total)
{
    __shared__ int wave_tot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                        // the previous call's reads of wave_tot are done
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < w) before += wave_tot[i];
        total += wave_tot[i];
    }
    return before + inc - v;
}

// n[k], summed over the workgroup, is added to words[k] by one agent-scope add per workgroup and word (none where the sum is 0):
// the adds of a launch meet on a few words per image, so they are reduced in the wave and in LDS first.  Every thread calls it.
template <int N, typename W>
__device__ __forceinline__ void block_counts(W *words, const unsigned (&n)[N])
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

// is element e of a mask non-zero (label.hip, clean.hip, prepare.hip, warp.hip; dtype 0: int64, 1: float32, 2: int32, 3: uint8)
__device__ __forceinline__ int mask_on(const void *mask, int dtype, size_t e)
{
    if (dtype == 0) return ((const long long *)mask)[e] != 0;
    if (dtype == 1) return ((const float *)mask)[e] != 0.0f;
    if (dtype == 2) return ((const int *)mask)[e] != 0;
    return ((const unsigned char *)mask)[e] != 0;
}

// Union-find on a plane of parent words, the smaller index always the parent (label.hip).  lds_*: a tile's words in
// LDS, workgroup scope.  gl_*: the image's words in global memory, where every read and update is an agent-scope atomic
// read-modify-write (per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores).
__device__ __forceinline__ int lds_find(int *lp, int p)
{
    for (;;) {
        const int q = __hip_atomic_load(&lp[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == p) return p;
        p = q;
    }
}
__device__ __forceinline__ void lds_union(int *lp, int a, int b)
{
    for (;;) {
        a = lds_find(lp, a);
        b = lds_find(lp, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        int expect = b;                   // link the larger root under the smaller one, only while it is still a root
        if (__hip_atomic_compare_exchange_strong(&lp[b], &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
            return;
        b = expect;
    }
}
__device__ __forceinline__ int gl_read(int *p) { return __hip_atomic_fetch_or(p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int gl_find(int *P, int p)
{
    for (;;) {
        const int q = gl_read(&P[p]);
        if (q == p) return p;
        p = q;
    }
}
__device__ __forceinline__ void gl_union(int *P, int a, int b)
{
    for (;;) {
        a = gl_find(P, a);
        b = gl_find(P, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        int expect = b;
        if (__hip_atomic_compare_exchange_strong(&P[b], &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        b = expect;
    }
}

static inline int grid_for(size_t total, int per_block = 256, int cap = 8192)
{
    size_t g = (total + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

// workgroups per image of a grid-stride pass that ends in block_counts: about 4096 in all, so that its adds stay few per word
static inline int count_blocks(size_t npx, int B) { return grid_for(npx, 256, 4096 / B > 1 ? 4096 / B : 1); }

// bytes of a [B,H,W] plane of elem_size-byte words inside a scratch buffer, 256-aligned
static inline size_t plane_bytes(int B, int H, int W, size_t elem_size) { return align_up((size_t)B * H * W * elem_size, 256); }

// Size limits of the [B,H,W] ops.  sizes_ok: H, W <= edge (65535: a grid dimension; 32767: H^2 + W^2 is an int32).
// label_sizes_ok: the labelling (label.hip) and what stands on its planes (wmap.hip, clean.hip); W is bounded by H * W alone
static inline bool sizes_ok(int B, int H, int W, int edge) { return (size_t)H * W < (1u << 31) && H <= edge && W <= edge && B <= 65535; }
static inline bool label_sizes_ok(int B, int H, int W) { return (size_t)H * W < (1u << 31) && H <= 65535 && B <= 65535; }

// The ops on instance maps (instances.hip, track.hip, measure.hip, hull.hip) take ids in [0, ID_MAX]: two ids and an image index
// fill a 64-bit key (ov_table.hpp).  The measurement family (measure.hip, hull.hip, unet_cell_contacts) takes H, W <=
// MEASURE_EDGE: every coordinate sum of a cell fits 64 bits
static constexpr int ID_BITS = 24, ID_MAX = (1 << ID_BITS) - 1;
static constexpr int MEASURE_EDGE = 32768;
static inline bool measure_sizes_ok(int B, int H, int W, int n_max)
{
    return H <= MEASURE_EDGE && W <= MEASURE_EDGE && B <= 65535 && n_max >= 0 && n_max <= ID_MAX;
}

// Launch dispatch: f is a generic lambda that receives the storage type as a value of it (es 2: bf16_t, else float), then the
// channel width (32 or 64; the callers have checked it) and for the K-class head KP = class_pad(K) (4, 8 or 16: K = 2 runs the
// head1x1 kernels) as std::integral_constant, so a launch function names its kernel and its arguments once; dispatch_bool does
// the same for one flag (tile.hip: 16-byte aligned or not), as std::bool_constant
template <class F>
static inline void dispatch_bool(bool v, F f)
{
    if (v) f(std::true_type{}); else f(std::false_type{});
}
template <class F>
static inline void dispatch_es(int es, F f)
{
    if (es == 2) f(bf16_t{}); else f(float{});
}
template <class F>
static inline void dispatch_es_width(int es, int width, F f)
{
    dispatch_es(es, [&](auto t) {
        if (width == 64) f(t, std::integral_constant<int, 64>{}); else f(t, std::integral_constant<int, 32>{});
    });
}
template <class F>
static inline void dispatch_es_width_kp(int es, int width, int kp, F f)
{
    dispatch_es_width(es, width, [&](auto t, auto c) {
        if (kp == 4) f(t, c, std::integral_constant<int, 4>{});
        else if (kp == 8) f(t, c, std::integral_constant<int, 8>{});
        else f(t, c, std::integral_constant<int, 16>{});
    });
}

}  // namespace unet
