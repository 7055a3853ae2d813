// dropout.hip — drop-out at the end of the contracting path (Ronneberger et al. 2015, section 3.1: "Drop-out layers at the
// end of the contracting path perform further implicit data augmentation").  The reference left it out (network.py:150-156
// feed conv42c's and conv52c's outputs straight on); Unet(dropout=p) puts it back at the two sites of the authors' network
// definition.  Inverted and in place, y = keep ? x * s : 0 with s = 1 / (1 - p); the keep flags are Philox4x32-10 words of
// (seed, step, site, element index), so no mask is stored and nothing depends on the launch geometry.  HBM-bound kernels:
//   dropout_pool_kernel   forward: one 2x2 window x 4 channels per thread, dropped in place, and (site 0) the 2x2 max-pool
//                         of the dropped values, which replaces the level's pool launch
//   dropout_scale_kernel  backward: g *= s in place (the consumers' ReLU masks read the dropped tensor, where a dropped
//                         element is exactly 0: the drop is already in their masks - DESIGN.md section 4k)
//   dropout_mask_kernel   the keep flags as bytes (tests)
#include "elem.hpp"
#include "philox.hpp"
#include "../../include/unet_hip.h"

namespace unet {

struct DropKey {
    unsigned k0, k1;      // seed
    unsigned c2, c3;      // step, and the site in the top bit of word 3
    unsigned thr;         // keep <=> word >= thr
    float s;              // 1 / (1 - p)
};

static DropKey drop_key(float p, unsigned long long seed, unsigned long long step, int site)
{
    DropKey k;
    k.k0 = (unsigned)(seed & 0xffffffffull); k.k1 = (unsigned)(seed >> 32);
    k.c2 = (unsigned)(step & 0xffffffffull);
    k.c3 = ((unsigned)(step >> 32) & 0x7fffffffu) | ((unsigned)site << 31);
    double t = (double)p * 4294967296.0;
    t = t < 0.0 ? 0.0 : (double)(unsigned long long)t;          // floor
    k.thr = (unsigned)(t < 4294967295.0 ? t : 4294967295.0);
    k.s = 1.0f / (1.0f - p);
    return k;
}

// Philox4x32-10 (philox.hpp) of counter (g, step | site) under key seed: the four words decide the four elements
// 4g .. 4g+3, i.e. four consecutive channels of one pixel
__device__ __forceinline__ u32x4 philox4x32_10(unsigned long long g, const DropKey &k)
{
    return philox4x32_10((unsigned)g, (unsigned)(g >> 32), k.c2, k.c3, k.k0, k.k1);
}

// the four channels at element index idx (a multiple of 4), dropped: one fp32 multiply per kept element
__device__ __forceinline__ f32x4 drop4(f32x4 x, unsigned long long idx, const DropKey &k)
{
    const u32x4 r = philox4x32_10(idx >> 2, k);
    f32x4 y;
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = r.v[c] >= k.thr ? x[c] * k.s : 0.f;
    return y;
}

// x [B,H,W,4*C4] in place; pooled [B,H/2,W/2,4*C4] or null
template <typename T>
__global__ __launch_bounds__(256) void dropout_pool_kernel(T *__restrict__ x, T *__restrict__ pooled, int B, int H, int W, int C4, const DropKey k)
{
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t total = (size_t)B * Ho * Wo * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        size_t pp = e / C4;
        const int ox = (int)(pp % Wo); pp /= Wo;
        const int oy = (int)(pp % Ho);
        const int img = (int)(pp / Ho);
        const size_t o00 = ((((size_t)img * H + 2 * oy) * W + 2 * ox) * C4 + c4) * 4;
        const size_t o01 = o00 + 4 * (size_t)C4, o10 = o00 + (size_t)W * C4 * 4, o11 = o10 + 4 * (size_t)C4;
        const f32x4 v00 = load4(x + o00), v01 = load4(x + o01), v10 = load4(x + o10), v11 = load4(x + o11);
        const f32x4 y00 = drop4(v00, o00, k), y01 = drop4(v01, o01, k), y10 = drop4(v10, o10, k), y11 = drop4(v11, o11, k);
        store4(x + o00, y00); store4(x + o01, y01);
        store4(x + o10, y10); store4(x + o11, y11);
        if (pooled) {
            f32x4 m;
#pragma unroll
            for (int c = 0; c < 4; ++c) m[c] = fmaxf(fmaxf(y00[c], y01[c]), fmaxf(y10[c], y11[c]));
            store4(pooled + e * 4, m);        // bf16: rounding is monotone, so this is the maximum of the four stored values
        }
    }
}

__device__ __forceinline__ float get1(const float *p) { return *p; }
__device__ __forceinline__ float get1(const bf16_t *p) { return __builtin_bit_cast(float, (unsigned)*p << 16); }

// g[0, n) *= s in place: 4 elements per thread, then the (per-op callers' only) tail of n % 4
template <typename T>
__global__ __launch_bounds__(256) void dropout_scale_kernel(T *__restrict__ g, size_t n, float s)
{
    const size_t n4 = n >> 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x) {
        f32x4 v = load4(g + e * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] *= s;
        store4(g + e * 4, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        put1(g + i, get1(g + i) * s);
    }
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char *__restrict__ keep, size_t first, size_t n, const DropKey k)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long idx = (unsigned long long)first + e;
        keep[e] = philox4x32_10(idx >> 2, k).v[idx & 3] >= k.thr ? 1 : 0;
    }
}

static bool drop_p_ok(float p) { return p >= 0.f && p < 1.f; }      // (false for a NaN)

int dropout_pool_fwd(void *x, void *pooled, int B, int H, int W, int C, float p, unsigned long long seed, unsigned long long step,
                     int site, int es, hipStream_t st)
{
    ARG_CHECK(x && B > 0 && H > 0 && W > 0 && C > 0, "dropout_pool_fwd: null or empty tensor");
    ARG_CHECK(H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "dropout_pool_fwd: H,W must be even and C a multiple of 4");
    ARG_CHECK(drop_p_ok(p), "dropout_pool_fwd: p must be in [0, 1), got %g", (double)p);
    ARG_CHECK(site == 0 || site == 1, "dropout_pool_fwd: site must be 0 or 1");
    const size_t total = (size_t)B * (H / 2) * (W / 2) * (C / 4);
    const DropKey k = drop_key(p, seed, step, site);
    return profiled(PK_ELEMWISE, "dropout_pool_fwd", st, 16.0 * (double)total, 0.0, 4.0 * es * (double)total * (pooled ? 9.0 : 8.0), [&] {
        dispatch_es(es, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(dropout_pool_kernel<T>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, st, (T *)x, (T *)pooled, B, H, W, C / 4, k);
        });
    });
}

int dropout_bwd(void *g, size_t n, float p, int es, hipStream_t st)
{
    ARG_CHECK(g || n == 0, "dropout_bwd: null tensor");
    ARG_CHECK(drop_p_ok(p), "dropout_bwd: p must be in [0, 1), got %g", (double)p);
    if (n == 0) return 0;
    const float s = 1.0f / (1.0f - p);
    return profiled(PK_ELEMWISE, "dropout_bwd", st, (double)n, 0.0, 2.0 * es * (double)n, [&] {
        dispatch_es(es, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(dropout_scale_kernel<T>, dim3(grid_for(n / 4, 256, 65536)), dim3(256), 0, st, (T *)g, n, s);
        });
    });
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_dropout_pool_fwd(void *x_inout, void *pooled_or_null, int B, int H, int W, int C, float p, unsigned long long seed,
                          unsigned long long step, int site, void *stream)
{
    ProfScope ps("op.dropout_pool_fwd");
    return dropout_pool_fwd(x_inout, pooled_or_null, B, H, W, C, p, seed, step, site, op_es(), (hipStream_t)stream);
}

int unet_dropout_bwd(void *g_inout, size_t n, float p, void *stream)
{
    ProfScope ps("op.dropout_bwd");
    return dropout_bwd(g_inout, n, p, op_es(), (hipStream_t)stream);
}

int unet_dropout_mask(unsigned long long seed, unsigned long long step, int site, size_t first, size_t n, float p, void *keep_u8,
                      void *stream)
{
    ARG_CHECK(keep_u8 || n == 0, "unet_dropout_mask: null output");
    ARG_CHECK(drop_p_ok(p), "unet_dropout_mask: p must be in [0, 1), got %g", (double)p);
    ARG_CHECK(site == 0 || site == 1, "unet_dropout_mask: site must be 0 or 1");
    if (n == 0) return 0;
    ProfScope ps("op.dropout_mask");
    hipStream_t st = (hipStream_t)stream;
    const DropKey k = drop_key(p, seed, step, site);
    return profiled(PK_ELEMWISE, "dropout_mask", st, 0.0, 0.0, (double)n, [&] {
        hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n, 256, 65536)), dim3(256), 0, st, (unsigned char *)keep_u8, first, n, k);
    });
}

}  // extern "C"
