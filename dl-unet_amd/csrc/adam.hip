// adam.hip — Adam / AdamW and the global gradient norm with its clipping coefficient, as multi-tensor passes over <= 46 tensors
// per call (unet_adam_step, unet_grad_sumsq, unet_grad_norm_finish, unet_grads_scale).  All HBM-bound and laid out like
// sgd_momentum_kernel (direct.hip): a workgroup of 256 threads takes ADAM_CHUNK = 4096 elements of ONE tensor, the grid is
// capped and strides over the chunks; 16 B per lane and access when every pointer of the call is 16-byte aligned and the chunk is
// full, 4 B otherwise (tails, misaligned tensors).  No allocation, no host sync and no floating-point atomics: every sum has one
// fixed order, so a result does not depend on the run or on the stream.  See DESIGN §4w.
//
// unet_adam_step, per element, every operation rounded once to fp32, in this order (the bound of tests/adam_ref.py counts them):
//    1  g = g * c                                   only with grad_scale_dev (c = *grad_scale_dev)
//    2  g = g + wd * p                              decoupled = 0 and wd != 0   (Adam, L2 decay)
//       p = p * decay                               decoupled = 1 and wd != 0   (AdamW; decay = fp32(1 - lr wd), formed on the host)
//    3  m = m + om1 * (g - m)                       om1 = fp32(1 - beta1);  step 1: m = 0 in place of the stored value
//    4  v = beta2 * v + om2 * (g * g)               om2 = fp32(1 - beta2);  step 1: v = 0 in place of the stored value
//    5  d = sqrt(v) * rbc2 + eps                    rbc2 = fp32(1 / sqrt(1 - beta2^step))
//    6  p = p - step_size * (m / d)                 step_size = fp32(lr / (1 - beta1^step))
// The host forms om1, om2, decay, rbc2 and step_size in double from the fp32 arguments and rounds each once.  Subnormals are kept.
//
// Arithmetic: this toolchain's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators compiled where contraction is allowed (an
// add of a product may still become one fused operation after inlining), and its __fsqrt_rn is the native square root (1 ulp).  So
// the file turns contraction off and uses the operators, the IEEE division and __builtin_sqrtf, which hipcc rounds correctly by
// default (-fhip-fp32-correctly-rounded-divide-sqrt); the Makefile passes no fast-math flag.
#include "common.hpp"
#include "elem.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

#pragma clang fp contract(off)

namespace unet {
namespace adam {

constexpr int ADAM_CHUNK = 4096;                    // elements of one tensor per workgroup pass: 256 lanes x 4 accesses x 16 B
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_GRID_CAP = 16384;

// the chunk table every kernel here walks: tensor t owns chunks [cstart[t], cstart[t + 1])
struct ChunkTable { unsigned long long numel[UNET_N_PARAMS]; unsigned cstart[UNET_N_PARAMS + 1]; int n; };
struct AdamTable { float *p[UNET_N_PARAMS]; const float *g[UNET_N_PARAMS]; float *m[UNET_N_PARAMS]; float *v[UNET_N_PARAMS]; ChunkTable ct; };
struct GradTable { float *g[UNET_N_PARAMS]; ChunkTable ct; };
struct AdamK { float step_size, rbc2, beta1, om1, beta2, om2, eps, wd, decay; int decoupled, first; const float *scale; };

// which tensor `chunk` belongs to, the element offset of the chunk inside it and the elements left from there (scalar: chunk is uniform)
__device__ __forceinline__ int locate(const ChunkTable &ct, unsigned chunk, unsigned long long &off, unsigned long long &left)
{
    int t = 0;
    while (ct.cstart[t + 1] <= chunk) ++t;
    off = (unsigned long long)(chunk - ct.cstart[t]) * ADAM_CHUNK;
    left = ct.numel[t] - off;
    return t;
}

__device__ __forceinline__ void adam_elem(float g, float &p, float &m, float &v, const AdamK &k, float c)
{
    if (k.scale) g = g * c;
    if (k.wd != 0.0f) {
        if (k.decoupled) p = p * k.decay;
        else g = g + k.wd * p;
    }
    m = m + k.om1 * (g - m);
    v = k.beta2 * v + k.om2 * (g * g);
    const float d = __builtin_sqrtf(v) * k.rbc2 + k.eps;
    p = p - k.step_size * (m / d);
}

template <bool VEC>
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamTable tb, const AdamK k)
{
    const unsigned nchunks = tb.ct.cstart[tb.ct.n];
    const float c = k.scale ? *k.scale : 1.0f;
    for (unsigned chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        unsigned long long off, left;
        const int t = locate(tb.ct, chunk, off, left);
        float *pp = tb.p[t] + off; const float *gp = tb.g[t] + off; float *mp = tb.m[t] + off; float *vp = tb.v[t] + off;
        if (VEC && left >= ADAM_CHUNK) {
            f32x4 g[4], q[4], m[4], v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = ((const f32x4 *)gp)[i * ADAM_THREADS + threadIdx.x];
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = ((const f32x4 *)pp)[i * ADAM_THREADS + threadIdx.x];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (k.first) { m[i] = f32x4{0.f, 0.f, 0.f, 0.f}; v[i] = m[i]; }
                else { m[i] = ((const f32x4 *)mp)[i * ADAM_THREADS + threadIdx.x]; v[i] = ((const f32x4 *)vp)[i * ADAM_THREADS + threadIdx.x]; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = q[i][e], me = m[i][e], ve = v[i][e];
                    adam_elem(g[i][e], pe, me, ve, k, c);
                    q[i][e] = pe; m[i][e] = me; v[i][e] = ve;
                }
                ((f32x4 *)mp)[i * ADAM_THREADS + threadIdx.x] = m[i];
                ((f32x4 *)vp)[i * ADAM_THREADS + threadIdx.x] = v[i];
                ((f32x4 *)pp)[i * ADAM_THREADS + threadIdx.x] = q[i];
            }
        } else {
            const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
            for (int i = threadIdx.x; i < cnt; i += ADAM_THREADS) {
                float pe = pp[i], me = k.first ? 0.f : mp[i], ve = k.first ? 0.f : vp[i];
                adam_elem(gp[i], pe, me, ve, k, c);
                mp[i] = me; vp[i] = ve; pp[i] = pe;
            }
        }
    }
}

// One fp64 partial per chunk: the squares are exact in fp64 (24 x 24 bits); a lane adds its <= 16 squares in index order, the
// wave adds its lanes in a butterfly, thread 0 the four waves in order.
template <bool VEC>
__global__ __launch_bounds__(ADAM_THREADS) void grad_sumsq_kernel(const GradTable tb, double *__restrict__ partials)
{
    __shared__ double wave_part[ADAM_THREADS / 64];
    const unsigned nchunks = tb.ct.cstart[tb.ct.n];
    for (unsigned chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        unsigned long long off, left;
        const int t = locate(tb.ct, chunk, off, left);
        const float *gp = tb.g[t] + off;
        double s = 0.0;
        if (VEC && left >= ADAM_CHUNK) {
            f32x4 g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = ((const f32x4 *)gp)[i * ADAM_THREADS + threadIdx.x];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double d = (double)g[i][e]; s = s + d * d; }
        } else {
            const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
            for (int i = threadIdx.x; i < cnt; i += ADAM_THREADS) { const double d = (double)gp[i]; s = s + d * d; }
        }
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) partials[chunk] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
        __syncthreads();                                    // wave_part is free for the block's next chunk
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in order, then the fixed tree of block_sum256
__global__ __launch_bounds__(ADAM_THREADS) void grad_norm_finish_kernel(const double *__restrict__ partials, unsigned long long n,
                                                                       float max_norm, float *__restrict__ out2)
{
    double s = 0.0;
    for (unsigned long long i = threadIdx.x; i < n; i += ADAM_THREADS) s = s + partials[i];
    s = block_sum256(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = c > 1.0f ? 1.0f : c;                      // a NaN norm stays a NaN coefficient (torch.clamp(max=1))
    }
}

template <bool VEC>
__global__ __launch_bounds__(ADAM_THREADS) void grads_scale_kernel(const GradTable tb, const float *__restrict__ scale)
{
    const unsigned nchunks = tb.ct.cstart[tb.ct.n];
    const float c = *scale;
    for (unsigned chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        unsigned long long off, left;
        const int t = locate(tb.ct, chunk, off, left);
        float *gp = tb.g[t] + off;
        if (VEC && left >= ADAM_CHUNK) {
            f32x4 g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = ((const f32x4 *)gp)[i * ADAM_THREADS + threadIdx.x];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[i][e] = g[i][e] * c;
                ((f32x4 *)gp)[i * ADAM_THREADS + threadIdx.x] = g[i];
            }
        } else {
            const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
            for (int i = threadIdx.x; i < cnt; i += ADAM_THREADS) gp[i] = gp[i] * c;
        }
    }
}

// fills the chunk table; returns the number of chunks and the total element count
static unsigned fill_chunks(ChunkTable &ct, const size_t *numel, int n, unsigned long long &total)
{
    unsigned chunks = 0;
    total = 0;
    ct.n = n;
    for (int i = 0; i < n; ++i) {
        ct.numel[i] = numel[i];
        ct.cstart[i] = chunks;
        chunks += (unsigned)((numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK);
        total += numel[i];
    }
    ct.cstart[n] = chunks;
    return chunks;
}

static bool fill_grads(GradTable &tb, void *const *grads, int n)
{
    bool vec = true;
    for (int i = 0; i < n; ++i) {
        tb.g[i] = (float *)grads[i];
        if ((uintptr_t)grads[i] & 15) vec = false;
    }
    return vec;
}

}  // namespace adam
}  // namespace unet

using namespace unet;
using namespace unet::adam;

extern "C" {

int unet_adam_step(void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq, const size_t *numel,
                   int n, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, long step,
                   const void *grad_scale_dev, void *stream)
{
    ARG_CHECK(n > 0 && n <= UNET_N_PARAMS, "adam: n=%d out of range (1..%d)", n, UNET_N_PARAMS);
    ARG_CHECK(step >= 1, "adam: step=%ld must be >= 1", step);
    ARG_CHECK(eps > 0.0f, "adam: eps=%g must be positive", (double)eps);
    ARG_CHECK(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f, "adam: betas (%g, %g) must lie in [0, 1)", (double)beta1,
              (double)beta2);
    AdamTable tb;
    unsigned long long total;
    const unsigned chunks = fill_chunks(tb.ct, numel, n, total);
    bool vec = true;
    for (int i = 0; i < n; ++i) {
        tb.p[i] = (float *)params[i]; tb.g[i] = (const float *)grads[i]; tb.m[i] = (float *)exp_avg[i]; tb.v[i] = (float *)exp_avg_sq[i];
        if (((uintptr_t)params[i] | (uintptr_t)grads[i] | (uintptr_t)exp_avg[i] | (uintptr_t)exp_avg_sq[i]) & 15) vec = false;
    }
    if (chunks == 0) return 0;
    AdamK k;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    k.step_size = (float)((double)lr / bc1);
    k.rbc2 = (float)(1.0 / std::sqrt(bc2));
    k.beta1 = beta1; k.om1 = (float)(1.0 - (double)beta1);
    k.beta2 = beta2; k.om2 = (float)(1.0 - (double)beta2);
    k.eps = eps; k.wd = weight_decay;
    k.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    k.decoupled = decoupled != 0; k.first = step == 1;
    k.scale = (const float *)grad_scale_dev;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(chunks, 1, ADAM_GRID_CAP);
    ProfScope ps("L3.adam");
    return profiled(PK_ELEMWISE, "adam_step", st, 12.0 * (double)total, 0.0, 4.0 * (double)total * (k.first ? 5 : 7), [&] {
        dispatch_bool(vec, [&](auto vec) {
            hipLaunchKernelGGL(adam_step_kernel<decltype(vec)::value>, dim3(grid), dim3(ADAM_THREADS), 0, st, tb, k);
        });
    });
}

size_t unet_grad_sumsq_partials(const size_t *numel, int n)
{
    size_t chunks = 0;
    for (int i = 0; i < n; ++i) chunks += (numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return chunks;
}

int unet_grad_sumsq(const void *const *grads, const size_t *numel, int n, void *partials, size_t partial_offset, void *stream)
{
    ARG_CHECK(n > 0 && n <= UNET_N_PARAMS, "grad_sumsq: n=%d out of range (1..%d)", n, UNET_N_PARAMS);
    GradTable tb;
    unsigned long long total;
    const unsigned chunks = fill_chunks(tb.ct, numel, n, total);
    const bool vec = fill_grads(tb, (void *const *)grads, n);
    if (chunks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(chunks, 1, ADAM_GRID_CAP);
    double *out = (double *)partials + partial_offset;
    ProfScope ps("L3.clip");
    return profiled(PK_ELEMWISE, "grad_sumsq", st, 2.0 * (double)total, 0.0, 4.0 * (double)total + 8.0 * chunks, [&] {
        dispatch_bool(vec, [&](auto vec) {
            hipLaunchKernelGGL(grad_sumsq_kernel<decltype(vec)::value>, dim3(grid), dim3(ADAM_THREADS), 0, st, tb, out);
        });
    });
}

int unet_grad_norm_finish(const void *partials, size_t n_partials, float max_norm, void *out2, void *stream)
{
    ARG_CHECK(max_norm > 0.0f, "grad_norm_finish: max_norm=%g must be positive", (double)max_norm);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("L3.clip");
    return profiled(PK_ELEMWISE, "grad_norm_finish", st, (double)n_partials, 0.0, 8.0 * (double)n_partials + 8.0, [&] {
        hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, (const double *)partials,
                           (unsigned long long)n_partials, max_norm, (float *)out2);
    });
}

int unet_grads_scale(void *const *grads, const size_t *numel, int n, const void *scale_dev, void *stream)
{
    ARG_CHECK(n > 0 && n <= UNET_N_PARAMS, "grads_scale: n=%d out of range (1..%d)", n, UNET_N_PARAMS);
    ARG_CHECK(scale_dev != nullptr, "grads_scale: scale_dev is NULL");
    GradTable tb;
    unsigned long long total;
    const unsigned chunks = fill_chunks(tb.ct, numel, n, total);
    const bool vec = fill_grads(tb, grads, n);
    if (chunks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(chunks, 1, ADAM_GRID_CAP);
    ProfScope ps("L3.clip");
    return profiled(PK_ELEMWISE, "grads_scale", st, (double)total, 0.0, 8.0 * (double)total, [&] {
        dispatch_bool(vec, [&](auto vec) {
            hipLaunchKernelGGL(grads_scale_kernel<decltype(vec)::value>, dim3(grid), dim3(ADAM_THREADS), 0, st, tb, (const float *)scale_dev);
        });
    });
}

}  // extern "C"
