// grey.hip — grey-value variation of training samples (Ronneberger et al. 2015, section 3.1: "robustness to ... gray value
// variations"): per sample contrast about its own mean and brightness, gamma (or its mirror image), Gaussian
// sensor noise and the final clip, optionally behind the [0,1] normalisation of unet_normalise01, in one pass over the pixels.
//   grey_sum_kernel      fp64 partial sums of the (normalised) pixels of the samples whose affine stage runs: a fixed number of
//                        workgroups per sample, one partial each, no atomics
//   grey_apply_kernel    every stage; a workgroup adds its sample's partials itself, in index order, so every workgroup of a
//                        sample holds the same mean
//   grey_normals_kernel  the standard normals alone (tests)
// The definition is stated at unet_grey_vary in include/unet_hip.h.  All arithmetic after the fp32 normalisation is fp64,
// narrowed once at the store, so that the tests get a bound that can be derived; the price is measured in DESIGN §4x (the fp64
// pow, log and sincos make the apply kernel VALU-bound: about 10 us per Mpixel, tens of microseconds per batch).  Contraction
// is off so that the affine stage is the three roundings the definition writes.
// HBM-bound family: 256 threads, four pixels (one Philox counter) per thread, 16-byte accesses when the sample's first pixel is
// 16-byte aligned in x and in out (else four 4-byte ones), the n % 4 last pixels by the first workgroup, grid-stride, 64-bit offsets.
#include "elem.hpp"
#include "philox.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

#pragma clang fp contract(off)

namespace unet {
namespace grey {

constexpr int GV_MAX = UNET_GREY_MAX_SAMPLES;
constexpr int GV_PARTS = 64;                        // partial sums per sample at the most
constexpr unsigned GV_KEY = 0x47524559u;            // "GREY": XOR-ed into the high key word, so drop-out's stream of a seed is another
enum { GM_AFFINE = 1, GM_GAMMA = 2, GM_INVERT = 4, GM_NOISE = 8 };      // the stages a sample runs

struct GreyArgs {
    double gamma[GV_MAX], contrast[GV_MAX], brightness[GV_MAX], sigma[GV_MAX];
    unsigned char mode[GV_MAX];
    unsigned k0, k1, c2, c3;      // key: seed, counter words 2 and 3: step
    unsigned first;               // global index of sample 0 of this call (counter word 1)
    int clip;
};

// one sample as its workgroups see it
struct Sample {
    double gamma, contrast, brightness, sigma, mean;
    float lo, range;
    int mode, clip, norm;
};

// workgroups (= partials) per sample of the sum pass: a function of n alone, so a chunked call sums in the order of one call
static inline int grey_parts(size_t n) { return grid_for((n + 3) / 4, 256, GV_PARTS); }

__device__ __forceinline__ double clamp01(double u) { return u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u); }      // a NaN stays a NaN

// unet_normalise01's arithmetic: fp32, true division
__device__ __forceinline__ float norm01(float v, const Sample &s) { return s.norm ? (v - s.lo) / s.range : v; }

// the two standard normals of a pair of words (Box-Muller; u1 > 0, so log is finite)
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, double &zc, double &zs)
{
    const double u1 = ((double)wa + 0.5) * 0x1p-32, u2 = ((double)wb + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
    double s, c;
    sincos(t, &s, &c);                               // one argument reduction for both
    zc = r * c;
    zs = r * s;
}

// z of pixels 4g .. 4g+3 of global sample `sample`
__device__ __forceinline__ void normals4(unsigned g, unsigned sample, unsigned c2, unsigned c3, unsigned k0, unsigned k1, double (&z)[4])
{
    const u32x4 r = philox4x32_10(g, sample, c2, c3, k0, k1);
    box_muller(r.v[0], r.v[1], z[0], z[1]);
    box_muller(r.v[2], r.v[3], z[2], z[3]);
}

__device__ __forceinline__ float grey_one(float xv, double z, const Sample &s)
{
    double u = (double)norm01(xv, s);
    if (s.mode & GM_AFFINE) u = clamp01((u - s.mean) * s.contrast + s.mean + s.brightness);
    if (s.mode & GM_GAMMA) u = (s.mode & GM_INVERT) ? 1.0 - pow(1.0 - u, s.gamma) : pow(u, s.gamma);
    if (s.mode & GM_NOISE) u = u + s.sigma * z;
    if (s.clip) u = clamp01(u);
    return (float)u;
}

__device__ __forceinline__ void load_norm(Sample &s, const float *minmax, int b)
{
    s.norm = minmax != nullptr;
    s.lo = 0.f; s.range = 1.f;
    if (minmax) { s.lo = minmax[2 * b]; s.range = minmax[2 * b + 1] - s.lo; }
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// four pixels of a sample from pixel 4g on
__device__ __forceinline__ void load_quad(const float *p, bool vec, float (&v)[4])
{
    if (vec) {
        const f32x4 q = load4(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = p[c];
    }
}

// parts [B][gridDim.x]: workgroup k's sum of sample b's normalised pixels; grid (grey_parts(n), B)
__global__ __launch_bounds__(256) void grey_sum_kernel(const float *__restrict__ x, size_t n, const float *__restrict__ minmax,
                                                        double *__restrict__ parts, const GreyArgs a)
{
    const int b = blockIdx.y;
    if (!(a.mode[b] & GM_AFFINE)) return;               // (the whole workgroup)
    Sample s;
    load_norm(s, minmax, b);
    const float *xs = x + (size_t)b * n;
    const bool vec = aligned16(xs);
    const size_t n4 = n >> 2;
    double acc = 0.0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (size_t)gridDim.x * blockDim.x) {
        float v[4];
        load_quad(xs + 4 * g, vec, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc += (double)norm01(v[c], s);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc += (double)norm01(xs[4 * n4 + threadIdx.x], s);
    acc = block_sum256(acc);
    if (threadIdx.x == 0) parts[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// x, out [B][n] (out == x: in place); grid (chunks of n, B)
__global__ __launch_bounds__(256) void grey_apply_kernel(const float *x, float *out, size_t n, const float *__restrict__ minmax,
                                                          const double *__restrict__ parts, int P, const GreyArgs a)
{
    const int b = blockIdx.y;
    Sample s;
    s.gamma = a.gamma[b]; s.contrast = a.contrast[b]; s.brightness = a.brightness[b]; s.sigma = a.sigma[b];
    s.mode = a.mode[b]; s.clip = a.clip; s.mean = 0.0;
    load_norm(s, minmax, b);
    if (s.mode & GM_AFFINE) {
        double t = 0.0;
        for (int k = 0; k < P; ++k) t += parts[(size_t)b * P + k];
        s.mean = t / (double)n;
    }
    const float *xs = x + (size_t)b * n;
    float *os = out + (size_t)b * n;
    const bool vec = aligned16(xs) && aligned16(os);
    const bool noise = (s.mode & GM_NOISE) != 0;
    const unsigned sample = a.first + (unsigned)b;
    const size_t n4 = n >> 2;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (size_t)gridDim.x * blockDim.x) {
        float v[4];
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        load_quad(xs + 4 * g, vec, v);
        if (noise) normals4((unsigned)g, sample, a.c2, a.c3, a.k0, a.k1, z);
        f32x4 y;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = grey_one(v[c], z[c], s);
        if (vec) {
            store4(os + 4 * g, y);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) os[4 * g + c] = y[c];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        if (noise) normals4((unsigned)n4, sample, a.c2, a.c3, a.k0, a.k1, z);
        const size_t i = 4 * n4 + threadIdx.x;
        os[i] = grey_one(xs[i], z[threadIdx.x], s);
    }
}

__global__ __launch_bounds__(256) void grey_normals_kernel(double *__restrict__ out, size_t first, size_t n, unsigned sample, unsigned c2,
                                                            unsigned c3, unsigned k0, unsigned k1)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = first + e;
        double z[4];
        normals4((unsigned)(i >> 2), sample, c2, c3, k0, k1, z);
        out[e] = z[i & 3];
    }
}

static void grey_key(GreyArgs &a, unsigned long long seed, unsigned long long step)
{
    a.k0 = (unsigned)(seed & 0xffffffffull); a.k1 = (unsigned)(seed >> 32) ^ GV_KEY;
    a.c2 = (unsigned)(step & 0xffffffffull); a.c3 = (unsigned)(step >> 32);
}

// the limits of the counter: pixel groups and sample indices are 32-bit words
static bool pixels_ok(size_t n) { return n >= 1 && n <= LIMIT_31BIT; }

}  // namespace grey
}  // namespace unet

using namespace unet;
using namespace unet::grey;

extern "C" {

size_t unet_grey_scratch_bytes(int B, size_t n)
{
    if (B < 1 || B > GV_MAX || !pixels_ok(n)) return 0;
    return align_up((size_t)B * grey_parts(n) * sizeof(double), 256);
}

int unet_grey_vary(const void *x, void *out, int B, size_t n, long long first_sample, const double *params_host, const void *minmax_or_null,
                   unsigned long long seed, unsigned long long step, int flags, void *scratch, void *stream)
{
    ARG_CHECK(x && out && params_host, "unet_grey_vary: null argument (x, out or params_host)");
    ARG_CHECK(B >= 1 && B <= GV_MAX, "unet_grey_vary: B = %d, need 1 <= B <= %d samples per call", B, GV_MAX);
    ARG_CHECK(pixels_ok(n), "unet_grey_vary: n = %zu pixels per sample, need 1 <= n < 2^31", n);
    ARG_CHECK(first_sample >= 0 && first_sample + B <= 0x100000000ll, "unet_grey_vary: first_sample = %lld, the sample index is a 32-bit word",
              first_sample);
    ARG_CHECK((flags & ~UNET_GREY_NO_CLIP) == 0, "unet_grey_vary: unknown flag bits 0x%x", flags & ~UNET_GREY_NO_CLIP);
    ARG_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)minmax_or_null & 3) == 0 && ((uintptr_t)scratch & 7) == 0,
              "unet_grey_vary: misaligned pointer (x, out, minmax: 4 bytes; scratch: 8)");
    GreyArgs a = {};
    bool any_mean = false;
    for (int b = 0; b < B; ++b) {
        const double *p = params_host + 5 * b;
        for (int k = 0; k < 5; ++k) ARG_CHECK(std::isfinite(p[k]), "unet_grey_vary: parameter %d of sample %d is not finite", k, b);
        ARG_CHECK(p[0] > 0.0, "unet_grey_vary: gamma = %g of sample %d, need gamma > 0", p[0], b);
        ARG_CHECK(p[1] >= 0.0, "unet_grey_vary: contrast = %g of sample %d, need contrast >= 0", p[1], b);
        ARG_CHECK(p[3] >= 0.0, "unet_grey_vary: sigma = %g of sample %d, need sigma >= 0", p[3], b);
        ARG_CHECK(p[4] == 0.0 || p[4] == 1.0, "unet_grey_vary: invert = %g of sample %d, need 0 or 1", p[4], b);
        a.gamma[b] = p[0]; a.contrast[b] = p[1]; a.brightness[b] = p[2]; a.sigma[b] = p[3];
        int mode = 0;
        if (p[1] != 1.0 || p[2] != 0.0) mode |= GM_AFFINE;
        if (p[0] != 1.0) mode |= GM_GAMMA | (p[4] != 0.0 ? GM_INVERT : 0);
        if (p[3] != 0.0) mode |= GM_NOISE;
        a.mode[b] = (unsigned char)mode;
        any_mean |= (mode & GM_AFFINE) != 0;
    }
    ARG_CHECK(scratch || !any_mean, "unet_grey_vary: null scratch (the sample mean needs unet_grey_scratch_bytes(B, n) bytes)");
    grey_key(a, seed, step);
    a.first = (unsigned)first_sample;
    a.clip = (flags & UNET_GREY_NO_CLIP) ? 0 : 1;
    hipStream_t st = (hipStream_t)stream;
    const int P = grey_parts(n);
    const double px = (double)B * (double)n;
    ProfScope ps("N1.grey_vary");
    return profiled(PK_ELEMWISE, "grey_vary", st, 0.0, 0.0, (any_mean ? 12.0 : 8.0) * px, [&] {
        if (any_mean)
            hipLaunchKernelGGL(grey_sum_kernel, dim3(P, B), dim3(256), 0, st, (const float *)x, n, (const float *)minmax_or_null, (double *)scratch, a);
        hipLaunchKernelGGL(grey_apply_kernel, dim3(grid_for((n + 3) / 4, 256, 1024), B), dim3(256), 0, st, (const float *)x, (float *)out, n,
                           (const float *)minmax_or_null, (const double *)scratch, P, a);
    });
}

int unet_grey_normals(unsigned long long seed, unsigned long long step, long long sample, size_t first, size_t n, void *out_f64, void *stream)
{
    ARG_CHECK(out_f64 || n == 0, "unet_grey_normals: null output");
    ARG_CHECK(sample >= 0 && sample < 0x100000000ll, "unet_grey_normals: sample = %lld, the sample index is a 32-bit word", sample);
    ARG_CHECK(first <= LIMIT_31BIT && n <= LIMIT_31BIT && first + n <= LIMIT_31BIT, "unet_grey_normals: pixels [%zu, %zu + %zu) lie past 2^31", first, first, n);
    ARG_CHECK(((uintptr_t)out_f64 & 7) == 0, "unet_grey_normals: misaligned output");
    if (n == 0) return 0;
    GreyArgs a = {};
    grey_key(a, seed, step);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("op.grey_normals");
    return profiled(PK_ELEMWISE, "grey_normals", st, 0.0, 0.0, 8.0 * (double)n, [&] {
        hipLaunchKernelGGL(grey_normals_kernel, dim3(grid_for(n, 256, 65536)), dim3(256), 0, st, (double *)out_f64, first, n, (unsigned)sample,
                           a.c2, a.c3, a.k0, a.k1);
    });
}

}  // extern "C"
