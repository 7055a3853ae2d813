// loss.hip — the step side of the net (the back end of N2), 2 and K classes (2 <= K <= 16) side by side,
// all HBM-bound: BCE-with-logits alone and fused with the argmax mask, one-hot; the soft-max cross-entropy step (Ronneberger et
// al. 2015, eq. 1: loss, gradient, argmax mask, one pass); argmax of a strided view; crop + argmax + metric / confusion counts.
// The K-class kernels are templated on KP = class_pad(K), the true K is a runtime bound.  Dice: dice.hip.  See DESIGN §4f.
#include "common.hpp"
#include "elem.hpp"
#include "softmax.hpp"
#include "../../include/unet_hip.h"

namespace unet {

// ---- 2 classes: BCE-with-logits (L1) -----------------------------------------------------------------------------------------
constexpr int BCE_PER_BLOCK = 4096;
__global__ __launch_bounds__(256) void bce_logits_kernel(const float *__restrict__ x, const float *__restrict__ z,
                                                         const float *__restrict__ w, long wsB, long wsC, long wsH, long wsW,
                                                         int H, int W, size_t n, float *__restrict__ dx, float gscale,
                                                         double *__restrict__ partial)
{
    const size_t b0 = (size_t)blockIdx.x * BCE_PER_BLOCK;
    double acc = 0.0;
    const float inv_n = (float)(1.0 / (double)n);
    for (int i = threadIdx.x; i < BCE_PER_BLOCK; i += 256) {
        const size_t e = b0 + i;
        if (e >= n) break;
        const float xv = x[e], zv = z[e];
        float wv = 1.f;
        if (w) {
            size_t r = e;
            const int xx = (int)(r % W); r /= W;
            const int yy = (int)(r % H); r /= H;
            const int cc = (int)(r % 2);
            const long bb = (long)(r / 2);
            wv = w[bb * wsB + cc * wsC + yy * wsH + xx * wsW];
        }
        const float ax = fabsf(xv);
        const float l = fmaxf(xv, 0.f) - xv * zv + log1pf(expf(-ax));
        acc += (double)(wv * l);
        if (dx) {
            const float ex = expf(-ax);
            const float sg = xv >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
            dx[e] = wv * (sg - zv) * inv_n * gscale;
        }
    }
    acc = block_sum256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void bce_final_kernel(const double *__restrict__ partial, int nb, size_t n, float *loss)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) a += partial[i];
    a = block_sum256(a);
    if (threadIdx.x == 0) *loss = (float)(a / (double)n);
}

// L1 + L2 in one pass over the logits (trainer.py:60-82): the one-hot target [1-y, y] is never materialised, the loss
// gradient and the argmax mask come out of the same read.  A thread owns a pixel (both class planes): 2 x 4 B logits + 8 B
// label in, 2 x 4 B dlogits + 8 B mask out.  Logits / weight are addressed through strides (the trainer's centre crop of
// preds is a view); dlogits and the mask are dense.  Loss partials per block in double, fixed-order finish in bce_final_kernel.
constexpr int BCE_PX_PER_BLOCK = 2048;
__global__ __launch_bounds__(256) void bce_step_kernel(const float *__restrict__ x, long xsB, long xsC, long xsH,
                                                       const long long *__restrict__ labels,
                                                       const float *__restrict__ w, long wsB, long wsC, long wsH, long wsW,
                                                       int H, int W, size_t npix, float *__restrict__ dx, float gscale,
                                                       long long *__restrict__ mask, double *__restrict__ partial)
{
    const size_t b0 = (size_t)blockIdx.x * BCE_PX_PER_BLOCK;
    double acc = 0.0;
    const float inv_n = (float)(1.0 / (double)(2 * npix));
    const size_t HW = (size_t)H * W;
    for (int i = threadIdx.x; i < BCE_PX_PER_BLOCK; i += 256) {
        const size_t e = b0 + i;
        if (e >= npix) break;
        const size_t bb = e / HW, rem = e - bb * HW;
        const int yy = (int)(rem / W), xx = (int)(rem - (size_t)yy * W);
        const float *px = x + bb * xsB + (long)yy * xsH + xx;
        const float x0 = px[0], x1 = px[xsC];
        const float y = (float)labels[e];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float xv = c ? x1 : x0, zv = c ? y : 1.f - y;
            const float wv = w ? w[bb * wsB + c * wsC + yy * wsH + xx * wsW] : 1.f;
            const float ax = fabsf(xv);
            const float ex = expf(-ax);
            const float l = fmaxf(xv, 0.f) - xv * zv + log1pf(ex);
            acc += (double)(wv * l);
            if (dx) {
                const float sg = xv >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
                dx[(bb * 2 + c) * HW + rem] = wv * (sg - zv) * inv_n * gscale;
            }
        }
        if (mask) mask[e] = x1 > x0 ? 1 : 0;              // first maximum wins on ties -> class 0
    }
    acc = block_sum256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void onehot2_kernel(const long long *__restrict__ labels, float *__restrict__ t, int B, size_t HW)
{
    const size_t total = (size_t)B * HW;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t img = e / HW, rem = e - img * HW;
        const float y = (float)labels[e];
        t[(img * 2) * HW + rem] = 1.f - y;
        t[(img * 2 + 1) * HW + rem] = y;
    }
}

// ---- 2 classes: argmax (L2) and the back end of the test step ----------------------------------------------------------------
__global__ void argmax2_kernel(const float *__restrict__ x, long bs, long ps, long rs, long long *__restrict__ out,
                               int B, int H, int W)
{
    const size_t total = (size_t)B * H * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t r = e;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H);
        const long b = (long)(r / H);
        const float *p = x + b * bs + yy * rs + xx;
        out[e] = p[ps] > p[0] ? 1 : 0;            // first maximum wins on ties -> class 0
    }
}

// crop + argmax + metric counts: stats[b] = {sum(pred&label), sum(pred|label), sum|pred-label|} (tester.py:29-42, functions.py:174-213)
__global__ __launch_bounds__(256) void eval_masks_kernel(const float *__restrict__ logits, long bs, long ps, long rs, int pad,
                                                         const long long *__restrict__ labels, long long *__restrict__ mask,
                                                         int n, unsigned long long *__restrict__ stats)
{
    const int b = blockIdx.y;
    const size_t npx = (size_t)n * n;
    unsigned long long inter = 0, uni = 0, diff = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int xx = (int)(e % n), yy = (int)(e / n);
        const float *p = logits + b * bs + (size_t)(yy + pad) * rs + xx + pad;
        const long long pr = p[ps] > p[0] ? 1 : 0;                       // first maximum on ties -> class 0
        mask[(size_t)b * npx + e] = pr;
        if (labels) {
            const long long lb = labels[(size_t)b * npx + e];
            inter += (pr != 0 && lb != 0); uni += (pr != 0 || lb != 0);
            diff += (unsigned long long)(pr > lb ? pr - lb : lb - pr);
        }
    }
    if (!labels) return;
    inter = wave_sum(inter); uni = wave_sum(uni); diff = wave_sum(diff);
    if ((threadIdx.x & 63) == 0) {       // integer atomics: order-independent, exact
        atomicAdd(&stats[3 * b], inter); atomicAdd(&stats[3 * b + 1], uni); atomicAdd(&stats[3 * b + 2], diff);
    }
}

namespace mc {

// ---- K classes: softmax cross-entropy step (eq. 1): a thread owns a pixel (all K planes) ---------------------------------------
// loss_px = w * (logsumexp(l) - l_label) formed as (m - l_label) + log(sum exp(l - m)), m = max l: both terms >= 0, so the
// per-pixel value keeps full relative precision.  Partials per block in double, fixed-order finish.
constexpr int CE_PX_PER_BLOCK = 2048;
template <int KP>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float *__restrict__ x, long xsB, long xsC, long xsH,
                                                         const long long *__restrict__ labels, const float *__restrict__ w,
                                                         long wsB, long wsH, long wsW, int K, int H, int W, size_t npix,
                                                         float *__restrict__ dx, float gscale, long long *__restrict__ mask,
                                                         double *__restrict__ partial, unsigned long long *__restrict__ bad_partial)
{
    const size_t b0 = (size_t)blockIdx.x * CE_PX_PER_BLOCK;
    double acc = 0.0;
    unsigned bad = 0;
    const float inv_n = (float)(1.0 / (double)npix);
    const unsigned HW = (unsigned)H * (unsigned)W;         // < 2^31 (checked on the host)
    // (image, pixel-in-image) of this thread's first pixel by one 64-bit division, then stepped by 256 pixels per trip
    size_t bb = (b0 + threadIdx.x) / HW;
    unsigned rem = (unsigned)(b0 + threadIdx.x - bb * HW);
    for (int i = threadIdx.x; i < CE_PX_PER_BLOCK; i += 256) {
        const size_t e = b0 + i;
        if (e >= npix) break;
        const int yy = (int)(rem / (unsigned)W), xx = (int)(rem - (unsigned)yy * W);
        // softmax.hpp's pixel_exps, inline: through the shared functions this kernel held 47 / 73 VGPRs at KP = 8 / 16 for 42 / 59
        const float *px = x + bb * xsB + (long)yy * xsH + xx;
        float l[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) l[k] = k < K ? px[k * xsC] : 0.f;
        float m = l[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K && l[k] > m) { m = l[k]; am = k; }      // first maximum: torch.argmax's tie rule
        const long long lab = labels[e];
        const bool ok = lab >= 0 && lab < (long long)K;
        float se = 0.f, ll = m, ex[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            ex[k] = k < K ? expf(l[k] - m) : 0.f;
            se += ex[k];
            if (k == lab) ll = l[k];
        }
        const float wv = w ? w[bb * wsB + (long)yy * wsH + (long)xx * wsW] : 1.f;
        if (ok) acc += (double)wv * ((double)(m - ll) + (double)logf(se));
        else ++bad;
        if (dx) {
            const float inv_se = 1.f / se;
            const float sc = ok ? wv * inv_n * gscale : 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) dx[(bb * K + k) * HW + rem] = sc * (ex[k] * inv_se - (k == lab ? 1.f : 0.f));
        }
        if (mask) mask[e] = am;
        rem += 256;
        while (rem >= HW) { rem -= HW; ++bb; }
    }
    __shared__ double red[256];            // one tree for both values: with one block_sum256 per value, here and in the finisher, the step took 1.6 us longer
    __shared__ unsigned redb[256];
    red[threadIdx.x] = acc;
    redb[threadIdx.x] = bad;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < s2) { red[threadIdx.x] += red[threadIdx.x + s2]; redb[threadIdx.x] += redb[threadIdx.x + s2]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[blockIdx.x] = red[0]; bad_partial[blockIdx.x] = redb[0]; }
}

__global__ __launch_bounds__(256) void softmax_ce_final_kernel(const double *__restrict__ partial, const unsigned long long *__restrict__ bad_partial,
                                                               int nb, size_t n, float *loss, unsigned long long *invalid)
{
    __shared__ double red[256];
    __shared__ unsigned long long redb[256];
    double a = 0.0;
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += partial[i]; c += bad_partial[i]; }
    red[threadIdx.x] = a;
    redb[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { red[threadIdx.x] += red[threadIdx.x + s]; redb[threadIdx.x] += redb[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *loss = (float)(red[0] / (double)n);
        if (invalid) *invalid = redb[0];
    }
}

// ---- K classes: argmax of a strided view --------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void argmaxk_kernel(const float *__restrict__ x, long bs, long ps, long rs, int K,
                                                      long long *__restrict__ out, int H, int W, size_t total)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t r = e;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H);
        const long b = (long)(r / H);
        const float *p = x + b * bs + yy * rs + xx;
        float m = p[0];                   // its own first-maximum loop: on softmax.hpp's first_max it took 0.3 us longer at K = 5 and 16
        int am = 0;
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K) { const float v = p[k * ps]; if (v > m) { m = v; am = k; } }
        out[e] = am;
    }
}

// ---- K classes: crop + argmax + confusion counts: conf[b][label][pred], labels outside [0, K) go to invalid[b] -----------------
// Per block an LDS histogram (32-bit, a block sees < 2^32 pixels), then one integer atomic per nonzero bin: exact, deterministic.
template <int KP>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const float *__restrict__ logits, long bs, long ps, long rs, int pad, int K,
                                                             const long long *__restrict__ labels, long long *__restrict__ mask, int n,
                                                             unsigned long long *__restrict__ conf, unsigned long long *__restrict__ invalid)
{
    __shared__ unsigned hist[KP * KP + 1];
    const int b = blockIdx.y;
    const size_t npx = (size_t)n * n;
    if (labels) {
        for (int i = threadIdx.x; i < KP * KP + 1; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int xx = (int)(e % n), yy = (int)(e / n);
        const float *p = logits + b * bs + (size_t)(yy + pad) * rs + xx + pad;
        int am;
        first_max<KP>([&](int k) { return p[k * ps]; }, K, am);
        mask[(size_t)b * npx + e] = am;
        if (labels) {
            const long long lb = labels[(size_t)b * npx + e];
            const int bin = (lb >= 0 && lb < (long long)K) ? (int)lb * K + am : KP * KP;
            atomicAdd(&hist[bin], 1u);
        }
    }
    if (!labels) return;
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += blockDim.x)
        if (hist[i]) atomicAdd(&conf[(size_t)b * K * K + i], (unsigned long long)hist[i]);
    if (threadIdx.x == 0 && hist[KP * KP]) atomicAdd(&invalid[b], (unsigned long long)hist[KP * KP]);
}

}  // namespace mc
}  // namespace unet

using namespace unet;
using namespace unet::mc;

extern "C" {

size_t unet_bce_scratch_bytes(size_t numel) { return ((numel + BCE_PER_BLOCK - 1) / BCE_PER_BLOCK) * sizeof(double); }
int unet_bce_logits(const void *logits, const void *target, const void *weight, long wsB, long wsC, long wsH, long wsW,
                    int B, int H, int W, void *loss_out, void *dlogits, float grad_scale, void *scratch, void *stream)
{
    const size_t n = (size_t)B * 2 * H * W;
    ARG_CHECK(n > 0 && loss_out && scratch, "bce: bad arguments");
    const int nb = (int)((n + BCE_PER_BLOCK - 1) / BCE_PER_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("L1.bce");
    return profiled(PK_ELEMWISE, "bce_logits", st, 0.0, 0.0, 4.0 * (double)n * (2 + (weight ? 1 : 0) + (dlogits ? 1 : 0)), [&] {
        hipLaunchKernelGGL(bce_logits_kernel, dim3(nb), dim3(256), 0, st, (const float *)logits, (const float *)target, (const float *)weight,
                           wsB, wsC, wsH, wsW, H, W, n, (float *)dlogits, grad_scale, (double *)scratch);
        hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, st, (const double *)scratch, nb, n, (float *)loss_out);
    });
}
size_t unet_bce_step_scratch_bytes(size_t npix) { return ((npix + BCE_PX_PER_BLOCK - 1) / BCE_PX_PER_BLOCK) * sizeof(double); }
int unet_bce_step(const void *logits, long xsB, long xsC, long xsH, const void *labels_i64, const void *weight, long wsB, long wsC,
                  long wsH, long wsW, int B, int H, int W, void *loss_out, void *dlogits, float grad_scale, void *mask_i64, void *scratch,
                  void *stream)
{
    const size_t npix = (size_t)B * H * W;
    ARG_CHECK(npix > 0 && logits && labels_i64 && loss_out && scratch, "bce_step: bad arguments");
    const int nb = (int)((npix + BCE_PX_PER_BLOCK - 1) / BCE_PX_PER_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("L1.bce+L2.argmax");
    // logits 8 B + label 8 B in, dlogits 8 B + mask 8 B out per pixel
    return profiled(PK_ELEMWISE, "bce_step", st, 24.0 * npix, 0.0,
                    (double)npix * (16.0 + (dlogits ? 8.0 : 0.0) + (mask_i64 ? 8.0 : 0.0) + (weight ? 8.0 : 0.0)), [&] {
        hipLaunchKernelGGL(bce_step_kernel, dim3(nb), dim3(256), 0, st, (const float *)logits, xsB, xsC, xsH, (const long long *)labels_i64,
                           (const float *)weight, wsB, wsC, wsH, wsW, H, W, npix, (float *)dlogits, grad_scale, (long long *)mask_i64, (double *)scratch);
        hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, st, (const double *)scratch, nb, 2 * npix, (float *)loss_out);
    });
}

int unet_onehot2(const void *labels_i64, void *target, int B, int H, int W, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("L1.onehot");
    return profiled(PK_ELEMWISE, "onehot2", st, 0.0, 0.0, 16.0 * (double)B * H * W, [&] {
        hipLaunchKernelGGL(onehot2_kernel, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, (const long long *)labels_i64, (float *)target, B, (size_t)H * W);
    });
}
int unet_argmax2(const void *logits, long batch_stride, long plane_stride, long row_stride, void *out_i64, int B, int H, int W, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("L2.argmax");
    return profiled(PK_ELEMWISE, "argmax2", st, 0.0, 0.0, 16.0 * (double)B * H * W, [&] {
        hipLaunchKernelGGL(argmax2_kernel, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, (const float *)logits, batch_stride, plane_stride, row_stride, (long long *)out_i64, B, H, W);
    });
}

int unet_eval_masks(const void *logits, long batch_stride, long plane_stride, long row_stride, int pad, const void *labels_i64,
                    void *mask_i64, int B, int n, void *stats_u64, void *stream)
{
    ARG_CHECK(logits && mask_i64 && B > 0 && n > 0 && pad >= 0, "unet_eval_masks: bad argument");
    ARG_CHECK(!labels_i64 || stats_u64, "unet_eval_masks: stats buffer needed with labels");
    hipStream_t st = (hipStream_t)stream;
    if (labels_i64) HIP_TRY(hipMemsetAsync(stats_u64, 0, (size_t)B * 3 * sizeof(unsigned long long), st));
    int gx = grid_for((size_t)n * n, 256, 256);
    hipLaunchKernelGGL(eval_masks_kernel, dim3(gx, B), dim3(256), 0, st, (const float *)logits, batch_stride, plane_stride, row_stride, pad,
                       (const long long *)labels_i64, (long long *)mask_i64, n, (unsigned long long *)stats_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t unet_softmax_ce_scratch_bytes(size_t npix) { return ((npix + CE_PX_PER_BLOCK - 1) / CE_PX_PER_BLOCK) * 2 * sizeof(double); }
int unet_softmax_ce_step(const void *logits, long xsB, long xsC, long xsH, int K, const void *labels_i64, const void *weight, long wsB,
                         long wsH, long wsW, int B, int H, int W, void *loss_out, void *dlogits, float grad_scale, void *mask_i64,
                         void *invalid_u64, void *scratch, void *stream)
{
    const size_t npix = (size_t)B * H * W;
    ARG_CHECK(B > 0 && H > 0 && W > 0 && logits && labels_i64 && loss_out && scratch, "unet_softmax_ce_step: bad arguments");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_softmax_ce_step: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK((size_t)H * W < ((size_t)1 << 31), "unet_softmax_ce_step: %d x %d pixels per image (must be < 2^31)", H, W);
    const int nb = (int)((npix + CE_PX_PER_BLOCK - 1) / CE_PX_PER_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)scratch;
    unsigned long long *bad = (unsigned long long *)(part + nb);
    ProfScope ps("L1.softmax_ce+L2.argmax");
    // K logits + label (+ weight) in, K dlogits + mask out per pixel
    return profiled(PK_ELEMWISE, "softmax_ce_step", st, 8.0 * K * npix, 0.0,
                    (double)npix * (4.0 * K + 8.0 + (dlogits ? 4.0 * K : 0.0) + (mask_i64 ? 8.0 : 0.0) + (weight ? 4.0 : 0.0)), [&] {
        CLASS_DISPATCH(K, hipLaunchKernelGGL(softmax_ce_kernel<KP_>, dim3(nb), dim3(256), 0, st, (const float *)logits, xsB, xsC, xsH,
                                          (const long long *)labels_i64, (const float *)weight, wsB, wsH, wsW, K, H, W, npix,
                                          (float *)dlogits, grad_scale, (long long *)mask_i64, part, bad));
        hipLaunchKernelGGL(softmax_ce_final_kernel, dim3(1), dim3(256), 0, st, (const double *)part, (const unsigned long long *)bad, nb, npix,
                           (float *)loss_out, (unsigned long long *)invalid_u64);
    });
}

int unet_argmaxk(const void *logits, long batch_stride, long plane_stride, long row_stride, int K, void *out_i64, int B, int H, int W,
                 void *stream)
{
    ARG_CHECK(logits && out_i64 && B > 0 && H > 0 && W > 0, "unet_argmaxk: bad argument");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_argmaxk: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)B * H * W;
    ProfScope ps("L2.argmax");
    return profiled(PK_ELEMWISE, "argmaxk", st, 0.0, 0.0, (4.0 * K + 8.0) * (double)total, [&] {
        CLASS_DISPATCH(K, hipLaunchKernelGGL(argmaxk_kernel<KP_>, dim3(grid_for(total)), dim3(256), 0, st, (const float *)logits, batch_stride,
                                          plane_stride, row_stride, K, (long long *)out_i64, H, W, total));
    });
}

int unet_eval_confusion(const void *logits, long batch_stride, long plane_stride, long row_stride, int pad, int K, const void *labels_i64,
                        void *mask_i64, int B, int n, void *conf_u64, void *invalid_u64, void *stream)
{
    ARG_CHECK(logits && mask_i64 && B > 0 && n > 0 && pad >= 0, "unet_eval_confusion: bad argument");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_eval_confusion: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK(!labels_i64 || (conf_u64 && invalid_u64), "unet_eval_confusion: conf and invalid buffers needed with labels");
    hipStream_t st = (hipStream_t)stream;
    if (labels_i64) {
        HIP_TRY(hipMemsetAsync(conf_u64, 0, (size_t)B * K * K * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(invalid_u64, 0, (size_t)B * sizeof(unsigned long long), st));
    }
    const int gx = grid_for((size_t)n * n, 256, 256);
    CLASS_DISPATCH(K, hipLaunchKernelGGL(eval_confusion_kernel<KP_>, dim3(gx, B), dim3(256), 0, st, (const float *)logits, batch_stride,
                                      plane_stride, row_stride, pad, K, (const long long *)labels_i64, (long long *)mask_i64, n,
                                      (unsigned long long *)conf_u64, (unsigned long long *)invalid_u64));
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
