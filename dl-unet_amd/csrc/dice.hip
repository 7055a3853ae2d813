// dice.hip — the soft Dice loss (Milletari et al. 2016) and the CE + Dice sum over the K-class soft-max, one training-step op
// (unet_dice_step), HBM-bound, three launches, no host sync, no floating-point atomics:
//   sums    : a thread owns a pixel (all K planes), a workgroup DICE_PX_PER_BLOCK pixels of ONE image (grid: blocks per image x
//             B); p by softmax.hpp's pixel_exps, softmax_ce_kernel's statements; per block the CE partial, the invalid count,
//             the I / P partials (double) and the label counts Y (integers); the argmax mask
//   finish  : one workgroup sums the partials in a fixed order per (image, class) or per class (batch Dice), forms the Dice
//             coefficients, the three losses and the coefficient table (a, c) the gradient reads
//   grad    : re-reads the logits, recomputes p, writes the dense gradient (CE term included)
// Every sum has one fixed order, so a result does not depend on the run or on the stream.  See DESIGN §4v.
#include "common.hpp"
#include "elem.hpp"
#include "softmax.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {
namespace dice {

constexpr int DICE_PX_PER_BLOCK = 2048;      // pixels of one image that a workgroup of the sums and gradient kernels covers
constexpr int DICE_THREADS = 256;
constexpr int DICE_PX_PER_THREAD = DICE_PX_PER_BLOCK / DICE_THREADS;      // summed in fp32 before widening
constexpr int DICE_FIN_THREADS = 256;        // the finisher: one workgroup ...
constexpr int DICE_FIN_GROUP = 16;           // ... of 16-lane groups, a group per (image, class) term, its lanes stride the partials
constexpr int DICE_FIN_GROUPS = DICE_FIN_THREADS / DICE_FIN_GROUP;

// ---- launch 1: sums -----------------------------------------------------------------------------------------------------------
// Partials of block (b, blockIdx.x) sit at slot = b * gridDim.x + blockIdx.x: ce_part[slot], bad_part[slot], and per class
// i_part / p_part / y_part[slot * K + k].
template <int KP>
__global__ __launch_bounds__(DICE_THREADS) void dice_sums_kernel(const float *__restrict__ x, long xsB, long xsC, long xsH,
                                                                 const long long *__restrict__ labels, const float *__restrict__ w,
                                                                 long wsB, long wsH, long wsW, int K, int H, int W,
                                                                 long long *__restrict__ mask, double *__restrict__ ce_part,
                                                                 unsigned long long *__restrict__ bad_part, double *__restrict__ i_part,
                                                                 double *__restrict__ p_part, unsigned *__restrict__ y_part)
{
    constexpr int ROWS = 2 * KP;                         // I and P of every class
    constexpr int TPR = DICE_THREADS / ROWS;             // threads that sum one row: 64 (KP = 2) .. 8 (KP = 16), inside one wave
    __shared__ float acc[ROWS][DICE_THREADS + 1];
    __shared__ unsigned ycnt[KP + 1];                    // labels per class, [KP]: labels outside [0, K)
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const unsigned HW = (unsigned)H * (unsigned)W;       // < 2^31 (checked on the host)
    const unsigned r0 = blockIdx.x * (unsigned)DICE_PX_PER_BLOCK;
    if (tid <= KP) ycnt[tid] = 0;
    __syncthreads();
    float aI[KP], aP[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) { aI[k] = 0.f; aP[k] = 0.f; }
    double ce = 0.0;
    for (int j = 0; j < DICE_PX_PER_THREAD; ++j) {
        const unsigned r = r0 + (unsigned)(j * DICE_THREADS + tid);
        if (r >= HW) break;
        const int yy = (int)(r / (unsigned)W), xx = (int)(r - (unsigned)yy * (unsigned)W);
        const size_t e = b * HW + r;
        const long long lab = labels[e];
        const bool ok = lab >= 0 && lab < (long long)K;
        float ex[KP], se, m_ll;
        int am;
        pixel_exps<KP>(x + b * xsB + (long)yy * xsH + xx, xsC, K, lab, ex, se, m_ll, am);
        if (ok) {
            const float wv = w ? w[b * wsB + (long)yy * wsH + (long)xx * wsW] : 1.f;
            ce += (double)wv * ((double)m_ll + (double)logf(se));
            const float inv_se = 1.f / se;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float p = ex[k] * inv_se;
                aP[k] += p;
                aI[k] += k == lab ? p : 0.f;
            }
            atomicAdd(&ycnt[(int)lab], 1u);
        } else {
            atomicAdd(&ycnt[KP], 1u);
        }
        if (mask) mask[e] = am;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) { acc[k][tid] = aI[k]; acc[KP + k][tid] = aP[k]; }
    __syncthreads();
    const size_t slot = b * gridDim.x + blockIdx.x;
    {
        const int row = tid / TPR, sub = tid - row * TPR;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) s += (double)acc[row][sub + i * TPR];
#pragma unroll
        for (int d = TPR / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        const int k = row < KP ? row : row - KP;
        if (sub == 0 && k < K) (row < KP ? i_part : p_part)[slot * K + k] = s;
    }
    if (tid < K) y_part[slot * K + tid] = ycnt[tid];
    if (tid == 0) bad_part[slot] = ycnt[KP];
    ce = block_sum256(ce);
    if (tid == 0) ce_part[slot] = ce;
}

// ---- launch 2: finish ---------------------------------------------------------------------------------------------------------
// coef[(t * K + k) * 2 + {0, 1}] = grad_scale * dice_weight / n_terms * {a, c}, a = 2 / D, c = (2 I + s) / D^2 (0, 0 for a class
// that is not counted); t = image, or 0 with UNET_DICE_BATCH.
__global__ __launch_bounds__(DICE_FIN_THREADS) void dice_finish_kernel(const double *__restrict__ ce_part,
                                                                       const unsigned long long *__restrict__ bad_part,
                                                                       const double *__restrict__ i_part, const double *__restrict__ p_part,
                                                                       const unsigned *__restrict__ y_part, int nbx, int B, int K, size_t npix,
                                                                       float ce_weight, float dice_weight, float smooth, float gscale, int flags,
                                                                       float *__restrict__ coef, float *__restrict__ loss_out,
                                                                       float *__restrict__ dice_out, unsigned long long *__restrict__ invalid)
{
    __shared__ double gsum[DICE_FIN_GROUPS];
    const int tid = threadIdx.x;
    const size_t nblk = (size_t)B * nbx;
    double ce = 0.0;
    unsigned long long bad = 0;
    for (size_t i = tid; i < nblk; i += DICE_FIN_THREADS) { ce += ce_part[i]; bad += bad_part[i]; }
    ce = block_sum256(ce);
    bad = block_sum256(bad);

    const bool batch = (flags & UNET_DICE_BATCH) != 0;
    const int first = (flags & UNET_DICE_SKIP_BACKGROUND) ? 1 : 0;
    const int images = batch ? 1 : B;
    const int terms = images * K;                        // every class gets its coefficient; the mean is over the counted ones
    const double n_terms = (double)images * (double)(K - first);
    const size_t span = batch ? nblk : (size_t)nbx;
    const double s = (double)smooth;
    const double sc = (double)gscale * (double)dice_weight / n_terms;
    const int g = tid / DICE_FIN_GROUP, sub = tid - g * DICE_FIN_GROUP;
    double dsum = 0.0;
    for (int t = g; t < terms; t += DICE_FIN_GROUPS) {
        const int img = t / K, k = t - img * K;
        const size_t base = (size_t)img * nbx;           // img is 0 with batch
        double I = 0.0, P = 0.0;
        unsigned long long Y = 0;
        for (size_t j = sub; j < span; j += DICE_FIN_GROUP) {
            const size_t idx = (base + j) * K + k;
            I += i_part[idx];
            P += p_part[idx];
            Y += y_part[idx];
        }
#pragma unroll
        for (int d = DICE_FIN_GROUP / 2; d >= 1; d >>= 1) {
            I += __shfl_xor(I, d, 64);
            P += __shfl_xor(P, d, 64);
            Y += __shfl_xor(Y, d, 64);
        }
        if (sub == 0) {
            const double D = P + (double)Y + s, N = 2.0 * I + s;
            const double dc = N / D;
            const bool counted = k >= first;
            if (dice_out) dice_out[t] = (float)dc;
            coef[(size_t)t * 2] = counted ? (float)(sc * 2.0 / D) : 0.f;
            coef[(size_t)t * 2 + 1] = counted ? (float)(sc * N / (D * D)) : 0.f;
            if (counted) dsum += dc;
        }
    }
    if (sub == 0) gsum[g] = dsum;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < DICE_FIN_GROUPS; ++i) tot += gsum[i];
        const double l_dice = 1.0 - tot / n_terms, l_ce = ce / (double)npix;
        loss_out[0] = (float)((double)ce_weight * l_ce + (double)dice_weight * l_dice);
        loss_out[1] = (float)l_ce;
        loss_out[2] = (float)l_dice;
        if (invalid) *invalid = bad;
    }
}

// ---- launch 3: gradient -------------------------------------------------------------------------------------------------------
// dl_j = ce_weight * (w / n) * grad_scale * (p_j - [y = j]) + p_j * (g_j - sum_k g_k p_k), g_k = C_k - A_k [y = k] with (A, C) the
// finisher's table (grad_scale, dice_weight and 1 / n_terms are in it); 0 on every plane of a pixel with an invalid label.
template <int KP>
__global__ __launch_bounds__(DICE_THREADS) void dice_grad_kernel(const float *__restrict__ x, long xsB, long xsC, long xsH,
                                                                 const long long *__restrict__ labels, const float *__restrict__ w,
                                                                 long wsB, long wsH, long wsW, int K, int H, int W, size_t npix,
                                                                 const float *__restrict__ coef, int coef_images, float ce_weight,
                                                                 float gscale, float *__restrict__ dx)
{
    __shared__ float cA[KP], cC[KP];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const unsigned r0 = blockIdx.x * (unsigned)DICE_PX_PER_BLOCK;
    if (tid < KP) {
        const size_t t = (coef_images > 1 ? b : 0) * K + tid;
        cA[tid] = tid < K ? coef[t * 2] : 0.f;
        cC[tid] = tid < K ? coef[t * 2 + 1] : 0.f;
    }
    __syncthreads();
    const float inv_n = (float)(1.0 / (double)npix);
    const bool with_ce = ce_weight != 0.f;
    for (int j = 0; j < DICE_PX_PER_THREAD; ++j) {
        const unsigned r = r0 + (unsigned)(j * DICE_THREADS + tid);
        if (r >= HW) break;
        const int yy = (int)(r / (unsigned)W), xx = (int)(r - (unsigned)yy * (unsigned)W);
        const long long lab = labels[b * HW + r];
        const bool ok = lab >= 0 && lab < (long long)K;
        float *out = dx + b * K * HW + r;
        if (!ok) {
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) out[(size_t)k * HW] = 0.f;
            continue;
        }
        float ex[KP], se, m_ll;
        int am;
        pixel_exps<KP>(x + b * xsB + (long)yy * xsH + xx, xsC, K, lab, ex, se, m_ll, am);
        const float inv_se = 1.f / se;
        float sc = 0.f;
        if (with_ce) {
            const float wv = w ? w[b * wsB + (long)yy * wsH + (long)xx * wsW] : 1.f;
            sc = wv * inv_n * gscale;                    // the CE step's scale ...
            sc *= ce_weight;                             // ... times the CE weight (exact at 1)
        }
        const float ay = cA[(int)lab];
        float p[KP], S = 0.f, py = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            p[k] = ex[k] * inv_se;
            S = fmaf(cC[k], p[k], S);
            if (k == lab) py = p[k];
        }
        S = fmaf(-ay, py, S);                            // sum_k g_k p_k
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k < K) {
                const bool hit = k == lab;
                const float gk = cC[k] - (hit ? ay : 0.f);
                out[(size_t)k * HW] = sc * (p[k] - (hit ? 1.f : 0.f)) + p[k] * (gk - S);
            }
        }
    }
}

}  // namespace dice
}  // namespace unet

using namespace unet;
using namespace unet::dice;

static inline size_t dice_blocks_per_image(int H, int W) { return ((size_t)H * W + DICE_PX_PER_BLOCK - 1) / DICE_PX_PER_BLOCK; }

extern "C" {

size_t unet_dice_scratch_bytes(int B, int K, int H, int W)
{
    if (B <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    const size_t nblk = (size_t)B * dice_blocks_per_image(H, W);
    // per block: the CE partial and the invalid count (8 + 8), per block and class: I, P (double) and Y (32-bit); the table: 2 floats
    // per (image, class)
    return nblk * (16 + (size_t)K * 20) + (size_t)B * K * 8;
}

int unet_dice_step(const void *logits, long xsB, long xsC, long xsH, int K, const void *labels_i64, const void *weight, long wsB,
                   long wsH, long wsW, int B, int H, int W, float ce_weight, float dice_weight, float smooth, int flags, void *loss_out,
                   void *dice_out, void *dlogits, float grad_scale, void *mask_i64, void *invalid_u64, void *scratch, void *stream)
{
    ARG_CHECK(B > 0 && H > 0 && W > 0 && logits && labels_i64 && loss_out && scratch, "unet_dice_step: bad arguments");
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "unet_dice_step: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    ARG_CHECK((size_t)H * W < ((size_t)1 << 31), "unet_dice_step: %d x %d pixels per image (must be < 2^31)", H, W);
    ARG_CHECK(B <= 65535, "unet_dice_step: B=%d (must be <= 65535)", B);
    ARG_CHECK(smooth > 0.f && std::isfinite(smooth), "unet_dice_step: smooth=%g (must be positive and finite)", (double)smooth);
    ARG_CHECK(ce_weight >= 0.f && dice_weight >= 0.f && ce_weight + dice_weight > 0.f && std::isfinite(ce_weight + dice_weight),
              "unet_dice_step: ce_weight=%g, dice_weight=%g (both >= 0, not both 0)", (double)ce_weight, (double)dice_weight);
    ARG_CHECK((flags & ~(UNET_DICE_BATCH | UNET_DICE_SKIP_BACKGROUND)) == 0, "unet_dice_step: flags=%d", flags);
    const size_t npix = (size_t)B * H * W;
    const int nbx = (int)dice_blocks_per_image(H, W);
    const size_t nblk = (size_t)B * nbx;
    hipStream_t st = (hipStream_t)stream;
    double *ce_part = (double *)scratch;
    double *i_part = ce_part + nblk;
    double *p_part = i_part + nblk * K;
    unsigned long long *bad_part = (unsigned long long *)(p_part + nblk * K);
    float *coef = (float *)(bad_part + nblk);
    unsigned *y_part = (unsigned *)(coef + (size_t)B * K * 2);
    const int coef_images = (flags & UNET_DICE_BATCH) ? 1 : B;
    const dim3 grid(nbx, B);
    ProfScope ps("L1.dice+L2.argmax");
    // sums: K logits + label (+ weight) in, mask out; gradient: K logits + label (+ weight) in, K dlogits out
    const double wbytes = weight ? 4.0 : 0.0;
    return profiled(PK_ELEMWISE, "dice_step", st, (dlogits ? 16.0 : 8.0) * K * npix, 0.0,
                    (double)npix * (4.0 * K + 8.0 + wbytes + (mask_i64 ? 8.0 : 0.0) + (dlogits ? 8.0 * K + 8.0 + wbytes : 0.0)), [&] {
        CLASS_DISPATCH(K, hipLaunchKernelGGL(dice_sums_kernel<KP_>, grid, dim3(DICE_THREADS), 0, st, (const float *)logits, xsB, xsC, xsH,
                                          (const long long *)labels_i64, (const float *)weight, wsB, wsH, wsW, K, H, W,
                                          (long long *)mask_i64, ce_part, bad_part, i_part, p_part, y_part));
        hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(DICE_FIN_THREADS), 0, st, (const double *)ce_part,
                           (const unsigned long long *)bad_part, (const double *)i_part, (const double *)p_part, (const unsigned *)y_part, nbx,
                           B, K, npix, ce_weight, dice_weight, smooth, grad_scale, flags, coef, (float *)loss_out, (float *)dice_out,
                           (unsigned long long *)invalid_u64);
        if (dlogits)
            CLASS_DISPATCH(K, hipLaunchKernelGGL(dice_grad_kernel<KP_>, grid, dim3(DICE_THREADS), 0, st, (const float *)logits, xsB, xsC,
                                              xsH, (const long long *)labels_i64, (const float *)weight, wsB, wsH, wsW, K, H, W, npix,
                                              (const float *)coef, coef_images, ce_weight, grad_scale, (float *)dlogits));
    });
}

}  // extern "C"
