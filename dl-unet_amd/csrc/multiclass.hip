// multiclass.hip — the K-class end of the net (2 <= K <= 16; the head at K = 2 stays direct.hip's head1x1), all HBM-bound:
//   head   : finalconv 1x1, C -> K, NHWC in, NCHW logits out, and its backward (dz, dw [K,C], db [K])
//   step   : pixel-wise softmax cross-entropy (Ronneberger et al. 2015, eq. 1) + its gradient + the argmax mask, one pass
//   argmax : K-way argmax of a strided [B,K,H,W] view; crop + argmax + per-image K x K confusion counts
// Kernels are templated on KP, the class count padded to 4, 8 or 16; the true K is a runtime bound (padded classes carry zero
// weights and are never written).  See DESIGN §4f.
#include "common.hpp"
#include "elem.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {
namespace mc {

// Reduce-scatter butterfly over the D*2 lanes of a pixel group: each lane starts with N partial sums (one per class), at every
// xor distance it keeps half of them and adds the partner's copy of that half, so a class costs N/2 + N/4 + ... shuffles in
// total instead of log2(lanes) each.  Once a lane is down to one value the remaining steps are a plain xor reduction.
// The sums are the same pairwise tree as a per-class xor reduction.
template <int N, int D>
__device__ __forceinline__ void butterfly(float *v, int lane)
{
    if constexpr (D >= 1) {
        if constexpr (N > 1) {
            constexpr int H = N / 2;
            const bool up = (lane & D) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float keep = up ? v[H + i] : v[i];
                const float send = up ? v[i] : v[H + i];
                v[i] = keep + __shfl_xor(send, D, 64);
            }
            butterfly<H, D / 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], D, 64);
            butterfly<1, D / 2>(v, lane);
        }
    }
}

// ---- head forward: 16 (C=64) or 8 (C=32) lanes x float4 per pixel, butterfly, LDS staging for coalesced plane writes -----
template <int C, int KP, typename T>
__global__ __launch_bounds__(256) void headk_fwd_kernel(const T *__restrict__ x, const float *__restrict__ w,
                                                        const float *__restrict__ bias, float *__restrict__ logits,
                                                        int K, int B, int HW)
{
    constexpr int CG = C / 4, PPP = 256 / CG;
    constexpr int PASSES = 16;
    constexpr int PPB = PPP * PASSES;
    constexpr int NV = KP > CG ? KP / CG : 1;        // classes a lane holds after the butterfly
    constexpr int R = CG > KP ? CG / KP : 1;         // lanes that end with the same classes (the first of them writes)
    __shared__ float outs[KP][PPB];
    const int cg = threadIdx.x % CG, pl = threadIdx.x / CG;
    f32x4 wr[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) wr[k] = k < K ? *(const f32x4 *)(w + k * C + cg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    int cb = 0;
    {
        int n = KP;
        for (int d = CG / 2; d >= 1 && n > 1; d >>= 1) { n >>= 1; if (cg & d) cb += n; }
    }
    float bv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) bv[i] = cb + i < K ? bias[cb + i] : 0.f;
    const bool writer = (cg & (R - 1)) == 0;
    const size_t npix = (size_t)B * HW;
    const size_t base = (size_t)blockIdx.x * PPB;
#pragma unroll 2
    for (int ps = 0; ps < PASSES; ++ps) {
        const int lp = ps * PPP + pl;
        const size_t pix = base + lp;
        float s[KP];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (pix < npix) v = load4(x + pix * C + cg * 4);
#pragma unroll
        for (int k = 0; k < KP; ++k) s[k] = v[0] * wr[k][0] + v[1] * wr[k][1] + v[2] * wr[k][2] + v[3] * wr[k][3];
        butterfly<KP, CG / 2>(s, cg);
        if (writer) {
#pragma unroll
            for (int i = 0; i < NV; ++i) if (cb + i < K) outs[cb + i][lp] = s[i] + bv[i];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < K * PPB; e += 256) {
        const int k = e / PPB, lp = e - k * PPB;
        const size_t pix = base + lp;
        if (pix < npix) {
            const size_t img = pix / HW, rem = pix - img * HW;
            logits[(img * K + k) * HW + rem] = outs[k][lp];
        }
    }
}

// ---- head backward: dz[m][c] = (sum_k dl_k[m] w[k][c]) * (x[m][c] > 0); dw[k][c] = sum_m dl_k[m] x[m][c]; db[k] = sum_m dl_k[m]
// A block takes chunks of HK_PPB consecutive pixels: the chunk's K dlogits planes are staged in LDS with coalesced loads (x
// grad scale), then the pixel groups (16 / 8 lanes x float4 of x) read them as LDS broadcasts.  Register accumulators, pixel
// groups of a wave combined by shuffles, waves through LDS, one partial row per block (fixed order).
constexpr int HK_PPB = 512;
template <int C, int KP, typename T>
__global__ __launch_bounds__(256) void headk_bwd_kernel(const T *__restrict__ x, const float *__restrict__ w,
                                                        const float *__restrict__ dlogits, float dls, T *__restrict__ dz,
                                                        float *__restrict__ partial, int K, int B, int HW)
{
    constexpr int CG = C / 4, PPP = 256 / CG, PASSES = HK_PPB / PPP;
    __shared__ __attribute__((aligned(16))) float dsh[KP][HK_PPB];
    const int cg = threadIdx.x % CG, pl = threadIdx.x / CG;
    f32x4 wr[KP], a[KP];
    float sb[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        wr[k] = k < K ? *(const f32x4 *)(w + k * C + cg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        a[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        sb[k] = 0.f;
    }
    const size_t npix = (size_t)B * HW;
    for (size_t base = (size_t)blockIdx.x * HK_PPB; base < npix; base += (size_t)gridDim.x * HK_PPB) {
        __syncthreads();                                   // the previous chunk's reads are done
        for (int e = threadIdx.x; e < KP * HK_PPB; e += 256) {
            const int k = e / HK_PPB, lp = e - k * HK_PPB;
            const size_t pix = base + lp;
            float v = 0.f;
            if (k < K && pix < npix) {
                const size_t img = pix / HW, rem = pix - img * HW;
                v = dlogits[(img * K + k) * HW + rem] * dls;
            }
            dsh[k][lp] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int ps = 0; ps < PASSES; ++ps) {
            const int lp = ps * PPP + pl;
            const size_t pix = base + lp;
            if (pix >= npix) break;
            const f32x4 v = load4(x + pix * C + cg * 4);
            float d[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) d[k] = dsh[k][lp];
            f32x4 g;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float s = d[0] * wr[0][c];
#pragma unroll
                for (int k = 1; k < KP; ++k) s = fmaf(d[k], wr[k][c], s);
                g[c] = v[c] > 0.f ? s : 0.f;
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) {
#pragma unroll
                for (int c = 0; c < 4; ++c) a[k][c] = fmaf(d[k], v[c], a[k][c]);
                sb[k] += d[k];
            }
            store4(dz + pix * C + cg * 4, g);
        }
    }
    // pixel groups of a wave: xor over the lane bits above the group
#pragma unroll
    for (int dd = CG; dd < 64; dd <<= 1) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
#pragma unroll
            for (int c = 0; c < 4; ++c) a[k][c] += __shfl_xor(a[k][c], dd, 64);
            sb[k] += __shfl_xor(sb[k], dd, 64);
        }
    }
    __syncthreads();                                       // dsh is reused below
    constexpr int ROW = KP * C + KP + 4;
    static_assert(4 * ROW <= KP * HK_PPB, "the wave partials must fit the dlogits stage");
    float (*red)[ROW] = reinterpret_cast<float (*)[ROW]>(&dsh[0][0]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < CG) {
#pragma unroll
        for (int k = 0; k < KP; ++k) *(f32x4 *)&red[wave][k * C + cg * 4] = a[k];
        if (cg == 0) {
#pragma unroll
            for (int k = 0; k < KP; ++k) red[wave][KP * C + k] = sb[k];
        }
    }
    __syncthreads();
    const int n = K * C + K;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int src = e < K * C ? e : KP * C + (e - K * C);
        partial[(size_t)blockIdx.x * n + e] = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
    }
}

__global__ __launch_bounds__(256) void headk_bwd_reduce_kernel(const float *__restrict__ partial, int nb, int K, int C,
                                                               float *__restrict__ dw, float *__restrict__ db)
{
    const int n = K * C + K;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= n) return;
    float s = 0.f;
    for (int b = lane; b < nb; b += 64) s += partial[(size_t)b * n + e];
    s = wave_sum(s);
    if (lane == 0) { if (e < K * C) { if (dw) dw[e] = s; } else if (db) db[e - K * C] = s; }
}

// ---- softmax cross-entropy step (eq. 1): a thread owns a pixel (all K planes) -------------------------------------------
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
    __shared__ double red[256];
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

// ---- K-way argmax of a strided view -------------------------------------------------------------------------------------
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
        float m = p[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K) { const float v = p[k * ps]; if (v > m) { m = v; am = k; } }
        out[e] = am;
    }
}

// ---- crop + argmax + confusion counts: conf[b][label][pred], labels outside [0, K) go to invalid[b] -------------------------
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
        float m = p[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K) { const float v = p[k * ps]; if (v > m) { m = v; am = k; } }
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

// one block per HK_PPB-pixel chunk up to 4096 blocks (a 572^2 batch of 8 is 2353 chunks: no block takes two)
static int headk_bwd_blocks(int B, int H, int W) { return grid_for((size_t)B * H * W, mc::HK_PPB, 4096); }

size_t headk_bwd_scratch_bytes(int B, int H, int W, int C, int K)
{
    if (K == 2) return unet_head1x1_bwd_scratch_bytes(B, H, W, C);        // the head1x1 kernels' partials
    return (size_t)headk_bwd_blocks(B, H, W) * (K * C + K) * sizeof(float);
}

int headk_fwd(const void *x, int B, int H, int W, int C, int K, const float *w, const float *bias, float *logits, int es, hipStream_t st)
{
    if (K == 2) return head1x1_fwd(x, B, H, W, C, w, bias, logits, es, st);
    ARG_CHECK(C == 64 || C == 32, "head1xk: C=%d unsupported (32 or 64)", C);
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "head1xk: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    using namespace mc;
    const size_t npix = (size_t)B * H * W;
    const int ppb = (256 / (C / 4)) * 16;
    const int grid = (int)((npix + ppb - 1) / ppb);
    return profiled(PK_ELEMWISE, "head1xk_fwd", st, 2.0 * npix * C * K, 0.0, (double)npix * (es * C + 4 * K), [&] {
        dispatch_es_width_kp(es, C, class_pad(K), [&](auto t, auto c, auto kp) {
            using T = decltype(t);
            hipLaunchKernelGGL((headk_fwd_kernel<c(), kp(), T>), dim3(grid), dim3(256), 0, st, (const T *)x, w, bias, logits, K, B, H * W);
        });
    });
}

int headk_bwd(const void *x, int B, int H, int W, int C, int K, const float *w, const float *dlogits, float dl_scale, void *dz, float *dw,
              float *db, float *scratch, int es, hipStream_t st)
{
    if (K == 2) return head1x1_bwd(x, B, H, W, C, w, dlogits, dl_scale, dz, dw, db, scratch, es, st);
    ARG_CHECK(C == 64 || C == 32, "head1xk: C=%d unsupported (32 or 64)", C);
    ARG_CHECK(K >= 2 && K <= UNET_MAX_CLASSES, "head1xk: K=%d unsupported (2..%d)", K, UNET_MAX_CLASSES);
    using namespace mc;
    const int nb = headk_bwd_blocks(B, H, W);
    const double npix = (double)B * H * W;
    return profiled(PK_ELEMWISE, "head1xk_bwd", st, 4.0 * npix * C * K, 0.0, npix * (2.0 * es * C + 4 * K), [&] {
        dispatch_es_width_kp(es, C, class_pad(K), [&](auto t, auto c, auto kp) {
            using T = decltype(t);
            hipLaunchKernelGGL((headk_bwd_kernel<c(), kp(), T>), dim3(nb), dim3(256), 0, st, (const T *)x, w, dlogits, dl_scale, (T *)dz, scratch, K, B, H * W);
        });
        hipLaunchKernelGGL(headk_bwd_reduce_kernel, dim3(cdiv(K * C + K, 4)), dim3(256), 0, st, (const float *)scratch, nb, K, C, dw, db);
    });
}

}  // namespace unet

using namespace unet;
using namespace unet::mc;

extern "C" {

int unet_head1xk_fwd(const void *x, int B, int H, int W, int C, int K, const void *w, const void *bias, void *logits, void *stream)
{
    ARG_CHECK(x && w && bias && logits && B > 0 && H > 0 && W > 0, "unet_head1xk_fwd: bad argument");
    return headk_fwd(x, B, H, W, C, K, (const float *)w, (const float *)bias, (float *)logits, op_es(), (hipStream_t)stream);
}
size_t unet_head1xk_bwd_scratch_bytes(int B, int H, int W, int C, int K) { return headk_bwd_scratch_bytes(B, H, W, C, K); }
int unet_head1xk_bwd(const void *x, int B, int H, int W, int C, int K, const void *w, const void *dlogits, void *dz, void *dw, void *db,
                     void *scratch, void *stream)
{
    ARG_CHECK(x && w && dlogits && dz && scratch && B > 0 && H > 0 && W > 0, "unet_head1xk_bwd: bad argument");
    return headk_bwd(x, B, H, W, C, K, (const float *)w, (const float *)dlogits, 1.0f, dz, (float *)dw, (float *)db, (float *)scratch,
                     op_es(), (hipStream_t)stream);
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
