// multiclass.hip — the K-class head of the net (2 < K <= 16; the head at K = 2 stays direct.hip's head1x1), HBM-bound: finalconv
// 1x1, C -> K, NHWC in, NCHW logits out, and its backward (dz, dw [K,C], db [K]).  The kernels are templated on KP, the class
// count padded to 4, 8 or 16; the true K is a runtime bound (padded classes carry zero weights and are never written).  The
// K-class loss, argmax and confusion counts are loss.hip's.  See DESIGN §4f.
#include "common.hpp"
#include "elem.hpp"
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

}  // extern "C"
