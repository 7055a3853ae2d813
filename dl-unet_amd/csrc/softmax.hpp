// softmax.hpp — the class axis of one pixel: K logits, KP = class_pad(K); the classes K .. KP-1 are padding (in no maximum, exp = 0).
// For the Dice kernels, eval_confusion_kernel and tile.hip's class_probs; softmax_ce_kernel and argmaxk_kernel keep inline copies.
#pragma once
#include "common.hpp"

namespace unet {

// The first maximum of logit(0 .. K-1) and its index am (torch.argmax's tie rule); logit(k) is called once per k < K, so
// eval_confusion_kernel hands in the load itself and holds one logit at a time (with all KP loaded first, KP = 16 spills)
template <int KP, class Logit>
__device__ __forceinline__ float first_max(Logit logit, int K, int &am)
{
    float m = logit(0);
    am = 0;
#pragma unroll
    for (int k = 1; k < KP; ++k)
        if (k < K) { const float v = logit(k); if (v > m) { m = v; am = k; } }
    return m;
}

// ex[k] = exp(l_k - m) for k < K, 0 for the padded classes; returns their sum, taken in increasing k
template <int KP>
__device__ __forceinline__ float class_exps(const float (&l)[KP], int K, float m, float (&ex)[KP])
{
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ex[k] = k < K ? expf(l[k] - m) : 0.f;
        se += ex[k];
    }
    return se;
}

// The strided loader on top: ex, se, the argmax am and m_ll = m - l_lab (0 for a lab outside [0, KP)) of the pixel at px with label
// lab; its loss is m_ll + log(se), its probabilities ex[k] * (1.f / se)
template <int KP>
__device__ __forceinline__ void pixel_exps(const float *__restrict__ px, long xsC, int K, long long lab, float (&ex)[KP], float &se,
                                           float &m_ll, int &am)
{
    float l[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) l[k] = k < K ? px[k * xsC] : 0.f;
    const float m = first_max<KP>([&](int k) { return l[k]; }, K, am);
    float ll = m;
#pragma unroll
    for (int k = 0; k < KP; ++k) if (k == lab) ll = l[k];       // before the exponentials: after them it costs KP = 16 13 VGPRs
    se = class_exps<KP>(l, K, m, ex);
    m_ll = m - ll;
}

}  // namespace unet
