// bd_latent.h -- per-element terms of the latent losses, shared by the loss kernels (reduce.hip) and the training
// diagnostics (diag.hip): ONE definition, so that a diagnostic of the KL is the KL the loss saw.
#pragma once
#include <hip/hip_runtime.h>

namespace bd {

// torch.distributions.kl._kl_normal_normal
__device__ __forceinline__ float kl_elem(float qm, float qs, float pm, float ps) {
    const float ratio = qs / ps;
    const float vr = ratio * ratio;
    const float t = (qm - pm) / ps;
    return 0.5f * (vr + t * t - 1.f - logf(vr));
}

// ---- Categorical latents (CategoricalBeliefModel, src/models.py:101-117; KL branch src/dreamer.py:102-106,131-144) ----
// rows x D groups of C classes (reference: 32 x 32).  A 32-lane half wave owns one group; a lane holds classes
// c = l, l+32, ... (C <= 128).  Reductions are xor-shuffles with offsets < 32, which stay inside the half wave.
constexpr int kCatPer = 4;     // classes per lane

__device__ __forceinline__ float half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// normalised log-probabilities of one group, as Categorical(logits=...) keeps them: x - logsumexp(x)
// (torch/distributions/categorical.py); lp[i] is class l + 32 i (-inf beyond C)
__device__ __forceinline__ void group_log_softmax(const float* __restrict__ x, int C, int l, float (&lp)[kCatPer]) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kCatPer; ++i) {
        const int c = l + 32 * i;
        lp[i] = c < C ? x[c] : -INFINITY;
        m = fmaxf(m, lp[i]);
    }
    m = half_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kCatPer; ++i) s += (l + 32 * i < C) ? expf(lp[i] - m) : 0.f;
    const float lse = m + logf(half_sum(s));
#pragma unroll
    for (int i = 0; i < kCatPer; ++i) lp[i] -= lse;
}

// KL(q || p) of one group from normalised log-probabilities (torch.distributions.kl._kl_categorical_categorical:
// t = q.probs * (q.logits - p.logits); t[p.probs == 0] = inf; t[q.probs == 0] = 0)
__device__ __forceinline__ float group_kl(const float (&lq)[kCatPer], const float (&lp)[kCatPer], int C, int l) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kCatPer; ++i) {
        if (l + 32 * i < C) {
            const float qv = expf(lq[i]), pv = expf(lp[i]);
            float t = qv * (lq[i] - lp[i]);
            if (pv == 0.f) t = INFINITY;
            if (qv == 0.f) t = 0.f;
            s += t;
        }
    }
    return half_sum(s);
}

}  // namespace bd
