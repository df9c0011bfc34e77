// bd_discrete.h -- the Categorical actor head (action_distribution = "Categorical"), one imagined row per wave and
// one lane per action class (A <= 64).  Used by the imagination scans (imagine.hip, scan_cat.hip) and the REINFORCE
// kernel (reduce.hip).  Operation order as torch.distributions.Categorical(logits=out): norm = out - logsumexp(out),
// p = softmax(norm); the same order as cat_sample / cat_jacobian (bd_categorical.h) with the class loop spread over lanes.
// Every reduction is an xor butterfly: each lane ends with the same bits, and the result does not depend on the launch.
#pragma once
#include "bd_device.h"

namespace bd {

__device__ __forceinline__ float wave_max_x(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_sum_x(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// p = softmax(norm) from the normalised log-probabilities (invalid lanes: norm = -inf, p = 0).  max(norm) is
// fl(max(out) - lse) exactly, so the forward (from out) and the backward (from the saved norm) get the same p.
__device__ __forceinline__ float disc_probs(float norm, bool valid) {
    const float m2 = wave_max_x(valid ? norm : -INFINITY);
    const float e = valid ? expf(norm - m2) : 0.f;
    return e / wave_sum_x(e);
}

// norm = out - logsumexp(out)
__device__ __forceinline__ float disc_norm(float out, bool valid) {
    const float m = wave_max_x(valid ? out : -INFINITY);
    const float s = wave_sum_x(valid ? expf(out - m) : 0.f);
    return valid ? out - (m + logf(s)) : -INFINITY;
}

// Categorical.entropy: -sum p * norm, the log-probabilities clamped at the lowest finite float (0 * -inf = 0)
__device__ __forceinline__ float disc_entropy(float norm, float p, bool valid) {
    return -wave_sum_x(valid ? p * fmaxf(norm, -3.4028234663852886e38f) : 0.f);
}

// k = argmax(p / q) over the valid lanes, the first maximum winning (torch.multinomial's single-draw path)
__device__ __forceinline__ int disc_sample(float p, float q, bool valid, int lane) {
    float best = valid ? p / q : -INFINITY;
    int arg = valid ? lane : 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    return arg;
}

// straight-through action value of class `lane`: (onehot + p) - p, evaluated in that order (the reference's
// `action + probs - probs.detach()`): the hot entry is fl(fl(1 + p) - p), not always 1
__device__ __forceinline__ float disc_action_value(float p, bool hot) {
    const float oh = hot ? 1.f : 0.f;
    return (oh + p) - p;
}

// d loss / d out of one row: the softmax Jacobian applied to g = d loss / d action, plus dent * dH / d out
__device__ __forceinline__ float disc_head_grad(float g, float norm, float p, float H, float dent, bool valid) {
    const float dot = wave_sum_x(valid ? p * g : 0.f);
    return valid ? p * (g - dot) + dent * (-p * (norm + H)) : 0.f;
}

// Forward row pass of a 16-row tile (rows wave, wave + kWaves, ...): logits from the LDS image lg [16][A] -> action
// (global, and the embed layer's fragment tile af: rows past N stay zero), entropy, and norm into `save` (or NULL).
// eps: Exp(1) draws [.. x A] at row tn + row0 + row.
__device__ __forceinline__ void disc_rows(const float* lg, float* af, const float* __restrict__ eps, float* __restrict__ action,
                                          float* __restrict__ entropy, float* __restrict__ save, size_t tn, int row0, int N,
                                          int A, int lane, int wave) {
    for (int row = wave; row < 16; row += kWaves) {
        const int grow = row0 + row;
        const bool valid = grow < N && lane < A;
        float act = 0.f;
        if (grow < N) {                         // wave-uniform: the butterflies below see the whole wave
            const size_t i = (tn + grow) * A + lane;
            const float q = valid ? eps[i] : 1.f;
            const float norm = disc_norm(valid ? lg[row * A + lane] : 0.f, valid);
            const float p = disc_probs(norm, valid);
            const int k = disc_sample(p, q, valid, lane);
            const float H = disc_entropy(norm, p, valid);
            if (valid) {
                act = disc_action_value(p, lane == k);
                action[i] = act;
                if (save) save[i] = norm;
            }
            if (lane == 0) entropy[tn + grow] = H;
        }
        if (lane < A) af[frag_idx(row, lane)] = act;
    }
}

// Backward row pass: g = d loss / d action from the LDS image gimg [16][A], norm from the forward's save; writes
// d_actor_out [.. x A].  dentropy * ent_weight[row] (ent_weight NULL: 1) is the weight of d loss / d entropy.
__device__ __forceinline__ void disc_rows_bwd(const float* gimg, const float* __restrict__ norm_sv, float dentropy,
                                              const float* __restrict__ ent_weight, float* __restrict__ dout, size_t tn,
                                              int row0, int N, int A, int lane, int wave) {
    for (int row = wave; row < 16; row += kWaves) {
        const int grow = row0 + row;
        if (grow >= N) continue;                // wave-uniform
        const bool valid = lane < A;
        const size_t i = (tn + grow) * A + lane;
        const float norm = valid ? norm_sv[i] : -INFINITY;
        const float dent = ent_weight ? dentropy * ent_weight[tn + grow] : dentropy;
        const float p = disc_probs(norm, valid);
        const float H = disc_entropy(norm, p, valid);
        const float d = disc_head_grad(valid ? gimg[row * A + lane] : 0.f, norm, p, H, dent, valid);
        if (valid) dout[i] = d;
    }
}

}  // namespace bd
