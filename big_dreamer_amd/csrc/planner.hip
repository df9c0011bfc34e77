// planner.hip -- the hot loop of the CEM planner (MPCPlanner.forward, src/planner.py:28-90), for latent_distribution =
// Gaussian | Categorical (TransitionModel.forward's Categorical branches, src/models.py:226-228,258-260;
// CategoricalBeliefModel, src/models.py:76-117):
//
//   One kernel body, plan_rollout_kernel<LC>, templated on the latent kind; bd_plan_rollout launches <false>,
//     bd_plan_rollout_cat <true>.  One persistent launch per CEM iteration.  A workgroup owns 16 candidate action sequences
//     and walks the H planning steps with the belief resident in LDS (MFMA fragment order), weights stream from L2: the
//     candidate's action a_t = mean_t + std_t * eps (src/planner.py:60-62) is formed on load, the prior-only RSSM step follows
//     (TransitionModel.forward with embeddings=None, src/models.py:241-256: x = ELU(W_e [s; a]), h' = GRUCell(x, h),
//     s' ~ belief_prior(h')), then the reward model (DenseModel 4 x (Linear+ELU) + Linear, src/models.py:365-408) runs
//     on [h'; s'] and the prediction is added to the candidate's return (src/planner.py:68-72).  Beliefs and states
//     never leave the CU; the only outputs are the H x rows x A actions and one return per candidate.
//     With fewer candidate tiles than CUs (one environment: 63 tiles) the step is latency bound and the reward
//     model doubles its length, so the host may ask for the features instead (returns == null, feat != null) and run
//     the reward model as ONE dense chain over all H x rows rows, which fills the chip (bd_mlp_forward).
//     What the latent kind decides:
//       !LC: the state is a fragment tile; it enters the embed layer as a second K segment and the reward model's first
//            layer through ff = [h'; s'], ONE K range (that layer is packed over Be+S); the prior head is the dual
//            mean / std head, s' = mean + (softplus(raw) + min_std) * eps_state with standard normals.
//       LC:  the state is D class indices per row (+ one weight per factor: 1 after a sample, the stored value / 0 for the
//            caller's start state, the rule of state_to_indices); W_es s of the embed layer and the state columns of the
//            reward model's first layer are GATHERS of D rows of the plain transposed weights, added in the epilogue, not
//            K = D*C contractions; the prior head is hidden -> D*C logits into a swizzled LDS image (bd_categorical.h,
//            CatFull), then one thread per (row, factor): idx = argmax(softmax(logits) / q), q ~ Exp(1) --
//            torch.multinomial's single-draw path.  The state that continues is the one-hot forward value: no
//            straight-through term in a no-grad rollout.  The draws q are eps_state [H x rows x S] (parity path), or --
//            eps_state == NULL -- generated here from the Philox4x32-10 stream (seed, step, stream_id) with the element
//            layout of bd_rng_fill(BD_RNG_EXPONENTIAL, count = H*rows*S): bit-identical to a run fed that buffer, and the
//            61 MB per iteration (H 15, 1000 candidates, 32 x 32) never exist in HBM.  The unfused form also writes the
//            class indices (sidx), which the host's reward chain gathers by.
//   bd_cem_refit: per environment, pick the `top` candidates by return (src/planner.py:74-76) and refit the action
//     belief to them: mean and biased std over the selected sequences (src/planner.py:81-87).
//
// LDS budget of the rollout (floats; Kb_x = ceil(x / 16), 256 floats per fragment block, 8 waves), PlanDims:
//     h_cur, h_nxt, x            3 * Kb_h * 256
//     bufA, bufB                 2 * Kb_hd * 256          prior hidden, reward-model activations
//     action fragments           Kb_a * 256
//     state                      !LC: (Kb_s + Kb_f) * 256   the state tile and ff = [h'; s'], Kb_f = ceil((Be+S) / 16)
//                                LC:  16 * max(Be, Hd) + 2 * 16 * D   xs: the gathered state columns of the layer at
//                                     hand; then the factors' weights and class indices
//     returns                    16
//     uni                        !LC: kSplitScratchFloats = 10240   split-K partials and the dual head's plain area
//                                LC:  max(kSplitScratchFloats, 16 * (ceil(S / 16) * 16 + 8))
//                                     three tenants in disjoint phases: GRU block-12 scratch | logits image | split-K partials
//   Gaussian, Be = Hd = 200, S = 30, A <= 16:  (39 + 26 + 1 + 2 + 15) * 256 + 16 + 10240 = 31504 floats = 126 016 B.
//   Be = Hd = 200, 32 x 32, A <= 16:  (39 + 26 + 1) * 256 + 3200 + 1024 + 16 + 16512 = 37648 floats = 150 592 B of the
//   160 KiB a workgroup may use on gfx950.  Either way: one workgroup per CU.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_categorical.h"
#include "bd_rng.h"

namespace bd {

struct PlanDims {
    int Kb_h, Kb_s, Kb_a, Kb_hd, Kb_f;
    int n_xs;                // LC: floats of the gathered-columns tile [16][max(Be, Hd)]
    int n_state, n_uni;      // floats of the state region and of the scratch | logits image region
    __host__ __device__ PlanDims(int Be, int D, int C, int S, int A, int Hd, bool lc)
        : Kb_h(cdiv(Be, 16)), Kb_s(cdiv(S, 16)), Kb_a(cdiv(A, 16)), Kb_hd(cdiv(Hd, 16)), Kb_f(cdiv(Be + S, 16)),
          n_xs(16 * (Be > Hd ? Be : Hd)) {
        const int img = lc ? CatFull(D, C).image_floats() : 0;
        n_state = lc ? n_xs + 2 * 16 * D : (Kb_s + Kb_f) * kFragFloats;
        n_uni = kSplitScratchFloats > img ? kSplitScratchFloats : img;
    }
    __host__ __device__ size_t lds_floats() const {      // every term is a multiple of 16 floats
        return (size_t)(3 * Kb_h + 2 * Kb_hd + Kb_a) * kFragFloats + (size_t)n_state + 16 + (size_t)n_uni;
    }
};

template <bool LC>
__global__ __launch_bounds__(kThreads) void plan_rollout_kernel(bd_plan_args a_) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    BD_KARGS(bd_plan_args, ap);
#define a (*ap)
    const PlanDims d(a.Be, a.D, a.C, a.S, a.A, a.Hd, LC);
    const CatGeo g(LC ? a.D : 1, LC ? a.C : 1);
    const CatFull gf(g.D, g.C);
    const int row0 = blockIdx.x * 16;
    // S stays in a register over the phases (LC: as D*C, what the validator holds a.S to): re-read from the block in
    // every phase that uses it, the Categorical rollout measured 0.8 % slower per plan (profiles/r13_README.md)
    const int S = LC ? g.S : a.S, F = a.Be + S;
    const int nh = d.Kb_h * kFragFloats, nhd = d.Kb_hd * kFragFloats;
    const int rows_valid = a.rows - row0 < 16 ? a.rows - row0 : 16;
    float* h_cur = smem;
    float* h_nxt = h_cur + nh;
    float* xf = h_nxt + nh;
    float* bufA = xf + nh;
    float* bufB = bufA + nhd;
    float* af = bufB + nhd;
    float* sf = af + d.Kb_a * kFragFloats;        // !LC: the state tile
    float* ff = sf + d.Kb_s * kFragFloats;        // !LC: [h'; s'] as ONE K range: the reward model's first layer is packed over Be+S
    float* xs = sf;                               // LC: [16][max(Be, Hd)], then [16][D] weights and [16][D] class indices
    float* sw_l = xs + d.n_xs;
    int* sidx_l = reinterpret_cast<int*>(sw_l + 16 * g.D);
    float* ret_s = sf + d.n_state;                // [16] returns
    float* uni = ret_s + 16;                      // split-K partials; LC also GRU scratch | logits image (16-byte aligned)
    float* lg = uni;

    // every candidate of environment b starts from the same belief / state (src/planner.py:37-38)
    for (int i = threadIdx.x; i < 16 * d.Kb_h * 16; i += blockDim.x) {
        const int r = i / (d.Kb_h * 16), k = i - r * (d.Kb_h * 16), grow = row0 + r;
        h_cur[frag_idx(r, k)] = (grow < a.rows && k < a.Be) ? a.init_belief[(size_t)(grow / a.cand) * a.Be + k] : 0.f;
    }
    if constexpr (LC) {
        // start state: per factor all-zero (fed as zeros) or (scaled) one-hot -- the rule of state_to_indices
        for (int i = threadIdx.x; i < 16 * g.D; i += blockDim.x) {
            const int row = i / g.D, f = i - row * g.D;
            float best = 0.f;
            int arg = 0;
            if (row < rows_valid) {
                const float* p = a.init_state + (size_t)((row0 + row) / a.cand) * a.S + f * g.C;
                for (int c = 0; c < g.C; ++c)
                    if (fabsf(p[c]) > fabsf(best)) { best = p[c]; arg = c; }
            }
            sidx_l[i] = arg;
            sw_l[i] = best;
        }
    } else {
        for (int i = threadIdx.x; i < 16 * d.Kb_s * 16; i += blockDim.x) {
            const int r = i / (d.Kb_s * 16), k = i - r * (d.Kb_s * 16), grow = row0 + r;
            sf[frag_idx(r, k)] = (grow < a.rows && k < a.S) ? a.init_state[(size_t)(grow / a.cand) * a.S + k] : 0.f;
        }
        for (int i = threadIdx.x; i < d.Kb_f * kFragFloats; i += blockDim.x) ff[i] = 0.f;   // k >= Be+S stays zero
    }
    if (threadIdx.x < 16) ret_s[threadIdx.x] = 0.f;
    lds_barrier();

    const GruW gw{a.w_ir, a.w_iz, a.w_in, a.w_hr, a.w_hz, a.w_hn, a.b_ih, a.b_hh};
    const int B = a.rows / a.cand;
    const Rng rng{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stream_id, (uint32_t)a.step};      // LC, eps_state == null

    for (int t = 0; t < a.H; ++t) {
        const size_t tn = (size_t)t * a.rows;
        const int tid = bd_tid();                 // opaque: nothing thread-dependent leaves this step (bd_tid)
        const int lane = tid & 63;
        BD_KARGS_FRESH(ap);
        // ---- candidate actions (src/planner.py:60-62); LC: W_es s as a gather ----
        for (int i = tid; i < 16 * d.Kb_a * 16; i += blockDim.x) {
            const int r = i / (d.Kb_a * 16), k = i - r * (d.Kb_a * 16), grow = row0 + r;
            float v = 0.f;
            if (grow < a.rows && k < a.A) {
                const size_t mi = ((size_t)t * B + grow / a.cand) * a.A + k;
                v = a.act_mean[mi] + a.act_std[mi] * a.eps_action[(tn + grow) * a.A + k];
                a.actions[(tn + grow) * a.A + k] = v;
            }
            af[frag_idx(r, k)] = v;
        }
        if constexpr (LC) state_gather(g, a.w_embed_sT, a.Be, sidx_l, sw_l, nullptr, xs);
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- x = ELU(W_e [s; a] + b_e) ----
        if constexpr (LC) {
            const Seg segs[1] = {{af, a.w_embed_a, d.Kb_a}};
            tile_linear_seg<1>(segs, a.b_embed, a.Be, [&](int nb, floatx4 acc) {
                const int col = nb * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r;
                    const bool ok = row < rows_valid && col < a.Be;
                    xf[acc_frag_off(nb, lane, r)] = ok ? elu(acc[r] + xs[row * a.Be + col]) : 0.f;
                }
            });
        } else {
            const Seg segs[2] = {{sf, a.w_embed_s, d.Kb_s}, {af, a.w_embed_a, d.Kb_a}};
            tile_linear_seg<2>(segs, a.b_embed, a.Be, [&](int nb, floatx4 acc) {
                const int col = nb * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = 4 * (lane >> 4) + r < rows_valid && col < a.Be;
                    xf[acc_frag_off(nb, lane, r)] = ok ? elu(acc[r]) : 0.f;
                }
            });
        }
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- GRU ----
        gru_tile(xf, h_cur, d.Kb_h, a.Be, gw, [&](int nb, floatx4 R, floatx4 Z, floatx4 NI, floatx4 NH) {
            const int col = nb * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * (lane >> 4) + r;
                const int off = acc_frag_off(nb, lane, r);
                const float rr = sigmoidf(R[r]), zz = sigmoidf(Z[r]);
                const float nn = tanh_act(NI[r] + rr * NH[r]);
                const bool ok = row < rows_valid && col < a.Be;
                const float hn = ok ? (1.f - zz) * nn + zz * h_cur[off] : 0.f;
                h_nxt[off] = hn;
                if constexpr (!LC)
                    if (col < a.Be) ff[frag_idx(row, col)] = hn;
                if (a.feat && ok) a.feat[(tn + row0 + row) * F + col] = hn;
            }
        }, uni);
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- prior hidden ----
        {
            const Seg segs[1] = {{h_nxt, a.w_p1, d.Kb_h}};
            tile_linear_seg<1>(segs, a.b_p1, a.Hd, [&](int nb, floatx4 acc) {
                const int col = nb * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = 4 * (lane >> 4) + r < rows_valid && col < a.Hd;
                    bufA[acc_frag_off(nb, lane, r)] = ok ? elu(acc[r]) : 0.f;
                }
            });
        }
        lds_barrier();
        BD_KARGS_FRESH(ap);
        if constexpr (LC) {
            // ---- prior logits (all S columns into the image), sample: idx = argmax(probs / q) per (row, factor) ----
            {
                const Seg seg[1] = {{bufA, a.w_p2, d.Kb_hd}};
                tile_linear_g<1, 1>(seg, a.b_p2, S, [&](int, int nb, floatx4 acc) {
                    const int col = nb * 16 + (lane & 15);
                    if (col >= S) return;
                    const int f = col / g.C, c = col - f * g.C;
#pragma unroll
                    for (int r = 0; r < 4; ++r) lg[gf.addr(4 * (lane >> 4) + r, f, c)] = acc[r];
                });
            }
            lds_barrier();
            for (int i = tid; i < 16 * g.D; i += blockDim.x) {
                const int row = i / g.D, f = i - row * g.D;
                int arg = 0;
                if (row < rows_valid) {
                    const size_t e0 = (tn + row0 + row) * S + f * g.C;      // first class of this factor in [H x rows x S]
                    if (a.eps_state) {
                        const float* qrow = a.eps_state + e0;
                        arg = g.C == 32 ? cat_sample_reg<32>(gf, lg, qrow, row, f) : cat_sample_any(gf, lg, qrow, row, f);
                    } else {
                        arg = g.C == 32 ? cat_sample_reg_rng<32>(gf, lg, rng, e0, row, f) : cat_sample_any_rng(gf, lg, rng, e0, row, f);
                    }
                    if (a.sidx) a.sidx[(tn + row0) * g.D + i] = (unsigned char)arg;
                }
                sidx_l[i] = arg;
                sw_l[i] = row < rows_valid ? 1.f : 0.f;      // a sampled state is one-hot whatever the start state's weights were
            }
            lds_barrier();
            BD_KARGS_FRESH(ap);
            if (a.feat) write_onehot(g, sidx_l, sw_l, nullptr, a.feat + (tn + row0) * F + a.Be, (size_t)F, rows_valid);
        } else {
            // ---- prior: s' = mean + std * eps ----
            const Seg2 segs[1] = {{bufA, a.w_p2m, a.w_p2s, d.Kb_hd}};
            tile_dual_head_elem<1>(
                segs, a.b_p2, a.b_p2 + S, S, uni,
                [&](int row, int col) { return row < rows_valid ? a.eps_state[(tn + row0 + row) * S + col] : 0.f; },
                [&](int row, int col, float Mn, float Rw, float eps) {
                    const float st = row < rows_valid ? Mn + (softplusf(Rw) + a.min_std) * eps : 0.f;
                    sf[frag_idx(row, col)] = st;
                    ff[frag_idx(row, a.Be + col)] = st;
                    if (a.feat && row < rows_valid) a.feat[(tn + row0 + row) * F + a.Be + col] = st;
                });
            lds_barrier();
        }
        // ---- reward model on [h'; s'] (skipped when the host runs it batched over all H steps: a.returns == null) ----
        if (a.returns) {
            if constexpr (LC) {
                state_gather(g, a.w_r0sT, a.Hd, sidx_l, sw_l, nullptr, xs);
                lds_barrier();
                const Seg s0[1] = {{h_nxt, a.w_r0h, d.Kb_h}};
                tile_linear_seg<1>(s0, a.b_r[0], a.Hd, [&](int nb, floatx4 acc) {
                    const int col = nb * 16 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        bufA[acc_frag_off(nb, lane, r)] = col < a.Hd ? elu(acc[r] + xs[(4 * (lane >> 4) + r) * a.Hd + col]) : 0.f;
                });
            } else {
                const Seg s0[1] = {{ff, a.w_r[0], d.Kb_f}};
                tile_linear_seg<1>(s0, a.b_r[0], a.Hd, [&](int nb, floatx4 acc) {
                    const int col = nb * 16 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) bufA[acc_frag_off(nb, lane, r)] = col < a.Hd ? elu(acc[r]) : 0.f;
                });
            }
            lds_barrier();
            BD_KARGS_FRESH(ap);
            float* src = bufA;
            float* dst = bufB;
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                const Seg sl[1] = {{src, a.w_r[l], d.Kb_hd}};
                tile_linear_seg<1>(sl, a.b_r[l], a.Hd, [&](int nb, floatx4 acc) {
                    const int col = nb * 16 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[acc_frag_off(nb, lane, r)] = col < a.Hd ? elu(acc[r]) : 0.f;
                });
                lds_barrier();
                float* tmp = src; src = dst; dst = tmp;
            }
            const Seg so[1] = {{src, a.w_r[4], d.Kb_hd}};
            tile_linear_seg<1>(so, a.b_r[4], 1, [&](int nb, floatx4 acc) {
                if (nb == 0 && (lane & 15) == 0) {       // column 0: one lane per group of four rows
#pragma unroll
                    for (int r = 0; r < 4; ++r) ret_s[4 * (lane >> 4) + r] += acc[r];      // sum over the horizon (:72)
                }
            }, uni);
            lds_barrier();
        }
        float* tmp = h_cur; h_cur = h_nxt; h_nxt = tmp;
    }
    if (a.returns && threadIdx.x < 16 && row0 + threadIdx.x < a.rows) a.returns[row0 + threadIdx.x] = ret_s[threadIdx.x];
#undef a
}

// ---- CEM refit ---------------------------------------------------------------------------------------------
// One workgroup per environment.  Candidates are ordered by (return, lower index first; a NaN return ranks first, as
// torch.topk orders it) with a bitonic sort of 64-bit keys in LDS -- (order-preserving image of the float) << 32 |
// ~index -- padded to a power of two with keys below every real one; the first `top` entries are the selection, and
// every (t, a) pair is reduced over them by one wave.
// The image ranks +0 strictly above -0, the documented order does not: it holds because the caller's sum starts from 0.f
// (0.f + -0.f = +0.f, IEEE addition, no fast-math), so x is never -0 (tests/test_plan_kernels_gpu.py, the "zeros" returns).
__device__ __forceinline__ unsigned long long refit_key(float x, int i) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0xFFFFFFFFu;
    else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

__global__ __launch_bounds__(1024) void cem_refit_kernel(const float* __restrict__ returns, int ret_steps,
                                                         const float* __restrict__ actions, int H, int B, int cand, int top,
                                                         int A, int n2, float* __restrict__ mean, float* __restrict__ stdev) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [n2]
    __shared__ int idx[1024];                                                    // selected candidates (top <= 1024)
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        unsigned long long key = 0ull;
        if (i < cand) {                                 // return = sum of the per-step rewards (src/planner.py:72)
            float r = 0.f;
            for (int t = 0; t < ret_steps; ++t) r += returns[((size_t)t * B + b) * cand + i];
            key = refit_key(r, i);
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                const int q = i ^ j;
                if (q > i) {
                    const unsigned long long x = keys[i], y = keys[q];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) {
                        keys[i] = y;
                        keys[q] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int j = threadIdx.x; j < top; j += blockDim.x) idx[j] = (int)(0xFFFFFFFFu - (unsigned)(keys[j] & 0xFFFFFFFFull));
    __syncthreads();
    // one wave per (t, a) pair, lanes over the selected candidates: two load rounds per pair instead of 2 * top
    // dependent ones
    const size_t rows = (size_t)B * cand;
    const float inv = 1.f / (float)top;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int p = wave; p < H * A; p += nwaves) {
        const int t = p / A, k = p - t * A;
        const float* base = actions + ((size_t)t * rows + (size_t)b * cand) * A + k;
        float s = 0.f;
        for (int j = lane; j < top; j += 64) s += base[(size_t)idx[j] * A];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float m = s * inv;
        float v = 0.f;
        for (int j = lane; j < top; j += 64) {
            const float dlt = base[(size_t)idx[j] * A] - m;
            v += dlt * dlt;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) {
            const size_t o = ((size_t)t * B + b) * A + k;
            mean[o] = m;
            stdev[o] = sqrtf(v * inv);                    // std(unbiased=False), src/planner.py:87
        }
    }
}

template <bool LC>
static int plan_launch(const char* who, const bd_plan_args& a, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024 && allow_big_lds(plan_rollout_kernel<LC>)) return -1;
    hipLaunchKernelGGL((plan_rollout_kernel<LC>), dim3(cdiv(a.rows, 16)), dim3(kThreads), lds, stream, a);
    BD_CHECK_LAUNCH(who);
    return 0;
}

// the checks of both entry points (`who` names the one that was called, `lc` the latent kind it takes), then the launch.
// The dims come before the kind: a zeroed block is "bad dims" at either entry point.
static int plan_rollout(const char* who, bool lc, const bd_plan_args* a, hipStream_t stream) {
    BD_REQUIRE(a, "%s: null argument block", who);
    BD_REQUIRE(a->rows > 0 && a->H > 0 && a->cand > 0 && a->rows % a->cand == 0 && a->Be > 0 && a->S > 0 && a->A > 0 && a->Hd > 0 &&
                   (!a->latent_cat || (a->D > 0 && a->C > 0)), "%s: bad dims", who);
    BD_REQUIRE((a->latent_cat != 0) == lc, "%s: takes latent_cat %s; %s latents are %s", who, lc ? "!= 0 (Categorical latents)"
               : "= 0 (Gaussian latents)", lc ? "Gaussian" : "Categorical", lc ? "bd_plan_rollout" : "bd_plan_rollout_cat");
    if (lc)
        BD_REQUIRE((long long)a->D * a->C == a->S && CatGeo(a->D, a->C).ok(),
                   "%s: %d x %d latents with S = %d unsupported (S = D*C; C <= 256; S <= 256, or 256 %% C == 0 and S %% 16 == 0)", who,
                   a->D, a->C, a->S);
    else
        BD_REQUIRE(a->S <= kHeadMaxN, "%s: state_size %d > %d", who, a->S, kHeadMaxN);
    const size_t lds = PlanDims(a->Be, a->D, a->C, a->S, a->A, a->Hd, lc).lds_floats() * sizeof(float);
    BD_REQUIRE(lds <= (size_t)kMaxLds, "%s: needs %zu B of LDS (limit %d)", who, lds, kMaxLds);
    BD_REQUIRE(a->w_embed_a && a->b_embed && a->w_ir && a->w_iz && a->w_in && a->w_hr && a->w_hz && a->w_hn && a->b_ih && a->b_hh &&
                   a->w_p1 && a->b_p1 && a->b_p2 && (lc ? (a->w_embed_sT && a->w_p2) : (a->w_embed_s && a->w_p2m && a->w_p2s)),
               "%s: missing transition weights", who);
    if (a->returns)
        for (int l = 0; l < 5; ++l)
            BD_REQUIRE((l == 0 && lc ? (a->w_r0h && a->w_r0sT) : a->w_r[l] != nullptr) && a->b_r[l],
                       "%s: missing reward weights (layer %d)", who, l);
    BD_REQUIRE(a->init_belief && a->init_state && a->act_mean && a->act_std && a->eps_action && (lc || a->eps_state),
               "%s: missing inputs", who);
    BD_REQUIRE(a->eps_state || a->S % 4 == 0, "%s: in-kernel sampler noise (eps_state = NULL) needs D*C %% 4 == 0, got %d x %d", who,
               a->D, a->C);
    BD_REQUIRE(a->actions && (a->returns || (a->feat && (!lc || a->sidx))),
               "%s: missing outputs (actions and returns, or actions, feat and -- Categorical latents -- sidx)", who);
    return lc ? plan_launch<true>(who, *a, lds, stream) : plan_launch<false>(who, *a, lds, stream);
}

}  // namespace bd

extern "C" {
using namespace bd;

int bd_plan_rollout(const bd_plan_args* a, void* stream) { return plan_rollout("bd_plan_rollout", false, a, (hipStream_t)stream); }

int bd_plan_rollout_cat(const bd_plan_cat_args* a, void* stream) {
    return plan_rollout("bd_plan_rollout_cat", true, a, (hipStream_t)stream);
}

int bd_cem_refit(const float* returns, int ret_steps, const float* actions, int H, int B, int cand, int top, int A,
                 float* mean, float* stdev, void* stream) {
    BD_REQUIRE(returns && ret_steps > 0 && actions && mean && stdev && H > 0 && B > 0 && cand > 0 && A > 0,
               "bd_cem_refit: bad arguments");
    BD_REQUIRE(top > 0 && top <= cand, "bd_cem_refit: top_candidates %d must be in 1..%d", top, cand);
    BD_REQUIRE(top <= 1024 && cand <= 4096, "bd_cem_refit: at most 4096 candidates / 1024 top candidates (got %d / %d)", cand,
               top);
    int n2 = 2;
    while (n2 < cand) n2 <<= 1;
    const size_t lds = (size_t)n2 * sizeof(unsigned long long);
    hipLaunchKernelGGL(cem_refit_kernel, dim3(B), dim3(1024), lds, (hipStream_t)stream, returns, ret_steps, actions, H, B, cand,
                       top, A, n2, mean, stdev);
    BD_CHECK_LAUNCH("bd_cem_refit");
    return 0;
}

}  // extern "C"
