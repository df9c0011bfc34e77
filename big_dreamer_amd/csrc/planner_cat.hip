// planner_cat.hip -- the CEM planner's rollout for latent_distribution="Categorical" (MPCPlanner.forward,
// src/planner.py:28-90, on a TransitionModel with CategoricalBeliefModel heads, src/models.py:76-117):
//
//   bd_plan_rollout_cat: one persistent launch per CEM iteration, same ownership as bd_plan_rollout (planner.hip): a
//     workgroup owns 16 candidate action sequences for all H planning steps, belief in LDS in MFMA fragment order, weights
//     stream from L2.  What the one-hot state changes is what it changes in the imagination scan (scan_cat.hip):
//       * the state is D class indices per row (+ one weight per factor: 1 after a sample, the stored value / 0 for the
//         caller's start state); W_es s of the embed layer and the state columns of the reward model's first layer are
//         GATHERS of D rows of the plain transposed weights, not K = D*C contractions;
//       * the prior head is hidden -> D*C logits into a swizzled LDS image (bd_categorical.h, CatFull), then one thread per
//         (row, factor): softmax and idx = argmax(probs / q), q ~ Exp(1) -- torch.multinomial's single-draw path.  The
//         state that continues is the one-hot forward value: no straight-through term in a no-grad rollout.
//     The draws q are an explicit input [H x rows x S] (parity path), or -- q_prior == NULL -- generated here from the
//     Philox4x32-10 stream (seed, step, stream_id) with the element layout of bd_rng_fill(BD_RNG_EXPONENTIAL, count =
//     H*rows*S): bit-identical to a run fed that buffer, and the 61 MB per iteration (H 15, 1000 candidates, 32 x 32)
//     never exist in HBM.
//     returns == NULL selects the unfused form as in bd_plan_rollout: the kernel writes feat = [h'; one-hot s'] and the
//     class indices, and the host runs the reward model as one dense chain over all H x rows rows.
//
// LDS budget (floats; Kb_x = ceil(x / 16), 256 floats per fragment block, 8 waves):
//     h_cur, h_nxt, x            3 * Kb_h * 256
//     bufA, bufB                 2 * Kb_hd * 256          prior hidden, reward-model activations
//     action fragments           Kb_a * 256
//     xs                         16 * max(Be, Hd)         gathered state columns of the layer at hand
//     sw, sidx                   2 * 16 * D
//     returns                    16
//     uni                        max(kSplitScratchFloats, 16 * (ceil(S / 16) * 16 + 8))
//                                three tenants in disjoint phases: GRU block-12 scratch | logits image | split-K partials
//   Be = Hd = 200, 32 x 32, A <= 16:  (39 + 26 + 1) * 256 + 3200 + 1024 + 16 + 16512 = 37648 floats = 150 592 B of the
//   160 KiB a workgroup may use on gfx950: one workgroup per CU.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_categorical.h"
#include "bd_rng.h"

namespace bd {

__global__ __launch_bounds__(kThreads) void plan_rollout_cat_kernel(bd_plan_cat_args a_) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    BD_KARGS(bd_plan_cat_args, ap);
#define a (*ap)
    const CatGeo g(a.D, a.C);
    const CatFull gf(a.D, a.C);
    const int Kb_h = cdiv(a.Be, 16), Kb_a = cdiv(a.A, 16), Kb_hd = cdiv(a.Hd, 16);
    const int row0 = blockIdx.x * 16;
    const int S = g.S, F = a.Be + S;
    const int nh = Kb_h * kFragFloats, nhd = Kb_hd * kFragFloats;
    const int rows_valid = a.rows - row0 < 16 ? a.rows - row0 : 16;
    const int wmax = a.Be > a.Hd ? a.Be : a.Hd;
    float* h_cur = smem;
    float* h_nxt = h_cur + nh;
    float* xf = h_nxt + nh;
    float* bufA = xf + nh;
    float* bufB = bufA + nhd;
    float* af = bufB + nhd;
    float* xs = af + Kb_a * kFragFloats;          // [16][max(Be, Hd)]
    float* sw_l = xs + 16 * wmax;                 // [16][D]
    int* sidx_l = reinterpret_cast<int*>(sw_l + 16 * g.D);
    float* ret_s = reinterpret_cast<float*>(sidx_l + 16 * g.D);   // [16] returns
    float* uni = ret_s + 16;                      // GRU scratch | logits image | split-K partials (16-byte aligned)
    float* lg = uni;

    // every candidate of environment b starts from the same belief / state (src/planner.py:37-38)
    for (int i = threadIdx.x; i < 16 * Kb_h * 16; i += blockDim.x) {
        const int r = i / (Kb_h * 16), k = i - r * (Kb_h * 16), grow = row0 + r;
        h_cur[frag_idx(r, k)] = (grow < a.rows && k < a.Be) ? a.init_belief[(size_t)(grow / a.cand) * a.Be + k] : 0.f;
    }
    // start state: per factor all-zero (fed as zeros) or (scaled) one-hot -- the rule of state_to_indices
    for (int i = threadIdx.x; i < 16 * g.D; i += blockDim.x) {
        const int row = i / g.D, f = i - row * g.D;
        float best = 0.f;
        int arg = 0;
        if (row < rows_valid) {
            const float* p = a.init_state + (size_t)((row0 + row) / a.cand) * S + f * g.C;
            for (int c = 0; c < g.C; ++c)
                if (fabsf(p[c]) > fabsf(best)) { best = p[c]; arg = c; }
        }
        sidx_l[i] = arg;
        sw_l[i] = best;
    }
    if (threadIdx.x < 16) ret_s[threadIdx.x] = 0.f;
    lds_barrier();

    const GruW gw{a.w_ir, a.w_iz, a.w_in, a.w_hr, a.w_hz, a.w_hn, a.b_ih, a.b_hh};
    const int B = a.rows / a.cand;
    const Rng rng{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stream_id, (uint32_t)a.step};

    for (int t = 0; t < a.H; ++t) {
        const size_t tn = (size_t)t * a.rows;
        const int tid = bd_tid();                 // opaque: nothing thread-dependent leaves this step (bd_tid)
        const int lane = tid & 63;
        BD_KARGS_FRESH(ap);
        // ---- candidate actions (src/planner.py:60-62); W_es s as a gather ----
        for (int i = tid; i < 16 * Kb_a * 16; i += blockDim.x) {
            const int r = i / (Kb_a * 16), k = i - r * (Kb_a * 16), grow = row0 + r;
            float v = 0.f;
            if (grow < a.rows && k < a.A) {
                const size_t mi = ((size_t)t * B + grow / a.cand) * a.A + k;
                v = a.act_mean[mi] + a.act_std[mi] * a.eps_action[(tn + grow) * a.A + k];
                a.actions[(tn + grow) * a.A + k] = v;
            }
            af[frag_idx(r, k)] = v;
        }
        state_gather(g, a.w_embed_sT, a.Be, sidx_l, sw_l, nullptr, xs);
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- x = ELU(W_ea a + W_es s + b_e) ----
        {
            const Seg segs[1] = {{af, a.w_embed_a, Kb_a}};
            tile_linear_seg<1>(segs, a.b_embed, a.Be, [&](int nb, floatx4 acc) {
                const int col = nb * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r;
                    const bool ok = row < rows_valid && col < a.Be;
                    xf[acc_frag_off(nb, lane, r)] = ok ? elu(acc[r] + xs[row * a.Be + col]) : 0.f;
                }
            });
        }
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- GRU ----
        gru_tile(xf, h_cur, Kb_h, a.Be, gw, [&](int nb, floatx4 R, floatx4 Z, floatx4 NI, floatx4 NH) {
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
                if (a.feat && ok) a.feat[(tn + row0 + row) * F + col] = hn;
            }
        }, uni);
        lds_barrier();
        BD_KARGS_FRESH(ap);
        // ---- prior hidden ----
        {
            const Seg segs[1] = {{h_nxt, a.w_p1, Kb_h}};
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
        // ---- prior logits (all S columns into the image), sample: idx = argmax(probs / q) per (row, factor) ----
        {
            const Seg seg[1] = {{bufA, a.w_p2, Kb_hd}};
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
                if (a.q_prior) {
                    const float* qrow = a.q_prior + e0;
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
        // ---- reward model on [h'; one-hot s'] (skipped when the host runs it batched over all H steps: a.returns == null) ----
        if (a.returns) {
            state_gather(g, a.w_r0sT, a.Hd, sidx_l, sw_l, nullptr, xs);
            lds_barrier();
            const Seg s0[1] = {{h_nxt, a.w_r0h, Kb_h}};
            tile_linear_seg<1>(s0, a.b_r[0], a.Hd, [&](int nb, floatx4 acc) {
                const int col = nb * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    bufA[acc_frag_off(nb, lane, r)] = col < a.Hd ? elu(acc[r] + xs[(4 * (lane >> 4) + r) * a.Hd + col]) : 0.f;
            });
            lds_barrier();
            BD_KARGS_FRESH(ap);
            float* src = bufA;
            float* dst = bufB;
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                const Seg sl[1] = {{src, a.w_r[l - 1], Kb_hd}};
                tile_linear_seg<1>(sl, a.b_r[l], a.Hd, [&](int nb, floatx4 acc) {
                    const int col = nb * 16 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[acc_frag_off(nb, lane, r)] = col < a.Hd ? elu(acc[r]) : 0.f;
                });
                lds_barrier();
                float* tmp = src; src = dst; dst = tmp;
            }
            const Seg so[1] = {{src, a.w_r[3], Kb_hd}};
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

}  // namespace bd

extern "C" {
using namespace bd;

int bd_plan_rollout_cat(const bd_plan_cat_args* a, void* stream) {
    BD_REQUIRE(a && a->rows > 0 && a->H > 0 && a->cand > 0 && a->rows % a->cand == 0 && a->Be > 0 && a->D > 0 && a->C > 0 &&
                   a->A > 0 && a->Hd > 0, "bd_plan_rollout_cat: bad dims");
    const CatGeo g(a->D, a->C);
    BD_REQUIRE(g.ok(), "bd_plan_rollout_cat: %d x %d latents unsupported (C <= 256; S <= 256, or 256 %% C == 0 and S %% 16 == 0)",
               a->D, a->C);
    BD_REQUIRE(a->w_embed_sT && a->w_embed_a && a->b_embed && a->w_ir && a->w_iz && a->w_in && a->w_hr && a->w_hz && a->w_hn &&
                   a->b_ih && a->b_hh && a->w_p1 && a->b_p1 && a->w_p2 && a->b_p2, "bd_plan_rollout_cat: missing transition weights");
    BD_REQUIRE(a->init_belief && a->init_state && a->act_mean && a->act_std && a->eps_action, "bd_plan_rollout_cat: missing inputs");
    BD_REQUIRE(a->q_prior || g.S % 4 == 0,
               "bd_plan_rollout_cat: in-kernel sampler noise (q_prior = NULL) needs D*C %% 4 == 0, got %d x %d", a->D, a->C);
    BD_REQUIRE(a->actions && (a->returns || (a->feat && a->sidx)),
               "bd_plan_rollout_cat: missing outputs (actions and returns, or actions, feat and sidx)");
    if (a->returns) {
        BD_REQUIRE(a->w_r0h && a->w_r0sT && a->b_r[0], "bd_plan_rollout_cat: missing reward weights (layer 0)");
        for (int l = 1; l < 5; ++l)
            BD_REQUIRE(a->w_r[l - 1] && a->b_r[l], "bd_plan_rollout_cat: missing reward weights (layer %d)", l);
    }
    const int Kb_h = cdiv(a->Be, 16), Kb_a = cdiv(a->A, 16), Kb_hd = cdiv(a->Hd, 16);
    const int wmax = a->Be > a->Hd ? a->Be : a->Hd;
    const CatFull gf(a->D, a->C);
    size_t uni = (size_t)kSplitScratchFloats;
    if ((size_t)gf.image_floats() > uni) uni = (size_t)gf.image_floats();
    const size_t lds = ((size_t)(3 * Kb_h + 2 * Kb_hd + Kb_a) * kFragFloats + (size_t)16 * wmax + (size_t)2 * 16 * g.D + 16 + uni) *
                       sizeof(float);      // every term is a multiple of 16 floats
    BD_REQUIRE(lds <= (size_t)kMaxLds, "bd_plan_rollout_cat: needs %zu B of LDS (limit %d)", lds, kMaxLds);
    if (lds > 64 * 1024 && allow_big_lds(plan_rollout_cat_kernel)) return -1;
    hipLaunchKernelGGL(plan_rollout_cat_kernel, dim3(cdiv(a->rows, 16)), dim3(kThreads), lds, (hipStream_t)stream, *a);
    BD_CHECK_LAUNCH("bd_plan_rollout_cat");
    return 0;
}

}  // extern "C"
