// act.hip -- one decision of the collect / evaluation loop in ONE launch: Planet.update_belief_and_act
// (src/planet.py:370-403) with Dreamer.get_action (src/dreamer.py:429-444), for the four configurations of
// latent_distribution = Gaussian | Categorical (TransitionModel.forward's Categorical branches, src/models.py:226-228,258-260,
// 269-271; CategoricalBeliefModel, src/models.py:101-117) and action_distribution = tanh-Normal | Categorical
// (src/models.py:506-522).
//
//   One kernel body, act_step_kernel<LC, AC>, templated on the latent kind LC and the actor kind AC; all four are
//     instantiated.  bd_act_step launches (0, 0), bd_act_step_cat the other three.  A workgroup owns 16 environments; every
//     activation of the step stays in LDS in MFMA fragment order, the weights (3.9 MB at the reference's default sizes)
//     stream once from L2.  At B <= 16 the step is a single CU walking a chain of thirteen dependent layers.  Per tile:
//       e  = encoder(obs)                    DenseModel 4 x (Linear+ELU) + Linear (src/models.py:365-408), or a ready
//                                            embedding (pixel observations: the conv stack has run)
//       x  = ELU(W_es s + W_ea a + b_e);  h' = GRUCell(x, h)                       (src/models.py:251-252)
//            LC: the incoming state [B x S] (per factor all-zero or one-hot) becomes class indices (state_to_indices) and
//            W_es s a gather of D rows of the plain transpose embed_sT (bd_categorical.h), as in the scans
//       q  = ELU(W_q1 [h'; e] + b)                                                 (src/models.py:266-267)
//            !LC: s' = mean_q + std_q * eps_post                                   (src/models.py:70-73)
//            LC: all D*C logits into the swizzled CatFull image, one thread per (row, factor) takes argmax(probs / q),
//            first maximum winning: cat_sample_reg / cat_sample_any, the operation order of the scans; s' = the one-hot
//       actor: 4 x (Linear+ELU) on [h'; s'] (LC: the state columns of layer 0 are a gather of a0sT rows), then
//            !AC: mean = 5 tanh(m/5), std = softplus(r + c0) + 1e-4, a' = tanh(mean + std * eps_action)
//                 (src/models.py:506-517, src/dreamer.py:443); explore: a' = clamp(a' + action_noise * eps_explore, -1, 1)
//                 (src/planet.py:388-392)
//            AC:  norm = out - logsumexp(out), p = softmax(norm), k = argmax(p / eps_action) (bd_discrete.h, one lane per
//                 class), a' = (onehot(k) + p) - p in that order; explore: epsilon-greedy -- with (u, v) the row's two
//                 uniforms, u < action_noise replaces a' by the exact one-hot of class min(floor(v A), A - 1)
//     What the composed path computes besides and nobody reads is left out: the prior head of the belief update and its
//     sample (src/models.py:256: with an embedding the posterior sample is the state that continues), the prior sample of
//     get_action's one imagination step and the actor entropy (src/planet.py:386 drops it).  None of them feeds belief,
//     state or action, so the three outputs are exactly the composed path's.
//   The evaluation policy (the block's tail: action_mode, latent_mean; include/bigdreamer_hip.h) is a THIRD template
//     parameter EV: act_step_kernel<LC, AC, false> are the four sampling kernels, which look at none of it; a block with
//     anything of the tail set launches <LC, AC, true>, the same body with
//       latent_mean            !LC: eps_post = 0 (s' = mean_q)      LC: q = 1 (per-factor argmax of the posterior logits)
//       BD_POLICY_MEAN         !AC: a' = tanh(mean + std * 0)       AC: the exact one-hot of argmax p (q = 1)
//       BD_POLICY_MODE         !AC: SampleDist.mode (src/models.py:708-723) -- the row's (mean, std) go to LDS (the head of
//                              the split-K partials, dead by then), one wave per row picks among n_mode draws
//                              (tanh_normal_mode_index, also behind bd_tanh_normal_mode)      AC: as BD_POLICY_MEAN
//     and exploration on top as in the sampling step.
//   Noise: explicit buffers, or (all NULL) Philox4x32-10 draws made in the kernel with the element layout of bd_rng_fill
//     (Exp(1) where a Categorical sampler consumes them, uniforms for epsilon-greedy, normals otherwise), so a run with
//     in-kernel noise equals, bit for bit, a run fed bd_rng_fill's buffers for the same (seed, step, stream).
//
// LDS budget (floats; Kb_x = ceil(x / 16), 256 floats per fragment block, 8 waves):
//     t0, t1, t2                 3 * max(Kb_h, Kb_hd) * 256     a belief-wide or a hidden-wide vector each; with LC t0 / t2
//                                also hold the two gathers' [16][out] sums
//     ef | logits image          max(max(Kb_e, Kb_o) * 256, LC ? 16 * (ceil(S / 16) * 16 + 8) : 0)
//                                observation (dead after the encoder's first layer), then the embedding; the embedding is
//                                dead once the posterior's first layer has read it: the image takes its place
//     state                      LC: 2 * 16 * D (class indices, weights)     !LC: Kb_s * 256 (fragment tile)
//     action fragments           Kb_a * 256
//     split-K scratch            kSplitScratchFloats = 10240    (its plain area also holds the actor's [16][A] logits)
//   Gaussian, Be = Hd = 200, E = 1024, S = 30, A = 1:  9984 + 16384 + 512 + 256 + 10240 = 37376 floats = 149 504 B.
//   Be = Hd = 200, E = 1024, 32 x 32, A = 18:  9984 + 16512 + 1024 + 512 + 10240 = 38272 floats = 153 088 B of the 160 KiB a
//   workgroup may use on gfx950 (with the embedding tile and the image side by side: 218 624 B).  A = 17, tanh-Normal: the same.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_scan.h"
#include "bd_categorical.h"
#include "bd_discrete.h"
#include "bd_rng.h"

namespace bd {

struct ActDims {
    int Kb_h, Kb_s, Kb_a, Kb_hd, Kb_e, Kb_o, Kb_g, Kb_io;
    int n_ef, n_state;       // floats of the embedding | image region and of the state region
    __host__ __device__ ActDims(int Be, int D, int C, int S, int A, int Hd, int E, int O, bool lc)
        : Kb_h(cdiv(Be, 16)), Kb_s(cdiv(S, 16)), Kb_a(cdiv(A, 16)), Kb_hd(cdiv(Hd, 16)), Kb_e(cdiv(E, 16)), Kb_o(cdiv(O, 16)),
          Kb_g(Kb_h > Kb_hd ? Kb_h : Kb_hd), Kb_io(Kb_e > Kb_o ? Kb_e : Kb_o) {
        const int img = lc ? CatFull(D, C).image_floats() : 0;
        n_ef = Kb_io * kFragFloats > img ? Kb_io * kFragFloats : img;
        n_state = lc ? 2 * 16 * D : Kb_s * kFragFloats;
    }
    __host__ __device__ size_t lds_floats() const {
        return (size_t)(3 * Kb_g + Kb_a) * kFragFloats + (size_t)n_ef + (size_t)n_state + kSplitScratchFloats;
    }
};

struct ActEps {
    float sample, explore;
};

enum { kDrawNormal = 0, kDrawExp = 1, kDrawUniform = 2 };      // the kinds of bd_rng_fill

// ---- the evaluation policy (bd_act_args' tail) ---------------------------------------------------------------------------
// element e of a standard-normal tensor: the caller's buffer, or what bd_rng_fill(BD_RNG_NORMAL) writes there
__device__ __forceinline__ float normal_at(const float* __restrict__ eps, const Rng& r, size_t e) {
    if (eps != nullptr) return eps[e];
    float v[4];
    rng_normal4(r, e >> 2, v);
    const int j = (int)(e & 3);
    return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
}

// The n draws of one row, layout (n, rows, A): draw j, column c.
struct ModeDraws {
    const float* eps;
    Rng rng;
    size_t rows, row;
    int A;
    __device__ __forceinline__ float operator()(int j, int c) const { return normal_at(eps, rng, ((size_t)j * rows + row) * A + c); }
};

// SampleDist.mode (src/models.py:708-723), the selection: of the n draws y_j = tanh(mean + sd * e_j) of ONE row the index
// of the largest tanh-Normal log-density summed over the A columns, the first maximum winning.  One wave: lane l takes
// draws l, l + 64, ... (a later pass replaces the lane's best only when strictly larger), walks the A columns with
// entropy_const / entropy_sample, then an xor butterfly in which the lower index wins a tie.  mean, sd: the row's A values
// (LDS or global).  Every lane returns the same index; a row whose sums are all NaN returns 0.
__device__ __forceinline__ int tanh_normal_mode_index(const float* mean, const float* sd, int A, int n, const ModeDraws& draws,
                                                      int lane) {
    float best = -INFINITY;
    int arg = n;
    for (int j = lane; j < n; j += 64) {
        float sum = 0.f;
        for (int c = 0; c < A; ++c) {
            const EntConst ec = entropy_const(mean[c], sd[c]);
            float lp, dm, ds;
            entropy_sample(ec, draws(j, c), lp, dm, ds);
            sum += lp;
        }
        if (sum > best) { best = sum; arg = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    return arg < n ? arg : 0;
}

// cat_sample_any with every draw q = 1 (the same operations in the same order; x / 1 is x): the first largest class
__device__ __forceinline__ int cat_argmax_any(const CatFull& g, const float* __restrict__ lg, int row, int f) {
    float m = -INFINITY;
    for (int c = 0; c < g.C; ++c) m = fmaxf(m, lg[g.addr(row, f, c)]);
    float s = 0.f;
    for (int c = 0; c < g.C; ++c) s += expf(lg[g.addr(row, f, c)] - m);
    const float lse = m + logf(s);
    const float m2 = m - lse;
    float s2 = 0.f;
    for (int c = 0; c < g.C; ++c) s2 += expf((lg[g.addr(row, f, c)] - lse) - m2);
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < g.C; ++c) {
        const float r = (expf((lg[g.addr(row, f, c)] - lse) - m2) / s2) / 1.f;
        if (r > best) { best = r; arg = c; }
    }
    return arg;
}

// bd_tanh_normal_mode: one wave per row, kWaves rows per workgroup
__global__ __launch_bounds__(kThreads) void tanh_normal_mode_kernel(const float* __restrict__ mean, const float* __restrict__ sd,
                                                                    const float* __restrict__ eps, Rng rng, int N, int A, int n,
                                                                    float* __restrict__ action, int* __restrict__ index) {
    const int lane = bd_tid() & 63;
    const size_t row = (size_t)blockIdx.x * kWaves + bd_wave(bd_tid());
    if (row >= (size_t)N) return;                 // wave-uniform
    const float* mr = mean + row * A;
    const float* sr = sd + row * A;
    const ModeDraws draws{eps, rng, (size_t)N, row, A};
    const int j = tanh_normal_mode_index(mr, sr, A, n, draws, lane);
    if (lane < A) action[row * A + lane] = tanh_act(mr[lane] + sr[lane] * draws(j, lane));
    if (lane == 0 && index != nullptr) index[row] = j;
}

// EV = false: the sampling step; the evaluation fields of the block are not looked at.  EV = true: the same body with
// action_mode / latent_mean honoured (a second set of instantiations: the sampling kernels' registers stay as they were).
template <bool LC, bool AC, bool EV>
__global__ __launch_bounds__(kThreads) void act_step_kernel(bd_act_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ActDims d(a.Be, a.D, a.C, a.S, a.A, a.Hd, a.E, a.O, LC);
    const int row0 = blockIdx.x * 16;
    const int rows_valid = a.B - row0 < 16 ? a.B - row0 : 16;
    const int ng = d.Kb_g * kFragFloats;
    float* t0 = smem;                             // encoder pong, embed gather, h' (kept to the end: the actor reads it)
    float* t1 = t0 + ng;                          // h, posterior hidden, actor ping
    float* t2 = t1 + ng;                          // encoder ping, x, actor gather, actor pong
    float* ef = t2 + ng;                          // obs -> embedding -> (LC) the logits image
    float* sf = ef + d.n_ef;                      // !LC: s, then s' (fragment tile)
    float* sw_l = sf;                             // LC: [16][D] weights, [16][D] class indices
    int* sidx_l = reinterpret_cast<int*>(sw_l + 16 * a.D);
    float* af = sf + d.n_state;
    float* scratch = af + d.Kb_a * kFragFloats;   // split-K partials (kSplitScratchFloats), 16-byte aligned
    const int lane = bd_tid() & 63;
    const CatGeo g(LC ? a.D : 1, LC ? a.C : 1);
    // element e of a noise tensor: the caller's buffer, or what bd_rng_fill writes there for `kind`
    auto draw_at = [&](const float* __restrict__ eps, unsigned stream, int kind, size_t e) -> float {
        if (eps != nullptr) return eps[e];
        const Rng r{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), stream, (uint32_t)a.step};
        float v[4];
        if (kind == kDrawExp) rng_exp4(r, e >> 2, v);
        else if (kind == kDrawUniform) rng_uniform4(r, e >> 2, v);
        else rng_normal4(r, e >> 2, v);
        const int j = (int)(e & 3);
        return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
    };
    auto draw = [&](const float* __restrict__ eps, unsigned stream, int kind, int width, int row, int col) -> float {
        return row0 + row < a.B ? draw_at(eps, stream, kind, (size_t)(row0 + row) * width + col) : 0.f;
    };
    auto hidden_epi = [&](float* dst, int width) { return HiddenEpiTR{dst, nullptr, 0, width, a.B, row0, lane}; };
    // hidden layer whose state columns were gathered into xs [16][width]: ELU(acc + xs) -> fragment tile
    auto gather_epi = [&](float* dst, const float* xs, int width) {
        return [dst, xs, width, lane, rok_rows = a.B - row0](int nb, floatx4 acc) {
            const int row = lane & 15, col0 = nb * 16 + 4 * (lane >> 4);
            const bool rok = row < rok_rows;
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (rok && col0 + r < width) ? elu(acc[r] + xs[row * width + col0 + r]) : 0.f;
            reinterpret_cast<floatx4*>(dst)[nb * 64 + lane] = v;
        };
    };

    load_tile_concat<1>(t1, d.Kb_h, row0, a.B, a.belief, a.Be, a.Be, nullptr, 0, 0);
    if constexpr (LC) state_to_indices(g, a.state, (size_t)a.S, row0, a.B, sidx_l, sw_l);
    else load_tile_concat<1>(sf, d.Kb_s, row0, a.B, a.state, a.S, a.S, nullptr, 0, 0);
    load_tile_concat<1>(af, d.Kb_a, row0, a.B, a.action, a.A, a.A, nullptr, 0, 0);
    if (a.obs != nullptr) load_tile_concat<1>(ef, d.Kb_o, row0, a.B, a.obs, a.O, a.O, nullptr, 0, 0);
    else load_tile_concat<1>(ef, d.Kb_e, row0, a.B, a.embedding, a.E, a.E, nullptr, 0, 0);
    lds_barrier();

    // ---- 1: encoder (state observations) ----
    if (a.obs != nullptr) {
        {
            const Seg segs[1] = {{ef, a.w_enc[0], d.Kb_o}};
            tile_linear_seg_tr<1>(segs, a.b_enc[0], a.Hd, hidden_epi(t2, a.Hd));
        }
        lds_barrier();
        float* src = t2;
        float* dst = t0;
        for (int l = 1; l < 4; ++l) {
            const Seg segs[1] = {{src, a.w_enc[l], d.Kb_hd}};
            tile_linear_seg_tr<1>(segs, a.b_enc[l], a.Hd, hidden_epi(dst, a.Hd));
            lds_barrier();
            float* tmp = src; src = dst; dst = tmp;
        }
        // three swaps: layer 3's activations are in t0; the output layer is linear
        const Seg segs[1] = {{t0, a.w_enc[4], d.Kb_hd}};
        tile_linear_seg_tr<1>(segs, a.b_enc[4], a.E, [&](int nb, floatx4 acc) {
            const int col0 = nb * 16 + 4 * (lane >> 4);
            const bool rok = row0 + (lane & 15) < a.B;
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (rok && col0 + r < a.E) ? acc[r] : 0.f;
            reinterpret_cast<floatx4*>(ef)[nb * 64 + lane] = v;
        });
        lds_barrier();
    }
    // ---- 2: x = ELU(W_e [s; a] + b_e);  h' = GRUCell(x, h) ----
    if constexpr (LC) {
        state_gather(g, a.w_embed_sT, a.Be, sidx_l, sw_l, nullptr, t0);      // t0 is free until the GRU's epilogue
        lds_barrier();
        const Seg segs[1] = {{af, a.w_embed_a, d.Kb_a}};
        tile_linear_seg_tr<1>(segs, a.b_embed, a.Be, gather_epi(t2, t0, a.Be));
    } else {
        const Seg segs[2] = {{sf, a.w_embed_s, d.Kb_s}, {af, a.w_embed_a, d.Kb_a}};
        tile_linear_seg_tr<2>(segs, a.b_embed, a.Be, hidden_epi(t2, a.Be));
    }
    lds_barrier();
    {
        const GruW gw{a.w_ir, a.w_iz, a.w_in, a.w_hr, a.w_hz, a.w_hn, a.b_ih, a.b_hh};
        gru_tile(t2, t1, d.Kb_h, a.Be, gw, [&](int nb, floatx4 R, floatx4 Z, floatx4 NI, floatx4 NH) {
            const int col = nb * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int grow = row0 + 4 * (lane >> 4) + r;
                const int off = acc_frag_off(nb, lane, r);
                const float rr = sigmoidf(R[r]), zz = sigmoidf(Z[r]);
                const float nn = tanh_act(NI[r] + rr * NH[r]);
                const float hn = (1.f - zz) * nn + zz * t1[off];
                const bool ok = grow < a.B && col < a.Be;
                t0[off] = ok ? hn : 0.f;
                if (ok) a.belief_out[(size_t)grow * a.Be + col] = hn;
            }
        }, scratch);
    }
    lds_barrier();
    // ---- 3: posterior on [h'; e]; the prior head is not evaluated ----
    {
        const Seg segs[2] = {{t0, a.w_q1h, d.Kb_h}, {ef, a.w_q1e, d.Kb_e}};
        tile_linear_seg_tr<2>(segs, a.b_q1, a.Hd, hidden_epi(t1, a.Hd));
    }
    lds_barrier();
    if constexpr (LC) {
        const CatFull gf(a.D, a.C);
        float* lg = ef;                           // the embedding is dead: its storage holds the logits image
        const Seg seg[1] = {{t1, a.w_q2, d.Kb_hd}};
        tile_linear_g<1, 1>(seg, a.b_q2, a.S, [&](int, int nb, floatx4 acc) {
            const int col = nb * 16 + (lane & 15);
            if (col >= a.S) return;
            const int f = col / a.C, c = col - f * a.C;
#pragma unroll
            for (int r = 0; r < 4; ++r) lg[gf.addr(4 * (lane >> 4) + r, f, c)] = acc[r];
        });
        lds_barrier();
        const Rng rng{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stream_post, (uint32_t)a.step};
        for (int i = bd_tid(); i < 16 * a.D; i += blockDim.x) {
            const int row = i / a.D, f = i - row * a.D;
            int arg = 0;
            if (row < rows_valid) {
                const size_t e0 = (size_t)(row0 + row) * a.S + f * a.C;      // first class of this factor in [B x S]
                if (EV && a.latent_mean) {      // q = 1 for every class
                    if (a.C == 32) {
                        __attribute__((aligned(16))) float ones[32];
#pragma unroll
                        for (int c = 0; c < 32; ++c) ones[c] = 1.f;
                        arg = cat_sample_reg<32>(gf, lg, ones, row, f);
                    } else {
                        arg = cat_argmax_any(gf, lg, row, f);
                    }
                } else if (a.eps_post) {
                    const float* qrow = a.eps_post + e0;
                    arg = a.C == 32 ? cat_sample_reg<32>(gf, lg, qrow, row, f) : cat_sample_any(gf, lg, qrow, row, f);
                } else {
                    arg = a.C == 32 ? cat_sample_reg_rng<32>(gf, lg, rng, e0, row, f) : cat_sample_any_rng(gf, lg, rng, e0, row, f);
                }
            }
            sidx_l[i] = arg;
            sw_l[i] = row < rows_valid ? 1.f : 0.f;      // a sampled state is one-hot whatever the incoming state's weights were
        }
        lds_barrier();
        write_onehot(g, sidx_l, sw_l, nullptr, a.state_out + (size_t)row0 * a.S, (size_t)a.S, rows_valid);
    } else {
        const Seg2 segs[1] = {{t1, a.w_q2m, a.w_q2s, d.Kb_hd}};
        tile_dual_head_elem<1>(
            segs, a.b_q2, a.b_q2 + a.S, a.S, scratch,
            [&](int row, int col) {
                if (EV && a.latent_mean) return 0.f;
                return draw(a.eps_post, a.stream_post, kDrawNormal, a.S, row, col);
            },
            [&](int row, int col, float Mn, float Rw, float eps) {
                const int grow = row0 + row;
                float st = 0.f;
                if (grow < a.B) {
                    st = Mn + (softplusf(Rw) + a.min_std) * eps;
                    a.state_out[(size_t)grow * a.S + col] = st;
                }
                sf[frag_idx(row, col)] = st;
            });
        lds_barrier();
    }
    // ---- 4: actor on [h'; s'] ----
    if constexpr (LC) {
        state_gather(g, a.w_a0sT, a.Hd, sidx_l, sw_l, nullptr, t2);         // x is dead since the GRU
        lds_barrier();
        const Seg segs[1] = {{t0, a.w_a0h, d.Kb_h}};
        tile_linear_seg_tr<1>(segs, a.b_a[0], a.Hd, gather_epi(t1, t2, a.Hd));
    } else {
        const Seg segs[2] = {{t0, a.w_a0h, d.Kb_h}, {sf, a.w_a0s, d.Kb_s}};
        tile_linear_seg_tr<2>(segs, a.b_a[0], a.Hd, hidden_epi(t1, a.Hd));
    }
    lds_barrier();
    {
        float* src = t1;
        float* dst = t2;
        for (int l = 1; l < 4; ++l) {
            const Seg segs[1] = {{src, a.w_a[l - 1], d.Kb_hd}};
            tile_linear_seg_tr<1>(segs, a.b_a[l], a.Hd, hidden_epi(dst, a.Hd));
            lds_barrier();
            float* tmp = src; src = dst; dst = tmp;
        }
        // three swaps: layer 3's activations are in t2
    }
    // ---- 5: the action sample and exploration ----
    if constexpr (AC) {
        // A logits -> the plain area behind the split-K partials, [16][A]; then one wave per row, one lane per class
        float* out_s = scratch + kSplitPartialFloats;
        const Seg segs[1] = {{t2, a.w_a4m, d.Kb_hd}};
        tile_linear_seg<1>(segs, a.b_a4, a.A, [&](int nb, floatx4 acc) {
            const int col = nb * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (col < a.A) out_s[(4 * (lane >> 4) + r) * a.A + col] = acc[r];
        }, scratch);
        lds_barrier();
        const int wave = bd_wave(bd_tid());
        for (int row = wave; row < rows_valid; row += kWaves) {        // wave-uniform: the butterflies see the whole wave
            const int grow = row0 + row;
            const bool valid = lane < a.A;
            const bool greedy = EV && a.action_mode != BD_POLICY_SAMPLE;      // the mode and the mean: argmax p, q = 1
            const float q = valid && !greedy ? draw_at(a.eps_action, a.stream_action, kDrawExp, (size_t)grow * a.A + lane) : 1.f;
            const float norm = disc_norm(valid ? out_s[row * a.A + lane] : 0.f, valid);
            const float p = disc_probs(norm, valid);
            const int k = disc_sample(p, q, valid, lane);
            float act = greedy ? (lane == k ? 1.f : 0.f) : disc_action_value(p, lane == k);
            if (a.explore) {      // epsilon-greedy: (u, v) = the row's two uniforms
                const float u = draw_at(a.eps_explore, a.stream_explore, kDrawUniform, (size_t)grow * 2);
                const float v = draw_at(a.eps_explore, a.stream_explore, kDrawUniform, (size_t)grow * 2 + 1);
                int kr = (int)floorf(v * (float)a.A);
                kr = kr < a.A - 1 ? kr : a.A - 1;
                if (u < a.action_noise) act = lane == kr ? 1.f : 0.f;
            }
            if (valid) a.action_out[(size_t)grow * a.A + lane] = act;
        }
    } else {
        const Seg2 segs[1] = {{t2, a.w_a4m, a.w_a4s, d.Kb_hd}};
        if (EV && a.action_mode != BD_POLICY_SAMPLE) {
            // the row's (mean, std) -> LDS [2][16][A] at the head of the split-K partials (dead once the head's own barrier
            // has passed) and act_stats_out; BD_POLICY_MEAN finishes here, BD_POLICY_MODE with one wave per row below
            float* ms = scratch;
            float* ss = scratch + 16 * a.A;
            const Rng rng_x{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stream_explore, (uint32_t)a.step};
            auto explored = [&](float act, int grow, int col) {
                if (!a.explore) return act;
                return fminf(fmaxf(act + a.action_noise * normal_at(a.eps_explore, rng_x, (size_t)grow * a.A + col), -1.f), 1.f);
            };
            tile_dual_head_elem<1>(
                segs, a.b_a4, a.b_a4 + a.A, a.A, scratch, [](int, int) { return 0.f; },
                [&](int row, int col, float Mn, float Rw, float zero) {
                    const int grow = row0 + row;
                    const float mean = a.act_mean_scale * tanh_act(Mn / a.act_mean_scale);
                    const float sd = softplusf(Rw + a.act_raw_init_std) + a.act_min_std;
                    ms[row * a.A + col] = mean;
                    ss[row * a.A + col] = sd;
                    if (grow >= a.B) return;
                    if (a.act_stats_out) {
                        a.act_stats_out[(size_t)grow * 2 * a.A + col] = mean;
                        a.act_stats_out[(size_t)grow * 2 * a.A + a.A + col] = sd;
                    }
                    if (a.action_mode == BD_POLICY_MEAN)      // the sampling step's expression at eps_action = 0
                        a.action_out[(size_t)grow * a.A + col] = explored(tanh_act(mean + sd * zero), grow, col);
                });
            if (a.action_mode == BD_POLICY_MODE) {
                lds_barrier();
                const Rng rng_m{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stream_mode, (uint32_t)a.step};
                const int wave = bd_wave(bd_tid());
                for (int row = wave; row < rows_valid; row += kWaves) {        // wave-uniform: the butterfly sees the whole wave
                    const int grow = row0 + row;
                    const ModeDraws draws{a.eps_mode, rng_m, (size_t)a.B, (size_t)grow, a.A};
                    const int j = tanh_normal_mode_index(ms + row * a.A, ss + row * a.A, a.A, a.n_mode, draws, lane);
                    if (lane < a.A)
                        a.action_out[(size_t)grow * a.A + lane] =
                            explored(tanh_act(ms[row * a.A + lane] + ss[row * a.A + lane] * draws(j, lane)), grow, lane);
                    if (lane == 0 && a.mode_index_out) a.mode_index_out[grow] = j;
                }
            }
            return;
        }
        tile_dual_head_elem<1>(
            segs, a.b_a4, a.b_a4 + a.A, a.A, scratch,
            [&](int row, int col) {
                // ONE call site of the normal generator for both draws: with two, hipcc stops inlining the library's
                // sincosf, and the call's stack frame becomes the kernel's only scratch (544 B per lane, and 40 more VGPRs
                // on the Gaussian instantiation when the two draws were written as two calls)
                float ev[2] = {0.f, 0.f};
#pragma unroll 1
                for (int t = 0; t < (a.explore ? 2 : 1); ++t)
                    ev[t] = draw(t ? a.eps_explore : a.eps_action, t ? a.stream_explore : a.stream_action, kDrawNormal, a.A, row, col);
                return ActEps{ev[0], ev[1]};
            },
            [&](int row, int col, float Mn, float Rw, ActEps eps) {
                const int grow = row0 + row;
                if (grow >= a.B) return;
                const float mean = a.act_mean_scale * tanh_act(Mn / a.act_mean_scale);
                const float sd = softplusf(Rw + a.act_raw_init_std) + a.act_min_std;
                float act = tanh_act(mean + sd * eps.sample);
                if (a.explore) act = fminf(fmaxf(act + a.action_noise * eps.explore, -1.f), 1.f);
                a.action_out[(size_t)grow * a.A + col] = act;
            });
    }
}

// nullptr = dims the kernel takes (LDS aside); otherwise the reason
static const char* act_dims_error(int Be, int D, int C, int S, int A, int Hd, int E, int O, bool lc) {
    if (Be <= 0 || S <= 0 || A <= 0 || Hd <= 0 || E <= 0 || O < 0) return "bad dims";
    // (bounds first: the tile counts of the LDS figure must not overflow)
    if (Be > (1 << 20) || Hd > (1 << 20) || E > (1 << 20) || O > (1 << 20) || S > (1 << 20)) return "layer width above 2^20";
    if (A > kHeadMaxN) return "action width above 64 (one lane per class; the widest Gaussian head)";
    if (lc) {
        if (D <= 0 || C <= 0 || D > (1 << 20) || C > 256 || (long long)D * C != S || !CatGeo(D, C).ok())
            return "latents unsupported (S = D*C; C <= 256; S <= 256, or 256 % C == 0 and S % 16 == 0)";
    } else if (S > kHeadMaxN) {
        return "state width above 64";
    }
    return nullptr;
}

static bool act_supported(int Be, int D, int C, int S, int A, int Hd, int E, int O, bool lc) {
    return act_dims_error(Be, D, C, S, A, Hd, E, O, lc) == nullptr &&
           ActDims(Be, D, C, S, A, Hd, E, O, lc).lds_floats() * sizeof(float) <= (size_t)kMaxLds;
}

template <bool LC, bool AC, bool EV>
static int act_launch_ev(const char* who, const bd_act_args& k, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024 && allow_big_lds(act_step_kernel<LC, AC, EV>)) return -1;
    hipLaunchKernelGGL((act_step_kernel<LC, AC, EV>), dim3(cdiv(k.B, 16)), dim3(kThreads), lds, stream, k);
    BD_CHECK_LAUNCH(who);
    return 0;
}

// a zeroed evaluation tail: the sampling kernel; anything set: the evaluation instantiation
template <bool LC, bool AC>
static int act_launch(const char* who, const bd_act_args& k, size_t lds, hipStream_t stream) {
    if (k.action_mode != BD_POLICY_SAMPLE || k.latent_mean) return act_launch_ev<LC, AC, true>(who, k, lds, stream);
    return act_launch_ev<LC, AC, false>(who, k, lds, stream);
}

// the checks of both entry points (`who` names the one that was called), then the launch of the (latent_cat, actor_cat) kernel
static int act_step(const char* who, const bd_act_args* a, hipStream_t stream) {
    BD_REQUIRE(a->B > 0, "%s: bad dims", who);
    const bool lc = a->latent_cat != 0, ac = a->actor_cat != 0;
    BD_REQUIRE((a->obs != nullptr) != (a->embedding != nullptr),
               "%s: give the observation (state observations) or the embedding (pixels), not both", who);
    const int O = a->obs ? a->O : 0;
    const char* why = act_dims_error(a->Be, a->D, a->C, a->S, a->A, a->Hd, a->E, O, lc);
    BD_REQUIRE(why == nullptr, "%s: %s (Be %d, %d x %d, S %d, A %d, Hd %d, E %d, O %d)", who, why, a->Be, a->D, a->C, a->S, a->A,
               a->Hd, a->E, O);
    const size_t lds = ActDims(a->Be, a->D, a->C, a->S, a->A, a->Hd, a->E, O, lc).lds_floats() * sizeof(float);
    BD_REQUIRE(lds <= (size_t)kMaxLds, "%s: needs %zu B of LDS (limit %d)", who, lds, kMaxLds);
    if (a->obs != nullptr) {
        BD_REQUIRE(a->O > 0, "%s: obs given with O = 0", who);
        for (int l = 0; l < 5; ++l) BD_REQUIRE(a->w_enc[l] && a->b_enc[l], "%s: missing encoder weights (layer %d)", who, l);
    }
    BD_REQUIRE(a->w_embed_a && a->b_embed && a->w_ir && a->w_iz && a->w_in && a->w_hr && a->w_hz && a->w_hn && a->b_ih && a->b_hh &&
                   a->w_q1h && a->w_q1e && a->b_q1 && a->b_q2 &&
                   (lc ? (a->w_embed_sT && a->w_q2) : (a->w_embed_s && a->w_q2m && a->w_q2s)),
               "%s: missing transition weights", who);
    BD_REQUIRE(a->w_a0h && (lc ? a->w_a0sT : a->w_a0s) && a->w_a[0] && a->w_a[1] && a->w_a[2] && a->b_a[0] && a->b_a[1] &&
                   a->b_a[2] && a->b_a[3] && a->w_a4m && (ac || a->w_a4s) && a->b_a4, "%s: missing actor weights", who);
    BD_REQUIRE(a->belief && a->state && a->action, "%s: missing inputs", who);
    BD_REQUIRE(a->belief_out && a->state_out && a->action_out, "%s: missing outputs", who);
    BD_REQUIRE(a->belief_out != a->belief && a->state_out != a->state && a->action_out != a->action,
               "%s: an output aliases its input", who);
    BD_REQUIRE(a->action_mode == BD_POLICY_SAMPLE || a->action_mode == BD_POLICY_MODE || a->action_mode == BD_POLICY_MEAN,
               "%s: action_mode %d (BD_POLICY_SAMPLE, BD_POLICY_MODE or BD_POLICY_MEAN)", who, a->action_mode);
    // the draws this call consumes; eps_mode counts only where it is read (a sampling block may carry anything there)
    const bool use_post = !a->latent_mean, use_action = a->action_mode == BD_POLICY_SAMPLE;
    const bool use_mode = a->action_mode == BD_POLICY_MODE && !ac;
    BD_REQUIRE(!use_mode || (a->n_mode >= 1 && a->n_mode <= (1 << 20)), "%s: n_mode %d (1 .. 2^20 draws of the mode)", who, a->n_mode);
    const bool all_null = !a->eps_post && !a->eps_action && !a->eps_explore && !(use_mode && a->eps_mode);
    BD_REQUIRE(all_null || ((a->eps_post || !use_post) && (a->eps_action || !use_action) && (a->eps_explore || !a->explore) &&
                            (a->eps_mode || !use_mode)),
               "%s: noise buffers: eps_post, eps_action (and eps_explore when explore, eps_mode for the mode) or all NULL", who);
    bd_act_args k = *a;
    k.O = O;
    if (!use_mode) k.eps_mode = nullptr;
    if (lc) return ac ? act_launch<true, true>(who, k, lds, stream) : act_launch<true, false>(who, k, lds, stream);
    return ac ? act_launch<false, true>(who, k, lds, stream) : act_launch<false, false>(who, k, lds, stream);
}

}  // namespace bd

extern "C" {
using namespace bd;

int bd_act_step_supported(int Be, int S, int A, int Hd, int E, int O) { return act_supported(Be, 0, 0, S, A, Hd, E, O, false) ? 1 : 0; }

int bd_act_step_cat_supported(int Be, int D, int C, int S, int A, int Hd, int E, int O, int latent_cat, int actor_cat) {
    if (!latent_cat && !actor_cat) return 0;      // that configuration is bd_act_step
    return act_supported(Be, D, C, S, A, Hd, E, O, latent_cat != 0) ? 1 : 0;
}

int bd_act_step(const bd_act_args* a, void* stream) {
    BD_REQUIRE(a, "bd_act_step: null argument block");
    BD_REQUIRE(!a->latent_cat && !a->actor_cat,
               "bd_act_step: takes latent_cat = 0 and actor_cat = 0 (Gaussian latents with the tanh-Normal actor); the other "
               "configurations are bd_act_step_cat");
    return act_step("bd_act_step", a, (hipStream_t)stream);
}

int bd_act_step_cat(const bd_act_args* a, void* stream) {
    BD_REQUIRE(a, "bd_act_step_cat: null argument block");
    BD_REQUIRE(a->latent_cat || a->actor_cat,
               "bd_act_step_cat: Gaussian latents with the tanh-Normal actor: that configuration is bd_act_step");
    return act_step("bd_act_step_cat", a, (hipStream_t)stream);
}

int bd_tanh_normal_mode(const float* mean, const float* std, const float* eps_mode, unsigned long long seed,
                        unsigned long long step, unsigned stream_id, int N, int A, int n, float* action, int* index,
                        void* stream) {
    BD_REQUIRE(N >= 1 && A >= 1 && A <= 64 && n >= 1 && n <= (1 << 20),
               "bd_tanh_normal_mode: bad dims (N %d >= 1, 1 <= A %d <= 64, 1 <= n %d <= 2^20)", N, A, n);
    BD_REQUIRE(mean && std && action, "bd_tanh_normal_mode: missing mean, std or action");
    BD_REQUIRE(action != mean && action != std, "bd_tanh_normal_mode: the action aliases an input");
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (uint32_t)step};
    hipLaunchKernelGGL(tanh_normal_mode_kernel, dim3(cdiv(N, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, mean, std, eps_mode,
                       rng, N, A, n, action, index);
    BD_CHECK_LAUNCH("bd_tanh_normal_mode");
    return 0;
}

}  // extern "C"
