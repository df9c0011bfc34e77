// act.hip -- one decision of the collect / evaluation loop in ONE launch: Planet.update_belief_and_act
// (src/planet.py:370-403) with Dreamer.get_action (src/dreamer.py:429-444) on Gaussian latents and the tanh-Normal actor.
//
//   bd_act_step: a workgroup owns 16 environments; every activation of the step stays in LDS in MFMA fragment order, the
//     weights (3.9 MB at the reference's default sizes) stream once from L2.  Per tile:
//       e  = encoder(obs)                    DenseModel 4 x (Linear+ELU) + Linear (src/models.py:365-408), or a ready
//                                            embedding (pixel observations: the conv stack has run)
//       x  = ELU(W_e [s; a] + b_e);  h' = GRUCell(x, h)                          (src/models.py:251-252)
//       q  = ELU(W_q1 [h'; e] + b);  s' = mean_q + std_q * eps_post              (src/models.py:266-267, :70-73)
//       actor: 4 x (Linear+ELU) on [h'; s'], mean = 5 tanh(m/5), std = softplus(r + c0) + 1e-4,
//              a' = tanh(mean + std * eps_action)                                (src/models.py:506-517, src/dreamer.py:443)
//       explore: a' = clamp(a' + action_noise * eps_explore, -1, 1)              (src/planet.py:388-392)
//     What the composed path computes besides and nobody reads is left out: the prior head of the belief update
//     (src/models.py:256: with an embedding the posterior sample is the state that continues), the prior sample of
//     get_action's one imagination step and the 100-sample entropy estimate (src/planet.py:386 drops it).  None of them
//     feeds belief, state or action, so the three outputs are exactly the composed path's.
//   Noise: explicit buffers, or (all NULL) Philox4x32-10 draws made in the kernel with the element layout of bd_rng_fill,
//     so a run with in-kernel noise equals, bit for bit, a run fed bd_rng_fill's buffers for the same (seed, step, stream).
//   One workgroup per 16 rows: at B <= 16 the step is a single CU walking a chain of thirteen dependent layers.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_scan.h"
#include "bd_rng.h"

namespace bd {

struct ActDims {
    int Kb_h, Kb_s, Kb_a, Kb_hd, Kb_e, Kb_o;
    int Kb_g;     // the three general tiles hold a belief-wide or a hidden-wide vector
    int Kb_io;    // observation (dead after the encoder's first layer), then the embedding
    __host__ __device__ ActDims(int Be, int S, int A, int Hd, int E, int O)
        : Kb_h(cdiv(Be, 16)), Kb_s(cdiv(S, 16)), Kb_a(cdiv(A, 16)), Kb_hd(cdiv(Hd, 16)), Kb_e(cdiv(E, 16)), Kb_o(cdiv(O, 16)),
          Kb_g(Kb_h > Kb_hd ? Kb_h : Kb_hd), Kb_io(Kb_e > Kb_o ? Kb_e : Kb_o) {}
    __host__ __device__ size_t lds_floats() const {
        return (size_t)(3 * Kb_g + Kb_io + Kb_s + Kb_a) * kFragFloats + kSplitScratchFloats;
    }
};

struct ActEps {
    float sample, explore;
};

__global__ __launch_bounds__(kThreads) void act_step_kernel(bd_act_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ActDims d(a.Be, a.S, a.A, a.Hd, a.E, a.O);
    const int row0 = blockIdx.x * 16;
    const int ng = d.Kb_g * kFragFloats;
    float* t0 = smem;                             // encoder pong, h', (kept to the end: the actor reads it)
    float* t1 = t0 + ng;                          // h, posterior hidden, actor ping
    float* t2 = t1 + ng;                          // encoder ping, x, actor pong
    float* ef = t2 + ng;                          // obs -> embedding
    float* sf = ef + d.Kb_io * kFragFloats;       // s, then s'
    float* af = sf + d.Kb_s * kFragFloats;
    float* scratch = af + d.Kb_a * kFragFloats;   // split-K partials (kSplitScratchFloats), 16-byte aligned
    const int lane = bd_tid() & 63;
    const Rng key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), 0u, (uint32_t)a.step};
    // element (row, col) of a [B x width] noise tensor: the caller's buffer, or what bd_rng_fill writes there
    auto draw = [&](const float* __restrict__ eps, unsigned stream, int width, int row, int col) -> float {
        const int grow = row0 + row;
        if (grow >= a.B) return 0.f;
        const size_t e = (size_t)grow * width + col;
        if (eps != nullptr) return eps[e];
        float v[4];
        rng_normal4(Rng{key.k0, key.k1, stream, key.step}, e >> 2, v);
        const int j = (int)(e & 3);
        return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
    };
    auto hidden_epi = [&](float* dst, int width) { return HiddenEpiTR{dst, nullptr, 0, width, a.B, row0, lane}; };

    load_tile_concat<1>(t1, d.Kb_h, row0, a.B, a.belief, a.Be, a.Be, nullptr, 0, 0);
    load_tile_concat<1>(sf, d.Kb_s, row0, a.B, a.state, a.S, a.S, nullptr, 0, 0);
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
    {
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
    {
        const Seg2 segs[1] = {{t1, a.w_q2m, a.w_q2s, d.Kb_hd}};
        tile_dual_head_elem<1>(
            segs, a.b_q2, a.b_q2 + a.S, a.S, scratch,
            [&](int row, int col) { return draw(a.eps_post, a.stream_post, a.S, row, col); },
            [&](int row, int col, float Mn, float Rw, float eps) {
                const int grow = row0 + row;
                float st = 0.f;
                if (grow < a.B) {
                    st = Mn + (softplusf(Rw) + a.min_std) * eps;
                    a.state_out[(size_t)grow * a.S + col] = st;
                }
                sf[frag_idx(row, col)] = st;
            });
    }
    lds_barrier();
    // ---- 4: actor on [h'; s'] ----
    {
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
    // ---- 5: tanh-Normal sample, exploration noise ----
    {
        const Seg2 segs[1] = {{t2, a.w_a4m, a.w_a4s, d.Kb_hd}};
        tile_dual_head_elem<1>(
            segs, a.b_a4, a.b_a4 + a.A, a.A, scratch,
            [&](int row, int col) {
                return ActEps{draw(a.eps_action, a.stream_action, a.A, row, col),
                              a.explore ? draw(a.eps_explore, a.stream_explore, a.A, row, col) : 0.f};
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

static bool act_dims_ok(int Be, int S, int A, int Hd, int E, int O) {
    if (Be <= 0 || S <= 0 || A <= 0 || Hd <= 0 || E <= 0 || O < 0) return false;
    // (bounds first: the tile counts below must not overflow)
    if (Be > (1 << 20) || Hd > (1 << 20) || E > (1 << 20) || O > (1 << 20)) return false;
    if (S > kHeadMaxN || A > kHeadMaxN) return false;
    return ActDims(Be, S, A, Hd, E, O).lds_floats() * sizeof(float) <= (size_t)kMaxLds;
}

}  // namespace bd

extern "C" {
using namespace bd;

int bd_act_step_supported(int Be, int S, int A, int Hd, int E, int O) { return act_dims_ok(Be, S, A, Hd, E, O) ? 1 : 0; }

int bd_act_step(const bd_act_args* a, void* stream) {
    BD_REQUIRE(a, "bd_act_step: null argument block");
    BD_REQUIRE(a->B > 0 && a->Be > 0 && a->S > 0 && a->A > 0 && a->Hd > 0 && a->E > 0 && a->O >= 0, "bd_act_step: bad dims");
    BD_REQUIRE(a->S <= kHeadMaxN && a->A <= kHeadMaxN, "bd_act_step: state / action width above %d", kHeadMaxN);
    BD_REQUIRE(a->Be <= (1 << 20) && a->Hd <= (1 << 20) && a->E <= (1 << 20) && a->O <= (1 << 20),
               "bd_act_step: layer width above 2^20");
    BD_REQUIRE((a->obs != nullptr) != (a->embedding != nullptr),
               "bd_act_step: give the observation (state observations) or the embedding (pixels), not both");
    if (a->obs != nullptr) {
        BD_REQUIRE(a->O > 0, "bd_act_step: obs given with O = 0");
        for (int l = 0; l < 5; ++l) BD_REQUIRE(a->w_enc[l] && a->b_enc[l], "bd_act_step: missing encoder weights (layer %d)", l);
    }
    BD_REQUIRE(a->w_embed_s && a->w_embed_a && a->b_embed && a->w_ir && a->w_iz && a->w_in && a->w_hr && a->w_hz && a->w_hn &&
                   a->b_ih && a->b_hh && a->w_q1h && a->w_q1e && a->b_q1 && a->w_q2m && a->w_q2s && a->b_q2,
               "bd_act_step: missing transition weights");
    BD_REQUIRE(a->w_a0h && a->w_a0s && a->w_a[0] && a->w_a[1] && a->w_a[2] && a->b_a[0] && a->b_a[1] && a->b_a[2] && a->b_a[3] &&
                   a->w_a4m && a->w_a4s && a->b_a4, "bd_act_step: missing actor weights");
    BD_REQUIRE(a->belief && a->state && a->action, "bd_act_step: missing inputs");
    BD_REQUIRE(a->belief_out && a->state_out && a->action_out, "bd_act_step: missing outputs");
    BD_REQUIRE(a->belief_out != a->belief && a->state_out != a->state && a->action_out != a->action,
               "bd_act_step: an output aliases its input");
    const bool all_null = !a->eps_post && !a->eps_action && !a->eps_explore;
    BD_REQUIRE(all_null || (a->eps_post && a->eps_action && (a->eps_explore || !a->explore)),
               "bd_act_step: noise buffers: eps_post, eps_action (and eps_explore when explore) or all NULL");
    const ActDims d(a->Be, a->S, a->A, a->Hd, a->E, a->obs ? a->O : 0);
    const size_t lds = d.lds_floats() * sizeof(float);
    BD_REQUIRE(lds <= (size_t)kMaxLds, "bd_act_step: needs %zu B of LDS", lds);
    if (lds > 64 * 1024 && allow_big_lds(act_step_kernel)) return -1;
    bd_act_args k = *a;
    if (k.obs == nullptr) k.O = 0;
    hipLaunchKernelGGL(act_step_kernel, dim3(cdiv(a->B, 16)), dim3(kThreads), lds, (hipStream_t)stream, k);
    BD_CHECK_LAUNCH("bd_act_step");
    return 0;
}

}  // extern "C"
