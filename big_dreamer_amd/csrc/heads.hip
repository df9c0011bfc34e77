// heads.hip -- the two frozen heads over the imagined features (reward_model and critic_target, src/dreamer.py:320-331),
// forward AND dgrad in one launch: bd_img_heads_fwd_bwd.
//
// Both heads are frozen (FreezeParameters), so their backward needs no weight-gradient operands, and d(output) of each
// head comes from bd_lambda_return_backward, which does not read the rewards or values.  So each row tile runs a head's
// forward and then its backward while the activations are still on chip: the saved ELU outputs never go to HBM (the
// separate forward / backward pair writes and re-reads 8 x M x Hd floats), x is read once and d/d x written once.
//
// Per workgroup: 16*RT rows, kWaves waves, two LDS fragment images -- `xim` (the x tile, later the reward head's dpre0)
// and `img` (the working image, overwritten in place layer by layer: sweep -> barrier -> epilogue -> barrier).
// Ownership of the (row tile, column block) pairs follows the tall chain helpers (bd_device.h: tall_sweep / tall_fill /
// tall_foreach2), and is the same for every Hd-wide layer, forward or backward: the lane that produces a hidden
// layer's ELU output in the forward epilogue is the lane that needs it for elu' in the backward epilogue.  So each lane
// keeps its own four saves in registers (TallAcc per layer), and the reward head's dpre0 stays in registers while the
// value head runs.  The closing contraction  d x = [dpre0_r | dpre0_v] [W0_r^T ; W0_v^T]  is one two-segment sweep.
#include "bd_device.h"
#include "bd_host.h"
#include <stdlib.h>

namespace bd {

constexpr int kHeadHidden = BD_HEAD_HIDDEN;

// o = f(rt, nb, t, u) for every pair this wave holds (the tall helpers' pair set)
template <int RT, class F>
__device__ __forceinline__ void tall_map(int N, const TallAcc<RT>& t, const TallAcc<RT>& u, TallAcc<RT>& o, F&& f) {
    const int wave = bd_wave(bd_tid());
    const int Nb = (N + 15) >> 4, per = Nb / kWaves;
#pragma unroll
    for (int i = 0; i < kTallMaxPer; ++i)
        if (i < per) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) o.main[i][rt] = f(rt, wave + i * kWaves, t.main[i][rt], u.main[i][rt]);
        }
    int lrt = 0, lnb = 0;
    if (tall_left_pair(Nb, RT, wave, lrt, lnb)) o.left = f(lrt, lnb, t.left, u.left);
}

template <int RT>
__device__ __forceinline__ void img_store(float* img, int Nb, int rt, int nb, floatx4 v) {
    *reinterpret_cast<floatx4*>(img + ((rt * Nb + nb) * 64 + (bd_tid() & 63)) * 4) = v;
}

// One head: forward through the hidden layers (saves kept in `sv`), the Hd -> 1 output layer, then the dgrad chain down
// to d(pre-activation) of layer 0, returned in `d0` (not written to LDS).  On entry `xim` holds the x tile; `img` may
// still be read by other waves until the first barrier below.
// `ka` is the kernel's argument block in the constant address space (BD_KARGS): the head's ~15 pointers are loaded
// with s_load where they are used instead of being held (and spilled) across the whole chain.
template <int RT, class KA>
__device__ __forceinline__ void head_fwd_bwd(KA ka, int h, const float* xim, float* img, int KbF, int Hd,
                                             int row0, int M, TallAcc<RT>& d0) {
    const auto& H = ka->head[h];
    const int Nb = cdiv(Hd, 16);
    const int lane = bd_tid() & 63, m = lane & 15;
    TallAcc<RT> sv[kHeadHidden];
    // ---- forward
#pragma unroll
    for (int l = 0; l < kHeadHidden; ++l) {
        const Seg seg[1] = {{l == 0 ? xim : img, H.w[l], l == 0 ? KbF : Nb}};
        TallAcc<RT> t;
        tall_sweep<RT, 1>(seg, H.b[l], Hd, t);
        lds_barrier();      // every wave has read the layer's input (and, for l = 0, the previous phase's image)
        // columns >= Hd of the last block come out as ELU(0 + 0) = 0: bias and packed weights are zero there
        tall_map<RT>(Hd, t, t, sv[l], [&](int rt, int nb, floatx4 acc, floatx4) {
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = elu(acc[r]);
            img_store<RT>(img, Nb, rt, nb, v);
            return v;
        });
        lds_barrier();
    }
    // ---- output layer (Hd -> 1): TPR threads per row, fixed-order shuffle reduction
    {
        constexpr int kRows = 16 * RT, TPR = kThreads / kRows;
        static_assert(kThreads % kRows == 0 && TPR <= 64 && (TPR & (TPR - 1)) == 0, "threads per row");
        const int tid = bd_tid(), row = tid / TPR, part = tid - row * TPR;
        const int rt = row >> 4, mr = row & 15, n4 = cdiv(Hd, 4);
        const float* base = img + rt * Nb * kFragFloats;
        float s = 0.f;
        for (int c = part; c < n4; c += TPR) {
            const floatx4 v = *reinterpret_cast<const floatx4*>(base + ((c >> 2) * 64 + (c & 3) * 16 + mr) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * c + r < Hd) s += v[r] * H.w_out[4 * c + r];
        }
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, TPR);
        const int grow = row0 + row;
        if (part == 0 && grow < M) H.out[grow] = s + H.b_out[0];
    }
    lds_barrier();          // the output layer has read the last hidden image
    // ---- d(pre-activation) of the last hidden layer: d * w_out (x) elu'(a)
    {
        TallAcc<RT> t;
        tall_map<RT>(Hd, sv[kHeadHidden - 1], sv[kHeadHidden - 1], t, [&](int rt, int nb, floatx4 a, floatx4) {
            const int grow = row0 + rt * 16 + m;
            const float d = grow < M ? H.dout[grow] : 0.f;
            const floatx4 w = tall_bias(H.w_out, Hd, nb, lane);      // zero beyond Hd
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = d * w[r] * elu_grad_from_out(a[r]);
            img_store<RT>(img, Nb, rt, nb, v);
            return v;
        });
        lds_barrier();
    }
    // ---- dgrad chain: d pre_{l-1} = (d pre_l  W_l) (x) elu'(a_{l-1}), in place; the last one stays in registers
#pragma unroll
    for (int l = kHeadHidden - 1; l >= 1; --l) {
        const Seg seg[1] = {{img, H.wt[l], Nb}};
        TallAcc<RT> t;
        tall_sweep<RT, 1>(seg, nullptr, Hd, t);
        if (l > 1) lds_barrier();
        tall_map<RT>(Hd, t, sv[l - 1], l > 1 ? t : d0, [&](int rt, int nb, floatx4 acc, floatx4 a) {
            const bool in = row0 + rt * 16 + m < M;
            const int col0 = nb * 16 + 4 * (lane >> 4);
            floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (in && col0 + r < Hd) v[r] = acc[r] * elu_grad_from_out(a[r]);
            if (l > 1) img_store<RT>(img, Nb, rt, nb, v);
            return v;
        });
        if (l > 1) lds_barrier();
    }
}

template <int RT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4 - RT, 4 - RT))) void img_heads_kernel(bd_img_heads_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int KbF = cdiv(a.F, 16), Nb = cdiv(a.Hd, 16);
    float* xim = smem;
    float* img = smem + (size_t)RT * (KbF > Nb ? KbF : Nb) * kFragFloats;
    const int row0 = blockIdx.x * 16 * RT;
    if (tile_pairs_ok(a.x, a.F, a.F, nullptr, 0))
        load_tile_concat_pairs<RT>(xim, KbF, row0, a.M, a.x, a.F, a.F, nullptr, 0, 0);
    else
        load_tile_concat<RT>(xim, KbF, row0, a.M, a.x, a.F, a.F, nullptr, 0, 0);
    lds_barrier();
    BD_KARGS(bd_img_heads_args, ka);
    TallAcc<RT> d0r, d0v;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {        // one copy of the chain's code for both heads
        BD_KARGS_FRESH(ka);
        TallAcc<RT> d0;
        head_fwd_bwd<RT>(ka, h, xim, img, KbF, a.Hd, row0, a.M, d0);
        if (h == 0) d0r = d0;
        else d0v = d0;
    }
    lds_barrier();          // the value head's last dgrad sweep has read `img`
    tall_foreach2<RT>(a.Hd, d0r, d0v, [&](int rt, int nb, floatx4 r, floatx4 v) {
        img_store<RT>(xim, Nb, rt, nb, r);
        img_store<RT>(img, Nb, rt, nb, v);
    });
    lds_barrier();
    const Seg segs[2] = {{xim, a.head[0].wt[0], Nb}, {img, a.head[1].wt[0], Nb}};
    const bool rows_full = row0 + 16 * RT <= a.M;
    tile_linear_g<RT, 2>(segs, nullptr, a.F, [&](int rt, int nb, floatx4 acc) {
        const int ln = bd_tid() & 63, col = nb * 16 + (ln & 15);
        const unsigned r0 = (unsigned)(row0 + rt * 16 + 4 * (ln >> 4));
        if (col >= a.F) return;
        float* __restrict__ p = a.dx + (r0 * (unsigned)a.F + (unsigned)col);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (rows_full || (int)r0 + r < a.M) p[r * (unsigned)a.F] = acc[r];
    });
}

// 32-row tiles where the Hd-wide pairs balance over the waves (tall_shape_ok), 16-row tiles otherwise
static int heads_rt(int Hd) { return tall_shape_ok(Hd, 2) ? 2 : (tall_shape_ok(Hd, 1) ? 1 : 0); }

static size_t heads_lds(int RT, int F, int Hd) {
    const int KbF = cdiv(F, 16), Nb = cdiv(Hd, 16);
    return (size_t)RT * ((KbF > Nb ? KbF : Nb) + Nb) * kFragFloats * sizeof(float);
}

}  // namespace bd

extern "C" {

int bd_img_heads_supported(int F, int Hd) {
    using namespace bd;
    if (F <= 0 || Hd <= 0) return 0;
    const int rt = heads_rt(Hd);
    return rt > 0 && heads_lds(rt, F, Hd) <= (size_t)kMaxLds;
}

int bd_img_heads_fwd_bwd(const bd_img_heads_args* a, void* stream) {
    using namespace bd;
    BD_REQUIRE(a && a->M > 0 && a->x && a->dx, "bd_img_heads_fwd_bwd: bad M / x / dx");
    BD_REQUIRE(bd_img_heads_supported(a->F, a->Hd), "bd_img_heads_fwd_bwd: F=%d, Hd=%d not covered (Hd <= 240 in "
               "column blocks the waves can balance, LDS <= %d B)", a->F, a->Hd, kMaxLds);
    BD_REQUIRE((size_t)a->M * (size_t)a->F < ((size_t)1 << 31), "bd_img_heads_fwd_bwd: M*F=%zu needs 64-bit offsets",
               (size_t)a->M * (size_t)a->F);
    for (int h = 0; h < 2; ++h) {
        const bd_img_head& H = a->head[h];
        bool ok = H.w_out && H.b_out && H.dout && H.out;
        for (int l = 0; l < BD_HEAD_HIDDEN; ++l) ok = ok && H.w[l] && H.wt[l] && H.b[l];
        BD_REQUIRE(ok, "bd_img_heads_fwd_bwd: head %d is missing an operand", h);
    }
    const int rt = heads_rt(a->Hd);
    const size_t lds = heads_lds(rt, a->F, a->Hd);
    const dim3 grid(cdiv(a->M, 16 * rt));
    if (rt == 2) {
        if (lds > 64 * 1024 && allow_big_lds(img_heads_kernel<2>)) return -1;
        hipLaunchKernelGGL(img_heads_kernel<2>, grid, dim3(kThreads), lds, (hipStream_t)stream, *a);
    } else {
        if (lds > 64 * 1024 && allow_big_lds(img_heads_kernel<1>)) return -1;
        hipLaunchKernelGGL(img_heads_kernel<1>, grid, dim3(kThreads), lds, (hipStream_t)stream, *a);
    }
    BD_CHECK_LAUNCH("bd_img_heads_fwd_bwd");
    return 0;
}

}  // extern "C"
