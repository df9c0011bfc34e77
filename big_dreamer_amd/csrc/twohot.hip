// twohot.hip -- two-hot critic head in symlog space ("Two-hot critic"; ActorCritic.critic_head = twohot).
// Definitions in include/bigdreamer_hip.h.
//
// Three row-wise kernels over [rows x K] logits: decode (softmax mean over the bins, symexp), its backward, and the
// cross-entropy against the two-hot encoding of a scalar target.  One wave64 per row, kThRows rows per workgroup.  A row
// of K = 255 floats is 1020 bytes and not 16-byte aligned, so lane j takes elements j, j + 64, ... as single dwords: a
// wave's load is 256 contiguous bytes.  The row stays in registers across the max, sum, moment and gradient passes:
// 4 per lane for K <= 256, 16 per lane up to K = 1024 (pieces of 64, whole pieces beyond K skipped wave-uniformly), so
// the row is read from memory once.  Wave reductions are xor butterflies (every lane ends with the same bits, in an
// order that does not depend on the schedule): no LDS, no atomics.  Per-row scalars are written by lane 0.  The bins are
// computed from (K, zmax), never read: z_i = (2 i - (K - 1)) zmax / (K - 1), i.e. -zmax + i delta formed so that
// z_i = -z_{K-1-i} exactly.  Precise expf / logf / log1pf / expm1f, as the loss kernels of reduce.hip.
#include "bd_device.h"
#include "bd_host.h"

namespace bd {

constexpr int kThRows = 4;          // waves = rows per workgroup
constexpr int kThSmall = 4;         // registers per lane, K <= 256
constexpr int kThLarge = 16;        // K <= 1024

__device__ __forceinline__ float th_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float th_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float th_bin(int i, int K, float h) { return (float)(2 * i - (K - 1)) * h; }
__device__ __forceinline__ float th_symexp(float m) { return copysignf(expm1f(fabsf(m)), m); }

// The row's logits x, e_i = exp(x_i - max) (0 beyond K), their sum s, the row maximum and the softmax mean of the bins.
template <int NREG>
__device__ __forceinline__ void th_row(const float* __restrict__ l, int K, int lane, float h, float (&x)[NREG],
                                       float (&e)[NREG], float& mx, float& s, float& m) {
    mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NREG; ++j) {
        x[j] = -INFINITY;
        if (j * 64 < K) {                                   // wave-uniform
            const int i = lane + j * 64;
            if (i < K) x[j] = l[i];
            mx = fmaxf(mx, x[j]);
        }
    }
    mx = th_wave_max(mx);
    float ps = 0.f, pz = 0.f;
#pragma unroll
    for (int j = 0; j < NREG; ++j) {
        e[j] = 0.f;
        if (j * 64 < K) {
            const int i = lane + j * 64;
            if (i < K) e[j] = expf(x[j] - mx);
            ps += e[j];
            pz = fmaf(e[j], th_bin(i, K, h), pz);
        }
    }
    s = th_wave_sum(ps);
    m = th_wave_sum(pz) / s;
}

template <int NREG>
__global__ __launch_bounds__(kThRows * 64) void twohot_decode_kernel(const float* __restrict__ logits, int ld, int rows, int K,
                                                                     float h, float* __restrict__ value,
                                                                     float* __restrict__ mean) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * kThRows + (threadIdx.x >> 6);
    if (row >= rows) return;                                // wave-uniform
    float x[NREG], e[NREG], mx, s, m;
    th_row<NREG>(logits + (size_t)row * ld, K, lane, h, x, e, mx, s, m);
    if (lane == 0) {
        value[row] = th_symexp(m);
        if (mean) mean[row] = m;
    }
}

// dl_i = dv exp(|m|) p_i (z_i - m)
template <int NREG>
__global__ __launch_bounds__(kThRows * 64) void twohot_decode_bwd_kernel(const float* __restrict__ logits, int ld,
                                                                         const float* __restrict__ dvalue, int rows, int K,
                                                                         float h, float* __restrict__ dlogits, int ldd) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * kThRows + (threadIdx.x >> 6);
    if (row >= rows) return;
    float x[NREG], e[NREG], mx, s, m;
    th_row<NREG>(logits + (size_t)row * ld, K, lane, h, x, e, mx, s, m);
    const float g = dvalue[row] * expf(fabsf(m)) / s;
    float* __restrict__ dl = dlogits + (size_t)row * ldd;
#pragma unroll
    for (int j = 0; j < NREG; ++j) {
        const int i = lane + j * 64;
        if (i < K) dl[i] = g * e[j] * (th_bin(i, K, h) - m);
    }
}

// loss_r = w_r (logsumexp(l) - (1 - w) l_k - w l_{k+1}),   dl_i = grad_scale w_r (p_i - q_i)
template <int NREG>
__global__ __launch_bounds__(kThRows * 64) void twohot_nll_kernel(const float* __restrict__ logits, int ld,
                                                                  const float* __restrict__ target,
                                                                  const float* __restrict__ weight, int rows, int K, float zmax,
                                                                  float h, float grad_scale, float* __restrict__ dlogits, int ldd,
                                                                  float* __restrict__ value, float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * kThRows + (threadIdx.x >> 6);
    if (row >= rows) return;
    float x[NREG], e[NREG], mx, s, m;
    th_row<NREG>(logits + (size_t)row * ld, K, lane, h, x, e, mx, s, m);
    // two-hot encoding of the target: (k, w) is continuous across a bin edge; a NaN target stays NaN in w
    const float y = target[row];
    float t = copysignf(log1pf(fabsf(y)), y);
    t = t < -zmax ? -zmax : (t > zmax ? zmax : t);
    const float u = (t + zmax) / (2.f * h);
    const int k = u == u ? min((int)floorf(u), K - 2) : 0;
    const float w = u - (float)k;
    const float wr = weight ? weight[row] : 1.f;
    const float gs = grad_scale * wr, inv_s = 1.f / s;
    float* __restrict__ dl = dlogits + (size_t)row * ldd;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NREG; ++j) {
        const int i = lane + j * 64;
        if (i < K) {
            const float q = i == k ? 1.f - w : (i == k + 1 ? w : 0.f);
            if (i == k || i == k + 1) dot = fmaf(q, x[j] - mx, dot);
            dl[i] = gs * (e[j] * inv_s - q);
        }
    }
    dot = th_wave_sum(dot);
    if (lane == 0) {
        row_loss[row] = wr * (logf(s) - dot);           // the row maximum leaves both terms: sum q = 1
        if (value) value[row] = th_symexp(m);
    }
}

static int th_check(const char* name, int ld, int rows, int K, float zmax) {
    BD_REQUIRE(rows > 0, "%s: rows = %d", name, rows);
    BD_REQUIRE(K >= 2 && K <= 64 * kThLarge, "%s: %d bins (2 .. %d)", name, K, 64 * kThLarge);
    BD_REQUIRE(zmax > 0.f && zmax <= 80.f, "%s: bin range %g outside (0, 80]", name, (double)zmax);
    BD_REQUIRE(ld >= K, "%s: leading dimension %d < %d bins", name, ld, K);
    return 0;
}

}  // namespace bd

using namespace bd;

#define BD_TH_LAUNCH(kernel, ...)                                                                         \
    do {                                                                                                  \
        const dim3 grid_((unsigned)((rows + kThRows - 1) / kThRows)), block_(kThRows * 64);               \
        if (K <= 64 * kThSmall)                                                                           \
            hipLaunchKernelGGL(kernel<kThSmall>, grid_, block_, 0, (hipStream_t)stream, __VA_ARGS__);     \
        else                                                                                              \
            hipLaunchKernelGGL(kernel<kThLarge>, grid_, block_, 0, (hipStream_t)stream, __VA_ARGS__);     \
    } while (0)

extern "C" {

int bd_twohot_decode(const float* logits, int ld, int rows, int K, float zmax, float* value, float* mean, void* stream) {
    BD_REQUIRE(logits && value, "bd_twohot_decode: bad arguments");
    if (th_check("bd_twohot_decode", ld, rows, K, zmax)) return -1;
    const float h = zmax / (float)(K - 1);
    BD_TH_LAUNCH(twohot_decode_kernel, logits, ld, rows, K, h, value, mean);
    BD_CHECK_LAUNCH("bd_twohot_decode");
    return 0;
}

int bd_twohot_decode_backward(const float* logits, int ld, const float* dvalue, int rows, int K, float zmax, float* dlogits,
                              int ldd, void* stream) {
    BD_REQUIRE(logits && dvalue && dlogits, "bd_twohot_decode_backward: bad arguments");
    if (th_check("bd_twohot_decode_backward", ld < ldd ? ld : ldd, rows, K, zmax)) return -1;
    const float h = zmax / (float)(K - 1);
    BD_TH_LAUNCH(twohot_decode_bwd_kernel, logits, ld, dvalue, rows, K, h, dlogits, ldd);
    BD_CHECK_LAUNCH("bd_twohot_decode_backward");
    return 0;
}

int bd_twohot_nll(const float* logits, int ld, const float* target, const float* weight, int rows, int K, float zmax,
                  float grad_scale, float* dlogits, int ldd, float* value, float* row_loss, void* stream) {
    BD_REQUIRE(logits && target && dlogits && row_loss, "bd_twohot_nll: bad arguments");
    if (th_check("bd_twohot_nll", ld < ldd ? ld : ldd, rows, K, zmax)) return -1;
    const float h = zmax / (float)(K - 1);
    BD_TH_LAUNCH(twohot_nll_kernel, logits, ld, target, weight, rows, K, zmax, h, grad_scale, dlogits, ldd, value, row_loss);
    BD_CHECK_LAUNCH("bd_twohot_nll");
    return 0;
}

}  // extern "C"
