// retnorm.hip -- percentile return normalisation of the actor objective ("Return normalisation").
// Definitions in include/bigdreamer_hip.h.
//
// bd_return_range: two exact order statistics of the step's M lambda-returns, the update of the running range and the
// scale of the next step, in ONE launch of ONE workgroup.  Radix selection on the order-preserving integer image of the
// floats, most significant digit first, 8 bits per pass: a pass counts the digit of every element that still matches the
// prefix found so far into a 256-bin LDS histogram (integer LDS atomics), one wave then scans the bins for the one that
// holds the wanted rank.  Both ranks are selected in the same four sweeps; while their prefixes agree (always in the
// first pass) they share one histogram.  Counts are integers, so the selected values do not depend on the schedule.
// One workgroup needs no cross-workgroup protocol and no global workspace: the buffer (150 KB .. 2.4 MB) is read four
// times from L2 by one CU, off the behaviour chain (the engine puts the launch on the critic's stream).
//
// Lanes of a wave that hold the same digit -- the rule in the first pass, whose digit is the sign and the high exponent
// bits, and with tied values -- would serialise on one LDS address.  rn_count therefore lets the lanes that share the
// first active lane's digit add their number through one lane, kRnPeel times, before the rest add singly.
#include "bd_device.h"
#include "bd_host.h"

namespace bd {

constexpr int kRnThreads = 1024;
constexpr int kRnBins = 256;
constexpr int kRnPeel = 3;

// order-preserving image: sign bit set -> all bits flipped, else sign bit flipped (-0.0 sorts just below +0.0)
__device__ __forceinline__ unsigned rn_key(unsigned u) { return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
__device__ __forceinline__ float rn_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// every lane of the wave calls this (wave-uniform control flow at the call site)
__device__ __forceinline__ void rn_count(unsigned* hist, bool active, unsigned digit) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < kRnPeel; ++r) {
        const unsigned long long m = __ballot(active);
        if (m == 0) return;                                       // wave-uniform
        const int leader = __builtin_ctzll(m);
        const unsigned d0 = __shfl(digit, leader, 64);
        const unsigned long long same = __ballot(active && digit == d0);
        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
        if (digit == d0) active = false;
    }
    if (active) atomicAdd(&hist[digit], 1u);
}

struct RnSel {
    unsigned prefix[2];        // the digits found so far, in place (low bits zero)
    unsigned rank[2];          // the wanted rank among the elements that match the prefix
    unsigned nonfinite;
};

// one element in pass `shift` (24, 16, 8, 0): mask = the bits above the digit
__device__ __forceinline__ void rn_element(unsigned* hist, const RnSel& s, bool shared, int shift, unsigned mask, bool valid,
                                           float v, unsigned& bad) {
    const unsigned u = __float_as_uint(v);
    if (valid && (u & 0x7F800000u) == 0x7F800000u) bad = 1u;
    const unsigned k = rn_key(u), digit = (k >> shift) & 0xFFu;
    rn_count(hist, valid && (k & mask) == s.prefix[0], digit);
    if (!shared) rn_count(hist + kRnBins, valid && (k & mask) == s.prefix[1], digit);
}

// wave w < 2 finds the bin of rank[w] in its histogram: lane l owns bins 4 l .. 4 l + 3
__device__ __forceinline__ void rn_pick(const unsigned* hist, RnSel& s, int which, int shift) {
    const int lane = threadIdx.x & 63;
    unsigned c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += c[j] = hist[4 * lane + j];
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    unsigned before = incl - sum;
    const unsigned want = s.rank[which];
    if (before <= want && want < incl) {                          // exactly one lane: the counts sum to more than the rank
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (want >= before && want < before + c[j]) {
                s.prefix[which] |= (unsigned)(4 * lane + j) << shift;
                s.rank[which] = want - before;
            }
            before += c[j];
        }
    }
}

__global__ __launch_bounds__(kRnThreads) void return_range_kernel(const float* __restrict__ x, unsigned M, unsigned k_lo,
                                                                  unsigned k_hi, double decay, double floor_,
                                                                  double* __restrict__ state, float* __restrict__ range) {
    __shared__ unsigned hist[2 * kRnBins];
    __shared__ RnSel sel;
    const unsigned tid = threadIdx.x;
    if (tid == 0) {
        sel.prefix[0] = sel.prefix[1] = 0u;
        sel.rank[0] = k_lo, sel.rank[1] = k_hi;
        sel.nonfinite = 0u;
    }
    // 16-byte loads from the first aligned element on; head and tail singly (one sweep round of their own)
    unsigned head = ((16u - (unsigned)((size_t)x & 15u)) & 15u) >> 2;
    if (head > M) head = M;
    const unsigned nvec = (M - head) >> 2, tail0 = head + 4u * nvec;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + head);
    unsigned bad = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
        if (tid < 2 * kRnBins) hist[tid] = 0u;
        __syncthreads();                                          // the histograms are clear
        const RnSel s = sel;
        const bool shared = s.prefix[0] == s.prefix[1];           // one histogram serves both ranks
        // (issuing the next trip's loads ahead of this trip's counting measured 15-25 % slower: the sweep is bound by the
        // counting, not by load latency)
        for (unsigned v0 = 0; v0 < nvec; v0 += 2u * kRnThreads) {            // workgroup-uniform trip count
            const unsigned va = v0 + tid, vb = va + kRnThreads;
            const bool oka = va < nvec, okb = vb < nvec;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (oka) a = x4[va];
            if (okb) b = x4[vb];
            rn_element(hist, s, shared, shift, mask, oka, a.x, bad);
            rn_element(hist, s, shared, shift, mask, oka, a.y, bad);
            rn_element(hist, s, shared, shift, mask, oka, a.z, bad);
            rn_element(hist, s, shared, shift, mask, oka, a.w, bad);
            rn_element(hist, s, shared, shift, mask, okb, b.x, bad);
            rn_element(hist, s, shared, shift, mask, okb, b.y, bad);
            rn_element(hist, s, shared, shift, mask, okb, b.z, bad);
            rn_element(hist, s, shared, shift, mask, okb, b.w, bad);
        }
        if (tid < 64) {                                           // wave 0: lanes 0..3 the head, 4..7 the tail
            const bool is_head = tid < head, is_tail = tid >= 4 && tid < 8 && tail0 + (tid - 4) < M;
            const unsigned i = is_head ? tid : tail0 + (tid - 4);
            const bool ok = is_head || is_tail;
            rn_element(hist, s, shared, shift, mask, ok, ok ? x[i] : 0.f, bad);
        }
        __syncthreads();                                          // every count is in
        if (tid < 64) {
            rn_pick(hist, sel, 0, shift);
        } else if (tid < 128) {
            rn_pick(shared ? hist : hist + kRnBins, sel, 1, shift);
        }
        __syncthreads();                                          // the bins are read, `sel` is whole
    }
    if (bad) sel.nonfinite = 1u;                                  // racing writers all store 1
    __syncthreads();
    if (tid == 0) {
        double lo = state[0], hi = state[1];
        if (sel.nonfinite) {
            state[3] += 1.0;
        } else {
            const double p_lo = (double)rn_value(sel.prefix[0]), p_hi = (double)rn_value(sel.prefix[1]);
            if (state[2] == 0.0) {
                lo = p_lo, hi = p_hi;
            } else {                                              // separate roundings: no contraction into an fma
                lo = __dadd_rn(__dmul_rn(decay, lo), __dmul_rn(1.0 - decay, p_lo));
                hi = __dadd_rn(__dmul_rn(decay, hi), __dmul_rn(1.0 - decay, p_hi));
            }
            state[0] = lo, state[1] = hi;
            state[2] += 1.0;
        }
        range[0] = (float)fmax(floor_, hi - lo);
        range[1] = (float)lo;
        range[2] = (float)hi;
    }
}

__global__ __launch_bounds__(256) void return_seed_kernel(const float* __restrict__ range, float dconst,
                                                          const float* __restrict__ weight, size_t n,
                                                          float* __restrict__ dret, float* __restrict__ scalars, int slot) {
    const float g = dconst / range[0];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dret[i] = weight ? g * weight[i] : g;
    if (scalars && blockIdx.x == 0 && threadIdx.x < 3) scalars[slot + threadIdx.x] = range[threadIdx.x];
}

}  // namespace bd

extern "C" {
using namespace bd;

int bd_return_range(const float* returns, int M, int k_lo, int k_hi, double decay, double floor_, double* state,
                    float* range, void* stream) {
    BD_REQUIRE(M >= 1, "bd_return_range: M = %d (must be at least 1)", M);
    BD_REQUIRE(0 <= k_lo && k_lo <= k_hi && k_hi < M, "bd_return_range: ranks (%d, %d) are not 0 <= k_lo <= k_hi < M = %d",
               k_lo, k_hi, M);
    BD_REQUIRE(decay >= 0.0 && decay < 1.0, "bd_return_range: decay %g outside [0, 1)", decay);
    BD_REQUIRE(floor_ > 0.0 && floor_ <= 3.0e38, "bd_return_range: floor %g is not a positive fp32 number", floor_);
    BD_REQUIRE(returns != nullptr && ((size_t)returns & 3u) == 0, "bd_return_range: returns is null or not 4-byte aligned");
    BD_REQUIRE(state != nullptr && ((size_t)state & 7u) == 0, "bd_return_range: state is null or not 8-byte aligned");
    BD_REQUIRE(range != nullptr && ((size_t)range & 3u) == 0, "bd_return_range: range is null or not 4-byte aligned");
    hipLaunchKernelGGL(return_range_kernel, dim3(1), dim3(kRnThreads), 0, (hipStream_t)stream, returns, (unsigned)M,
                       (unsigned)k_lo, (unsigned)k_hi, decay, floor_, state, range);
    BD_CHECK_LAUNCH("bd_return_range");
    return 0;
}

int bd_return_seed(const float* range, float dret_const, const float* weight, size_t n, float* dreturns, float* scalars,
                   int slot, void* stream) {
    BD_REQUIRE(range != nullptr && ((size_t)range & 3u) == 0, "bd_return_seed: range is null or not 4-byte aligned");
    BD_REQUIRE(dreturns != nullptr || n == 0, "bd_return_seed: null dreturns with n = %zu", n);
    BD_REQUIRE((((size_t)dreturns | (size_t)weight | (size_t)scalars) & 3u) == 0,
               "bd_return_seed: dreturns, weight or scalars is not 4-byte aligned");
    BD_REQUIRE(scalars == nullptr || slot >= 0, "bd_return_seed: slot = %d is negative", slot);
    BD_REQUIRE(n > 0 || scalars != nullptr, "bd_return_seed: nothing to write");
    size_t nb = (n + 255) / 256;
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    hipLaunchKernelGGL(return_seed_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, range, dret_const, weight,
                       n, dreturns, scalars, slot);
    BD_CHECK_LAUNCH("bd_return_seed");
    return 0;
}

}  // extern "C"
