// diag.hip -- training diagnostics: moments of step buffers, latent statistics (entropies, raw KL, per-dimension KL, class
// usage), per-module sums of squares of a flat parameter / gradient buffer.  Definitions in include/bigdreamer_hip.h.
//
// All four are memory-bound sweeps over buffers of 10^4 .. 10^7 floats that the train step has just written (L2 / Infinity
// Cache resident).  Common shape: a sweep launch in which every workgroup reduces its share to a row of fp64 partials in
// the workspace -- registers, wave shuffles, then the workgroup's four waves in fixed order through LDS -- and a second,
// tiny launch that combines the rows in fixed order: one wave per result, a lane sums rows lane, lane + 64, ... in
// sequence and the lanes meet in an xor butterfly.  No floating-point atomics anywhere, so the bits do not depend on
// scheduling.  Every workgroup of the sweep writes its whole row (identities where it held nothing): the workspace needs
// no clearing.  Flat sweeps load 16 bytes per lane where the address allows (head / tail elements singly).
#include "bd_device.h"
#include "bd_host.h"
#include "bd_latent.h"

namespace bd {

constexpr int kDgThreads = 256;
constexpr int kDgWaves = kDgThreads / 64;
constexpr int kDgMomBlocks = 256;          // bd_moments: rows of partials
constexpr int kDgSegBlocks = 1024;         // bd_segment_sumsq (the flat gradient / weight buffers: up to 10^7 floats)
constexpr int kDgLatBlocks = 128;          // bd_latent_stats
constexpr int kDgCatBlocks = 1024;         // bd_latent_stats_categorical
constexpr int kDgColSlots = 16384;         // doubles for per-workgroup column partials
constexpr size_t kDgWsDoubles = 32768;
static_assert((size_t)kDgMomBlocks * BD_MOMENTS_MAX_BUFFERS * BD_MOMENTS_WORDS <= kDgWsDoubles, "moments partials");
static_assert((size_t)kDgSegBlocks * BD_SEGMENTS_MAX <= kDgWsDoubles, "segment partials");
static_assert((size_t)kDgLatBlocks * BD_LATENT_WORDS + kDgColSlots <= kDgWsDoubles, "latent partials");
static_assert((size_t)kDgCatBlocks * BD_LATENT_CAT_WORDS + kDgCatBlocks <= kDgWsDoubles, "categorical partials");
constexpr float kGaussEntConst = 1.4189385332046727418f;      // 0.5 ln(2 pi e)

enum { kSum = 0, kMin = 1, kMax = 2 };
// kind of result v in a row whose entries from `sext_from` on are moments sextuples
__host__ __device__ __forceinline__ int dg_kind(int v, int sext_from) {
    if (v < sext_from) return kSum;
    const int k = (v - sext_from) % BD_MOMENTS_WORDS;
    return k == 3 ? kMin : (k == 4 ? kMax : kSum);
}
__device__ __forceinline__ double dg_identity(int kind) {
    return kind == kSum ? 0.0 : (kind == kMin ? (double)INFINITY : -(double)INFINITY);
}
__device__ __forceinline__ double dg_combine(double a, double b, int kind) {
    return kind == kSum ? a + b : (kind == kMin ? fmin(a, b) : fmax(a, b));
}
// over the 64 lanes; every lane gets the result (the butterfly adds the same pairs in every lane)
__device__ __forceinline__ double dg_wave(double v, int kind) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = dg_combine(v, __shfl_xor(v, o, 64), kind);
    return v;
}

// moments of the finite values a lane has seen
struct Mom {
    double s = 0.0, ss = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned cnt = 0, nf = 0;
    __device__ __forceinline__ void add(float v) {
        if ((__float_as_uint(v) & 0x7F800000u) != 0x7F800000u) {
            s += (double)v;
            ss += (double)v * (double)v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            ++cnt;
        } else {
            ++nf;
        }
    }
    __device__ __forceinline__ void store(double* v) const {
        v[0] = (double)cnt, v[1] = s, v[2] = ss, v[3] = (double)mn, v[4] = (double)mx, v[5] = (double)nf;
    }
};

// K per-lane values -> one row of partials: dst[k], k < K, written by thread k.  red: K * kDgWaves doubles of LDS.
template <int K>
__device__ __forceinline__ void dg_block_row(double (&v)[K], int sext_from, double* red, double* __restrict__ dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                          // the previous reader of `red` is done
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double r = dg_wave(v[k], dg_kind(k, sext_from));
        if (lane == 0) red[k * kDgWaves + wave] = r;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int kind = dg_kind(threadIdx.x, sext_from);
        double r = red[threadIdx.x * kDgWaves];
        for (int w = 1; w < kDgWaves; ++w) r = dg_combine(r, red[threadIdx.x * kDgWaves + w], kind);
        dst[threadIdx.x] = r;
    }
}

// ---- final passes -----------------------------------------------------------------------------------------------
// part: [nb][nvals]; one wave per result; nb = 0 gives the identities
__global__ __launch_bounds__(kDgThreads) void dg_final_kernel(const double* __restrict__ part, int nb, int nvals,
                                                              int sext_from, double* __restrict__ out) {
    const int v = blockIdx.x * kDgWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= nvals) return;                   // wave-uniform
    const int kind = dg_kind(v, sext_from);
    double r = dg_identity(kind);
    for (int b = lane; b < nb; b += 64) r = dg_combine(r, part[(size_t)b * nvals + v], kind);
    r = dg_wave(r, kind);
    if (lane == 0) out[v] = r;
}

// colpart: [nb][ncols]; one lane per column, rows in sequence
__global__ __launch_bounds__(kDgThreads) void dg_col_final_kernel(const double* __restrict__ colpart, int nb, int ncols,
                                                                  double* __restrict__ colsum) {
    const int j = blockIdx.x * kDgThreads + threadIdx.x;
    if (j >= ncols) return;
    double r = 0.0;
    for (int b = 0; b < nb; ++b) r += colpart[(size_t)b * ncols + j];
    colsum[j] = r;
}

// ---- bd_moments --------------------------------------------------------------------------------------------------
struct MomTable {
    int n;
    const float* p[BD_MOMENTS_MAX_BUFFERS];
    const float* q[BD_MOMENTS_MAX_BUFFERS];
    unsigned long long count[BD_MOMENTS_MAX_BUFFERS];
};

__global__ __launch_bounds__(kDgThreads) void moments_kernel(const MomTable t, double* __restrict__ part) {
    __shared__ double red[BD_MOMENTS_WORDS * kDgWaves];
    const unsigned long long tid = (unsigned long long)blockIdx.x * kDgThreads + threadIdx.x;
    const unsigned long long nthr = (unsigned long long)gridDim.x * kDgThreads;
    for (int b = 0; b < t.n; ++b) {
        const float* __restrict__ p = t.p[b];
        const float* __restrict__ q = t.q[b];
        const unsigned long long n = t.count[b];
        double* dst = part + ((size_t)blockIdx.x * t.n + b) * BD_MOMENTS_WORDS;
        // 16-byte loads need p (and q) on the same 16-byte phase; otherwise every element is read singly
        const bool vec = q == nullptr || (((size_t)p ^ (size_t)q) & 15u) == 0;
        unsigned long long head = vec ? ((16u - (unsigned)((size_t)p & 15u)) & 15u) >> 2 : n;
        if (head > n) head = n;
        const unsigned long long nvec = (n - head) >> 2;
        const unsigned long long tail0 = head + 4 * nvec;
        // workgroup-uniform: workgroup 0 takes head and tail (and is the one that exists when n is tiny)
        const bool mine = n != 0 && (blockIdx.x == 0 || (unsigned long long)blockIdx.x * kDgThreads < (vec ? nvec : n));
        if (!mine) {
            if (threadIdx.x < BD_MOMENTS_WORDS) dst[threadIdx.x] = dg_identity(dg_kind(threadIdx.x, 0));
            continue;
        }
        Mom m;
        if (vec) {
            const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
            const float4* __restrict__ q4 = reinterpret_cast<const float4*>(q ? q + head : nullptr);
            for (unsigned long long v = tid; v < nvec; v += nthr) {
                float4 x = p4[v];
                if (q) {
                    const float4 y = q4[v];
                    x.x -= y.x, x.y -= y.y, x.z -= y.z, x.w -= y.w;
                }
                m.add(x.x), m.add(x.y), m.add(x.z), m.add(x.w);
            }
            if (tid < head) m.add(q ? p[tid] - q[tid] : p[tid]);                     // tid < 4: workgroup 0
            if (tid >= 4 && tid < 8) {
                const unsigned long long i = tail0 + (tid - 4);
                if (i < n) m.add(q ? p[i] - q[i] : p[i]);
            }
        } else {
            for (unsigned long long i = tid; i < n; i += nthr) m.add(p[i] - q[i]);
        }
        double v[BD_MOMENTS_WORDS];
        m.store(v);
        dg_block_row<BD_MOMENTS_WORDS>(v, 0, red, dst);
    }
}

// ---- bd_segment_sumsq ----------------------------------------------------------------------------------------------
struct SegTable {
    int n;
    unsigned long long off[BD_SEGMENTS_MAX + 1];
};

// workgroup b owns elements [begin + b * chunk, begin + (b + 1) * chunk) of the buffer; per segment it reduces the
// overlap of its chunk with the segment
__global__ __launch_bounds__(kDgThreads) void segment_sumsq_kernel(const float* __restrict__ x, const SegTable t,
                                                                   unsigned long long chunk, double* __restrict__ part) {
    __shared__ double red[kDgWaves];
    const unsigned long long c0 = t.off[0] + (unsigned long long)blockIdx.x * chunk, c1 = c0 + chunk;
    for (int s = 0; s < t.n; ++s) {
        const unsigned long long lo = t.off[s] > c0 ? t.off[s] : c0, hi = t.off[s + 1] < c1 ? t.off[s + 1] : c1;
        double* dst = part + (size_t)blockIdx.x * t.n + s;
        if (lo >= hi) {                                           // workgroup-uniform
            if (threadIdx.x == 0) *dst = 0.0;
            continue;
        }
        const float* __restrict__ p = x + lo;
        const unsigned long long n = hi - lo;
        unsigned long long head = ((16u - (unsigned)((size_t)p & 15u)) & 15u) >> 2;
        if (head > n) head = n;
        const unsigned long long nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
        // four independent 16-byte loads and accumulators per trip: the sweep is latency-bound otherwise
        double acc = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        unsigned long long g = threadIdx.x;
        for (; g + 3 * kDgThreads < nvec; g += 4 * kDgThreads) {
            const float4 a = p4[g], b = p4[g + kDgThreads], c = p4[g + 2 * kDgThreads], d = p4[g + 3 * kDgThreads];
            acc += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
            acc1 += (double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z + (double)b.w * b.w;
            acc2 += (double)c.x * c.x + (double)c.y * c.y + (double)c.z * c.z + (double)c.w * c.w;
            acc3 += (double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z + (double)d.w * d.w;
        }
        for (; g < nvec; g += kDgThreads) {
            const float4 a = p4[g];
            acc += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
        }
        acc = (acc + acc1) + (acc2 + acc3);
        if (threadIdx.x < head) acc += (double)p[threadIdx.x] * p[threadIdx.x];
        if (threadIdx.x >= 4 && threadIdx.x < 8) {
            const unsigned long long i = tail0 + (threadIdx.x - 4);
            if (i < n) acc += (double)p[i] * p[i];
        }
        double v[1] = {acc};
        dg_block_row<1>(v, 1, red, dst);
    }
}

// ---- bd_latent_stats (Gaussian) ------------------------------------------------------------------------------------
// A wave walks rows (wave w of workgroup b: rows 4 b + w, + 4 gridDim.x, ...), its lanes the columns j0 + lane of one
// 64-column slab at a time: coalesced, and a lane's KL sum IS a column partial.  nb == 1: colsum is written directly.
__global__ __launch_bounds__(kDgThreads) void latent_stats_kernel(const float* __restrict__ qm, const float* __restrict__ qs,
                                                                  const float* __restrict__ pm, const float* __restrict__ ps,
                                                                  int rows, int S, double* __restrict__ part,
                                                                  double* __restrict__ colpart) {
    __shared__ double red[BD_LATENT_WORDS * kDgWaves];
    __shared__ double colw[kDgWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double ent_q = 0.0, ent_p = 0.0, kl = 0.0;
    Mom mq, mp;
    for (int j0 = 0; j0 < S; j0 += 64) {                          // workgroup-uniform trip count
        const int j = j0 + lane;
        double col = 0.0;
        if (j < S) {
            for (int r = blockIdx.x * kDgWaves + wave; r < rows; r += gridDim.x * kDgWaves) {
                const size_t i = (size_t)r * S + j;
                const float a = qm[i], b = qs[i], c = pm[i], d = ps[i];
                const float k = kl_elem(a, b, c, d);
                col += (double)k;
                ent_q += (double)(kGaussEntConst + logf(b));
                ent_p += (double)(kGaussEntConst + logf(d));
                mq.add(b);
                mp.add(d);
            }
        }
        kl += col;
        __syncthreads();                      // the previous slab's reader of `colw` is done
        colw[wave][lane] = col;
        __syncthreads();
        if (wave == 0 && j < S) {
            double r = colw[0][lane];
            for (int w = 1; w < kDgWaves; ++w) r += colw[w][lane];
            colpart[(size_t)blockIdx.x * S + j] = r;
        }
    }
    double v[BD_LATENT_WORDS];
    v[0] = ent_q, v[1] = ent_p, v[2] = kl;
    mq.store(v + 3);
    mp.store(v + 9);
    dg_block_row<BD_LATENT_WORDS>(v, 3, red, part + (size_t)blockIdx.x * BD_LATENT_WORDS);
}

// ---- bd_latent_stats_categorical -----------------------------------------------------------------------------------
// grid (rb, gy): workgroup (bx, by) takes factors d = by, by + gy, ... and of each the rows 8 bx + hw, + 8 rb, ... on its
// eight half waves (the group layout of the loss kernels, bd_latent.h).  rb == 1: colsum is written directly.
__global__ __launch_bounds__(kDgThreads) void latent_stats_cat_kernel(const float* __restrict__ ql, const float* __restrict__ pl,
                                                                      int rows, int D, int C, double* __restrict__ part,
                                                                      double* __restrict__ colpart, unsigned* __restrict__ used) {
    __shared__ double red[BD_LATENT_CAT_WORDS * kDgWaves];
    __shared__ double colh[2 * kDgWaves];
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    double hq = 0.0, hp = 0.0, kl = 0.0, mxq = 0.0, mxp = 0.0;    // held by lane 0 of each half wave
    for (int d = blockIdx.y; d < D; d += gridDim.y) {             // workgroup-uniform trip count
        double col = 0.0;
        for (int r = blockIdx.x * 8 + hw; r < rows; r += gridDim.x * 8) {
            const size_t base = ((size_t)r * D + d) * C;
            float lq[kCatPer], lp[kCatPer];
            group_log_softmax(ql + base, C, l, lq);
            group_log_softmax(pl + base, C, l, lp);
            const float k = group_kl(lq, lp, C, l);
            float eq = 0.f, ep = 0.f, bp = -INFINITY, best = -INFINITY;
            int arg = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < kCatPer; ++i) {
                const int c = l + 32 * i;
                if (c < C) {
                    const float qv = expf(lq[i]), pv = expf(lp[i]);
                    eq -= qv == 0.f ? 0.f : qv * lq[i];
                    ep -= pv == 0.f ? 0.f : pv * lp[i];
                    bp = fmaxf(bp, lp[i]);
                    if (lq[i] > best) { best = lq[i]; arg = c; }      // first maximum wins (argmax)
                }
            }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oa = __shfl_xor(arg, o, 64);
                if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
            }
            eq = half_sum(eq);
            ep = half_sum(ep);
            bp = half_max(bp);
            if (l == 0) {
                col += (double)k;
                hq += (double)eq;
                hp += (double)ep;
                mxq += (double)expf(best);
                mxp += (double)expf(bp);
                if (arg < C) used[(size_t)d * C + arg] = 1u;      // racing writers all store 1
            }
        }
        kl += col;
        __syncthreads();                      // the previous factor's reader of `colh` is done
        if (l == 0) colh[hw] = col;
        __syncthreads();
        if (threadIdx.x == 0) {
            double r = colh[0];
            for (int h = 1; h < 2 * kDgWaves; ++h) r += colh[h];
            colpart[(size_t)blockIdx.x * D + d] = r;
        }
    }
    double v[BD_LATENT_CAT_WORDS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (l == 0) v[0] = hq, v[1] = hp, v[2] = kl, v[3] = mxq, v[4] = mxp;
    dg_block_row<BD_LATENT_CAT_WORDS>(v, BD_LATENT_CAT_WORDS, red,
                                      part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * BD_LATENT_CAT_WORDS);
}

static int dg_final(const double* part, int nb, int nvals, int sext_from, double* out, hipStream_t s, const char* name) {
    hipLaunchKernelGGL(dg_final_kernel, dim3((nvals + kDgWaves - 1) / kDgWaves), dim3(kDgThreads), 0, s, part, nb, nvals,
                       sext_from, out);
    BD_CHECK_LAUNCH(name);
    return 0;
}

static int dg_col_final(const double* colpart, int nb, int ncols, double* colsum, hipStream_t s, const char* name) {
    hipLaunchKernelGGL(dg_col_final_kernel, dim3((ncols + kDgThreads - 1) / kDgThreads), dim3(kDgThreads), 0, s, colpart, nb,
                       ncols, colsum);
    BD_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace bd

extern "C" {
using namespace bd;

size_t bd_diag_ws_floats(void) { return 2 * kDgWsDoubles; }

int bd_moments(const bd_moments_args* a, double* out, float* ws, void* stream) {
    BD_REQUIRE(a != nullptr, "bd_moments: null argument block");
    BD_REQUIRE(out != nullptr && ((size_t)out & 7u) == 0, "bd_moments: output is null or not 8-byte aligned");
    BD_REQUIRE(ws != nullptr && ((size_t)ws & 7u) == 0, "bd_moments: workspace is null or not 8-byte aligned");
    BD_REQUIRE(a->n_buf >= 0, "bd_moments: n_buf = %d is negative", a->n_buf);
    BD_REQUIRE(a->n_buf <= BD_MOMENTS_MAX_BUFFERS, "bd_moments: %d buffers (max %d)", a->n_buf, BD_MOMENTS_MAX_BUFFERS);
    MomTable t;
    t.n = a->n_buf;
    size_t longest = 0;
    for (int b = 0; b < BD_MOMENTS_MAX_BUFFERS; ++b) {
        t.p[b] = t.q[b] = nullptr;
        t.count[b] = 0;
        if (b >= a->n_buf) continue;
        BD_REQUIRE(a->buf[b].p != nullptr || a->buf[b].n == 0, "bd_moments: buffer %d is null with n = %zu", b, a->buf[b].n);
        BD_REQUIRE((((size_t)a->buf[b].p | (size_t)a->buf[b].q) & 3u) == 0, "bd_moments: buffer %d is not 4-byte aligned", b);
        t.p[b] = a->buf[b].p;
        t.q[b] = a->buf[b].n ? a->buf[b].q : nullptr;
        t.count[b] = a->buf[b].n;
        if (a->buf[b].n > longest) longest = a->buf[b].n;
    }
    if (a->n_buf == 0) return 0;
    int nb = 0;
    if (longest > 0) {
        size_t want = (longest / 4 + kDgThreads - 1) / kDgThreads;
        nb = (int)(want < 1 ? 1 : (want > (size_t)kDgMomBlocks ? (size_t)kDgMomBlocks : want));
        hipLaunchKernelGGL(moments_kernel, dim3(nb), dim3(kDgThreads), 0, (hipStream_t)stream, t, (double*)ws);
        BD_CHECK_LAUNCH("bd_moments");
    }
    return dg_final((const double*)ws, nb, a->n_buf * BD_MOMENTS_WORDS, 0, out, (hipStream_t)stream, "bd_moments(final)");
}

int bd_segment_sumsq(const float* x, int n_seg, const size_t* offsets, double* out, float* ws, void* stream) {
    BD_REQUIRE(out != nullptr && ((size_t)out & 7u) == 0, "bd_segment_sumsq: output is null or not 8-byte aligned");
    BD_REQUIRE(ws != nullptr && ((size_t)ws & 7u) == 0, "bd_segment_sumsq: workspace is null or not 8-byte aligned");
    BD_REQUIRE(n_seg >= 0, "bd_segment_sumsq: n_seg = %d is negative", n_seg);
    BD_REQUIRE(n_seg <= BD_SEGMENTS_MAX, "bd_segment_sumsq: %d segments (max %d)", n_seg, BD_SEGMENTS_MAX);
    if (n_seg == 0) return 0;
    BD_REQUIRE(offsets != nullptr, "bd_segment_sumsq: null offsets");
    SegTable t;
    t.n = n_seg;
    for (int s = 0; s <= BD_SEGMENTS_MAX; ++s) t.off[s] = offsets[s <= n_seg ? s : n_seg];
    for (int s = 0; s < n_seg; ++s)
        BD_REQUIRE(offsets[s] <= offsets[s + 1], "bd_segment_sumsq: offsets decrease at segment %d (%zu > %zu)", s, offsets[s],
                   offsets[s + 1]);
    const size_t total = offsets[n_seg] - offsets[0];
    BD_REQUIRE(x != nullptr || total == 0, "bd_segment_sumsq: null buffer");
    BD_REQUIRE(((size_t)x & 3u) == 0, "bd_segment_sumsq: buffer is not 4-byte aligned");
    int nb = 0;
    if (total > 0) {
        // chunks of whole 16-byte groups, at least four loads per lane before a workgroup is worth adding
        size_t want = (total + 4 * 4 * kDgThreads - 1) / (4 * 4 * kDgThreads);
        nb = (int)(want > (size_t)kDgSegBlocks ? (size_t)kDgSegBlocks : want);
        size_t chunk = (total + nb - 1) / nb;
        chunk = (chunk + 3) & ~(size_t)3;
        hipLaunchKernelGGL(segment_sumsq_kernel, dim3(nb), dim3(kDgThreads), 0, (hipStream_t)stream, x, t,
                           (unsigned long long)chunk, (double*)ws);
        BD_CHECK_LAUNCH("bd_segment_sumsq");
    }
    return dg_final((const double*)ws, nb, n_seg, n_seg, out, (hipStream_t)stream, "bd_segment_sumsq(final)");
}

int bd_latent_stats(const float* qm, const float* qs, const float* pm, const float* ps, int rows, int S, double* out,
                    double* colsum, float* ws, void* stream) {
    BD_REQUIRE(qm && qs && pm && ps, "bd_latent_stats: null input");
    BD_REQUIRE((((size_t)qm | (size_t)qs | (size_t)pm | (size_t)ps) & 3u) == 0, "bd_latent_stats: input is not 4-byte aligned");
    BD_REQUIRE(out != nullptr && ((size_t)out & 7u) == 0, "bd_latent_stats: output is null or not 8-byte aligned");
    BD_REQUIRE(colsum != nullptr && ((size_t)colsum & 7u) == 0, "bd_latent_stats: colsum is null or not 8-byte aligned");
    BD_REQUIRE(ws != nullptr && ((size_t)ws & 7u) == 0, "bd_latent_stats: workspace is null or not 8-byte aligned");
    BD_REQUIRE(rows > 0 && S > 0, "bd_latent_stats: bad dims (rows=%d S=%d)", rows, S);
    int cap = kDgColSlots / S;
    cap = cap < 1 ? 1 : (cap > kDgLatBlocks ? kDgLatBlocks : cap);
    int nb = (rows + kDgWaves - 1) / kDgWaves;
    nb = nb > cap ? cap : nb;
    double* part = (double*)ws;
    double* colpart = nb == 1 ? colsum : part + (size_t)kDgLatBlocks * BD_LATENT_WORDS;
    hipLaunchKernelGGL(latent_stats_kernel, dim3(nb), dim3(kDgThreads), 0, (hipStream_t)stream, qm, qs, pm, ps, rows, S, part,
                       colpart);
    BD_CHECK_LAUNCH("bd_latent_stats");
    if (nb > 1 && dg_col_final(colpart, nb, S, colsum, (hipStream_t)stream, "bd_latent_stats(columns)")) return -1;
    return dg_final(part, nb, BD_LATENT_WORDS, 3, out, (hipStream_t)stream, "bd_latent_stats(final)");
}

int bd_latent_stats_categorical(const float* post_logits, const float* prior_logits, int rows, int D, int C, double* out,
                                double* colsum, unsigned* used, float* ws, void* stream) {
    BD_REQUIRE(post_logits && prior_logits, "bd_latent_stats_categorical: null input");
    BD_REQUIRE((((size_t)post_logits | (size_t)prior_logits | (size_t)used) & 3u) == 0,
               "bd_latent_stats_categorical: input or `used` is not 4-byte aligned");
    BD_REQUIRE(out != nullptr && ((size_t)out & 7u) == 0, "bd_latent_stats_categorical: output is null or not 8-byte aligned");
    BD_REQUIRE(colsum != nullptr && ((size_t)colsum & 7u) == 0,
               "bd_latent_stats_categorical: colsum is null or not 8-byte aligned");
    BD_REQUIRE(used != nullptr, "bd_latent_stats_categorical: null `used`");
    BD_REQUIRE(ws != nullptr && ((size_t)ws & 7u) == 0, "bd_latent_stats_categorical: workspace is null or not 8-byte aligned");
    BD_REQUIRE(rows > 0 && D > 0, "bd_latent_stats_categorical: bad dims (rows=%d D=%d)", rows, D);
    BD_REQUIRE(C > 0 && C <= 32 * kCatPer, "bd_latent_stats_categorical: %d classes (max %d)", C, 32 * kCatPer);
    const int gy = D > kDgCatBlocks ? kDgCatBlocks : D;
    int rb = (rows + 7) / 8;
    const int cap = kDgCatBlocks / gy;                            // gy * rb <= kDgCatBlocks, D * rb <= kDgCatBlocks if rb > 1
    rb = rb > cap ? cap : rb;
    double* part = (double*)ws;
    double* colpart = rb == 1 ? colsum : part + (size_t)kDgCatBlocks * BD_LATENT_CAT_WORDS;
    hipError_t e = hipMemsetAsync(used, 0, sizeof(unsigned) * (size_t)D * C, (hipStream_t)stream);
    if (e != hipSuccess) return fail("bd_latent_stats_categorical: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(latent_stats_cat_kernel, dim3(rb, gy), dim3(kDgThreads), 0, (hipStream_t)stream, post_logits,
                       prior_logits, rows, D, C, part, colpart, used);
    BD_CHECK_LAUNCH("bd_latent_stats_categorical");
    if (rb > 1 && dg_col_final(colpart, rb, D, colsum, (hipStream_t)stream, "bd_latent_stats_categorical(columns)")) return -1;
    return dg_final(part, rb * gy, BD_LATENT_CAT_WORDS, BD_LATENT_CAT_WORDS, out, (hipStream_t)stream,
                    "bd_latent_stats_categorical(final)");
}

}  // extern "C"
