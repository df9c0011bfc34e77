// fingerprint.hip -- bd_fingerprint: 64-bit fingerprint and non-finite count of up to BD_FP_MAX_BUFFERS fp32 buffers in
// ONE launch (data-parallel replica check, NaN watch).  Definition in include/bigdreamer_hip.h; all integer arithmetic, the
// sum mod 2^64 is commutative, so the words do not depend on how elements fall on lanes, waves and workgroups.
//
// Geometry: kFpThreads lanes x up to kFpMaxBlocks workgroups, one 16-byte load per lane and trip: one pass of a full
// grid covers kFpMaxBlocks * kFpThreads * 4 = 1 048 576 elements; longer buffers are walked grid-stride.  Every workgroup
// walks every buffer of the table, sums in registers, reduces over the wave by shuffles and over the workgroup through
// LDS, and adds ONE 64-bit integer atomic per word to the output -- only for buffers it held elements of (a 200k-element
// buffer draws 196 atomics, not 1024).  Integer atomics: exact in any order.  The multiplier (i + 1) * golden is carried
// by additions, so an element costs two 64-bit multiplies, not three.
#include "bd_host.h"

namespace bd {

constexpr int kFpThreads = 256;
constexpr int kFpMaxBlocks = 1024;
constexpr unsigned long long kFpGolden = 0x9E3779B97F4A7C15ull;

struct FpTable {
    int n;
    const float* p[BD_FP_MAX_BUFFERS];
    unsigned long long count[BD_FP_MAX_BUFFERS];
};

// k = (i + 1) * golden of the element
__device__ __forceinline__ void fp_elem(unsigned u, unsigned long long k, unsigned long long& h, unsigned long long& nf) {
    unsigned long long x = (unsigned long long)u ^ k;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    h += x ^ (x >> 31);
    nf += (u & 0x7F800000u) == 0x7F800000u ? 1ull : 0ull;
}

__device__ __forceinline__ unsigned long long fp_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kFpThreads) void fingerprint_kernel(const FpTable t, unsigned long long* __restrict__ out) {
    constexpr int kW = kFpThreads / 64;
    __shared__ unsigned long long red[2][kW];
    const unsigned long long tid = (unsigned long long)blockIdx.x * kFpThreads + threadIdx.x;
    const unsigned long long nthr = (unsigned long long)gridDim.x * kFpThreads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = 0; b < t.n; ++b) {
        const unsigned* __restrict__ p = reinterpret_cast<const unsigned*>(t.p[b]);
        const unsigned long long n = t.count[b];
        // elements before the first 16-byte boundary (0 .. 3), then whole 16-byte groups, then the tail (0 .. 3)
        unsigned long long head = ((16u - (unsigned)((size_t)p & 15u)) & 15u) >> 2;
        if (head > n) head = n;
        const unsigned long long nvec = (n - head) >> 2;
        const unsigned long long tail0 = head + 4 * nvec;
        // workgroup-uniform: workgroup 0 takes head and tail, the others only their 16-byte groups
        if (n == 0 || (blockIdx.x != 0 && (unsigned long long)blockIdx.x * kFpThreads >= nvec)) continue;
        unsigned long long h = 0, nf = 0;
        const uint4* __restrict__ p4 = reinterpret_cast<const uint4*>(p + head);
        unsigned long long k = (head + 4 * tid + 1) * kFpGolden;
        const unsigned long long kstep = 4 * nthr * kFpGolden;
        for (unsigned long long v = tid; v < nvec; v += nthr, k += kstep) {
            const uint4 q = p4[v];
            fp_elem(q.x, k, h, nf);
            fp_elem(q.y, k + kFpGolden, h, nf);
            fp_elem(q.z, k + 2 * kFpGolden, h, nf);
            fp_elem(q.w, k + 3 * kFpGolden, h, nf);
        }
        if (tid < head) fp_elem(p[tid], (tid + 1) * kFpGolden, h, nf);                       // tid < 4: workgroup 0
        if (tid >= 4 && tid < 8) {
            const unsigned long long i = tail0 + (tid - 4);
            if (i < n) fp_elem(p[i], (i + 1) * kFpGolden, h, nf);
        }
        h = fp_wave_sum(h);
        nf = fp_wave_sum(nf);
        __syncthreads();                       // the previous buffer's reader of `red` is done
        if (lane == 0) {
            red[0][wave] = h;
            red[1][wave] = nf;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            unsigned long long s = 0;
#pragma unroll
            for (int w = 0; w < kW; ++w) s += red[threadIdx.x][w];
            if (s) atomicAdd(out + 2 * b + threadIdx.x, s);
        }
    }
}

}  // namespace bd

extern "C" {
using namespace bd;

int bd_fingerprint(const bd_fingerprint_args* a, unsigned long long* out, void* stream) {
    BD_REQUIRE(a != nullptr, "bd_fingerprint: null argument block");
    BD_REQUIRE(out != nullptr, "bd_fingerprint: null output");
    BD_REQUIRE(a->n_buf >= 0, "bd_fingerprint: n_buf = %d is negative", a->n_buf);
    BD_REQUIRE(a->n_buf <= BD_FP_MAX_BUFFERS, "bd_fingerprint: %d buffers (max %d)", a->n_buf, BD_FP_MAX_BUFFERS);
    FpTable t;
    t.n = a->n_buf;
    size_t longest = 0;
    for (int b = 0; b < a->n_buf; ++b) {
        BD_REQUIRE(a->buf[b].p != nullptr || a->buf[b].n == 0, "bd_fingerprint: buffer %d is null with n = %zu", b,
                   a->buf[b].n);
        BD_REQUIRE(((size_t)a->buf[b].p & 3u) == 0, "bd_fingerprint: buffer %d is not 4-byte aligned", b);
        t.p[b] = a->buf[b].p;
        t.count[b] = a->buf[b].n;
        if (a->buf[b].n > longest) longest = a->buf[b].n;
    }
    for (int b = a->n_buf; b < BD_FP_MAX_BUFFERS; ++b) {
        t.p[b] = nullptr;
        t.count[b] = 0;
    }
    if (a->n_buf == 0) return 0;
    hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(unsigned long long) * (size_t)a->n_buf, (hipStream_t)stream);
    if (e != hipSuccess) return fail("bd_fingerprint: hipMemsetAsync: %s", hipGetErrorString(e));
    if (longest == 0) return 0;
    size_t nb = (longest / 4 + kFpThreads - 1) / kFpThreads;      // 16-byte groups over the lanes; head and tail: workgroup 0
    if (nb < 1) nb = 1;
    if (nb > (size_t)kFpMaxBlocks) nb = kFpMaxBlocks;
    hipLaunchKernelGGL(fingerprint_kernel, dim3((unsigned)nb), dim3(kFpThreads), 0, (hipStream_t)stream, t, out);
    BD_CHECK_LAUNCH("bd_fingerprint");
    return 0;
}

}  // extern "C"
