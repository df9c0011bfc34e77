// symlog.hip -- symlog / symexp of a flat fp32 array ("World-model heads on any scale"; symlog_observations).
// Definitions in include/bigdreamer_hip.h.
//
// Two elementwise kernels, out of place: out = sign(x) log1p(|x|) and out = sign(x) expm1(|x|).  Precise log1pf / expm1f
// under copysignf: the sign bit of x goes to the result unchanged, so +-0 -> +-0 and f(-x) = -f(x) bit for bit; a NaN
// stays a NaN, +-inf stays +-inf (symexp overflows to +-inf where expm1f does).
// Memory: where x and out sit at the same offset from a 16-byte boundary the array is a dword head of up to three
// elements (up to the boundary), a body of float4 loads and stores, and a dword tail of up to three elements; where they
// do not, every element goes through the dword path.  The body is a grid-stride loop over float4s, head and tail are one
// grid-stride loop over at most six elements: every output element is written exactly once, nothing outside out[0, n).
// No LDS, no atomics, no scratch.
#include "bd_device.h"
#include "bd_host.h"

namespace bd {

constexpr int kSlThreads = 256;
constexpr unsigned kSlMaxBlocks = 2048;     // memory-bound: cap the grid and stride over the rest

template <bool EXP>
__device__ __forceinline__ float sl_apply(float v) {
    const float a = fabsf(v);
    return copysignf(EXP ? expm1f(a) : log1pf(a), v);
}

// x / out + head are 16-byte aligned (or nvec = 0); the dword elements are [0, head) and [head + 4 nvec, n)
template <bool EXP>
__global__ __launch_bounds__(kSlThreads) void symlog_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out,
                                                            size_t head, size_t nvec) {
    const size_t tid = (size_t)blockIdx.x * kSlThreads + threadIdx.x, stride = (size_t)gridDim.x * kSlThreads;
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
    float4* __restrict__ ov = reinterpret_cast<float4*>(out + head);
    for (size_t i = tid; i < nvec; i += stride) {
        float4 v = xv[i];
        v.x = sl_apply<EXP>(v.x);
        v.y = sl_apply<EXP>(v.y);
        v.z = sl_apply<EXP>(v.z);
        v.w = sl_apply<EXP>(v.w);
        ov[i] = v;
    }
    const size_t tail0 = head + 4 * nvec, nsingle = head + (n - tail0);
    for (size_t i = tid; i < nsingle; i += stride) {
        const size_t j = i < head ? i : tail0 + (i - head);
        out[j] = sl_apply<EXP>(x[j]);
    }
}

template <bool EXP>
static int sl_launch(const char* name, const float* x, size_t n, float* out, void* stream) {
    BD_REQUIRE(x && out, "%s: bad arguments", name);
    BD_REQUIRE(n > 0, "%s: n = 0", name);
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    BD_REQUIRE(xa % 4 == 0 && oa % 4 == 0, "%s: x and out must be 4-byte aligned", name);
    // out of place: out == x, and any other overlap of the two arrays, is refused
    BD_REQUIRE(oa + n * sizeof(float) <= xa || xa + n * sizeof(float) <= oa, "%s: out overlaps x (out of place only)", name);
    size_t head = n, nvec = 0;
    if (xa % 16 == oa % 16) {
        head = ((16 - xa % 16) % 16) / 4;
        if (head > n) head = n;
        nvec = (n - head) / 4;
    }
    const size_t work = nvec > head + 3 ? nvec : head + 3;       // (the dword loop has at most n - 4 nvec elements)
    size_t blocks = (work + kSlThreads - 1) / kSlThreads;
    if (nvec == 0) blocks = (n + kSlThreads - 1) / kSlThreads;
    if (blocks > kSlMaxBlocks) blocks = kSlMaxBlocks;
    hipLaunchKernelGGL(symlog_kernel<EXP>, dim3((unsigned)blocks), dim3(kSlThreads), 0, (hipStream_t)stream, x, n, out, head,
                       nvec);
    BD_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace bd

extern "C" {

int bd_symlog(const float* x, size_t n, float* out, void* stream) { return bd::sl_launch<false>("bd_symlog", x, n, out, stream); }

int bd_symexp(const float* x, size_t n, float* out, void* stream) { return bd::sl_launch<true>("bd_symexp", x, n, out, stream); }

}  // extern "C"
