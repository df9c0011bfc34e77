// cabi.hip -- error reporting, version, weight packing, replay gather.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_rng.h"

namespace bd {
char* err_buf() {
    static thread_local char buf[512] = "";
    return buf;
}

// One block column per descriptor (blockIdx.y); blockIdx.x strides over its 16x16 blocks; each thread
// writes one packed float4: dst[(nb*Kb + kb)*64 + lane] = {W[n][k0..k0+3]}, n = nb*16 + (lane&15),
// k0 = kb*16 + 4*(lane>>4); transposed descriptors read W[k][n] instead.
//
// Product descriptors (BD_PACK_PRODUCT: dst = packed A.B, A = src [N x E], B = src2 [E x K]): a workgroup takes one 16x16
// block C[n][k] of the product at a time and walks e in pieces of kPackE staged through LDS (each source element is
// loaded once per block -- register-level broadcast loads made the same work four times as long; the next piece's loads
// are in flight while this one is multiplied).  Wave w sums the w-th quarter of every piece, pieces in ascending order,
// and the four partial sums are added in wave order: one fixed order whatever the grid.  The block is then written in
// the packed lane order of A.B or of its transpose.  BD_PACK_PRODUCT_VEC (dst[n] = A[n].b): one wave per n, 64 strided
// partial sums combined by a butterfly.
//
// The grid is one-dimensional: kPackCopyX workgroups per copy descriptor, then kPackProdX per trailing product descriptor
// (bd_pack_weights).
constexpr int kPackThreads = 256, kPackWaves = kPackThreads / 64;
constexpr int kPackCopyX = 16;
constexpr int kPackProdX = 192;      // product blocks of a 200 x 200 output (169) get a workgroup each
constexpr int kPackE = 256;          // e per staged piece: 16 x 256 of A and 256 x 16 of B, four float4s each per thread
struct alignas(16) PackLds {
    float a[16][kPackE + 1];         // [n][e], odd pitch: the 16 rows a wave reads at one e lie in 16 banks
    float b[kPackE][16];             // [e][k]
    float part[kPackWaves][16][17];  // [wave][n][k]
};
__device__ __forceinline__ void pack_product(const bd_pack_desc& d, int bx, int nx, PackLds& L) {
    const int Nb = (d.N + 15) >> 4, Kb = (d.K + 15) >> 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ A = d.src;
    const float* __restrict__ B = d.src2;
    // float4 loads along e (rows of A) / along k (rows of B) where every address they touch is 16-byte aligned
    const bool vec = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 && (d.ld & 3) == 0 &&
                     (d.ld2 & 3) == 0 && (d.K & 3) == 0 && (d.E & 3) == 0;
    floatx4* __restrict__ dst = reinterpret_cast<floatx4*>(d.dst);
    for (int blk = bx; blk < Nb * Kb; blk += nx) {
        const int nb = blk / Kb, kb = blk - nb * Kb;
        const int n0 = nb * 16, k0 = kb * 16;
        floatx4 ar[4], br[4];
        // thread -> (row n0 + idx / 64, e = 4 (idx % 64)) of A and (e = idx / 4, k = k0 + 4 (idx % 4)) of B, idx = tid + 256 j
        auto fetch = [&](int e0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = tid + 256 * j;
                const int n = n0 + (idx >> 6), ea = e0 + 4 * (idx & 63);
                const int eb = e0 + (idx >> 2), k = k0 + 4 * (idx & 3);
                if (vec) {
                    ar[j] = (n < d.N && ea < d.E) ? *reinterpret_cast<const floatx4*>(A + (size_t)n * d.ld + ea) : floatx4{0.f, 0.f, 0.f, 0.f};
                    br[j] = (eb < d.E && k < d.K) ? *reinterpret_cast<const floatx4*>(B + (size_t)eb * d.ld2 + k) : floatx4{0.f, 0.f, 0.f, 0.f};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ar[j][i] = (n < d.N && ea + i < d.E) ? A[(size_t)n * d.ld + ea + i] : 0.f;
                        br[j][i] = (eb < d.E && k + i < d.K) ? B[(size_t)eb * d.ld2 + k + i] : 0.f;
                    }
                }
            }
        };
        const int n = lane & 15, kq = 4 * (lane >> 4);        // this lane's C[n][kq .. kq + 3] over its wave's quarter
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        fetch(0);
        for (int e0 = 0; e0 < d.E; e0 += kPackE) {
            __syncthreads();            // the previous piece (and the previous block's partial sums) have been read
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = tid + 256 * j;
#pragma unroll
                for (int i = 0; i < 4; ++i) L.a[idx >> 6][4 * (idx & 63) + i] = ar[j][i];
                *reinterpret_cast<floatx4*>(&L.b[idx >> 2][4 * (idx & 3)]) = br[j];
            }
            __syncthreads();
            if (e0 + kPackE < d.E) fetch(e0 + kPackE);
            const int w0 = wave * (kPackE / kPackWaves);
#pragma unroll 8
            for (int e = w0; e < w0 + kPackE / kPackWaves; ++e) {      // (entries past E are zero)
                const float av = L.a[n][e];
                const floatx4 bv = *reinterpret_cast<const floatx4*>(&L.b[e][kq]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(av, bv[i], acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) L.part[wave][n][kq + i] = acc[i];
        __syncthreads();
        if (wave == 0) {                // packed lane order: (out, 4 x in) = (n, k ..) of A.B, (k, n ..) of its transpose
            floatx4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cn = d.transpose ? kq + i : n, ck = d.transpose ? n : kq + i;
                float t = L.part[0][cn][ck];
#pragma unroll
                for (int w = 1; w < kPackWaves; ++w) t += L.part[w][cn][ck];
                v[i] = t;
            }
            const int ob = d.transpose ? kb * Nb + nb : blk;
            dst[(size_t)ob * 64 + lane] = v;
        }
    }
}

__device__ __forceinline__ void pack_product_vec(const bd_pack_desc& d, int bx, int nx) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int n = bx * kPackWaves + wave; n < d.N; n += nx * kPackWaves) {
        float s = 0.f;
        for (int e = lane; e < d.E; e += 64) s = fmaf(d.src[(size_t)n * d.ld + e], d.src2[e], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) d.dst[n] = s;
    }
}

__global__ __launch_bounds__(kPackThreads) void pack_kernel(const bd_pack_desc* __restrict__ descs, int n_copy) {
    extern __shared__ floatx4 pack_lds[];       // sizeof(PackLds) when the table has product descriptors, else nothing
    PackLds& lds = *reinterpret_cast<PackLds*>(pack_lds);
    const int pb = (int)blockIdx.x - n_copy * kPackCopyX;         // >= 0: a workgroup of the product descriptors
    const bd_pack_desc d = descs[pb < 0 ? blockIdx.x / kPackCopyX : n_copy + pb / kPackProdX];
    // (a product descriptor must be counted in n_prod: its workgroups need the LDS the launch then asks for)
    const int bx = pb < 0 ? blockIdx.x % kPackCopyX : pb % kPackProdX, nx = pb < 0 ? kPackCopyX : kPackProdX;
    if (pb >= 0 && d.kind == BD_PACK_PRODUCT) return pack_product(d, bx, nx, lds);
    if (pb >= 0 && d.kind == BD_PACK_PRODUCT_VEC) return pack_product_vec(d, bx, nx);
    const int No = d.transpose ? d.K : d.N;   // packed "out" dim
    const int Ki = d.transpose ? d.N : d.K;   // packed "in" dim
    const int Nb = (No + 15) >> 4, Kb = (Ki + 15) >> 4;
    const int total = Nb * Kb * 64;
    floatx4* __restrict__ dst = reinterpret_cast<floatx4*>(d.dst);
    for (int e = bx * kPackThreads + threadIdx.x; e < total; e += nx * kPackThreads) {
        const int lane = e & 63, blk = e >> 6;
        const int nb = blk / Kb, kb = blk - nb * Kb;
        const int n = nb * 16 + (lane & 15);
        const int k0 = kb * 16 + 4 * (lane >> 4);
        floatx4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + i;
            float x = 0.f;
            if (n < No && k < Ki) x = d.transpose ? d.src[(size_t)k * d.ld + n] : d.src[(size_t)n * d.ld + k];
            v[i] = x;
        }
        dst[e] = v;
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                          int n_idx, int width, float* __restrict__ dst) {
    const size_t total = (size_t)n_idx * width;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / width, c = e - r * width;
        dst[e] = src[(size_t)idx[r] * width + c];
    }
}
// Pixel replay: gather uint8 frames by row index and undo the bit-depth quantisation in one pass
// (ExperienceReplay._retrieve_batch + preprocess_observation_, src/memory.py:70-85, src/utils.py:299-317):
//   out = floor(u8 / 2^(8-bits)) / 2^bits - 0.5 + noise / 2^bits        (noise ~ U[0,1), explicit input)
// HBM-bound byte work: 4 pixels per thread (uchar4 in, float4 noise in, float4 out), fully coalesced.
// RNG = true (perf mode): the dequantisation noise U[0, 1) of the four pixels is one Philox4x32-10 call (bd_rng.h) instead of
// a 16-byte read of a noise tensor that a library kernel wrote (120 MB per step at configs[2], written and read once).
template <bool RNG>
__global__ __launch_bounds__(256) void gather_pixels_kernel(const unsigned char* __restrict__ src,
                                                            const int64_t* __restrict__ idx, int n_idx, int pixels,
                                                            float inv_q, float inv_b, const float* __restrict__ noise,
                                                            float* __restrict__ dst, Rng rng) {
    const int quads = pixels >> 2;
    const size_t total = (size_t)n_idx * quads;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / quads, q = e - r * quads;
        const uchar4 u = reinterpret_cast<const uchar4*>(src + (size_t)idx[r] * pixels)[q];
        floatx4 nz;
        if constexpr (RNG) {
            const Philox4 p = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), rng.stream, rng.step, rng.k0, rng.k1);
#pragma unroll
            for (int j = 0; j < 4; ++j) nz[j] = (float)(p.x[j] >> 8) * (1.0f / 16777216.0f);       // [0, 1) as rand_like
        } else {
            nz = reinterpret_cast<const floatx4*>(noise)[e];
        }
        floatx4 o;
        o[0] = floorf((float)u.x * inv_q) * inv_b - 0.5f + nz[0] * inv_b;
        o[1] = floorf((float)u.y * inv_q) * inv_b - 0.5f + nz[1] * inv_b;
        o[2] = floorf((float)u.z * inv_q) * inv_b - 0.5f + nz[2] * inv_b;
        o[3] = floorf((float)u.w * inv_q) * inv_b - 0.5f + nz[3] * inv_b;
        reinterpret_cast<floatx4*>(dst)[e] = o;
    }
}
}  // namespace bd

extern "C" {

const char* bd_last_error(void) { return bd::err_buf(); }
int bd_version(void) { return 3; }

size_t bd_packed_floats(int N, int K) { return (size_t)bd::cdiv(N, 16) * bd::cdiv(K, 16) * 256; }

int bd_pack_weights(const bd_pack_desc* descs, int n, void* stream) {
    const int n_prod = n > 0 ? n / BD_PACK_PRODUCTS : 0;
    n = n > 0 ? n % BD_PACK_PRODUCTS : n;
    BD_REQUIRE(descs != nullptr && n > 0 && n_prod <= n, "bd_pack_weights: no descriptors");
    hipLaunchKernelGGL(bd::pack_kernel, dim3((n - n_prod) * bd::kPackCopyX + n_prod * bd::kPackProdX), dim3(bd::kPackThreads),
                       n_prod > 0 ? sizeof(bd::PackLds) : 0, (hipStream_t)stream, descs, n - n_prod);
    BD_CHECK_LAUNCH("bd_pack_weights");
    return 0;
}

int bd_replay_gather(const float* src, const int64_t* idx, int n_idx, int width, float* dst, void* stream) {
    BD_REQUIRE(src && idx && dst && n_idx > 0 && width > 0, "bd_replay_gather: bad arguments");
    const size_t total = (size_t)n_idx * width;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(bd::gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, idx, n_idx, width, dst);
    BD_CHECK_LAUNCH("bd_replay_gather");
    return 0;
}

int bd_replay_gather_pixels(const unsigned char* src, const int64_t* idx, int n_idx, int pixels, int bit_depth,
                            const float* noise, float* dst, void* stream) {
    BD_REQUIRE(src && idx && noise && dst && n_idx > 0 && pixels > 0 && (pixels & 3) == 0 && bit_depth >= 1 && bit_depth <= 8,
               "bd_replay_gather_pixels: bad arguments");
    const size_t total = (size_t)n_idx * (pixels >> 2);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(bd::gather_pixels_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, idx, n_idx, pixels,
                       1.0f / (float)(1 << (8 - bit_depth)), 1.0f / (float)(1 << bit_depth), noise, dst, bd::Rng{0, 0, 0, 0});
    BD_CHECK_LAUNCH("bd_replay_gather_pixels");
    return 0;
}

int bd_replay_gather_pixels_rng(const unsigned char* src, const int64_t* idx, int n_idx, int pixels, int bit_depth,
                                unsigned long long seed, unsigned long long step, float* dst, void* stream) {
    BD_REQUIRE(src && idx && dst && n_idx > 0 && pixels > 0 && (pixels & 3) == 0 && bit_depth >= 1 && bit_depth <= 8,
               "bd_replay_gather_pixels_rng: bad arguments");
    const size_t total = (size_t)n_idx * (pixels >> 2);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(bd::gather_pixels_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, idx, n_idx, pixels,
                       1.0f / (float)(1 << (8 - bit_depth)), 1.0f / (float)(1 << bit_depth), nullptr, dst,
                       bd::Rng{(uint32_t)seed, (uint32_t)(seed >> 32), 6u, (uint32_t)step});
    BD_CHECK_LAUNCH("bd_replay_gather_pixels_rng");
    return 0;
}

}  // extern "C"
