// replay.hip -- ExperienceReplay.append for n environments (src/memory.py:33-49): ONE launch writes n transitions --
// observation, action, reward, nonterminal -- into the rows `rows[i]` of the replay buffer's device mirror, reading the
// observation batch and the action where they already are on the device (the batch uploaded for the encoder, the acting
// step's output).  Pixel observations are quantised on the way (postprocess_observation, src/utils.py:320-337).
//
// The launch is a flat walk over n * (obs units + A + 2) units, transition-major: within a transition consecutive lanes
// take consecutive observation units (state: one float each; pixels: four floats with one 16-byte load, their four bytes
// with one dword store), then the A action floats, the reward and the nonterminal.  Memory bound: no LDS, no atomics,
// every destination element written at most once (the caller keeps the rows distinct).  A row outside [0, size) is
// skipped whole.
//
// ExperienceReplay.sample on the device (bd_replay_sample_gather, DESIGN.md "Device-side sampling"): ONE launch draws the
// n chunks of a batch and gathers them time-major -- no host RNG, no index upload.  Every workgroup first computes the n
// (lane base, start) pairs into LDS, one Philox4x32-10 call per sequence (stream 12, counter = (b, 0, 12, step)): the
// starts the reference's rejection loop (src/memory.py:51-68) accepts form one cyclic range of n_valid rows, so
// start = u (ring not full) or (head + u) mod R (full) with u = mulhi64(word, n_valid), and nothing is rejected.  The
// workgroup then walks its share of L*n * (obs units + A + 2) units, output-row-major: observation units (state: one
// float; pixels: one uchar4 load, four floats out, dequantised with the arithmetic and the Philox counter of
// gather_pixels_kernel<true> in cabi.hip, bit for bit), the A action floats, the reward (that lane also writes idx_out),
// the nonterminal.  Memory bound; 8 B * n of LDS, no atomics, no scratch, every destination element written once.
#include "bd_device.h"
#include "bd_host.h"
#include "bd_rng.h"

namespace bd {

// uint8(clip(floor((v + 0.5) * 2^bits) * 2^(8 - bits), 0, 255)), each operation rounded to fp32 on its own (no
// contraction): the arithmetic of ExperienceReplay.append on float32 input, bit for bit
__device__ __forceinline__ unsigned quantise_bits(float v, float up, float spread) {
    const float q = __fmul_rn(floorf(__fmul_rn(__fadd_rn(v, 0.5f), up)), spread);
    return (unsigned)fminf(fmaxf(q, 0.0f), 255.0f);
}

template <bool PIXELS>
__global__ __launch_bounds__(256) void replay_append_kernel(const bd_replay_append_args a, float up, float spread) {
    const int obs_units = PIXELS ? a.obs_width >> 2 : a.obs_width;
    const int per_row = obs_units + a.A + 2;
    const size_t total = (size_t)a.n * per_row;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / per_row);                  // transition of this call
        const int c = (int)(e - (size_t)i * per_row);      // unit inside it
        const int row = a.rows[i];
        if (row < 0 || row >= a.size) continue;            // guard: such a transition writes nothing
        if (c < obs_units) {
            if constexpr (PIXELS) {
                const floatx4 v = reinterpret_cast<const floatx4*>(a.obs + (size_t)i * a.obs_width)[c];
                const unsigned packed = quantise_bits(v[0], up, spread) | quantise_bits(v[1], up, spread) << 8 |
                                        quantise_bits(v[2], up, spread) << 16 | quantise_bits(v[3], up, spread) << 24;
                reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.dst_obs) + (size_t)row * a.obs_width)[c] = packed;
            } else {
                static_cast<float*>(a.dst_obs)[(size_t)row * a.obs_width + c] = a.obs[(size_t)i * a.obs_width + c];
            }
        } else if (c < obs_units + a.A) {
            const int k = c - obs_units;
            a.dst_act[(size_t)row * a.A + k] = a.act[(size_t)i * a.A + k];
        } else if (c == obs_units + a.A) {
            a.dst_reward[row] = a.reward[i];
        } else {
            a.dst_nonterminal[row] = a.nonterminal[i];
        }
    }
}

// mirror row of output row r = t * n + b: lane base + (start + t) mod R, from the (base, start) pairs in LDS
template <bool PIXELS>
__global__ __launch_bounds__(256) void replay_sample_gather_kernel(const bd_replay_sample_args a, int R,
                                                                   unsigned long long n_valid, float inv_q, float inv_b) {
    extern __shared__ int2 chunk[];                        // [n] (lane base, start)
    for (int b = threadIdx.x; b < a.n; b += blockDim.x) {
        const Philox4 x = philox4x32_10((uint32_t)b, 0u, 12u, (uint32_t)a.step, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const int lane = (int)__umulhi(x.x[0], (unsigned)a.lanes);
        const unsigned long long u = __umul64hi((unsigned long long)x.x[2] | (unsigned long long)x.x[3] << 32, n_valid);
        unsigned long long start = u;                      // u < n_valid <= R
        if (a.full) {
            start += (unsigned long long)a.idx;            // < 2 R
            if (start >= (unsigned long long)R) start -= (unsigned long long)R;
        }
        chunk[b] = make_int2(lane * R, (int)start);
    }
    __syncthreads();
    const int obs_units = PIXELS ? a.obs_width >> 2 : a.obs_width;
    const int per_row = obs_units + a.A + 2;
    const size_t total = (size_t)a.L * a.n * per_row;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / per_row);                  // output row t * n + b
        const int c = (int)(e - (size_t)r * per_row);      // unit inside it
        const int t = r / a.n;
        const int2 ch = chunk[r - t * a.n];
        unsigned local = (unsigned)ch.y + (unsigned)t;     // < 2 R <= 2^32 - 2
        if (local >= (unsigned)R) local -= (unsigned)R;
        const size_t row = (size_t)ch.x + local;           // < lanes * R <= size
        if (c < obs_units) {
            if constexpr (PIXELS) {
                const size_t q = (size_t)r * obs_units + c;        // the element quad of gather_pixels_kernel
                const uchar4 u = reinterpret_cast<const uchar4*>(static_cast<const unsigned char*>(a.obs) + row * a.obs_width)[c];
                const Philox4 p = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 6u, (uint32_t)a.pix_step, (uint32_t)a.pix_seed,
                                                (uint32_t)(a.pix_seed >> 32));
                floatx4 nz;
#pragma unroll
                for (int j = 0; j < 4; ++j) nz[j] = (float)(p.x[j] >> 8) * (1.0f / 16777216.0f);       // [0, 1) as rand_like
                floatx4 o;
                o[0] = floorf((float)u.x * inv_q) * inv_b - 0.5f + nz[0] * inv_b;
                o[1] = floorf((float)u.y * inv_q) * inv_b - 0.5f + nz[1] * inv_b;
                o[2] = floorf((float)u.z * inv_q) * inv_b - 0.5f + nz[2] * inv_b;
                o[3] = floorf((float)u.w * inv_q) * inv_b - 0.5f + nz[3] * inv_b;
                reinterpret_cast<floatx4*>(a.dst_obs)[q] = o;
            } else {
                a.dst_obs[(size_t)r * a.obs_width + c] = static_cast<const float*>(a.obs)[row * a.obs_width + c];
            }
        } else if (c < obs_units + a.A) {
            const int k = c - obs_units;
            a.dst_act[(size_t)r * a.A + k] = a.act[row * a.A + k];
        } else if (c == obs_units + a.A) {
            a.dst_reward[r] = a.reward[row];
            if (a.idx_out) a.idx_out[r] = (int64_t)row;
        } else {
            a.dst_nonterminal[r] = a.nonterminal[row];
        }
    }
}

}  // namespace bd

using namespace bd;

int bd_replay_append(const bd_replay_append_args* a, void* stream) {
    BD_REQUIRE(a != nullptr, "bd_replay_append: null argument struct");
    BD_REQUIRE(a->rows && a->obs && a->dst_obs && a->act && a->dst_act && a->reward && a->nonterminal && a->dst_reward &&
                   a->dst_nonterminal, "bd_replay_append: null pointer");
    BD_REQUIRE(a->n >= 1 && a->n <= 4096, "bd_replay_append: n must be in [1, 4096] (got %d)", a->n);
    BD_REQUIRE(a->size > 0, "bd_replay_append: the mirror has %d rows", a->size);
    BD_REQUIRE(a->A > 0, "bd_replay_append: action width %d", a->A);
    BD_REQUIRE(a->obs_width > 0, "bd_replay_append: observation width %d", a->obs_width);
    BD_REQUIRE(a->bit_depth >= 0 && a->bit_depth <= 8, "bd_replay_append: bit_depth must be in [0, 8] (got %d)", a->bit_depth);
    BD_REQUIRE((size_t)a->obs_width + (size_t)a->A + 2 <= (size_t)0x7FFFFFFF, "bd_replay_append: a transition of %d + %d floats",
               a->obs_width, a->A);
    const bool pixels = a->bit_depth > 0;
    if (pixels) {
        BD_REQUIRE(a->obs_width % 4 == 0, "bd_replay_append: pixel rows are whole 4-byte words (obs_width %d)", a->obs_width);
        BD_REQUIRE((reinterpret_cast<size_t>(a->obs) & 15) == 0, "bd_replay_append: pixel obs must be 16-byte aligned");
        BD_REQUIRE((reinterpret_cast<size_t>(a->dst_obs) & 3) == 0, "bd_replay_append: pixel dst_obs must be 4-byte aligned");
    }
    const size_t total = (size_t)a->n * ((pixels ? a->obs_width / 4 : a->obs_width) + (size_t)a->A + 2);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    const float up = (float)(1 << a->bit_depth), spread = (float)(1 << (8 - a->bit_depth));
    if (pixels)
        hipLaunchKernelGGL(replay_append_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, up, spread);
    else
        hipLaunchKernelGGL(replay_append_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, up, spread);
    BD_CHECK_LAUNCH("bd_replay_append");
    return 0;
}

int bd_replay_sample_gather(const bd_replay_sample_args* a, void* stream) {
    BD_REQUIRE(a != nullptr, "bd_replay_sample_gather: null argument struct");
    BD_REQUIRE(a->obs && a->act && a->reward && a->nonterminal && a->dst_obs && a->dst_act && a->dst_reward &&
                   a->dst_nonterminal, "bd_replay_sample_gather: null pointer");
    BD_REQUIRE(a->n >= 1 && a->n <= 4096, "bd_replay_sample_gather: n must be in [1, 4096] (got %d)", a->n);
    BD_REQUIRE(a->L >= 1, "bd_replay_sample_gather: chunk length L must be at least 1 (got %d)", a->L);
    BD_REQUIRE(a->size > 0 && a->lanes >= 1 && a->lane_size >= 1, "bd_replay_sample_gather: a mirror of %d rows in %d lanes of %d",
               a->size, a->lanes, a->lane_size);
    BD_REQUIRE((long long)a->lanes * a->lane_size <= (long long)a->size,
               "bd_replay_sample_gather: lanes * lane_size = %d * %d exceeds size %d", a->lanes, a->lane_size, a->size);
    BD_REQUIRE(a->A > 0, "bd_replay_sample_gather: action width %d", a->A);
    BD_REQUIRE(a->obs_width > 0, "bd_replay_sample_gather: observation width %d", a->obs_width);
    BD_REQUIRE((size_t)a->obs_width + (size_t)a->A + 2 <= (size_t)0x7FFFFFFF, "bd_replay_sample_gather: a transition of %d + %d floats",
               a->obs_width, a->A);
    const int R = a->lanes == 1 ? a->size : a->lane_size;      // the ring a chunk lives in
    BD_REQUIRE(a->L <= R, "bd_replay_sample_gather: a chunk of L = %d does not fit a ring of %d rows", a->L, R);
    BD_REQUIRE(a->idx >= 0 && a->idx < R, "bd_replay_sample_gather: idx must be in [0, %d) (got %d)", R, a->idx);
    BD_REQUIRE(a->full || a->idx > a->L, "bd_replay_sample_gather: the ring is not full and holds idx = %d rows, a chunk of L = %d "
               "needs more", a->idx, a->L);
    BD_REQUIRE((size_t)a->L * (size_t)a->n <= (size_t)0x7FFFFFFF, "bd_replay_sample_gather: L * n = %d * %d output rows", a->L, a->n);
    BD_REQUIRE(a->bit_depth >= 0 && a->bit_depth <= 8, "bd_replay_sample_gather: bit_depth must be in [0, 8] (got %d)", a->bit_depth);
    const bool pixels = a->bit_depth > 0;
    if (pixels) {
        BD_REQUIRE(a->obs_width % 4 == 0, "bd_replay_sample_gather: pixel rows are whole 4-byte words (obs_width %d)", a->obs_width);
        BD_REQUIRE((reinterpret_cast<size_t>(a->obs) & 3) == 0, "bd_replay_sample_gather: pixel obs must be 4-byte aligned");
        BD_REQUIRE((reinterpret_cast<size_t>(a->dst_obs) & 15) == 0, "bd_replay_sample_gather: pixel dst_obs must be 16-byte aligned");
    }
    const unsigned long long n_valid = a->full ? (unsigned long long)(R - a->L + 1) : (unsigned long long)(a->idx - a->L);
    const size_t total = (size_t)a->L * a->n * ((pixels ? a->obs_width / 4 : a->obs_width) + (size_t)a->A + 2);
    const size_t cap = pixels ? 4096 : 2048;
    const int blocks = (int)((total + 255) / 256 < cap ? (total + 255) / 256 : cap);
    const size_t lds = sizeof(int2) * (size_t)a->n;
    const float inv_q = 1.0f / (float)(1 << (8 - a->bit_depth)), inv_b = 1.0f / (float)(1 << a->bit_depth);
    if (pixels)
        hipLaunchKernelGGL(replay_sample_gather_kernel<true>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, *a, R, n_valid,
                           inv_q, inv_b);
    else
        hipLaunchKernelGGL(replay_sample_gather_kernel<false>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, *a, R, n_valid,
                           inv_q, inv_b);
    BD_CHECK_LAUNCH("bd_replay_sample_gather");
    return 0;
}
