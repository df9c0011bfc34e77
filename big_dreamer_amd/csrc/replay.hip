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
#include "bd_device.h"
#include "bd_host.h"

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
