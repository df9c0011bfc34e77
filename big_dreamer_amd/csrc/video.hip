// video.hip -- the evaluation loop's real-vs-predicted frame (src/main.py:237-253): one launch per decision assembles
// make_grid(cat([observation, observation_model(belief, posterior)], dim=3) + 0.5, nrow=5) as bytes
// (postprocess_observation(., 8), src/utils.py:320-337) into frame t of a device uint8 video buffer.
//
// The frame is walked as a flat array of 4-byte words: a lane decodes the (channel, row, column) of its first byte once,
// steps through the next three (a word may straddle a row end), looks each up -- grid padding, the observation (NCHW,
// as it was uploaded for the encoder) or the decoder's output (NHWC, where the conv stack leaves it) -- and writes the
// four bytes with ONE dword store.  Consecutive lanes write consecutive words, every byte of the frame exactly once;
// no LDS, no atomics.
#include "bd_host.h"

namespace bd {

constexpr int kImg = 64;               // observations are 3 x 64 x 64
constexpr int kTileW = 2 * kImg;       // real | predicted
constexpr int kPad = 2;                // make_grid's padding
constexpr int kGridCols = 5;           // nrow=5: tiles per grid row

struct FrameGeo {
    int xmaps, ymaps, GH, GW, pad;
    __host__ __device__ explicit FrameGeo(int n) {
        if (n == 1) {                  // make_grid returns a single image as it is
            xmaps = ymaps = 1; pad = 0; GH = kImg; GW = kTileW;
        } else {
            xmaps = n < kGridCols ? n : kGridCols;
            ymaps = (n + xmaps - 1) / xmaps;
            pad = kPad;
            GH = ymaps * (kImg + kPad) + kPad;
            GW = xmaps * (kTileW + kPad) + kPad;
        }
    }
};

// uint8(clip(floor((v + 0.5) * 256), 0, 255)), each operation rounded to fp32 on its own (no contraction)
__device__ __forceinline__ unsigned quantise(float v) {
    const float q = floorf(__fmul_rn(__fadd_rn(v, 0.5f), 256.0f));
    return (unsigned)fminf(fmaxf(q, 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void eval_frame_kernel(const float* __restrict__ obs, const float* __restrict__ dec, int n,
                                                         unsigned* __restrict__ frame, int words) {
    const FrameGeo g(n);
    const int cellH = kImg + g.pad, cellW = kTileW + g.pad;
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < words; w += gridDim.x * blockDim.x) {
        const int first = 4 * w;
        int row = first / g.GW;                  // row of the (3 * GH) x GW byte matrix
        int x = first - row * g.GW;
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = row / g.GH, y = row - c * g.GH;
            unsigned b = 0;
            const int ty = y / cellH, iy = y - ty * cellH - g.pad;       // tile row of the grid, row inside the tile
            const int tx = x / cellW, ix = x - tx * cellW - g.pad;
            const int k = ty * g.xmaps + tx;
            if (iy >= 0 && ix >= 0 && ty < g.ymaps && tx < g.xmaps && k < n) {
                const float v = ix < kImg ? obs[(((size_t)k * 3 + c) * kImg + iy) * kImg + ix]
                                          : dec[(((size_t)k * kImg + iy) * kImg + (ix - kImg)) * 3 + c];
                b = quantise(v);
            }
            packed |= b << (8 * j);
            if (++x == g.GW) { x = 0; ++row; }
        }
        frame[w] = packed;
    }
}

}  // namespace bd

using namespace bd;

int bd_eval_frame(const float* obs, const float* dec, int n, unsigned char* video, int frames, int t, void* stream) {
    BD_REQUIRE(obs && dec && video, "bd_eval_frame: null pointer");
    BD_REQUIRE(n > 0 && n <= 4096, "bd_eval_frame: n must be in [1, 4096] (got %d)", n);
    BD_REQUIRE(frames > 0 && t >= 0 && t < frames, "bd_eval_frame: frame %d outside the buffer's %d", t, frames);
    const FrameGeo g(n);
    const size_t bytes = (size_t)3 * g.GH * g.GW;          // GH and GW are even: whole words
    BD_REQUIRE((reinterpret_cast<size_t>(video) & 3) == 0, "bd_eval_frame: the video buffer must be 4-byte aligned");
    BD_REQUIRE(bytes % 4 == 0 && bytes / 4 <= (size_t)0x1FFFFFFF, "bd_eval_frame: frame of %zu bytes", bytes);
    const int words = (int)(bytes / 4);
    const int blocks = (words + 255) / 256 < 2048 ? (words + 255) / 256 : 2048;
    hipLaunchKernelGGL(eval_frame_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, obs, dec, n,
                       reinterpret_cast<unsigned*>(video + (size_t)t * bytes), words);
    BD_CHECK_LAUNCH("bd_eval_frame");
    return 0;
}
