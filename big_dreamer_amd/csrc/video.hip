// video.hip -- the evaluation loop's real-vs-predicted frame (src/main.py:237-253): one launch per decision assembles
// make_grid(cat([observation, observation_model(belief, posterior)], dim=3) + 0.5, nrow=5) as bytes
// (postprocess_observation(., 8), src/utils.py:320-337) into frame t of a device uint8 video buffer.
//
// The frame is walked as a flat array of 4-byte words: a lane decodes the (channel, row, column) of its first byte once,
// steps through the next three (a word may straddle a row end), looks each up -- grid padding, the observation (NCHW,
// as it was uploaded for the encoder) or the decoder's output (NHWC, where the conv stack leaves it) -- and writes the
// four bytes with ONE dword store.  Consecutive lanes write consecutive words, every byte of the frame exactly once;
// no LDS, no atomics.
//
// Open-loop prediction (Dreamer.open_loop, openloop.py; DreamerV1's image_summaries / DreamerV2's video_pred): bd_openl_video
// writes all T frames of truth over model over error in one launch by the same word walk, and bd_openl_error reduces
// (model - truth)^2 to one mean per step in a fixed order.
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

// ---- open-loop prediction (Dreamer.open_loop): T frames of n sequences, truth over model over error -------------------------
constexpr int kBands = 3;                        // truth | model | error, 64 rows each
constexpr int kTileWords = kImg / 4;             // a 64-pixel tile row is 16 words: a word never leaves it
constexpr int kPix = 3 * kImg * kImg;            // floats per image

// uint8(clip(floor(((m - t) + 1) * 0.5 * 256), 0, 255)), each operation rounded to fp32 on its own
__device__ __forceinline__ unsigned quantise_error(float m, float t) {
    const float e = __fmul_rn(__fadd_rn(__fsub_rn(m, t), 1.0f), 0.5f);
    const float q = floorf(__fmul_rn(e, 256.0f));
    return (unsigned)fminf(fmaxf(q, 0.0f), 255.0f);
}

// The video (T, 3, 192, 64 n) as a flat array of words, as eval_frame_kernel walks its frame: word w is 4 pixels of one tile
// row -- (t, channel, band, y, sequence k, x0) decoded once -- and is written with one dword store; every byte exactly once.
__global__ __launch_bounds__(256) void openl_video_kernel(const float* __restrict__ truth, const float* __restrict__ model,
                                                          int n, unsigned* __restrict__ video, int words) {
    const int rowWords = kTileWords * n;
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < words; w += gridDim.x * blockDim.x) {
        const int row = w / rowWords;                    // row of the (T * 3 * 192) x (64 n) byte matrix
        const int xw = w - row * rowWords;
        const int k = xw / kTileWords, x0 = 4 * (xw - k * kTileWords);
        const int tc = row / (kBands * kImg), r = row - tc * (kBands * kImg);
        const int t = tc / 3, c = tc - 3 * t;
        const int band = r / kImg, y = r - band * kImg;
        const size_t img = (size_t)t * n + k;
        const float* tp = truth + ((img * 3 + c) * kImg + y) * kImg + x0;            // NCHW: 4 consecutive floats
        const float* mp = model + ((img * kImg + y) * kImg + x0) * 3 + c;            // NHWC: stride 3
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = band == 0 ? quantise(tp[j]) : band == 1 ? quantise(mp[3 * j]) : quantise_error(mp[3 * j], tp[j]);
            packed |= b << (8 * j);
        }
        video[w] = packed;
    }
}

// out[t] = mean over the N = n * width elements of step t of (model - truth)^2.  One workgroup of 256 lanes per t; the order
// of additions is fixed:
//   1. lane l adds its terms i = l, l + 256, l + 512, ... (i: the element's index in the MODEL's layout) in that order into
//      one fp32 accumulator that starts at 0: acc = fma(d, d, acc), d = model[i] - truth[pair(i)] -- ceil(N / 256) additions;
//   2. a butterfly over the wave's 64 lanes (xor 32, 16, 8, 4, 2, 1: every lane ends with the same bits) -- 6 additions;
//   3. the four wave sums as (w0 + w1) + (w2 + w3) -- 2 additions;
// then one division by N.  The longest chain of additions is ceil(N / 256) + 8.  No atomics: two runs give the same bits.
// nhwc: model element (k, y, x, c) pairs with truth (k, c, y, x) of 3 x 64 x 64 images; otherwise pair(i) = i.
__global__ __launch_bounds__(256) void openl_error_kernel(const float* __restrict__ truth, const float* __restrict__ model,
                                                          int N, int nhwc, float* __restrict__ out) {
    __shared__ float red[4];
    const float* tp = truth + (size_t)blockIdx.x * N;
    const float* mp = model + (size_t)blockIdx.x * N;
    float acc = 0.0f;
#pragma unroll 4
    for (int i = threadIdx.x; i < N; i += 256) {
        int ti = i;
        if (nhwc) {
            const int k = i / kPix, rem = i - k * kPix;
            const int pix = rem / 3, c = rem - 3 * pix;
            ti = k * kPix + c * (kImg * kImg) + pix;
        }
        const float d = __fsub_rn(mp[i], tp[ti]);
        acc = __fmaf_rn(d, d, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = __fdiv_rn(__fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3])), (float)N);
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

int bd_openl_video(const float* truth, const float* model, int T, int n, unsigned char* video, void* stream) {
    BD_REQUIRE(truth && model && video, "bd_openl_video: null pointer");
    BD_REQUIRE(T >= 1 && n >= 1, "bd_openl_video: T and n must be at least 1 (got %d, %d)", T, n);
    BD_REQUIRE((reinterpret_cast<size_t>(video) & 3) == 0, "bd_openl_video: the video buffer must be 4-byte aligned");
    constexpr size_t kTileAll = 3 * kBands * kImg * kTileWords;           // words of one sequence's column block in one frame
    BD_REQUIRE((size_t)T * n <= (size_t)0x1FFFFFFF / kTileAll,
               "bd_openl_video: the words of %d frames of %d sequences do not fit an int", T, n);
    const size_t words = (size_t)T * n * kTileAll;
    const int blocks = (words + 255) / 256 < 2048 ? (int)((words + 255) / 256) : 2048;
    hipLaunchKernelGGL(openl_video_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, truth, model, n,
                       reinterpret_cast<unsigned*>(video), (int)words);
    BD_CHECK_LAUNCH("bd_openl_video");
    return 0;
}

int bd_openl_error(const float* truth, const float* model, int T, int n, int width, int model_nhwc, float* out, void* stream) {
    BD_REQUIRE(truth && model && out, "bd_openl_error: null pointer");
    BD_REQUIRE(T >= 1 && n >= 1 && width >= 1, "bd_openl_error: T, n and width must be at least 1 (got %d, %d, %d)", T, n, width);
    BD_REQUIRE(model_nhwc == 0 || model_nhwc == 1, "bd_openl_error: model_nhwc must be 0 or 1 (got %d)", model_nhwc);
    BD_REQUIRE(!model_nhwc || width == kPix, "bd_openl_error: an NHWC model holds 64 x 64 x 3 images, width %d (got %d)", kPix,
               width);
    BD_REQUIRE((size_t)n * width <= (size_t)0x3FFFFFFF, "bd_openl_error: %d x %d elements per step do not fit an int", n, width);
    hipLaunchKernelGGL(openl_error_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, truth, model, n * width, model_nhwc, out);
    BD_CHECK_LAUNCH("bd_openl_error");
    return 0;
}
