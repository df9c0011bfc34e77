/*
 * bigdreamer_hip.h -- C ABI of the MI355X-native Dreamer world-model training step.
 *
 * The reference (jgsimard/big-dreamer) has no FFI / plugin interface: its hot path is a chain of
 * ATen ops issued from Python.  This library is what a binding for that path
 * binds instead; each entry point names the reference code it replaces.  The Python host in
 * big_dreamer_amd/ (ctypes) mirrors the reference's own call surface on top of it
 * (TransitionModel.forward, Dreamer.imagine_ahead, lambda_return, Dreamer.train_step ...).
 *
 * Conventions
 *   - plain C, no torch types: raw device pointers (fp32 unless said otherwise), explicit sizes,
 *     hipStream_t passed as void*;
 *   - nothing allocates, frees or synchronises: every buffer (inputs, outputs, saved activations,
 *     workspaces) is caller-owned device memory, every launch is asynchronous on `stream`;
 *   - return value 0 = launched, negative = rejected (bd_last_error() has the text); never throws;
 *   - tensors are contiguous row-major "rows x features" with an explicit leading dimension where one
 *     is given; time-major (time, batch, feature) arrays are passed flattened to rows = time*batch;
 *   - re-entrant per device: one host thread per GPU (one process per rank).
 *
 * Weight layout.  Kernels read weights in a packed MFMA-fragment layout produced by
 * bd_pack_weights() from the PyTorch (out, in) row-major tensors: for W[N][K],
 *   packed[nb][kb][lane][i] = W[nb*16 + (lane&15)][kb*16 + 4*(lane>>4) + i]   (zero padded),
 * i.e. one coalesced 1 KiB read per 16x16 block feeds four v_mfma_f32_16x16x4_f32.
 */
#ifndef BIGDREAMER_HIP_H
#define BIGDREAMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BD_MAX_LAYERS 6
#define BD_ACT_NONE 0
#define BD_ACT_ELU 1
#define BD_ACT_ELU_GRAD 2   /* conv entry points only: out = value * ELU'(aux), aux = the SAVED ELU output at the same
                            * index as out (the dgrad of a layer and the ELU backward of the layer below in one pass) */
/* cnn_activation_function of the pixel stacks: the conv entry points, bd_act_backward and the dense chains (bd_layer.act /
 * bd_layer_bwd.act, forward codes only) take these too; the scans, heads and planners are ELU throughout.  A _GRAD code is
 * its forward code + 1 and takes f' from the saved OUTPUT y:  ELU' = y > 0 ? 1 : y + 1,  ReLU' = y > 0 ? 1 : 0,
 * Tanh' = 1 - y^2.  Any other value is rejected by every entry point. */
#define BD_ACT_RELU 3
#define BD_ACT_RELU_GRAD 4
#define BD_ACT_TANH 5
#define BD_ACT_TANH_GRAD 6

const char* bd_last_error(void);
int bd_version(void);

/* ---- weight packing ------------------------------------------------------------------------- */
#define BD_PACK_COPY 0       /* dst = packed src (or its transpose)                                                    */
#define BD_PACK_PRODUCT 1    /* dst = packed A.B (or its transpose): A = src [N x E] (ld), B = src2 [E x K] (ld2)       */
#define BD_PACK_PRODUCT_VEC 2 /* dst[n] = sum_e A[n][e] b[e], plain floats: A = src [N x E] (ld), b = src2 [E]; K unused */
typedef struct {
    const float* src; /* PyTorch-layout matrix, element (n,k) at src[n*ld + k]                  */
    float* dst;       /* packed destination, bd_packed_floats(N,K) floats (transposed: (K,N))    */
    int ld;           /* leading dimension of src                                                 */
    int N, K;         /* logical sub-block to pack (rows n < N, cols k < K of src)                */
    int transpose;    /* 0: pack W (out=N,in=K); 1: pack W^T (out=K,in=N) for the dgrad kernels  */
    /* Product kinds (kind = 0 and the fields below zero: a plain copy, as before).  Two linear layers with nothing
     * between them are one layer: the pack launch forms the composed weight from the two SOURCE matrices (never from
     * another packed output, so the descriptors of one launch stay independent).  Every dot product is summed in a fixed
     * order (four contiguous quarters of e, each in ascending e, added in quarter order; the vector kind: 64 strided
     * partial sums combined by a fixed butterfly), no atomics.  A product is ~E times the work of a copy, with a grid and
     * an LDS allocation of its own: product descriptors close the table and the caller says how many there are,
     * n = descriptors + BD_PACK_PRODUCTS * (trailing product descriptors).  (A product descriptor that is not counted is
     * treated as a copy of src.) */
    int kind;         /* BD_PACK_*                                                                */
    const float* src2;/* B (element (e,k) at src2[e*ld2 + k]) or b                                */
    int ld2;
    int E;            /* contraction length                                                       */
} bd_pack_desc;

size_t bd_packed_floats(int N, int K);
/* descs: DEVICE array of n descriptors (the table lives on the device, so the count of trailing product descriptors,
 * which take a grid of their own size, rides on n: see bd_pack_desc). */
#define BD_PACK_PRODUCTS 65536
int bd_pack_weights(const bd_pack_desc* descs, int n, void* stream);

/* ---- dense chains: DenseModel / build_mlp (src/models.py:365-408, src/utils.py:368-404) ------ */
typedef struct {
    const float* w;    /* packed weights (out=N, in=K)                                            */
    const float* bias; /* [N] or NULL                                                             */
    int N, K;
    int act;           /* BD_ACT_*: applied to this layer's output                                */
    float* save;       /* optional [M x N] post-activation output kept for the backward, or NULL  */
} bd_layer;

typedef struct {
    int M;                          /* rows                                                       */
    const float* in0; int ld0, w0;  /* input = [in0 | in1] (torch.cat(..., dim=-1)); in1 optional  */
    const float* in1; int ld1, w1;
    int n_layers;
    bd_layer layer[BD_MAX_LAYERS];
    float* out; int ldo;            /* last layer's output [M x N_last]                            */
    /* Optional one-hot (Categorical) input segment BESIDE [in0 | in1]: gD factors of gC classes given as class indices
     * gidx [M x gD] (uint8).  Layer 0 then computes  act(W0 [in0 | in1] + sum_f gWT[f*gC + gidx[m][f]] + b)  with
     * gWT the plain row-major TRANSPOSE [gD*gC x N0] of the layer's one-hot columns: a gather of gD rows instead of a
     * K = gD*gC contraction (DenseModel(belief, state) on [h; one-hot s]).  gD = 0: absent. */
    const unsigned char* gidx; const float* gWT; int gD, gC;
} bd_mlp_fwd_args;
int bd_mlp_forward(const bd_mlp_fwd_args* a, void* stream);

typedef struct {
    const float* wt;   /* packed W^T (out=K, in=N) -- unused for layer 0 unless din requested      */
    const float* saved;/* this layer's saved post-activation output [M x N] (needed iff act!=NONE) */
    int N, K;
    int act;
    float* dpre;       /* optional [M x N] gradient w.r.t. the pre-activation (for bd_wgrad)        */
} bd_layer_bwd;

typedef struct {
    int M;
    const float* dout; int lddo;    /* gradient w.r.t. the last layer's output [M x N_last]        */
    float dout_scale;               /* multiplies dout on load (1.0f for none)                     */
    int n_layers;
    bd_layer_bwd layer[BD_MAX_LAYERS];
    float* din0; int ld0, w0;       /* optional gradient w.r.t. the input, split like the forward   */
    float* din1; int ld1, w1;
    int accumulate;                 /* 1: din += , 0: din =                                         */
} bd_mlp_bwd_args;
int bd_mlp_backward(const bd_mlp_bwd_args* a, void* stream);

/* Tall form of the two chain entry points (csrc/mlp.hip, mlp_*_tall_kernel): for M >= 8192 rows and layer widths of at
 * most 15 column blocks, 48-row workgroups with one in-place LDS image and (row tile, column block) pairs balanced over
 * the four waves, accumulators in the transposed (row x 4 consecutive columns) form; layer widths must be multiples of
 * 4 floats and saved / dpre buffers 16-byte aligned, otherwise the 16-row form runs.  Same arguments, same results
 * (summation order within a dot product is unchanged).  mode 1: on (the default), 0: always the 16/32-row form,
 * 2: on for every M (diagnostics), -1: as the environment says (BD_MLP_TALL=0 switches it off). */
int bd_mlp_set_tall(int mode);

/* dW[N x K] (+)= dpre^T[N x M] * act[M x K],  db[N] (+)= column sums of dpre (db may be NULL).
 * Deterministic split-M (slabs in `ws`, then a fixed-order reduction); accumulate=1 adds to dW/db;
 * ws must hold bd_wgrad_ws_floats(M,N,K) floats (its capacity ws_floats is checked).
 * (What autograd's AddmmBackward computes for every nn.Linear on the path.) */
size_t bd_wgrad_ws_floats(int M, int N, int K);
int bd_wgrad(const float* dpre, int ldp, const float* act, int lda, int M, int N, int K,
             float* dW, int ldw, float* db, int accumulate, float* ws, size_t ws_floats, void* stream);

/* Grouped form: every weight-gradient GEMM of one backward pass in ONE launch (+ one grouped reduce).  Fill the
 * caller fields of each descriptor on the host, let bd_wgrad_plan add the launch plan (and tell the slab workspace
 * size), copy the table to device memory once, then call bd_wgrad_grouped every step.  Rows [0, M1) take their
 * activations from act1, rows [M1, M) from act2[row - M1] (set M1 = M and act2 = NULL for a single source).
 * The slab workspace `ws` must be 16-byte aligned (slab rows are written and read as float4s). */
typedef struct {
    const float* dpre; int ldp;               /* [M x N] pre-activation gradients                            */
    const float* act1; int lda1; int M1;
    const float* act2; int lda2;
    int M, N, K;
    float* dW; int ldw;                        /* [N x K] output                                              */
    float* db;                                 /* [N] or NULL                                                 */
    /* filled by bd_wgrad_plan */
    int splits, rows_per, tiles_n, tiles_k, block_begin, red_begin;
    unsigned long long ws_off;
    /* optional gathered `act` (conv weight gradients, pattern F of bd_conv_gemm): when g_nseg > 0, row m = (img, y, x)
     * over g_gh x g_gw per image takes act(m, k) = act1[((img*g_IH + 2y + s)*g_IW + 2x)*g_C + off], s = k / g_seglen,
     * off = k % g_seglen (K = g_nseg * g_seglen; lda1 / act2 unused, M1 = M). */
    int g_nseg, g_seglen, g_gh, g_gw, g_IH, g_IW, g_C, g_pad;
    /* Chain records (kind = BD_WGRAD_CHAIN; they follow every GEMM descriptor of the table).  Where the forward ran a
     * composed layer Wc = A.B, bc = A.b (BD_PACK_PRODUCT: A [N x E], B [E x K], b [E]) a GEMM descriptor of the same table
     * leaves dWc [N x K] and dbc [N] in scratch; the chain record names that result as its (dW, ldw, db) and the call
     * finishes the job after the reduce, in one more launch (fixed summation order, no atomics):
     *   c_dA[n][e] = sum_k dWc[n][k] B[e][k] + dbc[n] b[e],   c_dB[e][k] = sum_n A[n][e] dWc[n][k],
     *   c_db[e]    = sum_n A[n][e] dbc[n].
     * Only the E columns of c_dA named here are written.  dpre / act1 / M are unused in a chain record. */
    int kind;                                  /* BD_WGRAD_GEMM (0) | BD_WGRAD_CHAIN                            */
    int c_E;
    const float* c_A; int c_lda;
    const float* c_B; int c_ldb;
    const float* c_b;
    float* c_dA; int c_ldda;
    float* c_dB; int c_lddb;
    float* c_db;
} bd_wgrad_desc;
#define BD_WGRAD_GEMM 0
#define BD_WGRAD_CHAIN 1
/* total_red_blocks is an opaque plan word (reduce workgroups, and the number of chain records above bit 24): pass it on
 * as bd_wgrad_plan returned it. */
int bd_wgrad_plan(bd_wgrad_desc* descs_host, int n, int* total_blocks, int* total_red_blocks, size_t* ws_floats);
int bd_wgrad_grouped(const bd_wgrad_desc* descs_dev, int n, int total_blocks, int total_red_blocks, float* ws,
                     void* stream);
/* The two launches of bd_wgrad_grouped separately (phase 1: the slab GEMM kernel; phase 2: the fixed-order reduce), so
 * that a benchmark can bracket the GEMM kernel alone with HIP events.  phase 0 = both = bd_wgrad_grouped.  The chain
 * records' launch belongs to phase 2. */
int bd_wgrad_grouped_phase(const bd_wgrad_desc* descs_dev, int n, int total_blocks, int total_red_blocks, float* ws,
                           int phase, void* stream);

/* ---- conv stacks of the pixel configurations (CnnImageEncoder src/models.py:527-564, ObservationModel
 * src/models.py:319-362; F.conv2d / F.conv_transpose2d and their autograd backward) as gather-GEMMs on NHWC images:
 *   out[m][n] = act( sum_k A(m, k) W[n][k] + bias[n] ),  m = (img, y, x) over an imgs x gh x gw row grid,
 *   A(m, k): s = k / seglen, off = k % seglen;  iy = y*sy + y0 + s*ss;  ix0 = x*sx + x0;
 *            value = in[((img*IH + iy)*IW + ix0)*C + off]   (0 outside the image when mask = 1),
 *   out row of m: out + ((img*OH + y*osy + oy0)*OW + x*osx + ox0)*ldo.
 * Pattern F (stride-2 VALID conv forward, transposed-conv dgrad): nseg = k, seglen = k*C, sy = sx = 2, ss = 1, dense output.
 * Pattern T (one parity class (py,px) of a stride-2 transposed conv forward / conv dgrad): nseg = Ta, seglen = Tb*C,
 *   sy = sx = 1, ss = -1, x0 = -(Tb-1), mask = 1, osy = osx = 2, oy0 = py, ox0 = px; weights from bd_conv_pack_class. */
typedef struct {
    const float* in; float* out;
    const float* w;       /* packed (bd_pack_weights / bd_conv_pack_class): out = N, in = K                 */
    const float* bias;    /* [N] or NULL                                                                   */
    int imgs, gh, gw, N, K;
    int nseg, seglen, C, IH, IW, sy, y0, ss, sx, x0, mask, cshift, vec4;
    int OH, OW, osy, oy0, osx, ox0, ldo;
    int act;              /* BD_ACT_*                                                                      */
    int fuse_cq;          /* pattern T with its four parity classes fused: N = 4*fuse_cq columns, column n = cls*fuse_cq
                           * + c goes to pixel (2y + (cls>>1), 2x + (cls&1)), channel c (osy = osx = 2, oy0 = ox0 = 0;
                           * gh x gw = the class-(0,0) grid; bias indexed by c); 0 = one class per call                */
    const float* aux;     /* BD_ACT_*_GRAD: saved outputs, same layout as `out`; else unused                           */
} bd_conv_args;
int bd_conv_gemm(const bd_conv_args* a, void* stream);
/* Stride-2 VALID convolution of a THIN image (C <= 4 channels) into 32 channels, NHWC: out (imgs, OH, OW, 32) =
 * act(conv(in (imgs, IH, IW, C), W) + bias), W plain row-major [32][(ky, kx, c)] with row stride ldw (the stored parameter
 * as it lies in the buffer; bias may be NULL).  Conv2d(3 -> 32, k4) forward (src/models.py:538) and the dgrad of
 * ConvTranspose2d(32 -> 3, k6) (src/models.py:347).  k*k*C <= 108, OW <= 32. */
int bd_conv_thin_forward(const float* in, int imgs, int IH, int IW, int C, int k, const float* W, int ldw, const float* bias,
                         int act, const float* aux, float* out, void* stream);   /* aux: BD_ACT_*_GRAD only (else NULL) */
/* dst (packed) [n = inner][k = (a, b', outer)] = src[outer][py+2a][px+2(Tb-1-b')][inner], src stored (outer, ky, kx, inner) */
int bd_conv_pack_class(const float* src, float* dst, int Couter, int Cinner, int ksz, int py, int px, int Ta, int Tb,
                       void* stream);
/* all four parity classes at once (bd_conv_args.fuse_cq): dst [n = cls*Cinner + c][k = (a, b', outer)], T x T taps with
 * T = (ksz+1)/2, zero where the tap falls outside the kernel (odd ksz, parity 1) */
int bd_conv_pack_fused(const float* src, float* dst, int Couter, int Cinner, int ksz, void* stream);
/* g *= f'(y) in place from the saved outputs y of activation `act` (a forward code BD_ACT_ELU / _RELU / _TANH or its
 * _GRAD code; n a multiple of 4): the standalone form of the _GRAD epilogues */
int bd_act_backward(float* g, const float* y, size_t n, int act, void* stream);
/* bd_act_backward(g, y, n, BD_ACT_ELU, stream) */
int bd_elu_backward(float* g, const float* y, size_t n, void* stream);
/* out[n] = sum_m rows[m][n] of an [M x N] row-major matrix, N <= 256 (bias gradient of a transposed-conv layer);
 * ws: bd_colsum_ws_floats(N) floats; fixed summation order */
size_t bd_colsum_ws_floats(int N);
int bd_colsum(const float* rows, size_t M, int N, float* out, float* ws, void* stream);
/* (imgs, C, HW) -> (imgs, HW, C) when to_nhwc, the reverse otherwise */
int bd_image_layout(const float* src, float* dst, int imgs, int C, int HW, int to_nhwc, void* stream);
/* Evaluation video (src/main.py:237-253): frame t of `video`, a device uint8 buffer of `frames` frames (3, GH, GW), 4-byte
 * aligned = make_grid(cat([obs, prediction], dim=3) + 0.5, nrow=5) as bytes, one launch.
 *   obs (n, 3, 64, 64) NCHW fp32: the observations the decision consumed, as uploaded for the encoder;
 *   dec (n, 64, 64, 3) NHWC fp32: the decoder's output where the conv stack leaves it (no layout pass in between).
 * A tile is 3 x 64 x 128 (real in columns 0-63, predicted in 64-127).  n == 1: the frame is the tile (GH = 64, GW = 128).
 * Otherwise xmaps = min(5, n), ymaps = ceil(n / xmaps), GH = 66 ymaps + 2, GW = 130 xmaps + 2, tile k starts at row
 * (k / xmaps) 66 + 2, column (k % xmaps) 130 + 2, and every other byte is 0.  A pixel is
 * uint8(clip(floor((v + 0.5) * 256), 0, 255)) in fp32 arithmetic (postprocess_observation(., 8), src/utils.py:320-337).
 * Every byte of the frame is written, padding included (the buffer needs no clearing); no other frame is touched.
 * n <= 4096, 0 <= t < frames. */
int bd_eval_frame(const float* obs, const float* dec, int n, unsigned char* video, int frames, int t, void* stream);
/* Open-loop prediction video (DreamerV1 image_summaries / DreamerV2 video_pred; Dreamer.open_loop): the whole device uint8
 * video (T, 3, 192, 64 n), 4-byte aligned, in one launch.  Frame t, columns 64 k .. 64 k + 63 hold sequence k: rows 0-63 the
 * truth, 64-127 the model's image, 128-191 their difference; no padding.
 *   truth (T n, 3, 64, 64) NCHW fp32: the batch's observations obs[1:], as the replay gathered them;
 *   model (T n, 64, 64, 3) NHWC fp32: the decoder's output where the conv stack leaves it; row t n + k is step t of sequence k.
 * Truth and model bytes are bd_eval_frame's uint8(clip(floor((v + 0.5) * 256), 0, 255)); an error byte is
 * uint8(clip(floor(e * 256), 0, 255)) with e = ((model - truth) + 1) * 0.5; every operation rounded to fp32 on its own.
 * Every byte is written exactly once.  T, n >= 1, T n 9216 words must fit an int. */
int bd_openl_video(const float* truth, const float* model, int T, int n, unsigned char* video, void* stream);
/* Open-loop error curve: out[t] = mean over the n * width elements of step t of (model - truth)^2, fp32; truth and model are
 * [T n x width] with row t n + k = step t of sequence k.  model_nhwc = 1 (width must be 12288): model is the decoder's NHWC
 * buffer and its element (k, y, x, c) pairs with truth (k, c, y, x); 0: element by element (the state observations' dense
 * decoder).  Deterministic: one workgroup per t, per-lane strided partial sums, then a fixed tree (no atomics); the longest
 * chain of additions is ceil(n width / 256) + 8.  n * width < 2^30. */
int bd_openl_error(const float* truth, const float* model, int T, int n, int width, int model_nhwc, float* out, void* stream);

/* ---- RSSM observe scan: TransitionModel.forward with embeddings (src/models.py:191-299) ------
 * One persistent launch walks all T steps; a workgroup owns 16 batch rows (rows are independent, so
 * there is no inter-workgroup synchronisation).  The prior head (src/models.py:256) does not feed the
 * recurrence when embeddings are given, so the host runs it batched over all T*B rows afterwards
 * (bd_mlp_forward + bd_gauss_head_forward).  The embedding half of the posterior's first layer is
 * hoisted out of the loop: pre_emb = embeddings @ W_q1[:, Be:]^T. */
typedef struct {
    int T, B, Be, S, A, Hd;
    /* packed weights */
    const float* w_embed_s; const float* w_embed_a; const float* b_embed; /* fc_embed_state_action.0[:, :S] / [:, S:] */
    const float* w_ir; const float* w_iz; const float* w_in;   /* rnn.weight_ih rows r,z,n (Be,Be) */
    const float* w_hr; const float* w_hz; const float* w_hn;   /* rnn.weight_hh rows r,z,n (Be,Be) */
    const float* b_ih; const float* b_hh;                       /* [3*Be] each                      */
    const float* w_q1h; const float* b_q1;         /* belief_posterior.model.0[:, :Be]: (Hd, Be)   */
    const float* w_q2m; const float* w_q2s;        /* belief_posterior.model.2 rows [0,S) / [S,2S) */
    const float* b_q2;                             /* [2*S]                                        */
    /* inputs */
    const float* init_belief;  /* [B x Be]                                                        */
    const float* init_state;   /* [B x S]                                                         */
    const float* actions;      /* [T x B x A]                                                     */
    const float* nonterm;      /* [T x B] or NULL (nonterminals=None, src/models.py:247)          */
    const float* pre_emb;      /* [T x B x Hd] hoisted embedding projection (no bias)              */
    const float* eps_post;     /* [T x B x S] standard normal                                     */
    float min_std;             /* 0.1                                                             */
    /* outputs */
    float* feat;      /* [T x B x (Be+S)]: [belief_{t+1} | posterior_state_{t+1}]                  */
    float* post_mean; /* [T x B x S]                                                              */
    float* post_std;  /* [T x B x S]                                                              */
    /* saved for the backward (all NULL for inference) */
    float* sv_s;      /* [T x B x S]  masked previous state (input of the embed layer)             */
    float* sv_x;      /* [T x B x Be] embed output                                                 */
    float* sv_gates;  /* [T x B x 4*Be]: r, z, n, (W_hn h + b_hn)                                  */
    float* sv_q;      /* [T x B x Hd] posterior hidden (post-ELU)                                  */
} bd_observe_fwd_args;
int bd_observe_forward(const bd_observe_fwd_args* a, void* stream);

typedef struct {
    int T, B, Be, S, A, Hd;
    /* transposed packed weights */
    const float* wt_embed_s;                                 /* (S, Be)                            */
    const float* wt_ir; const float* wt_iz; const float* wt_in;
    const float* wt_hr; const float* wt_hz; const float* wt_hn;
    const float* wt_q1h;                                     /* (Be, Hd)                           */
    const float* wt_q2m; const float* wt_q2s;                /* (Hd, S) each                        */
    /* forward inputs / saved */
    const float* init_belief; const float* nonterm; const float* eps_post;
    const float* feat; const float* post_std;
    const float* sv_x; const float* sv_gates; const float* sv_q;
    /* incoming gradients */
    const float* dfeat;      /* [T x B x (Be+S)] from the obs/reward heads (+ prior head on the belief part) */
    const float* dpost_mean; /* [T x B x S] from the KL term (or NULL)                              */
    const float* dpost_std;  /* [T x B x S] (or NULL)                                               */
    float min_std;
    /* outputs: pre-activation gradients for bd_wgrad */
    float* d_embed_pre;  /* [T x B x Be]                                                            */
    float* d_gi;         /* [T x B x 3*Be] (r,z,n) gradient w.r.t. W_ih x + b_ih                     */
    float* d_gh;         /* [T x B x 3*Be] gradient w.r.t. W_hh h + b_hh                             */
    float* d_q1_pre;     /* [T x B x Hd]   (also the gradient of pre_emb)                            */
    float* d_q2_out;     /* [T x B x 2*S]                                                           */
} bd_observe_bwd_args;
int bd_observe_backward(const bd_observe_bwd_args* a, void* stream);

/* Cluster variant of the observe scan for small batches (B=50 -> only 4 row tiles): C = bd_observe_cluster_size(B, Be)
 * workgroups (CUs) share each 16-row tile.  The GRU contraction is split by output column blocks over the members,
 * everything small is computed redundantly, and one all-gather per time step goes through `ws` (write-through
 * stores + per-member flags + sc1 loads, bounded spins).  Same arguments and results as bd_observe_forward /
 * bd_observe_backward; `ws` holds bd_observe_cluster_ws_floats(B, Be) floats, is zero-filled ONCE by the caller when
 * it is allocated, and its flags are zeroed by a memset node on `stream` ahead of each launch.  The error word inside
 * it (float index bd_observe_cluster_err_offset(B), a u32) is STICKY: a member that times out waiting for its peers
 * ORs 1 (forward) / 2 (backward) into it, launches never clear it, so a time-out of any launch stays visible until
 * bd_observe_cluster_status reads it.  bd_observe_cluster_status synchronises `stream`, returns non-zero with the
 * error text if the word is set, and clears it.  A host that already copies results back every step (the engine's
 * log fetch) reads the word in the same transfer instead.  bd_observe_cluster_set_spin_limit (0 = default, about
 * seconds) exists so that tests can force a time-out.  The launches return an error (never abort the queue) when the
 * kernel's static + dynamic LDS would exceed the CU's 160 KiB. */
int bd_observe_cluster_size(int B, int Be);   /* workgroups per 16-row tile; 0 = use bd_observe_forward/backward */
/* Two cluster forms sit behind the same calls.  Round 3 (csrc/observe_ksplit.hip, the default where the cluster has one
 * member per 16-column belief block and Hd <= Be): the layers of the step are split over the members with the weight
 * slices resident in registers -- forward: GRU split by output columns, posterior-hidden partials reduce-scatter, head
 * partials all-reduce (two hand-offs per step); backward: every layer split along K (three hand-offs per step); nothing
 * but the small embed layer computed redundantly.  Round 1 (csrc/observe_cluster.hip, wide batches with two belief
 * blocks per member, or bd_observe_cluster_set_ksplit(0)): only the GRU is split, by output columns, one all-gather per
 * step, the small layers recomputed by every member.  Identical arguments and results. */
int bd_observe_cluster_set_ksplit(int mode);  /* -1 = the K-split form wherever the shapes allow it (the default);
                                               * 0 = the round-1 form everywhere.  Any other value returns an error
                                               * and leaves the setting unchanged. */
size_t bd_observe_cluster_ws_floats(int B, int Be);
int bd_observe_forward_cluster(const bd_observe_fwd_args* a, float* ws, size_t ws_floats, void* stream);
int bd_observe_backward_cluster(const bd_observe_bwd_args* a, float* ws, size_t ws_floats, void* stream);
int bd_observe_cluster_status(float* ws, int B, void* stream);
size_t bd_observe_cluster_err_offset(int B);
int bd_observe_cluster_set_spin_limit(unsigned limit);   /* returns 0 */

/* Dynamic LDS, in bytes, that the launcher of one recurrent scan kernel asks for at a shape, before any rounding up to the
 * CU's whole LDS: the total of the layout that kernel and launcher share (csrc/bd_scan_layout.h).  Gaussian kernels read
 * (Be, S, A, Hd), Categorical ones (Be, D, C, A, Hd), the Categorical cluster forms also their cluster size Cm; what a kernel
 * does not read is ignored.  Returns 0 with the error text set for an unknown kernel, a non-positive width, Cm not dividing
 * D, or a layout whose float4 regions are misaligned.  Host only: no device call. */
#define BD_SCAN_OBSERVE_FWD 0        /* observe_fwd_kernel        (bd_observe_forward) */
#define BD_SCAN_OBSERVE_BWD 1        /* observe_bwd_kernel        (bd_observe_backward) */
#define BD_SCAN_OBSERVE_CFWD 2       /* observe_cfwd_kernel       (bd_observe_forward_cluster, round-1 form) */
#define BD_SCAN_OBSERVE_CBWD 3       /* observe_cbwd_kernel       (bd_observe_backward_cluster, round-1 form) */
#define BD_SCAN_OBSERVE_KFWD 4       /* observe_kfwd_ns_kernel    (bd_observe_forward_cluster, K-split form) */
#define BD_SCAN_OBSERVE_KBWD 5       /* observe_kbwd_kernel       (bd_observe_backward_cluster, K-split form) */
#define BD_SCAN_IMAGINE_FWD 6        /* imagine_fwd_kernel */
#define BD_SCAN_IMAGINE_BWD 7        /* imagine_bwd_kernel */
#define BD_SCAN_OBSERVE_CAT_FWD 8    /* observe_cat_fwd_kernel */
#define BD_SCAN_OBSERVE_CAT_BWD 9    /* observe_cat_bwd_kernel */
#define BD_SCAN_IMAGINE_CAT_FWD 10   /* imagine_cat_fwd_kernel */
#define BD_SCAN_IMAGINE_CAT_BWD 11   /* imagine_cat_bwd_kernel */
#define BD_SCAN_OBSERVE_CAT_CFWD 12  /* observe_cat_cfwd_kernel   (bd_observe_cat_forward_cluster) */
#define BD_SCAN_OBSERVE_CAT_CBWD 13  /* observe_cat_cbwd_kernel   (bd_observe_cat_backward_cluster) */
size_t bd_scan_lds_bytes(int kernel, int Be, int S, int D, int C, int A, int Hd, int Cm);

/* GaussianBeliefModel tail (src/models.py:70-73): out[M x 2S] -> mean, std=softplus(raw)+min_std,
 * state = mean + std*eps.  Used for the batched prior of the observe scan. */
int bd_gauss_head_forward(const float* out, const float* eps, int M, int S, float min_std,
                          float* mean, float* std, float* state, void* stream);
/* d out = [dmean + dstate, (dstd + dstate*eps) * sigmoid(raw)];  dstate/dmean/dstd may be NULL */
int bd_gauss_head_backward(const float* out, const float* eps, const float* dstate, const float* dmean,
                           const float* dstd, int M, int S, float* dout, void* stream);

/* ---- imagination rollout: Dreamer.imagine_ahead + get_action (src/dreamer.py:179-237,429-444),
 *      ActorModel (src/models.py:506-517), SampleDist.entropy / TanhBijector (src/models.py:630-733).
 * One persistent launch walks all Hm = planning_horizon-1 steps; a workgroup owns 16 trajectories. */
typedef struct {
    int N, Hm, Be, S, A, Hd, n_samples;
    /* frozen world model (packed) */
    const float* w_embed_s; const float* w_embed_a; const float* b_embed;
    const float* w_ir; const float* w_iz; const float* w_in;
    const float* w_hr; const float* w_hz; const float* w_hn;
    const float* b_ih; const float* b_hh;
    const float* w_p1; const float* b_p1;          /* belief_prior.model.0 (Hd, Be)                 */
    const float* w_p2m; const float* w_p2s; const float* b_p2;
    /* actor (packed): layer 0 split in belief / state columns, 3 more hidden layers, output layer split
       in mean rows / std rows (model.8: (2A, Hd)) */
    const float* w_a0h; const float* w_a0s; const float* w_a[3]; const float* b_a[4];
    const float* w_a4m; const float* w_a4s; const float* b_a4;
    /* inputs */
    const float* start_feat;   /* [N x (Be+S)] detached posterior features                          */
    const float* eps_action;   /* [Hm x N x A]                                                      */
    const float* eps_entropy;  /* [Hm x n_samples x N x A]                                          */
    const float* eps_prior;    /* [Hm x N x S]                                                      */
    float min_std, act_raw_init_std, act_min_std, act_mean_scale;
    /* outputs */
    float* feat;          /* [Hm x N x (Be+S)] imagined [belief | prior_state]                      */
    float* prior_mean;    /* [Hm x N x S] (may be NULL)                                             */
    float* prior_std;     /* [Hm x N x S]                                                           */
    float* entropy;       /* [Hm x N]                                                               */
    float* action;        /* [Hm x N x A] tanh-squashed sample                                      */
    /* saved for the backward (all NULL for inference) */
    float* sv_actor;      /* [4][Hm x N x Hd] actor hidden activations                              */
    float* sv_act_stats;  /* [Hm x N x 4A]: tanh(m/scale), sigmoid(raw+init), d ent/d mean, d ent/d std */
    float* sv_x;          /* [Hm x N x Be]                                                          */
    float* sv_gates;      /* [Hm x N x 4*Be]                                                        */
    float* sv_p;          /* [Hm x N x Hd]                                                          */
    size_t sv_actor_stride; /* floats between the layers of sv_actor; 0 = Hm*N*Hd.  Lets a rollout be launched in
                               time segments (a segment [t0, t1): Hm = t1 - t0, start_feat = feat of step t0 - 1, every
                               [Hm x ...] pointer shifted by t0 steps, sv_actor_stride = the whole rollout's Hm*N*Hd):
                               the segments give the bits of the single launch */
    float* sv_act_us;     /* [Hm x N x 2A] or NULL: the exact pre-tanh sample u = mean + std*eps (columns 0..A-1) and
                             std (columns A..2A-1) of every action, for bd_actor_reinforce (slot 3 of sv_act_stats
                             holds std only until bd_actor_entropy replaces it) */
    int discrete_actions; /* 0: tanh-Normal actor (everything above).  1: Categorical actor (action_distribution=
                           * "Categorical"): the head w_a4m / b_a4 has A outputs `out` (w_a4s unused, may be NULL),
                           * norm = out - logsumexp(out), p = softmax(norm), k = argmax(p / eps_action) (eps_action:
                           * Exp(1) draws, the first maximum wins), action = (onehot(k) + p) - p (straight-through, in
                           * that order), entropy = -sum p * norm exactly (eps_entropy unused, no bd_actor_entropy);
                           * sv_act_stats is [Hm x N x A] and holds norm; sv_act_us must be NULL                   */
} bd_imagine_fwd_args;
int bd_imagine_forward(const bd_imagine_fwd_args* a, void* stream);
/* The two launches of bd_imagine_forward separately (a caller that saves the actor statistics may run the entropy
 * estimate on another stream: it is off the recurrence).  bd_imagine_forward_scan leaves (mean, std) of every action in
 * slots 2, 3 of sv_act_stats and writes no entropy when sv_act_stats != NULL (with NULL it computes the entropy in the
 * scan and the second call is not needed); bd_actor_entropy turns them into entropy[Hm x N] and d entropy / d mean, / d std
 * in the same slots (SampleDist.entropy / TanhBijector, src/models.py:630-733). */
int bd_imagine_forward_scan(const bd_imagine_fwd_args* a, void* stream);
int bd_actor_entropy(const float* eps_entropy, float* act_stats, float* entropy, int Hm, int N, int A, int n_samples,
                     void* stream);

typedef struct {
    int N, Hm, Be, S, A, Hd;
    const float* wt_embed_s; const float* wt_embed_a;        /* (S, Be), (A, Be)                    */
    const float* wt_ir; const float* wt_iz; const float* wt_in;
    const float* wt_hr; const float* wt_hz; const float* wt_hn;
    const float* wt_p1; const float* wt_p2m; const float* wt_p2s;
    const float* wt_a[3];                 /* transposes of actor layers 1..3 (layer 0: input detached) */
    const float* wt_a4m; const float* wt_a4s;                /* (Hd, A) each                        */
    /* forward tensors */
    const float* start_feat; const float* feat; const float* prior_std; const float* action;
    const float* eps_action; const float* eps_prior;
    const float* sv_actor; const float* sv_act_stats; const float* sv_x; const float* sv_gates;
    const float* sv_p;
    float min_std;
    /* incoming gradients */
    const float* dfeat;     /* [Hm x N x (Be+S)] from reward / value heads                           */
    float dentropy;         /* d loss / d entropy[t][n] (constant: -entropy_weight/(Hm*N))           */
    /* outputs for bd_wgrad */
    float* d_actor_pre;     /* [4][Hm x N x Hd], or NULL: the actor's hidden layers are off the recurrence (detached
                             * input); the caller then runs them as one chain over all rows from d_actor_out:
                             * bd_mlp_backward(layers = actor, dout = d_actor_out, saved = sv_actor, dpre outputs)  */
    float* d_actor_out;     /* [Hm x N x 2A]                                                        */
    const float* ent_weight; /* optional [Hm x N] per-element factor on dentropy (use_discount=True: the cumulative
                              * discount weights of the actor objective, src/dreamer.py:346-351), or NULL          */
    int discrete_actions;   /* 1: Categorical actor (see bd_imagine_fwd_args): d_actor_out is [Hm x N x A],
                             * d out = p * (g - p.g) + dent * (-p * (norm + H)) with g = d loss / d action and
                             * dent = dentropy (* ent_weight); wt_a4m is the (Hd, A) head transpose, wt_a4s, eps_action
                             * unused; d_actor_pre must be NULL (the hidden layers run as the caller's chain)         */
} bd_imagine_bwd_args;
int bd_imagine_backward(const bd_imagine_bwd_args* a, void* stream);

/* ---- lambda-return (src/dreamer.py:447-471); bootstrap = value[Hm-1] as at dreamer.py:332 ----- */
int bd_lambda_return_forward(const float* reward, const float* value, int Hm, int N, float discount,
                             float lambda_, float* returns, void* stream);
/* gradient of the scan: d returns = dreturns[Hm x N] if non-NULL else the constant dret_const.
 * Writes dreward and dvalue (dvalue[0] = 0: value[0] is never used; the bootstrap duplicate of
 * value[Hm-1] is folded into dvalue[Hm-1]). */
int bd_lambda_return_backward(const float* dreturns, float dret_const, int Hm, int N, float discount,
                              float lambda_, float* dreward, float* dvalue, void* stream);

/* ---- frozen imagined heads, forward + dgrad in one launch (csrc/heads.hip) ---------------------------------------
 * reward_model and critic_target (DenseModel: BD_HEAD_HIDDEN ELU layers of width Hd, then Hd -> 1) over M rows of
 * x = [h; s] (row-major, ld = F):  out = head(x), and  dx = d out_r/dx^T dout_r + d out_v/dx^T dout_v  (plain store).
 * The saved activations stay on chip; no weight gradients (the heads are frozen).  Returns -1 without launching for
 * shapes bd_img_heads_supported(F, Hd) rejects. */
#define BD_HEAD_HIDDEN 4
typedef struct {
    const float* w[BD_HEAD_HIDDEN];   /* packed W_l (forward): [Hd x F], then [Hd x Hd]                          */
    const float* wt[BD_HEAD_HIDDEN];  /* packed W_l^T (dgrad): [F x Hd], then [Hd x Hd]                          */
    const float* b[BD_HEAD_HIDDEN];   /* [Hd]                                                                    */
    const float* w_out;               /* output layer weight, plain [Hd]                                         */
    const float* b_out;               /* output layer bias [1]                                                   */
    const float* dout;                /* d loss / d out [M]                                                      */
    float* out;                       /* [M]                                                                     */
} bd_img_head;
typedef struct {
    int M, F, Hd;
    const float* x;                   /* [M x F]                                                                 */
    bd_img_head head[2];
    float* dx;                        /* [M x F]                                                                 */
} bd_img_heads_args;
int bd_img_heads_supported(int F, int Hd);
int bd_img_heads_fwd_bwd(const bd_img_heads_args* a, void* stream);

/* ---- REINFORCE term of the mixed actor gradient (ActorCritic.gradient_mixing = rho; DreamerV2 eq. 6) ----------
 * Row i of the Hm*N imagined decisions (slot k = i / N) took u = mean + std*eps (act_us), baseline
 * b_i = base0[i] for i < N (critic_target on the start features) and value[i - N] after (the target value of the
 * state the action was taken in), advantage adv = returns[i] - b_i (a constant), weight w = weight[i] (NULL: 1), and
 *   l_i = sum_a [ log N(u; mean, std) - log(1 - tanh^2 u) ]      (tanh-Normal log-density of the taken action).
 * d_actor_out [Hm*N x 2A] (the layout bd_imagine_backward writes) receives the head gradient of c * l with
 * c = -(1 - rho) * grad_scale * w * adv (grad_scale = 1 / element count of the objective's mean):
 *   d mean-half += c * (eps/std) * (1 - th^2),   d std-half += c * ((eps^2 - 1)/std) * sg
 * with th, sg = slots 0, 1 of act_stats, rho in [0, 1].  write != 0: d_actor_out is written from scratch as that plus
 * the entropy term bd_imagine_backward would add (dentropy * w * slots 2, 3 of act_stats, through th / sg), i.e. the
 * gradient of the rho = 0 objective without the imagination backward.  value may be NULL when Hm = 1.
 * scalars[slot] = sum_i w * l_i * adv (RAW sum; per-workgroup fp64 partials in ws, fixed-order final sum: the same
 * bits in either mode). */
int bd_actor_reinforce(const float* eps_action, const float* act_us, const float* act_stats, const float* returns,
                       const float* base0, const float* value, const float* weight, int Hm, int N, int A, float rho,
                       float grad_scale, float dentropy, int write, float* d_actor_out, float* scalars, int slot, float* ws,
                       void* stream);
/* The same for the Categorical actor (discrete_actions = 1): row i took class k_i (action: the straight-through
 * one-hot, [Hm*N x A]; k_i = the column above 0.5), act_stats = the scan's norm [Hm*N x A], p = softmax(norm),
 *   l_i = norm[k_i],   d l / d out = onehot(k_i) - p.
 * d_actor_out [Hm*N x A] += c * (onehot(k_i) - p) with c as above; write != 0: written from scratch as that plus the
 * entropy term dentropy * w * (-p * (norm + H)).  scalars[slot] as bd_actor_reinforce. */
int bd_actor_reinforce_cat(const float* action, const float* act_stats, const float* returns, const float* base0,
                           const float* value, const float* weight, int Hm, int N, int A, float rho, float grad_scale,
                           float dentropy, int write, float* d_actor_out, float* scalars, int slot, float* ws,
                           void* stream);
/* Both with the advantage term divided by a return scale held on the device (return normalisation, below): c =
 * -(1 - rho) * (grad_scale / ret_scale[0]) * w * adv.  The entropy term (dentropy) and scalars[slot] are not divided.
 * ret_scale = NULL is the entry point above. */
int bd_actor_reinforce_norm(const float* eps_action, const float* act_us, const float* act_stats, const float* returns,
                            const float* base0, const float* value, const float* weight, const float* ret_scale, int Hm,
                            int N, int A, float rho, float grad_scale, float dentropy, int write, float* d_actor_out,
                            float* scalars, int slot, float* ws, void* stream);
int bd_actor_reinforce_cat_norm(const float* action, const float* act_stats, const float* returns, const float* base0,
                                const float* value, const float* weight, const float* ret_scale, int Hm, int N, int A,
                                float rho, float grad_scale, float dentropy, int write, float* d_actor_out, float* scalars,
                                int slot, float* ws, void* stream);

/* ---- perf-mode noise: Philox4x32-10, counter-based (csrc/bd_rng.h).  key = seed, counter = (index of a group of four
 * values, stream id, step): any element of any stream of any step is computable on its own.  The parity path never uses
 * this: tests pass the reference's draws as explicit arrays.
 * bd_rng_fill: up to BD_RNG_MAX_TENSORS noise tensors in ONE launch (standard normals: src/models.py:72 randn_like,
 * src/dreamer.py:443 rsample; Exp(1): the variates torch.multinomial's single-draw path consumes, src/models.py:114-115). */
#define BD_RNG_MAX_TENSORS 6
#define BD_RNG_NORMAL 0
#define BD_RNG_EXPONENTIAL 1
#define BD_RNG_UNIFORM 2          /* u = (word >> 8) * 2^-24 in [0, 1): torch.rand of the epsilon-greedy exploration */
typedef struct {
    int n;
    unsigned long long seed;
    unsigned long long step;
    struct {
        float* p;
        size_t count;
        int kind;                 /* BD_RNG_NORMAL | BD_RNG_EXPONENTIAL | BD_RNG_UNIFORM */
        unsigned stream_id;       /* distinct per tensor */
    } t[BD_RNG_MAX_TENSORS];
} bd_rng_fill_args;
int bd_rng_fill(const bd_rng_fill_args* a, void* stream);
/* The generator's core on the host: out4 = Philox4x32-10(counter ctr4, key key2) (known-answer tests, no GPU needed). */
int bd_philox4x32_10(const unsigned* ctr4, const unsigned* key2, unsigned* out4);
/* bd_actor_entropy with the n_samples draws per (row, action dim) generated IN the kernel (stream `stream_id` of `seed`,
 * `step`): the (Hm x n_samples x N x A) entropy noise tensor -- 13.7 MB per step at configs[1], 233 MB at A = 17 -- is never
 * written to or read from HBM.  Same estimator, same outputs as bd_actor_entropy (SampleDist.entropy, src/models.py:725-733). */
int bd_actor_entropy_rng(unsigned long long seed, unsigned long long step, unsigned stream_id, float* act_stats,
                         float* entropy, int Hm, int N, int A, int n_samples, void* stream);

/* ---- plain GEMM  C[M x N] (+)= A[M x K] B[N x K]^T  (csrc/gemm.hip; fp32 MFMA, exact fp32 products and sums).
 * The pixel decoder's one plain GEMM: the dgrad of ConvTranspose2d(E -> 128, k5, s2) on a 1 x 1 map
 * (src/models.py:338-341), d l0[M x E] = g[M x 3200] W[E x 3200]^T.  Any K / leading dimensions / alignment (16-byte
 * loads per operand where its base, leading dimension and K allow them). */
int bd_gemm_nt(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, int accumulate,
               void* stream);

/* ---- Categorical latents: CategoricalBeliefModel tail (src/models.py:108-117) and the Categorical branch of
 * Dreamer._kl_loss (src/dreamer.py:102-106,131-144).  logits / state / probs are [rows x D*C], D groups of C classes.
 * Forward: probs = softmax(logits) per group; state = one_hot(argmax(probs / q_noise)) with q_noise ~ Exp(1), which is
 * torch.multinomial's single-draw algorithm behind OneHotCategoricalStraightThrough.rsample(); the straight-through
 * term adds exactly zero.  Backward: dlogits = probs * (dstate - sum_c probs * dstate) per group. */
int bd_categorical_head_forward(const float* logits, const float* q_noise, int rows, int D, int C, float* state,
                                float* probs, void* stream);
int bd_categorical_head_backward(const float* dstate, const float* probs, int rows, int D, int C, float* dlogits,
                                 void* stream);
/* KL(post || prior) between the D categorical factors.  Forward writes the RAW sum into scalars[slot] (sum over all
 * rows*D groups; with sum_form -- kl_balance == -1 -- the sum over rows of max(sum_D KL, free_nats)); ws as for the
 * other reductions.  Backward (same conventions as bd_kl_backward): balanced form lhs -> dprior, rhs -> dpost, both
 * gated by the free-nats clamp of the mean scalars[slot] * inv_count. */
int bd_kl_categorical_forward(const float* post_logits, const float* prior_logits, int rows, int D, int C, float free_nats,
                              int sum_form, float* scalars, int slot, float* ws, void* stream);
int bd_kl_categorical_backward(const float* post_logits, const float* prior_logits, int rows, int D, int C, float free_nats,
                               float kl_balance, float weight, float inv_count, const float* scalars, int slot,
                               float* dpost, float* dprior, void* stream);

/* ---- Categorical RSSM scans: latent_distribution="Categorical" (BASELINE configs[4], algorithm=dreamerV2) ----
 * TransitionModel.forward (src/models.py:191-299, Categorical branches :226-228,258-260,269-271) and
 * Dreamer.imagine_ahead (src/dreamer.py:179-237, :205-206,224-227) with CategoricalBeliefModel heads
 * (src/models.py:76-117): the state is D one-hot factors of C classes, S = D*C (src/planet.py:56-57), sampled with
 * straight-through gradients (OneHotCategoricalStraightThrough.rsample()).
 * Same persistent 16-row-tile design as the Gaussian scans.  What changes with the latent:
 *   - the state is carried as D class indices per row; W [s; a] of the embed layer (and W0 [h; s] of the actor) is the
 *     MFMA contraction over the action / belief columns PLUS A GATHER of D rows of the transposed state weights
 *     (`*_sT`: plain row-major [S x out], row k = W[:, k]) -- 32 x out adds instead of a K = 1024 contraction;
 *   - the head is hidden -> S logits (MFMA, 256 columns at a time through LDS), then per factor softmax and
 *     sample = argmax(probs / q), q ~ Exp(1): torch.multinomial's single-draw path, q is an explicit input [rows x S];
 *   - backward: d logits = probs * (g - sum_c probs * g) per factor (straight-through: d state / d probs = I) with
 *     g = d loss / d state = heads' gradient + W_es^T (d embed pre-activation of the next step) (* nonterminal).
 * Outputs: feat [rows x (Be+S)] = [h; one-hot s] (dense: the reward / value / decoder chains read it as any other
 * feature matrix), the class indices sidx [rows x D] (uint8), the logits [rows x S].
 * C <= 256; S <= 256, or 256 % C == 0 and S % 16 == 0. */
typedef struct {
    int T, B, Be, D, C, A, Hd;
    const float* w_embed_sT;                                   /* plain [S x Be]: row k = W_e[:, k]           */
    const float* w_embed_a; const float* b_embed;              /* packed (Be, A), [Be]                        */
    const float* w_ir; const float* w_iz; const float* w_in;
    const float* w_hr; const float* w_hz; const float* w_hn;
    const float* b_ih; const float* b_hh;
    const float* w_q1h; const float* b_q1;                     /* posterior layer 0, belief columns           */
    const float* w_q2; const float* b_q2;                      /* packed (S, Hd), [S]: posterior logits       */
    const float* init_belief;                                  /* [B x Be]                                    */
    const float* init_state;                                   /* [B x S]: zeros, or one-hot per factor       */
    const float* actions;                                      /* [T x B x A]                                 */
    const float* nonterm;                                      /* [T x B] or NULL                             */
    const float* pre_emb;                                      /* [T x B x Hd] hoisted embeddings @ W_q1[:, Be:]^T */
    const float* q_post;                                       /* [T x B x S] Exp(1) draws of the sampler     */
    float* feat;                                               /* out [T x B x (Be+S)]                        */
    float* post_logits;                                        /* out [T x B x S]                             */
    unsigned char* sidx;                                       /* out [T x B x D] sampled class per factor    */
    float* sv_s;       /* [T x B x S] masked input state of every step (dense; embed weight gradient), or NULL */
    float* sv_x; float* sv_gates; float* sv_q;                 /* as bd_observe_fwd_args, or NULL              */
} bd_observe_cat_fwd_args;
int bd_observe_cat_forward(const bd_observe_cat_fwd_args* a, void* stream);

typedef struct {
    int T, B, Be, D, C, A, Hd;
    const float* wt_embed_s;                                   /* packed transpose (S, Be): d state = W_es^T d pre */
    const float* wt_ir; const float* wt_iz; const float* wt_in;
    const float* wt_hr; const float* wt_hz; const float* wt_hn;
    const float* wt_q1h;                                       /* (Be, Hd)                                    */
    const float* wt_q2;                                        /* packed transpose (Hd, S)                    */
    const float* init_belief; const float* nonterm;
    const float* feat; const float* post_logits;
    const float* sv_x; const float* sv_gates; const float* sv_q;
    const float* dfeat;          /* [T x B x (Be+S)] from the obs / reward heads (+ prior head on the belief part) */
    const float* dpost_logits;   /* [T x B x S] from the KL term, or NULL                                        */
    float* d_embed_pre; float* d_gi; float* d_gh; float* d_q1_pre;   /* as bd_observe_bwd_args                   */
    float* d_q2_out;             /* [T x B x S] gradient of the posterior logits                                */
} bd_observe_cat_bwd_args;
int bd_observe_cat_backward(const bd_observe_cat_bwd_args* a, void* stream);

/* Cluster variant of the Categorical observe scan (csrc/observe_cat_cluster.hip): Cm = bd_observe_cat_cluster_size(B, Be,
 * D, C, max_wgs) workgroups, one per CU, share each 16-row tile -- GRU column blocks and groups of D / Cm factors of the
 * posterior head are split over the members, two hand-offs per time step through `ws` (forward: new belief, sampled class
 * indices; backward: d posterior-hidden all-reduce, [belief-gradient carry | d embed pre-activation]).  Same arguments,
 * same results as bd_observe_cat_forward / bd_observe_cat_backward (TransitionModel.forward, src/models.py:191-299,
 * Categorical branches).  cluster size 0 = shape not supported or tiles * Cm > max_wgs: use the one-workgroup-per-tile
 * calls.  `ws`: bd_observe_cat_cluster_ws_floats(B, Be, Hd, D, Cm) floats, zero-filled ONCE by the caller; header, sticky
 * error word (bd_observe_cluster_err_offset / bd_observe_cluster_status) and time-out behaviour as for
 * bd_observe_forward_cluster. */
int bd_observe_cat_cluster_size(int B, int Be, int D, int C, int max_wgs);
size_t bd_observe_cat_cluster_ws_floats(int B, int Be, int Hd, int D, int Cm);
int bd_observe_cat_forward_cluster(const bd_observe_cat_fwd_args* a, int Cm, float* ws, size_t ws_floats, void* stream);
int bd_observe_cat_backward_cluster(const bd_observe_cat_bwd_args* a, int Cm, float* ws, size_t ws_floats, void* stream);

typedef struct {
    int N, Hm, Be, D, C, A, Hd, n_samples;
    const float* w_embed_sT; const float* w_embed_a; const float* b_embed;
    const float* w_ir; const float* w_iz; const float* w_in;
    const float* w_hr; const float* w_hz; const float* w_hn;
    const float* b_ih; const float* b_hh;
    const float* w_p1; const float* b_p1;                      /* belief_prior.model.0                        */
    const float* w_p2; const float* b_p2;                      /* packed (S, Hd), [S]: prior logits           */
    const float* w_a0h;                                        /* actor layer 0, belief columns, packed       */
    const float* w_a0sT;                                       /* actor layer 0, state columns: plain [S x Hd] */
    const float* w_a[3]; const float* b_a[4];
    const float* w_a4m; const float* w_a4s; const float* b_a4;
    const float* start_feat;                                   /* [N x (Be+S)] posterior features (one-hot s)  */
    const unsigned char* start_sidx;                           /* [N x D] class indices of start_feat's one-hot state, or NULL: every
                                                                  factor of start_feat[:, Be:] is then all-zero (fed as zeros, like
                                                                  the reference does with its initial state) or (scaled) one-hot   */
    const float* eps_action; const float* eps_entropy;         /* as bd_imagine_fwd_args                      */
    const float* q_prior;                                      /* [Hm x N x S] Exp(1) draws                   */
    float act_raw_init_std, act_min_std, act_mean_scale;
    float* feat;                                               /* out [Hm x N x (Be+S)]                       */
    unsigned char* sidx;                                       /* out [Hm x N x D]                            */
    float* prior_logits;                                       /* out [Hm x N x S]                            */
    float* entropy; float* action;
    float* sv_actor; float* sv_act_stats; float* sv_x; float* sv_gates; float* sv_p;   /* or NULL            */
    float* sv_act_us;                                          /* as bd_imagine_fwd_args, or NULL             */
    int discrete_actions;                                      /* as bd_imagine_fwd_args                      */
} bd_imagine_cat_fwd_args;
int bd_imagine_cat_forward(const bd_imagine_cat_fwd_args* a, void* stream);
/* (eps_entropy == NULL with sv_act_stats != NULL: the scan alone -- the caller runs the entropy estimate itself,
 * bd_actor_entropy or bd_actor_entropy_rng on sv_act_stats, as after bd_imagine_forward_scan) */

typedef struct {
    int N, Hm, Be, D, C, A, Hd;
    const float* wt_embed_s; const float* wt_embed_a;
    const float* wt_ir; const float* wt_iz; const float* wt_in;
    const float* wt_hr; const float* wt_hz; const float* wt_hn;
    const float* wt_p1;                                        /* (Be, Hd)                                    */
    const float* wt_p2;                                        /* packed transpose (Hd, S)                    */
    const float* wt_a[3]; const float* wt_a4m; const float* wt_a4s;
    const float* start_feat; const float* feat; const float* prior_logits; const float* action;
    const float* eps_action;
    const float* sv_actor; const float* sv_act_stats; const float* sv_x; const float* sv_gates; const float* sv_p;
    const float* dfeat;          /* [Hm x N x (Be+S)] from the reward / value heads                            */
    float dentropy;
    float* d_actor_pre; float* d_actor_out;                    /* as bd_imagine_bwd_args                      */
    const float* ent_weight;     /* as bd_imagine_bwd_args, or NULL                                              */
    int discrete_actions;        /* as bd_imagine_bwd_args                                                       */
} bd_imagine_cat_bwd_args;
int bd_imagine_cat_backward(const bd_imagine_cat_bwd_args* a, void* stream);

/* ---- CEM planner: MPCPlanner.forward (src/planner.py:28-90), csrc/planner.hip ---------------------
 * One CEM iteration = a rollout + bd_cem_refit.  rows = B * cand candidate action sequences (row = b * cand + c);
 * the rollout forms a_t = act_mean[t][b] + act_std[t][b] * eps_action[t][row] (src/planner.py:60-62), runs the
 * prior-only RSSM step (src/models.py:241-256, embeddings=None, nonterminals=None) and the reward model
 * (src/models.py:365-408) per step in LDS and writes the actions [H x rows x A] and the summed predicted reward per
 * candidate (src/planner.py:68-72).
 * One argument block and one kernel body for both latent kinds; latent_cat selects the instantiation.  bd_plan_rollout
 * takes latent_cat = 0 only (a zeroed block with the Gaussian fields filled in), bd_plan_rollout_cat latent_cat != 0 only.
 *   latent_cat = 0: Gaussian latents (w_embed_s, w_p2m / w_p2s, w_r[0] packed over K = Be+S, min_std; D, C, seed, step,
 *     stream_id, sidx ignored): s' = mean + (softplus(raw) + min_std) * eps_state, eps_state standard normal.  S <= 64.
 *   latent_cat: latent_distribution="Categorical" (TransitionModel.forward's Categorical branches, src/models.py:226-228,
 *     241-260; CategoricalBeliefModel, src/models.py:101-117), S = D*C.  The state is carried as D class indices: W_es s and
 *     the state columns of the reward model's first layer are gathers of rows of the plain transposes (w_embed_sT, w_r0sT:
 *     [S x out], as in bd_imagine_cat_fwd_args; w_r0h holds that layer's belief columns, w_r[0] is ignored); the prior head
 *     w_p2 gives S logits, per factor idx = argmax(softmax(logits) / q) with q = eps_state ~ Exp(1), first maximum winning
 *     (torch.multinomial's single-draw path, src/models.py:114-115), and the one-hot of idx is the state that continues.
 *     init_state: every factor all-zero (fed as zeros) or (scaled) one-hot, as bd_imagine_cat_forward with start_sidx = NULL.
 *     eps_state = NULL: the draws are generated in the kernel, element i of the [H x rows x S] tensor being what
 *     bd_rng_fill(kind = BD_RNG_EXPONENTIAL, seed, step, stream_id, count = H*rows*S) writes at i (needs S % 4 == 0).
 *     C <= 256; S <= 256, or 256 % C == 0 and S % 16 == 0.
 * returns = NULL: the unfused form -- feat [H x rows x (Be+S)] = [h'; s'] (the one-hot s' with latent_cat, and then sidx
 * [H x rows x D] too) is written and the caller runs the reward model (bd_mlp_forward, with the one-hot segment there);
 * the reward weights may then be NULL.  returns and feat (with latent_cat: and sidx) may also BOTH be given: one launch then
 * writes all of them, each with the bits of the launch that asks for it alone (tests/test_plan_kernels_gpu.py).
 * LDS as csrc/planner.hip states (<= 160 KiB). */
typedef struct {
    int rows, H, cand, Be, D, C, S, A, Hd;
    int latent_cat;
    const float* w_embed_s;                               /* Gaussian latents: packed (Be, S) */
    const float* w_embed_sT;                              /* Categorical latents: plain [S x Be]: row k = W_e[:, k] */
    const float* w_embed_a; const float* b_embed;         /* packed (Be, A), [Be] */
    const float* w_ir; const float* w_iz; const float* w_in;
    const float* w_hr; const float* w_hz; const float* w_hn;
    const float* b_ih; const float* b_hh;
    const float* w_p1; const float* b_p1;                 /* belief_prior.model.0 */
    const float* w_p2m; const float* w_p2s;               /* Gaussian latents: belief_prior.model.2 rows [:S] / [S:] */
    const float* w_p2;                                    /* Categorical latents: packed (S, Hd): prior logits */
    const float* b_p2;                                    /* [2*S] / [S] */
    const float* w_r[5];                                  /* reward_model.model.{0,2,4,6,8}, packed; [0]: Gaussian latents only */
    const float* w_r0h;                                   /* Categorical latents: model.0, belief columns, packed (Hd, Be) */
    const float* w_r0sT;                                  /* Categorical latents: model.0, state columns: plain [S x Hd] */
    const float* b_r[5];                                  /* reward_model.model.{0,2,4,6,8}.bias */
    float min_std;
    const float* init_belief;   /* [B x Be]  (every candidate of environment b starts from row b, src/planner.py:37) */
    const float* init_state;    /* [B x S]   */
    const float* act_mean;      /* [H x B x A] */
    const float* act_std;       /* [H x B x A] */
    const float* eps_action;    /* [H x rows x A]  the torch.randn draws of src/planner.py:53-59 */
    const float* eps_state;     /* [H x rows x S]  the prior-state draws (src/models.py:72); with latent_cat NULL = in-kernel */
    unsigned long long seed; unsigned long long step; unsigned stream_id;   /* in-kernel noise (latent_cat, eps_state = NULL) */
    float* actions;             /* out [H x rows x A] */
    float* returns;             /* out [rows]; NULL: skip the reward model and write `feat` (and sidx) instead */
    float* feat;                /* out [H x rows x (Be+S)] ([h'; s'] per step) or NULL */
    unsigned char* sidx;        /* out [H x rows x D] sampled class per factor (latent_cat), or NULL */
} bd_plan_args;
typedef bd_plan_args bd_plan_cat_args;
int bd_plan_rollout(const bd_plan_args* a, void* stream);
int bd_plan_rollout_cat(const bd_plan_cat_args* a, void* stream);
/* Re-fit the action belief to the `top` best candidates of every environment (src/planner.py:74-87):
 * mean / stdev [H x B x A] <- mean and biased standard deviation over the selected action sequences.
 * returns is [ret_steps x B*cand]: ret_steps = 1 for summed returns, H for per-step reward predictions (summed here). */
int bd_cem_refit(const float* returns, int ret_steps, const float* actions, int H, int B, int cand, int top, int A,
                 float* mean, float* stdev, void* stream);

/* ---- acting: one decision of the collect / evaluation loop in ONE launch (csrc/act.hip) -------------------------
 * Planet.update_belief_and_act (src/planet.py:370-403) with Dreamer.get_action (src/dreamer.py:429-444) for B
 * environments: encoder chain (or a ready embedding), embed layer + GRU cell (one step of bd_observe_forward, same weights),
 * posterior head on [h'; embedding] and its sample s', actor chain on [h'; s'], the action sample and exploration.  The
 * prior head and its sample (src/models.py:256), get_action's prior sample and the entropy estimate (src/planet.py:386
 * drops it) feed none of the three outputs and are not evaluated.
 * One argument block and one kernel body for the four configurations; latent_cat / actor_cat select the instantiation.
 * bd_act_step takes latent_cat = actor_cat = 0 only (a zeroed block with the Gaussian fields filled in), bd_act_step_cat
 * the other three and rejects both 0 (that is bd_act_step).
 *   latent_cat = 0: Gaussian latents (w_embed_s, w_q2m / w_q2s, w_a0s; D, C ignored): s' = mean + std * eps_post with
 *     eps_post standard normal, std = softplus(raw) + min_std.  S <= 64.
 *   latent_cat: latent_distribution="Categorical" (TransitionModel.forward's Categorical branches, src/models.py:226-228,
 *     258-260,269-271, CategoricalBeliefModel src/models.py:101-117): the incoming state [B x S], S = D*C, is all-zero or
 *     (scaled) one-hot per factor and is carried as class indices (the rule of bd_imagine_cat_forward with start_sidx =
 *     NULL); W_es s and the state columns of the actor's first layer are gathers of rows of w_embed_sT / w_a0sT (plain
 *     [S x out]); the posterior head w_q2 (packed (S, Hd)) gives D*C logits, per factor idx = argmax(softmax(logits) / q)
 *     with q = eps_post ~ Exp(1), first maximum winning; state_out is the one-hot.  The host must have checked the incoming
 *     one-hot state (a factor with two non-zero classes cannot be carried as an index; the kernel would take the larger).
 *   actor_cat = 0: the tanh-Normal actor: action = tanh(mean + std * eps_action) (mean scaling / init_std / min_std as
 *     bd_imagine_forward), and with explore != 0 action = clamp(action + action_noise * eps_explore, -1, 1); eps_action,
 *     eps_explore [B x A] standard normal.
 *   actor_cat: action_distribution="Categorical" (src/models.py:518-522): the head w_a4m / b_a4 has A outputs (w_a4s
 *     unused), norm = out - logsumexp(out), p = softmax(norm), k = argmax(p / eps_action) with eps_action ~ Exp(1), action =
 *     (onehot(k) + p) - p in that order (what bd_imagine_forward returns with discrete_actions = 1); explore != 0 is
 *     epsilon-greedy (the port's update_belief_and_act): eps_explore is [B x 2] uniforms (u, v) in [0, 1), and where
 *     u < action_noise the action is the exact one-hot of class min(floor(v * A), A - 1).
 * Observation: obs [B x O] with the encoder DenseModel's five layers (w_enc packed, model.{0,2,4,6,8}), or -- obs = NULL --
 * embedding [B x E] (pixel observations: the conv stack has already run; O and the encoder fields are then ignored).
 * Noise: explicit buffers (eps_explore may be NULL when explore = 0), or ALL NULL: drawn in the kernel, element i of each
 * tensor being what bd_rng_fill(kind, seed, step, stream_post / stream_action / stream_explore) writes at i, with the kinds
 * above (BD_RNG_EXPONENTIAL for a Categorical sampler, BD_RNG_UNIFORM for epsilon-greedy, BD_RNG_NORMAL otherwise).
 * The kernel never writes its inputs: belief_out / state_out / action_out must be other buffers than belief / state /
 * action (the host ping-pongs).  One workgroup per 16 rows.  A <= 64; LDS as csrc/act.hip states (<= 160 KiB):
 * bd_act_step_supported / bd_act_step_cat_supported answer from the launcher's own arithmetic without raising an error
 * (O = 0: the embedding form).
 * Evaluation policy (Dreamer v1 / v2 evaluate with the actor's mode, v2 optionally with the posterior mean): the fields
 * behind action_out.  All zero: the step above, from the same four kernels as before the fields existed; anything set
 * selects a second instantiation of the same body, so the sampling kernels carry none of it.
 *   action_mode = BD_POLICY_MODE, tanh-Normal actor: SampleDist.mode (src/models.py:708-723).  Of n_mode draws y_j =
 *     tanh(mean + std * eps_mode[j, row, :]) the action is the y_j with the largest log-density summed over the A
 *     dimensions (the formula of the entropy estimator, csrc/bd_scan.h: clamp at 1 - 2^-24, atanh, log-det), the FIRST
 *     maximum winning.  One wave per row, a lane per draw in passes of 64, a wave argmax; mode_index_out gets j.
 *   action_mode = BD_POLICY_MEAN, tanh-Normal actor: action = tanh(mean), no draw (bit-equal to eps_action = 0).
 *   actor_cat, either mode: the exact one-hot of argmax p, the first maximum winning (q = 1 in the sampler).
 *   Exploration, where asked for, is applied on top as in the sampling step.
 *   latent_mean: Gaussian latents s' = mean_q (bit-equal to eps_post = 0); Categorical latents the per-factor argmax of
 *     the posterior logits (bit-equal to eps_post = 1).
 *   Noise: a buffer is required only for a draw that is consumed (eps_post unless latent_mean, eps_action with
 *     BD_POLICY_SAMPLE, eps_mode with BD_POLICY_MODE and the tanh-Normal actor, eps_explore with explore); as above either every
 *     consumed buffer is given or every one is NULL, and then element i of eps_mode, layout (n_mode, B, A), is what
 *     bd_rng_fill(BD_RNG_NORMAL, seed, step, stream_mode) writes at i. */
#define BD_POLICY_SAMPLE 0
#define BD_POLICY_MODE 1
#define BD_POLICY_MEAN 2
typedef struct {
    int B, Be, D, C, S, A, Hd, E, O;
    int latent_cat, actor_cat;
    const float* w_enc[5]; const float* b_enc[5];         /* encoder.model.{0,2,4,6,8} (obs form only) */
    const float* w_embed_s;                               /* Gaussian latents: packed (Be, S) */
    const float* w_embed_sT;                              /* Categorical latents: plain [S x Be] */
    const float* w_embed_a; const float* b_embed;
    const float* w_ir; const float* w_iz; const float* w_in;
    const float* w_hr; const float* w_hz; const float* w_hn;
    const float* b_ih; const float* b_hh;
    const float* w_q1h; const float* w_q1e; const float* b_q1;   /* belief_posterior.model.0[:, :Be] / [:, Be:] */
    const float* w_q2m; const float* w_q2s;               /* Gaussian latents: belief_posterior.model.2 rows [:S] / [S:] */
    const float* w_q2;                                    /* Categorical latents: packed (S, Hd) */
    const float* b_q2;                                    /* [2*S] / [S] */
    const float* w_a0h;
    const float* w_a0s;                                   /* Gaussian latents: packed (Hd, S) */
    const float* w_a0sT;                                  /* Categorical latents: plain [S x Hd] */
    const float* w_a[3]; const float* b_a[4];
    const float* w_a4m; const float* w_a4s; const float* b_a4;   /* as bd_imagine_fwd_args (discrete_actions = actor_cat) */
    const float* belief;       /* [B x Be] */
    const float* state;        /* [B x S]  */
    const float* action;       /* [B x A]  previous action */
    const float* obs;          /* [B x O] or NULL */
    const float* embedding;    /* [B x E] or NULL (exactly one of obs / embedding) */
    const float* eps_post;     /* [B x S] */
    const float* eps_action;   /* [B x A] */
    const float* eps_explore;  /* [B x A], or [B x 2] with actor_cat; may be NULL when explore = 0 */
    unsigned long long seed; unsigned long long step;     /* in-kernel noise: Philox key and decision counter */
    unsigned stream_post, stream_action, stream_explore;  /* distinct Philox stream ids */
    float min_std, act_raw_init_std, act_min_std, act_mean_scale, action_noise;
    int explore;
    float* belief_out;         /* [B x Be] */
    float* state_out;          /* [B x S]  */
    float* action_out;         /* [B x A]  */
    /* evaluation policy (appended: a zeroed tail is the sampling step above, bit for bit) */
    int action_mode;           /* BD_POLICY_SAMPLE | BD_POLICY_MODE | BD_POLICY_MEAN */
    int latent_mean;           /* s' = the posterior's mean (Gaussian) / per-factor argmax of its logits (Categorical) */
    int n_mode;                /* draws of BD_POLICY_MODE with the tanh-Normal actor (SampleDist's n_samples = 100), >= 1 */
    const float* eps_mode;     /* [n_mode x B x A] standard normal, or NULL; read only by BD_POLICY_MODE, tanh-Normal actor */
    unsigned stream_mode;      /* Philox stream id of the in-kernel eps_mode */
    float* act_stats_out;      /* [B x 2A] actor mean | std per row; may be NULL; tanh-Normal actor, action_mode != 0 */
    int* mode_index_out;       /* [B] index of the winning draw; may be NULL; BD_POLICY_MODE, tanh-Normal actor */
} bd_act_args;
typedef bd_act_args bd_act_cat_args;
int bd_act_step_supported(int Be, int S, int A, int Hd, int E, int O);
int bd_act_step(const bd_act_args* a, void* stream);
int bd_act_step_cat_supported(int Be, int D, int C, int S, int A, int Hd, int E, int O, int latent_cat, int actor_cat);
int bd_act_step_cat(const bd_act_cat_args* a, void* stream);
/* SampleDist.mode on given statistics, the selection rule of BD_POLICY_MODE by the same device function: mean, std [N x A],
 * eps_mode [n x N x A] standard normal or NULL (then element i is what bd_rng_fill(BD_RNG_NORMAL, seed, step, stream_id)
 * writes at i) -> action [N x A] = tanh(mean + std * eps_mode[j]) of the first j with the largest summed log-density,
 * index [N] = j (may be NULL).  One wave per row; any N >= 1, 1 <= A <= 64, 1 <= n <= 2^20. */
int bd_tanh_normal_mode(const float* mean, const float* std, const float* eps_mode, unsigned long long seed,
                        unsigned long long step, unsigned stream_id, int N, int A, int n, float* action, int* index,
                        void* stream);

/* ---- losses (src/planet.py:252-284, src/dreamer.py:110-146,342-383) ---------------------------
 * Reductions write RAW SUMS into a small device "scalar board" (float array); the host turns them
 * into the logged means after one D2H copy per step, and multi-GPU runs all-reduce the board's KL slot
 * before the free-nats clamp.  Each reduction is two launches: per-workgroup fp64 partials in `ws`
 * (bd_reduce_ws_floats() floats), then a fixed-order final sum (deterministic, no float atomics). */
/* scalars[slot] = sum over all elements of 0.5 (t-p)^2 + 0.5 ln 2pi;  dpred = (p-t) * grad_scale
 * (-Independent(Normal(pred,1)).log_prob(target); dpred may be NULL) */
int bd_normal_nll(const float* pred, int ldp, const float* target, int ldt, int rows, int D,
                  float grad_scale, float* dpred, int ldd, float* scalars, int slot, float* ws, void* stream);
/* Dreamer._discount_loss (src/dreamer.py:239-251, use_discount=True): RAW sum over n elements of
 * -log Bernoulli(logits).prob(target) into scalars[slot]; dlogits (may be NULL) = (sigmoid(logit) - target) * grad_scale. */
int bd_bernoulli_nll(const float* logits, const float* target, size_t n, float grad_scale, float* dlogits, float* scalars,
                     int slot, float* ws, void* stream);

/* balanced form (sum_form=0): scalars[slot] = sum of elementwise KL(N(qm,qs) || N(pm,ps));
 * summed form  (sum_form=1, kl_balance == -1): scalars[slot] = sum_rows max(sum_S KL, free_nats) */
int bd_kl_forward(const float* qm, const float* qs, const float* pm, const float* ps, int rows, int S,
                  float free_nats, int sum_form, float* scalars, int slot, float* ws, void* stream);
/* Gradients of weight * kl_loss.  Balanced: the clamp decision uses mean = scalars[slot] * inv_count
 * (inv_count = 1 / global element count, after any all-reduce of the slot). */
int bd_kl_backward(const float* qm, const float* qs, const float* pm, const float* ps, int rows, int S,
                   float free_nats, float kl_balance, float weight, float inv_count, const float* scalars,
                   int slot, float* dqm, float* dqs, float* dpm, float* dps, void* stream);
/* scalars[slot] = sum(x) / sum(x^2) */
int bd_sum(const float* x, size_t n, float* scalars, int slot, float* ws, void* stream);
int bd_sumsq(const float* x, size_t n, float* scalars, int slot, float* ws, void* stream);

/* ---- clip_grad_norm_ + Adam (src/dreamer.py:299-302,362-367,386-391; torch.optim.Adam with
 *      weight_decay = L2-in-gradient).  total_norm = sqrt(scalars[sqnorm_slot]); the gradient buffer
 *      is left clipped, as the reference leaves .grad. */
int bd_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float max_norm, const float* scalars,
                 int sqnorm_slot, void* stream);
/* polyak_update (src/utils.py:56-78): target = src*weight + target*(1-weight) */
int bd_polyak(float* target, const float* src, size_t n, float weight, void* stream);

/* ---- replay gather: ExperienceReplay._retrieve_batch (src/memory.py:70-85) --------------------- */
int bd_replay_gather(const float* src, const int64_t* idx, int n_idx, int width, float* dst, void* stream);

/* pixel replay: gather uint8 frames (pixels bytes per row, multiple of 4) and dequantise in one pass:
 * out = floor(u8 / 2^(8-bits)) / 2^bits - 0.5 + noise / 2^bits  (preprocess_observation_, src/utils.py:299-317;
 * noise ~ U[0,1) is an explicit [n_idx x pixels] input) */
int bd_replay_gather_pixels(const unsigned char* src, const int64_t* idx, int n_idx, int pixels, int bit_depth,
                            const float* noise, float* dst, void* stream);
/* The same with the dequantisation noise U[0, 1) drawn in the kernel (Philox4x32-10, csrc/bd_rng.h; stream 6 of `seed`,
 * counter = element quad, `step`): perf mode -- no noise tensor, no library RNG launch. */
int bd_replay_gather_pixels_rng(const unsigned char* src, const int64_t* idx, int n_idx, int pixels, int bit_depth,
                                unsigned long long seed, unsigned long long step, float* dst, void* stream);

/* ---- replay append: ExperienceReplay.append (src/memory.py:33-49) for n environments at once (csrc/replay.hip) ----
 * ONE launch writes n transitions into the device mirror of the replay buffer: transition i goes to row rows[i] of the
 * four arrays.  The sources are read where they already are on the device -- the observation batch uploaded for the
 * encoder, the action the acting step returned.
 *   bit_depth = 0: state observations, obs [n x obs_width] fp32 copied into dst_obs (float [size x obs_width]);
 *   bit_depth = 1 .. 8: pixels, obs [n x obs_width] fp32 in [-0.5, 0.5] (NCHW, obs_width = 3*64*64), dst_obs unsigned
 *     char [size x obs_width]; a byte is uint8(clip(floor((v + 0.5) * 2^bits) * 2^(8 - bits), 0, 255)), every operation
 *     rounded to fp32 on its own (postprocess_observation, src/utils.py:320-337): bit for bit what the host path stores.
 *     obs_width is a multiple of 4, obs 16-byte and dst_obs 4-byte aligned (four values per lane, one dword store).
 * The caller guarantees distinct rows.  A row outside [0, size) writes nothing (a guard: there is no device-side error
 * word).  Asynchronous on `stream`; never allocates, never synchronises.  1 <= n <= 4096. */
typedef struct {
    int n;                       /* transitions in this call */
    int size;                    /* rows of the mirror */
    const int32_t* rows;         /* [n] destination row of each transition */
    const float* obs;            /* [n x obs_width] */
    int obs_width;
    int bit_depth;               /* 0: fp32 copy; 1 .. 8: quantise to bytes */
    void* dst_obs;               /* float* (bit_depth = 0) or unsigned char* [size x obs_width] */
    const float* act;            /* [n x A] */
    int A;
    float* dst_act;              /* [size x A] */
    const float* reward;         /* [n] */
    const float* nonterminal;    /* [n] */
    float* dst_reward;           /* [size] */
    float* dst_nonterminal;      /* [size] */
} bd_replay_append_args;
int bd_replay_append(const bd_replay_append_args* a, void* stream);

/* ---- replay sample: ExperienceReplay.sample (src/memory.py:51-104) drawn AND gathered on the device (csrc/replay.hip) ----
 * ONE launch draws n chunks of L consecutive rows from the device mirror and writes them time-major (output row t * n + b)
 * into the four destinations: no host RNG, no index upload.
 *   The ring of a chunk has R = size rows (lanes = 1) or lane_size rows (lanes > 1, lane e = rows [e * R, (e + 1) * R));
 *   idx is the write head inside the ring.  The reference's rule -- a uniform start, redrawn while the head is among rows
 *   1 .. L-1 of the chunk -- accepts one cyclic range of starts, so sequence b draws
 *     x       = philox4x32_10(ctr = (b, 0, 12, step lo 32), key = (seed lo, seed hi))          (stream 12, "replay_sample")
 *     lane    = (x[0] * lanes) >> 32
 *     u       = ((x[2] | x[3] << 32) * n_valid) >> 64
 *     not full: n_valid = idx - L,      start = u                      (needs idx > L)
 *     full:     n_valid = R - L + 1,    start = (idx + u) mod R        (needs R >= L)
 *   and takes rows lane * R + (start + t) mod R, t = 0 .. L-1.
 *   bit_depth = 0: state observations, obs float [size x obs_width], copied;
 *   bit_depth = 1 .. 8: pixels, obs unsigned char [size x obs_width] (obs_width a multiple of 4, obs 4-byte and dst_obs
 *     16-byte aligned), dequantised as bd_replay_gather_pixels_rng does with (pix_seed, pix_step): bit for bit what that
 *     entry point writes from the same rows.
 * Every destination element is written exactly once; idx_out (may be NULL) receives the rows drawn.  Asynchronous on
 * `stream`; never allocates, never synchronises.  1 <= n <= 4096, 1 <= L <= R. */
typedef struct {
    const void* obs;             /* mirror: float* (bit_depth = 0) or unsigned char* [size x obs_width] */
    const float* act;            /* [size x A] */
    const float* reward;         /* [size] */
    const float* nonterminal;    /* [size] */
    int obs_width;
    int A;
    int size;                    /* rows of the mirror */
    int lanes;
    int lane_size;
    int idx;                     /* write head inside the ring */
    int full;
    int n;                       /* sequences */
    int L;                       /* chunk length */
    int bit_depth;               /* 0: fp32 copy; 1 .. 8: dequantise bytes */
    unsigned long long seed;     /* sampler key */
    unsigned long long step;     /* sampler counter (low 32 bits used) */
    unsigned long long pix_seed; /* pixels: key and counter of the dequantisation noise (stream 6) */
    unsigned long long pix_step;
    float* dst_obs;              /* [L*n x obs_width] */
    float* dst_act;              /* [L*n x A] */
    float* dst_reward;           /* [L*n] */
    float* dst_nonterminal;      /* [L*n] */
    int64_t* idx_out;            /* [L*n] rows drawn, element t * n + b; NULL: not written */
} bd_replay_sample_args;
int bd_replay_sample_gather(const bd_replay_sample_args* a, void* stream);

size_t bd_reduce_ws_floats(void);

/* ---- replica fingerprint (csrc/fingerprint.hip): are two sets of fp32 buffers bit-identical, and is anything non-finite?
 * For each of n_buf <= BD_FP_MAX_BUFFERS buffers, ONE launch (plus a memset of `out`) writes two words to device memory,
 * out[2 b] = hash and out[2 b + 1] = nonfinite.  For element i (0-based, 64-bit) with 32-bit pattern u, arithmetic mod 2^64:
 *     x = u64(u) ^ ((i + 1) * 0x9E3779B97F4A7C15)
 *     x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9
 *     x = (x ^ (x >> 27)) * 0x94D049BB133111EB
 *     x =  x ^ (x >> 31)
 *     hash      = sum of x over the buffer
 *     nonfinite = number of i with (u & 0x7F800000) == 0x7F800000          (+-Inf and NaNs of any payload)
 * Over bit patterns on purpose: -0.0 and +0.0, or two NaN payloads, differ.  The mixer is a bijection of u for a fixed i, so
 * a change of one element always changes the hash.  The sum is commutative: the words do not depend on scheduling.
 * A buffer needs 4-byte alignment only; n = 0 is legal (p may be NULL then) and gives (0, 0).  Asynchronous on `stream`;
 * never allocates, never synchronises.  Bad arguments are refused before anything is enqueued. */
#define BD_FP_MAX_BUFFERS 16
typedef struct {
    int n_buf;
    struct {
        const float* p;
        size_t n;                 /* elements */
    } buf[BD_FP_MAX_BUFFERS];
} bd_fingerprint_args;
int bd_fingerprint(const bd_fingerprint_args* a, unsigned long long* out, void* stream);

/* ---- training diagnostics (csrc/diag.hip): statistics of buffers a train step holds anyway, reduced on the device.
 * Common to the four entry points: asynchronous on `stream`, never allocate, never synchronise; bad arguments are refused
 * before anything is enqueued.  Deterministic: every workgroup writes fp64 partials into `ws`, a second launch combines them
 * in a fixed order (no floating-point atomics).  Per-element terms are fp32 with the formulas of the loss kernels
 * (bd_kl_forward, bd_kl_categorical_forward), accumulation is fp64, results are doubles; nothing but `out`, `colsum`, `used`
 * and `ws` is written.  fp32 inputs need 4-byte alignment, `out` / `colsum` / `ws` 8-byte alignment.
 * ws: bd_diag_ws_floats() floats, private to the stream while a call is in flight.
 *
 * A "moments sextuple" of a set of fp32 values is six doubles: the number of finite values, their sum, their sum of squares
 * (each square formed in fp64), their minimum (+Inf if none), their maximum (-Inf if none), and the number of non-finite values. */
size_t bd_diag_ws_floats(void);

/* bd_moments: out[6 b ..] = sextuple of entry b, b < n_buf <= BD_MOMENTS_MAX_BUFFERS.  Element i of an entry is p[i], or the
 * fp32 difference p[i] - q[i] when q is not NULL.  n = 0 is legal (p may be NULL) and gives 0, 0, 0, +Inf, -Inf, 0. */
#define BD_MOMENTS_MAX_BUFFERS 16
#define BD_MOMENTS_WORDS 6
typedef struct {
    int n_buf;
    struct {
        const float* p;
        const float* q;           /* NULL: the values are p[i] */
        size_t n;                 /* elements */
    } buf[BD_MOMENTS_MAX_BUFFERS];
} bd_moments_args;
int bd_moments(const bd_moments_args* a, double* out, float* ws, void* stream);

/* bd_latent_stats: Gaussian posterior N(qm, qs) and prior N(pm, ps), each [rows x S] dense.  out (BD_LATENT_WORDS doubles):
 *   out[0] = sum over rows and j of 0.5 ln(2 pi e) + ln qs            (posterior entropy)
 *   out[1] = the same for ps                                          (prior entropy)
 *   out[2] = sum over rows and j of KL_j = ln(ps / qs) + (qs^2 + (qm - pm)^2) / (2 ps^2) - 1/2    (raw: no free nats, no balancing)
 *   out[3..8] = sextuple of qs, out[9..14] = sextuple of ps
 * colsum[j] = sum over rows of KL_j (S doubles). */
#define BD_LATENT_WORDS 15
int bd_latent_stats(const float* qm, const float* qs, const float* pm, const float* ps, int rows, int S, double* out,
                    double* colsum, float* ws, void* stream);

/* bd_latent_stats_categorical: logits [rows x D x C] of posterior q and prior p (softmax per factor), 1 <= C <= 128 as
 * bd_kl_categorical_forward.  out (BD_LATENT_CAT_WORDS doubles), each a sum over rows and factors d:
 *   out[0] = H(q_d), out[1] = H(p_d), out[2] = KL(q_d || p_d) (0 ln 0 = 0), out[3] = max_c q, out[4] = max_c p
 * colsum[d] = sum over rows of KL(q_d || p_d) (D doubles).  used[d C + c] (D*C 32-bit words) is 1 iff some row's posterior
 * argmax of factor d is class c (the first maximum wins on ties), else 0. */
#define BD_LATENT_CAT_WORDS 5
int bd_latent_stats_categorical(const float* post_logits, const float* prior_logits, int rows, int D, int C, double* out,
                                double* colsum, unsigned* used, float* ws, void* stream);

/* bd_segment_sumsq: out[s] = sum of x[i]^2 (squares in fp64) over offsets[s] <= i < offsets[s + 1], s < n_seg <=
 * BD_SEGMENTS_MAX.  `offsets` is a HOST array of n_seg + 1 non-decreasing element indices (read before the call returns);
 * empty segments give 0. */
#define BD_SEGMENTS_MAX 32
int bd_segment_sumsq(const float* x, int n_seg, const size_t* offsets, double* out, float* ws, void* stream);

/* ---- percentile return normalisation (csrc/retnorm.hip; ActorCritic.return_normalization = percentile) -----------
 * bd_return_range: ONE launch.  With the M fp32 `returns` sorted ascending (-0.0 and +0.0 are one value), p_lo and p_hi
 * are elements k_lo and k_hi (0 <= k_lo <= k_hi < M), selected exactly by radix selection with integer counts: the same
 * bits whatever the schedule.  state = four doubles on the device, {lo, hi, count, skipped}:
 *     count == 0:  lo = p_lo, hi = p_hi;      else  lo = decay lo + (1 - decay) p_lo,  hi likewise   (fp64, each product
 *     and the sum rounded once);  count += 1.
 * If any return is NaN or +-Inf nothing changes but skipped += 1.  Then, from the state as it now stands,
 *     range[0] = (float) max(floor, hi - lo)   (the scale of the NEXT step),   range[1] = (float) lo,   range[2] = (float) hi.
 * 0 <= decay < 1, floor > 0.  returns / range need 4-byte alignment, state 8-byte.  One workgroup, no global workspace.
 * Asynchronous on `stream`; never allocates, never synchronises; bad arguments are refused before anything is enqueued. */
int bd_return_range(const float* returns, int M, int k_lo, int k_hi, double decay, double floor_, double* state,
                    float* range, void* stream);
/* bd_return_seed: the gradient seed of the normalised dynamics term, dreturns[i] = (dret_const / range[0]) * weight[i]
 * (weight = NULL: 1), i < n, for bd_lambda_return_backward; and, scalars != NULL, scalars[slot .. slot + 2] = range[0 .. 2]
 * (the scale and the range the step uses, for its logs).  n = 0 (dreturns may be NULL) only copies. */
int bd_return_seed(const float* range, float dret_const, const float* weight, size_t n, float* dreturns, float* scalars,
                   int slot, void* stream);

/* ---- two-hot critic head in symlog space (csrc/twohot.hip; ActorCritic.critic_head = twohot) ---------------------
 * A row holds K logits l_0 .. l_{K-1} (2 <= K <= 1024) over bins that are uniform in symlog space,
 *     z_i = -Z + i delta,  delta = 2 Z / (K - 1),  Z = zmax in (0, 80]       (formed as (2 i - (K - 1)) Z / (K - 1), so
 *     that z_i = -z_{K-1-i} exactly; computed in the kernel, never read),
 * with symlog(y) = sign(y) log1p(|y|) and symexp(z) = sign(z) expm1(|z|).
 * bd_twohot_decode:   p = softmax(l) (maximum subtracted),  m = sum_i p_i z_i,  value[r] = symexp(m),  mean[r] = m (mean
 *     may be NULL).
 * bd_twohot_decode_backward:   dlogits[r, i] = dvalue[r] exp(|m|) p_i (z_i - m)   (stored).
 * bd_twohot_nll: target y = target[r], row weight w_r = weight[r] (weight NULL: 1):
 *     t = clamp(symlog(y), -Z, Z),  u = (t + Z) / delta,  k = min(floor(u), K - 2),  w = u - k,  q_k = 1 - w,  q_{k+1} = w,
 *     row_loss[r] = w_r (logsumexp(l) - (1 - w) l_k - w l_{k+1}),    dlogits[r, i] = grad_scale w_r (p_i - q_i)   (stored),
 *     value[r] = symexp(m) of the same logits (value may be NULL).
 *   The row L1 norm of dlogits is at most 2 grad_scale w_r whatever the target.  A NaN target gives a NaN row_loss.
 * logits / dlogits are row-major with leading dimensions ld, ldd >= K; nothing beyond column K of a row or beyond row
 * `rows` is written, every output element exactly once.  One wave per row, the sums of a row in a fixed order: the same
 * bits on every launch.  4-byte alignment.  Asynchronous on `stream`; never allocate, never synchronise; bad arguments
 * (NULLs, ld < K, K or zmax outside the ranges above, rows <= 0) are refused before anything is enqueued. */
int bd_twohot_decode(const float* logits, int ld, int rows, int K, float zmax, float* value, float* mean, void* stream);
int bd_twohot_decode_backward(const float* logits, int ld, const float* dvalue, int rows, int K, float zmax, float* dlogits,
                              int ldd, void* stream);
int bd_twohot_nll(const float* logits, int ld, const float* target, const float* weight, int rows, int K, float zmax,
                  float grad_scale, float* dlogits, int ldd, float* value, float* row_loss, void* stream);

/* ---- symlog / symexp of a flat fp32 array (csrc/symlog.hip; symlog_observations) -----------------------------------
 * bd_symlog: out[i] = sign(x[i]) log1p(|x[i]|);   bd_symexp: out[i] = sign(x[i]) expm1(|x[i]|),   0 <= i < n.
 * Precise log1pf / expm1f under copysignf: +-0 -> +-0, f(-x) = -f(x) bit for bit, NaN -> NaN, +-inf -> +-inf; symexp
 * overflows to +-inf where expm1f does (|x| above about 88.72).
 * Out of place: out == x, or any other overlap of the two arrays, is refused.  4-byte alignment; where x and out sit at
 * the same offset from a 16-byte boundary the body moves as 16-byte loads and stores, with a dword path for the head up
 * to the boundary and for the tail, else every element takes the dword path.  Every output element is written exactly
 * once, nothing before out[0] or from out[n] on.  No LDS, no atomics.  Asynchronous on `stream`; never allocate, never
 * synchronise; NULLs, n = 0 and overlapping arrays are refused before anything is enqueued. */
int bd_symlog(const float* x, size_t n, float* out, void* stream);
int bd_symexp(const float* x, size_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BIGDREAMER_HIP_H */
