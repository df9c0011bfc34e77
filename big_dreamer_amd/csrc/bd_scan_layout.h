// bd_scan_layout.h -- the ONE place that knows how the recurrent scan kernels cut their dynamic LDS into regions and how the
// cluster forms cut their exchange workspace.  A kernel takes its pointers as `smem + L.region`, its launcher asks for
// `L.total` floats, bd_scan_lds_bytes reports the same figure to the tests: the three cannot drift apart.
//
// Every layout is a plain struct built from the shape: offsets in floats, regions in address order, `total` behind the last
// one.  vec_ok() is true when every region that is read or written as float4 (fragment tiles, split-K partials, logit
// images) starts on a multiple of 4 floats; each launcher requires it.  A region with several tenants (disjoint phases of a
// step) is sized by lds_max over its NAMED tenants: a new tenant is one more argument in one place.
//
// Some kernels chain their pointers off one another, `b = a + (L.b - L.a)`, where the others write `smem + L.b`: the same
// addresses.  hipcc's register allocation and its packing / contraction of the heads' float arithmetic follow the shape of
// the address expressions, and the chained form is the one those kernels were compiled from before (equal VGPR counts and
// equal float instruction mix, hence equal bits).  Either form reads every offset from the layout.
//
// kWaves is a property of the translation unit (BD_WAVES): the figures are those of the scan kernels only in a unit built
// with the scans' wave count -- every user of this header is.
#pragma once
#include "bd_scan.h"
#include "bd_categorical.h"

namespace bd {

constexpr int kMaxCluster = 16;
constexpr int kLocalBlocks = 2;             // column blocks a cluster member owns at most (host picks C accordingly)

__host__ __device__ constexpr int lds_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ constexpr int lds_max(int a, int b, int c) { return lds_max(lds_max(a, b), c); }
__host__ __device__ constexpr int lds_round4(int n) { return (n + 3) & ~3; }

// ---- scratch tenants ---------------------------------------------------------------------------------------------------------
// kSplitScratchFloats: split-K partials + the plain image of tile_dual_head_elem (bd_device.h); kSplitPartialFloats: the
// partials alone, all a kernel without an element-wise Gaussian head needs.
constexpr int kGruPartFwdFloats = kWaves * kLocalBlocks * 4 * kFragFloats;   // cluster GRU: [wave][block][R, Z, NI, NH][64][4]
constexpr int kGruPartBwdFloats = kWaves * kLocalBlocks * 2 * kFragFloats;   // cluster GRU dgrad: [wave][block][DX, DH][64][4]

// observe_fwd_kernel: the split-K scratch alone.  observe_cfwd_kernel: GRU partials | split-K scratch (constants: the GRU
// partials decide, 16384 against 10240 floats at 8 waves).
constexpr int kObsFwdScratch = kSplitScratchFloats;
constexpr int kObsCfwdScratch = lds_max(kGruPartFwdFloats, kSplitScratchFloats);
// observe_bwd_kernel uses the partials only; its launcher has always asked for the forward's figure: kHeadPlainFloats of slack.
constexpr int kObsBwdScratch = kSplitPartialFloats + kHeadPlainFloats;
constexpr int kObsCbwdScratch = lds_max(kGruPartBwdFloats, kSplitPartialFloats);   // (equal at 8 waves)
// Categorical cluster forms: GRU partials | split-K partials of the member's own `nbl` logit blocks | split-K scratch.
// nbl <= 8 (kCatOwnBlocks).  Forward: the GRU partials decide at every nbl (the head reaches them at nbl = 8).  Backward: the
// scratch decides up to nbl = 5 (c32_d32 at Cm = 16), the head from nbl = 6 (c32_d32 at Cm = 8); the GRU partials never do.
__host__ __device__ constexpr int cat_cluster_scratch(int nbl, bool fwd) {
    return lds_max(fwd ? kGruPartFwdFloats : kGruPartBwdFloats, kWaves * nbl * kFragFloats, kSplitScratchFloats);
}

// ---- Gaussian latents ------------------------------------------------------------------------------------------------------------
// observe_fwd_kernel (scratch = kObsFwdScratch), observe_cfwd_kernel (kObsCfwdScratch)
struct ObserveFwdLds {
    int h_cur, h_nxt, xf, qf, sf, af;   // fragment tiles: Kb_h, Kb_h, Kb_h, Kb_hd, Kb_s, Kb_a blocks
    int s_plain;                        // [16][S] unmasked posterior state of the previous step
    int scratch, total;
    __host__ __device__ __forceinline__ ObserveFwdLds(const ScanDims& d, int S, int scratch_floats) {
        const int nh = d.Kb_h * kFragFloats;
        h_cur = 0;
        h_nxt = h_cur + nh;
        xf = h_nxt + nh;
        qf = xf + nh;
        sf = qf + d.Kb_hd * kFragFloats;
        af = sf + d.Kb_s * kFragFloats;
        s_plain = af + d.Kb_a * kFragFloats;
        scratch = s_plain + 16 * S;
        total = scratch + scratch_floats;
    }
    __host__ __device__ bool vec_ok() const { return ((h_cur | h_nxt | xf | qf | sf | af | scratch) & 3) == 0; }
};

// observe_bwd_kernel (scratch = kObsBwdScratch), observe_cbwd_kernel (kObsCbwdScratch)
struct ObserveBwdLds {
    int dhc, dE;                        // Kb_h blocks each, CONTIGUOUS: the cluster form exchanges [dhc | dE] as one payload
    int dR, dZ, dNI, dNH;               // Kb_h blocks each
    int dQ, dM, dRaw;                   // Kb_hd, Kb_s, Kb_s blocks
    int ds_plain;                       // [16][S] carry: d loss / d posterior_state_t
    int scratch, total;
    __host__ __device__ __forceinline__ ObserveBwdLds(const ScanDims& d, int S, int scratch_floats) {
        const int nh = d.Kb_h * kFragFloats, ns = d.Kb_s * kFragFloats;
        dhc = 0;
        dE = dhc + nh;
        dR = dE + nh;
        dZ = dR + nh;
        dNI = dZ + nh;
        dNH = dNI + nh;
        dQ = dNH + nh;
        dM = dQ + d.Kb_hd * kFragFloats;
        dRaw = dM + ns;
        ds_plain = dRaw + ns;
        scratch = ds_plain + 16 * S;
        total = scratch + scratch_floats;
    }
    __host__ __device__ bool vec_ok() const { return ((dhc | dE | dR | dZ | dNI | dNH | dQ | dM | dRaw | scratch) & 3) == 0; }
};

// observe_kfwd_ns_kernel
struct KsplitFwdLds {
    int sf, af;                         // Kb_s, Kb_a fragment blocks
    int s_plain;                        // [16][S] rounded up to whole float4s: the kernel no longer touches it (the state stays
                                        // in fragment order); kept as slack so that the launch's request does not move
    int red;                            // [2][kWaves][64][4]: the two reductions of a step alternate
    int plain;                          // [nparts][2][16][16 Kb_s] head sums, one copy per helper wave group
    int xf, hf;                         // x and h, all Kb_h blocks
    int gpart;                          // [kWaves][4 gates][64][4]: the waves' K-partial gate sums
    int total;
    // head sums of the nparts = kWaves / (2 Kb_s) wave groups: nparts * 2 Kb_s blocks, which the division keeps at or below
    // kWaves blocks for every Kb_s (equal for Kb_s in {1, 2, 4}: every shape ksplit_ok admits; 6 of 8 for Kb_s = 3)
    static constexpr int kPlainFloats = kWaves * kFragFloats;
    __host__ __device__ __forceinline__ KsplitFwdLds(const ScanDims& d, int S) {
        sf = 0;
        af = sf + d.Kb_s * kFragFloats;
        s_plain = af + d.Kb_a * kFragFloats;
        red = s_plain + lds_round4(16 * S);
        plain = red + 2 * kWaves * kFragFloats;
        xf = plain + kPlainFloats;
        hf = xf + d.Kb_h * kFragFloats;
        gpart = hf + d.Kb_h * kFragFloats;
        total = gpart + kWaves * 4 * kFragFloats;
    }
    __host__ __device__ bool vec_ok() const { return ((sf | af | red | plain | xf | hf | gpart) & 3) == 0; }
};

// observe_kbwd_kernel
struct KsplitBwdLds {
    int dM, dRaw;                       // Kb_s fragment blocks each
    int ds_plain, dsp_stride, nparts;   // [nparts][16][S] d state of the next step, one partial sum per wave group (stride: whole float4s)
    int red;                            // [2][kWaves][64][4]
    int total;
    __host__ __device__ __forceinline__ KsplitBwdLds(const ScanDims& d, int S) {
        nparts = kWaves / d.Kb_s;       // wave w: state block w % Kb_s, members part = w / Kb_s, part + nparts, ...
        dsp_stride = lds_round4(16 * S);
        dM = 0;
        dRaw = dM + d.Kb_s * kFragFloats;
        ds_plain = dRaw + d.Kb_s * kFragFloats;
        red = ds_plain + nparts * dsp_stride;
        total = red + 2 * kWaves * kFragFloats;
    }
    __host__ __device__ bool vec_ok() const { return ((dM | dRaw | ds_plain | dsp_stride | red) & 3) == 0; }
};

// imagine_fwd_kernel
struct ImagineFwdLds {
    int h_cur, h_nxt, xf, bufA, bufB, sf, af;   // fragment tiles: Kb_h x 3, Kb_hd x 2, Kb_s, Kb_a blocks
    int mean_s, std_s, lp_rj;                   // [16][A] each
    int part;                                   // [kWaves][16][A][3] entropy partial sums
    int scratch, total;                         // split-K scratch (kSplitScratchFloats)
    // discrete (the Categorical actor): mean_s holds the logits image and nothing reads std_s, lp_rj or part, so the scratch
    // starts where std_s would (432 A floats less: A = 64 fits the CU's 160 KiB, which it never does with them)
    __host__ __device__ __forceinline__ ImagineFwdLds(const ScanDims& d, int A, bool discrete = false) {
        const int nh = d.Kb_h * kFragFloats, nhd = d.Kb_hd * kFragFloats;
        h_cur = 0;
        h_nxt = h_cur + nh;
        xf = h_nxt + nh;
        bufA = xf + nh;
        bufB = bufA + nhd;
        sf = bufB + nhd;
        af = sf + d.Kb_s * kFragFloats;
        mean_s = af + d.Kb_a * kFragFloats;
        std_s = mean_s + 16 * A;
        lp_rj = std_s + 16 * A;
        part = lp_rj + 16 * A;
        scratch = discrete ? std_s : part + kWaves * 16 * A * 3;
        total = scratch + kSplitScratchFloats;
    }
    __host__ __device__ bool vec_ok() const { return ((h_cur | h_nxt | xf | bufA | bufB | sf | af | scratch) & 3) == 0; }
};

// imagine_bwd_kernel
struct ImagineBwdLds {
    int dhc, dR, dZ, dNI, dNH, dE;              // Kb_h blocks each
    int dP, bufA, bufB;                         // Kb_hd blocks each
    int dM, dRaw, dAm, dAr;                     // Kb_s, Kb_s, Kb_a, Kb_a blocks
    int ds_plain;                               // [16][S]
    int scratch, total;                         // split-K partials (no element-wise Gaussian head: kSplitPartialFloats)
    __host__ __device__ __forceinline__ ImagineBwdLds(const ScanDims& d, int S) {
        const int nh = d.Kb_h * kFragFloats, nhd = d.Kb_hd * kFragFloats, ns = d.Kb_s * kFragFloats, na = d.Kb_a * kFragFloats;
        dhc = 0;
        dR = dhc + nh;
        dZ = dR + nh;
        dNI = dZ + nh;
        dNH = dNI + nh;
        dE = dNH + nh;
        dP = dE + nh;
        bufA = dP + nhd;
        bufB = bufA + nhd;
        dM = bufB + nhd;
        dRaw = dM + ns;
        dAm = dRaw + ns;
        dAr = dAm + na;
        ds_plain = dAr + na;
        scratch = ds_plain + 16 * S;
        total = scratch + kSplitPartialFloats;
    }
    __host__ __device__ bool vec_ok() const {
        return ((dhc | dR | dZ | dNI | dNH | dE | dP | bufA | bufB | dM | dRaw | dAm | dAr | scratch) & 3) == 0;
    }
};

// ---- Categorical latents ----------------------------------------------------------------------------------------------------------
// observe_cat_fwd_kernel (image = CatFull(D, C): all factors, no scratch), observe_cat_cfwd_kernel (image = CatFull(D / Cm, C):
// the member's own factors; scratch = cat_cluster_scratch(nbl, true)).  The geometry objects come from the caller: the
// kernels hold one already, and a second construction is a second out-of-line call in the largest of them.
struct CatObserveFwdLds {
    int h_cur, h_nxt, xf, qf, af;       // fragment tiles: Kb_h x 3, Kb_hd, Kb_a blocks
    int xs;                             // [16][Be] gathered W_es s~
    int lg;                             // logits of the `image` factors
    int sw_l, mrow, sidx_l;             // [16][D] factor weights, [16] nonterminal mask, [16][D] class indices (int)
    int scratch, total;
    __host__ __device__ __forceinline__ CatObserveFwdLds(const ScanDims& d, int Be, int D, const CatFull& image, int scratch_floats) {
        const int nh = d.Kb_h * kFragFloats;
        h_cur = 0;
        h_nxt = h_cur + nh;
        xf = h_nxt + nh;
        qf = xf + nh;
        af = qf + d.Kb_hd * kFragFloats;
        xs = af + d.Kb_a * kFragFloats;
        lg = xs + 16 * Be;
        sw_l = lg + image.image_floats();
        mrow = sw_l + 16 * D;
        sidx_l = mrow + 16;
        scratch = sidx_l + 16 * D;
        total = scratch + scratch_floats;
    }
    __host__ __device__ bool vec_ok() const { return ((h_cur | h_nxt | xf | qf | af | xs | lg | scratch) & 3) == 0; }
};

// observe_cat_bwd_kernel (g = CatGeo(D, C), no scratch), observe_cat_cbwd_kernel (g = CatGeo(D / Cm, C): one chunk, scratch =
// cat_cluster_scratch(nbl, false))
struct CatObserveBwdLds {
    int dhc, dE;                        // Kb_h blocks each, CONTIGUOUS: the cluster form exchanges [dhc | dE] as one payload
    int dR, dZ, dNI, dNH;               // Kb_h blocks each
    int dQ;                             // Kb_hd blocks
    int pl, lgs;                        // one chunk image of `g` each: g then d logits | logits
    int dLf;                            // the chunk's d logits as CW / 16 fragment blocks
    int mrow;                           // [16]
    int scratch, total;
    __host__ __device__ __forceinline__ CatObserveBwdLds(const ScanDims& d, const CatGeo& g, int scratch_floats) {
        const int nh = d.Kb_h * kFragFloats;
        dhc = 0;
        dE = dhc + nh;
        dR = dE + nh;
        dZ = dR + nh;
        dNI = dZ + nh;
        dNH = dNI + nh;
        dQ = dNH + nh;
        pl = dQ + d.Kb_hd * kFragFloats;
        lgs = pl + g.image_floats();
        dLf = lgs + g.image_floats();
        mrow = dLf + (g.CW / 16) * kFragFloats;
        scratch = mrow + 16;
        total = scratch + scratch_floats;
    }
    __host__ __device__ bool vec_ok() const { return ((dhc | dE | dR | dZ | dNI | dNH | dQ | pl | lgs | dLf | scratch) & 3) == 0; }
};

// imagine_cat_fwd_kernel
struct CatImagineFwdLds {
    int h_cur, h_nxt, xf, bufA, bufB, af;       // fragment tiles: Kb_h x 3, Kb_hd x 2, Kb_a blocks
    int xs;                                     // [16][max(Be, Hd)] gathered state columns of the layer at hand
    int mean_s, std_s, lp_rj;                   // [16][A] each
    int sw_l, sidx_l;                           // [16][D] each (sidx_l: int)
    // one region, three tenants in disjoint phases.  Which decides: the split-K scratch at every narrow shape (n1_h1), the
    // entropy sums from A = 27 on narrow latents (a28), the logit image above S = 624 (c32_d32_a17).
    int uni;
    int scratch;                                // = uni: the actor head's split-K scratch (kSplitScratchFloats)
    int part;                                   // = uni: [kWaves][16][A][3] entropy partial sums
    int lg;                                     // = uni: all S prior logits of the tile (CatFull image)
    int total;
    __host__ __device__ __forceinline__ CatImagineFwdLds(const ScanDims& d, int Be, int Hd, int D, int A, const CatFull& image) {
        const int nh = d.Kb_h * kFragFloats, nhd = d.Kb_hd * kFragFloats;
        h_cur = 0;
        h_nxt = h_cur + nh;
        xf = h_nxt + nh;
        bufA = xf + nh;
        bufB = bufA + nhd;
        af = bufB + nhd;
        xs = af + d.Kb_a * kFragFloats;
        mean_s = xs + 16 * lds_max(Be, Hd);
        std_s = mean_s + 16 * A;
        lp_rj = std_s + 16 * A;
        sw_l = lp_rj + 16 * A;
        sidx_l = sw_l + 16 * D;
        uni = sidx_l + 16 * D;
        scratch = part = lg = uni;
        total = uni + lds_max(kSplitScratchFloats, kWaves * 16 * A * 3, image.image_floats());
    }
    __host__ __device__ bool vec_ok() const { return ((h_cur | h_nxt | xf | bufA | bufB | af | xs | uni) & 3) == 0; }
};

// imagine_cat_bwd_kernel
struct CatImagineBwdLds {
    int dhc, dR, dZ, dNI, dNH, dE;              // Kb_h blocks each
    int dP, dAm, dAr;                           // Kb_hd, Kb_a, Kb_a blocks
    // one region, three tenants in disjoint phases.  Which decides: the head backward's images above S = 208 (c32_d32_a17,
    // c32_d12, c16_d20), the split-K scratch below (n1_h1); the actor backward's two buffers are at most
    // 2 * 16 blocks = 8192 floats while Hd <= 256 (every launcher requires it) and never reach the scratch's 10240.
    int uni;
    int pl, lgs, dLf;                           // = uni ...: two chunk images and the chunk's d logits as CW / 16 fragment blocks
    int scratch;                                // = uni: split-K scratch (kSplitScratchFloats)
    int bufA, bufB;                             // = uni ...: Kb_hd blocks each
    int total;
    __host__ __device__ __forceinline__ CatImagineBwdLds(const ScanDims& d, const CatGeo& g) {
        const int nh = d.Kb_h * kFragFloats, nhd = d.Kb_hd * kFragFloats, na = d.Kb_a * kFragFloats;
        dhc = 0;
        dR = dhc + nh;
        dZ = dR + nh;
        dNI = dZ + nh;
        dNH = dNI + nh;
        dE = dNH + nh;
        dP = dE + nh;
        dAm = dP + nhd;
        dAr = dAm + na;
        uni = dAr + na;
        pl = uni;
        lgs = pl + g.image_floats();
        dLf = lgs + g.image_floats();
        scratch = uni;
        bufA = uni;
        bufB = bufA + nhd;
        total = uni + lds_max(dLf - uni + (g.CW / 16) * kFragFloats, kSplitScratchFloats, 2 * nhd);
    }
    __host__ __device__ bool vec_ok() const {
        return ((dhc | dR | dZ | dNI | dNH | dE | dP | dAm | dAr | uni | lgs | dLf | bufB) & 3) == 0;
    }
};

// ---- exchange workspace of the cluster forms (floats) ---------------------------------------------------------------------------
// [flags: tiles * kMaxCluster u32][err: 16 u32, sticky][tiles x per-tile payload]; every payload has two copies (step parity).
__host__ __device__ inline size_t cluster_ws_flag_floats(int tiles) { return (size_t)tiles * kMaxCluster; }
__host__ __device__ inline size_t cluster_ws_header_floats(int tiles) { return cluster_ws_flag_floats(tiles) + 16; }

// round-1 Gaussian form (observe_cluster.hip).  Each direction strides the tiles by its own payload.
struct ObsClusterWs {
    size_t fwd_copy, fwd_tile;          // forward: [2][Kb_h blocks] the new belief
    size_t bwd_copy, bwd_tile;          // backward: [2][dhc | dE], as the LDS layout
    size_t per_tile;
    __host__ __device__ __forceinline__ ObsClusterWs(int Kb_h) {
        fwd_copy = (size_t)Kb_h * kFragFloats;
        fwd_tile = 2 * fwd_copy;
        bwd_copy = 2 * (size_t)Kb_h * kFragFloats;
        bwd_tile = 2 * bwd_copy;
        per_tile = fwd_tile > bwd_tile ? fwd_tile : bwd_tile;
    }
};

// K-split Gaussian form (observe_ksplit.hip): exchange buffers of one tile, kKsCopies copies
constexpr int kKsImg = 256;        // an image = the float4 of 64 lanes
constexpr int kKsCopies = 2;
struct KsBuf {
    size_t g, q, s, total;
    __host__ __device__ __forceinline__ KsBuf(int C) {
        g = 0;
        q = g + (size_t)C * C * 4 * kKsImg;     // [dest][src][4][image]: forward belief blocks, backward (DX, DH)
        s = q + (size_t)C * C * kKsImg;         // [dest][src][image]
        total = s + (size_t)C * 8 * kKsImg;     // [src][<= 8 (block, mean | raw) pairs][image]
    }
};

// Categorical form (observe_cat_cluster.hip)
struct CatClusterWs {
    size_t fwd_h, fwd_s, fwd_tile;      // forward: [2][Kb_h blocks] the new belief | [2][16][D] class indices (u32)
    size_t bwd_c, bwd_q, bwd_tile;      // backward: [2][dhc | dE] | [2][Cm][Kb_hd blocks] d hidden partials
    size_t per_tile;
    __host__ __device__ __forceinline__ CatClusterWs(int Kb_h, int Kb_hd, int D, int Cm) {
        const size_t nh = (size_t)Kb_h * kFragFloats, nhd = (size_t)Kb_hd * kFragFloats;
        fwd_h = 0;
        fwd_s = fwd_h + 2 * nh;
        fwd_tile = fwd_s + (size_t)2 * 16 * D;
        bwd_c = 0;
        bwd_q = bwd_c + 2 * (2 * nh);
        bwd_tile = bwd_q + (size_t)2 * Cm * nhd;
        per_tile = fwd_tile > bwd_tile ? fwd_tile : bwd_tile;
    }
};

}  // namespace bd
