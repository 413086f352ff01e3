/*
 * libciaosr_hip.so -- C ABI of the MI355X (gfx950) implementation of CiaoSR's LocalImplicitSR
 * forward path.  Plain pointers and sizes only; no torch types.  Every pointer is a DEVICE
 * pointer unless marked "host".  Every function is asynchronous on `stream` (a hipStream_t passed
 * as void*; NULL = default stream), never allocates persistent device memory (the caller passes
 * a workspace), returns 0 on success or a negative CIAOSR_ERR_* code, and never throws.
 *
 * The reference (caojiezhang/CiaoSR) has no FFI: its hot path is Python nn.Modules.  Each entry
 * point below names the reference code it replaces (paths relative to the reference root):
 *   net  = mmedited/models/backbones/sr_backbones/ciaosr_net.py
 *   csa  = mmedited/models/common/arch_csnln.py
 *   mlp  = mmedited/models/components/refiners/mlp_refiner.py
 *   rest = mmedited/models/restorers/ciaosr.py
 *
 * Device data layout ("device channel order"):
 *   feature maps are channels-last  [H][W][C]  fp32;
 *   an "unfold row" of LR pixel (y,x) is  U[(ki*3+kj)*C + c] = F[y+ki-1][x+kj-1][c]  (0 outside),
 *   i.e. the reference's F.unfold index c*9+ki*3+kj (net:132) permuted to (ki,kj,c) so that one
 *   3x3 tap is C contiguous floats; optionally followed by the Cn non-local channels (net:137).
 *   The host packs MLP weights once with the same permutation (ciaosr_amd/head_hip.py).
 */
#ifndef CIAOSR_HIP_H
#define CIAOSR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIAOSR_OK 0
#define CIAOSR_ERR_BAD_ARG (-1)
#define CIAOSR_ERR_LAUNCH (-2)
#define CIAOSR_ERR_UNSUPPORTED (-3)
#define CIAOSR_ERR_WORKSPACE (-4)

#define CIAOSR_ACT_NONE 0
#define CIAOSR_ACT_RELU 1
#define CIAOSR_ACT_PRELU 2
#define CIAOSR_ACT_GELU 3   /* exact erf form (nn.GELU default); convolution epilogues only */
#define CIAOSR_ACT_SIN 4    /* MLPRefiner(act='sin'), mlp:81-86; ciaosr_gemm_f32 and the staged head route */
#define CIAOSR_ACT_COS 5    /* MLPRefiner(act='cos') */

#define CIAOSR_MAX_LAYERS 8

/* ---- library ---------------------------------------------------------------------------- */
int ciaosr_version(void);
const char* ciaosr_error_string(int code);
/* sizeof() of an ABI struct by its typedef name ("ciaosr_mlp_t", ...), 0 if unknown: layout check for bindings */
size_t ciaosr_sizeof(const char* type_name /*host*/);

/* Opt-in per-kernel HIP-event timing used by bench.py's roofline leg. */
int ciaosr_prof_enable(int on);
int ciaosr_prof_filter(const char* kernel /*host; NULL or "" = all kernels*/);
int ciaosr_prof_reset(void);
int ciaosr_prof_collect(void); /* synchronises the recorded events and accumulates totals */
int ciaosr_prof_get(const char* kernel, double* total_ms /*host*/, long* launches /*host*/);
int ciaosr_prof_names(char* buf /*host*/, int buflen); /* ';'-separated kernel names seen */

/* ---- per-call options --------------------------------------------------------------------
 * The library keeps NO mutable state besides the opt-in profiler above: precision is selected by the entry point's
 * _f32 / _bf16 / _f16 suffix, and every route choice is an argument.  `opt` may be NULL (all defaults); a zero field means
 * "default".  The struct only selects between result-equivalent evaluation routes (tests force each of them). */
#define CIAOSR_HEAD_STAGED 1          /* head_route bit 0: per-layer GEMM path instead of the fused kernels */
#define CIAOSR_HEAD_TABLE_GEMM 4      /* head_route bit 2: _f32 logit table as the 576-deep GEMM of (q*key) rows even when
                                       * ciaosr_head_weights_t.k_out_wino is given */
#define CIAOSR_HEAD_NO_LOGIT_TABLE 2  /* head_route bit 1: fused path, imnet_k output layer on the MFMA per (query, sample)
                                       * row instead of the exact 9-rows-per-LR-pixel fold */
#define CIAOSR_HEAD_WIDE_WG 8         /* head_route bit 3: _f16 entries (f16 / f16-pairs): the fused kernels with ONE 256-row workgroup per CU
                                       * (head_fused_wide.hip: half the weight stream per MFMA) instead of two 128-row workgroups per CU;
                                       * same result up to the fp32 summation order of the logit dot product, measured equal in time
                                       * (f16x3 always runs its 128-row two-array form of that kernel) */
#define CIAOSR_HEAD_TABLE_WINO2 16    /* head_route bit 4: _f32 logit table in Winograd F(2x2, 3x3) form even when k_out_wino4 is given */
#define CIAOSR_HEAD_NO_CHAIN 32       /* head_route bit 5: _bf16 / _f16 entries: the 128-row kernels that stream every weight fragment from L2
                                       * (head_fused_h16.hip) even when ciaosr_head_weights_t.chain16 is given; default = the weights-stationary,
                                       * register-chained kernel (head_chain_h16.hip).  Same products, other fp32 summation order of the logit dot
                                       * product and of z; the tail term of layer 0 enters through the MFMA as hi + lo pairs */
#define CIAOSR_HEAD_NO_DECODE_CHAIN 64 /* head_route bit 6: keep imnet_q on the 128-row kernel while phi_k / phi_v run chained (imnet_q follows the
                                       * chained form where the blob carries its stream: Dv a multiple of 128, four 256-wide layers + the 3-row
                                       * output layer, which then enters the MFMA as a hi + lo pair instead of an fp32 VALU tail) */
/* Precision modes.  The entry suffix, f16_pairs and bf16_single together name one of eight modes; "hi + lo pair" = w as h16(w) +
 * h16(w - h16(w)), two MFMAs per product; "x3" = weights AND activations of the head's three MLP chains as pairs, three MFMAs per
 * product (w_hi a_hi + w_lo a_hi + w_hi a_lo, head_fused_wide_h16.hip), Z in fp32.  Max |delta| against the reference on the full C3
 * tile unless stated.
 *
 *   mode         entry  f16_pairs  bf16_single  trunk dense layers     head                   logit table  hoist  accuracy
 *   fp32         _f32   0          0            fp32                   fp32                   fp32         fp32   the contract precision
 *   bf16         _bf16  0          0            bf16, weight pairs     bf16, weight pairs     bf16         fp32   PSNR-gated
 *   bf16-single  _bf16  0          1            bf16, single weights   bf16, single weights   bf16         fp32   PSNR-gated (0.0004 dB, below)
 *   bf16x3       _bf16  2          0            fp32                   bf16 x3                fp32         fp32   1.8e-4; SwinIR-CiaoSR at BASELINE
 *                                                                                                                 config 5: 9.3e-6
 *   f16          _f16   0          0            half, single weights   half, single weights   half         half   PSNR-gated
 *   f16-pairs    _f16   1          0            half, weight pairs     half, weight pairs     half         fp32   1.04e-3, PSNR-gated
 *   f16x3        _f16   2          0            fp32                   half x3                fp32         fp32   2.7e-5 (rms 2.1e-6)
 *   f16x3-fast   _f16   3          0            half, weight pairs     half x3                fp32         fp32   4.0e-4; 2.7e-2 on trained-like
 *                                                                                                                 trunk statistics: PSNR-gated
 *
 * Trunk dense layers: the RDN's big-map route; its 1x1 fusion layers run in half in f16 only, fp32 elsewhere.  Activations are single
 * 16-bit values outside the x3 heads; cs_attn's contractions run in the entry's element type; "hoist" = the layer-0 tables of the fused
 * head.  Ignored combinations -- accepted, and resolved as listed:
 *   _f32 entries: both fields ignored                                                   -> fp32
 *   _bf16 entries: f16_pairs 1 or 3 ignored                                             -> bf16 / bf16-single by bf16_single
 *                  bf16_single ignored under f16_pairs 2                                -> bf16x3
 *   _f16 entries: bf16_single ignored                                                   -> the mode of f16_pairs
 * Single bf16 weights rounded to nearest fail the 0.01 dB PSNR gate on smooth features (0.042 dB on the full C3 tile: a fixed,
 * spatially coherent perturbation).  A binding that wants bf16-single INSIDE the gate packs the head's weights the way
 * ciaosr_amd/head_hip.py::_build_single does: error-feedback rounding along K (a weight that already is a bf16 number passes through
 * the pack entries unchanged) and bias[i] += (w - w_q) E[x] with the layer's mean input measured once on a calibration image. */
typedef struct ciaosr_options {
    int head_route;         /* CIAOSR_HEAD_* bits; 0 = automatic */
    int csa_composed_min;   /* cs_attn: LR pixels (after padding) from which the composed fold+down tail applies;
                             * 0 = default (4096), < 0 = never */
    int dense_min_tiles;    /* RDN trunk: 12x12-pixel tiles from which the halo-resident dense-layer kernels apply;
                             * 0 = default (128), < 0 = never */
    int scatter_small_max;  /* RDN trunk: largest map (pixels) for the small-map dense-block kernels; 0 = default (18432),
                             * < 0 = never */
    int kv_rows;            /* fp32 fused head: (query, sample) rows per workgroup, 32 or 64; 0 = automatic (64 from 32768 queries) */
    int decode_rows;        /* fp32 fused decode: queries per workgroup, 32 or 64; 0 = automatic (64 from 131072 queries) */
    int bf16_single;        /* 0 or 1: selects a precision mode (table above) */
    int dense_direct;       /* _f32 RDN trunk, big maps: 0 (default) = dense layers in Winograd form -- F(4x4, 3x3) when ciaosr_conv_t.frag_wino4
                             * is given, else F(2x2, 3x3) when frag_wino is (fp32 arithmetic on transformed operands: not bitwise a direct
                             * convolution; the trunk stays within 2e-4 x its scale of the direct form, tests/test_hip_parity.py);
                             * 1 = the direct halo-resident kernel (exact fmaf chains); 2 = F(2x2, 3x3) even when frag_wino4 is given.
                             * _bf16 / _f16 RDN trunk, big maps (round 6): 0 = the dense layers on 16x32-pixel tiles with one persistent
                             * workgroup per CU (dense_h16_wide_kernel; from 32 such tiles per image on), 1 = the 12x12-pixel kernels of
                             * rounds 1-3 (same 16-bit products, K split over the waves: another summation order) */
    int csa_scores_gemm;    /* _f32 cs_attn with 32 match channels: 0 (default) = correlation scores as a 3x3 diagonal box sum of the
                             * per-pixel correlation (K = 32, no patch rows); 1 = the 288-wide patch-row GEMM.  Same fp32 products, other order */
    int csa_attn_tile128;   /* _f32 cs_attn, attn.V (softmax formed in the operand staging), 0 or 1.  Four-block route (csa_attn_v16 below):
                             * 0 (default) = work items of 192 queries (one query row) per workgroup, 1 = items of 96 queries.  16C route:
                             * 0 = the 192 x 256 one-workgroup-per-CU kernel (gemm_big_f32.hip) where the problem fills the chip (>= 256
                             * workgroup tiles, K a multiple of 16), else and with 1 the 128 x 128 kernel.  Either way bitwise the same result */
    int query_grid_w;       /* traversal hint of the 16-bit fused head, >= 0 (a negative value is CIAOSR_ERR_BAD_ARG): W > 0 = the Q queries of
                             * the call are the rows of a row-major grid with W columns (q = i W + j, Q a multiple of W: what
                             * ciaosr_make_coord_cell_f32 produces); the chained kernel then walks them in 16 x 4 blocks so that a wave's rows
                             * gather from a handful of LR pixels.  Results do not depend on it; 0 = walk them in index order */
    int f16_pairs;          /* 0 to 3: selects a precision mode (table above) */
    int csa_attn_v16;       /* _f32 cs_attn, composed tail, 64 channels: 0 (default) = attn.V on the four diagonal tap blocks
                             * (csa_attn_v4_f32.hip: K = 4 (Hp/2+3)(Wp/2+3) instead of 16 L; where the logit matrix -- under csa_block_mb: a band's -- is under 2 GiB);
                             * 1 = the 16C route of 16 offset columns.  Same products summed in another order */
    int edsr_resident;      /* EDSR trunk, 0 or 1 (added in front of swin_h16; version 260), read by ciaosr_edsr_forward_batch_f32 and its two
                             * companions alone: 0 (default) = the images one after the other through ciaosr_edsr_forward_f32; 1 = the body
                             * convolutions of the whole batch on the halo-resident fp32 kernel where the route rule below that entry holds */
    int swin_h16;           /* SwinIR trunk, 0 or 1 (added in front of csa_block_mb, which stays the last field; version 240); READ ABOVE THE ABI (as query_grid_w is produced there): no entry point changes what it runs
                             * on it.  0 (default) = ciaosr_swinir_forward_f32 in every precision mode; 1 = the callers (PackedSwinIR, the
                             * restorer's tile loop) take ciaosr_swinir_forward_batch_f16 in the modes whose trunk element type is half
                             * (f16, f16-pairs, f16x3-fast) and keep the fp32 trunk elsewhere (fp32, f16x3 and every bf16 mode) */
    int csa_block_mb;       /* cs_attn in bands of query rows: 0 (default) = off, the logit matrix S [Hp Wp][L] (and the 16-bit entries' probability
                             * matrix P16) whole in the workspace; n > 0 = at most n MiB of score storage at a time -- one band's S rows plus, in
                             * the _bf16 / _f16 entries, its P16 rows (ciaosr_cs_attn_block_rows names the band height).  Scores, softmax and
                             * attn.V run per band, every other stage once; the route is chosen for a band, so maps whose whole S is past the
                             * 2 GiB of the four-block route or the 4 GiB of a buffer descriptor keep the fast kernels.  Size the workspace
                             * with the _opt functions.  The result does not depend on the band height where the same route runs; a negative
                             * value is CIAOSR_ERR_BAD_ARG */
} ciaosr_options_t;

/* ---- layout plumbing -------------------------------------------------------------------- */
/* [C][H][W] -> [H][W][ld_dst] (first C columns).  Encoder output (net:100) enters here. */
int ciaosr_nchw_to_hwc_f32(const float* src, float* dst, int C, int H, int W, int ld_dst, void* stream);
int ciaosr_hwc_to_nchw_f32(const float* src, int ld_src, float* dst, int C, int H, int W, void* stream);

/* ---- dense contraction (exact-fp32 MFMA, v_mfma_f32_32x32x2_f32) ------------------------- */
/* C[M][N] = act((A[M][K] . B^T + bias[N]) * alpha).  B is [N][K] (b_is_kn == 0, the PyTorch
 * Linear / 1x1-conv weight layout; replaces addmm at mlp:79-89 and conv2d at csa:418-420,499)
 * or [K][N] (b_is_kn == 1; the attn.V contraction csa:511).  lda/ldb/ldc multiples of 4, bases
 * 16-byte aligned.  act: CIAOSR_ACT_*; slope = PReLU slope (host scalar). */
int ciaosr_gemm_f32(const float* A, int lda, const float* B, int ldb, int b_is_kn, float* C, int ldc,
                    const float* bias, int M, int N, int K, float alpha, int act, float slope,
                    void* stream);

/* ---- patch extraction (implicit F.unfold / extract_image_patches) -------------------------- */
/* out[oy*OW+ox][(i*k+j)*Cs + c] = src[oy*stride-pad+i][ox*stride-pad+j][c] (0 outside), rows
 * optionally L2-normalised with floor `norm_floor` (csa:494-496).  Replaces F.unfold (net:132-136)
 * and extract_image_patches (csa:59-87, call sites :462-465, :476-479). */
int ciaosr_patch_rows_f32(const float* src_hwc, int ld_src, int Hs, int Ws, int Cs, int ksize, int stride,
                          int pad, int OH, int OW, float* out, int ld_out, int l2_normalize,
                          float norm_floor, void* stream);

/* ---- CrossScaleAttention, scale 2 (csa:430-532) ------------------------------------------- */
typedef struct ciaosr_csattn_weights {
    int channels;                 /* C */
    int scale;                    /* 2 (also when 0), 3 or 4: ONE entry of CrossScaleAttention's scale list (csa:436); a module built
                                   * with scale=[2,3] is two structs sharing the match / assembly weights and differing in `down`
                                   * (csa:421-427: down / downx3 / downx4), evaluated one after the other into consecutive C-column
                                   * slices of the output (csa:528) */
    /* Ch = C/2 rounded up to a multiple of 4; rows >= C/2 of the two match weights and biases are 0 */
    const float* w_match1;        /* [Ch][C]   conv_match_1.0.weight  (csa:418) */
    const float* b_match1;        /* [Ch] */
    float slope_match1;           /* conv_match_1.1.weight (PReLU), host scalar */
    const float* w_match2;        /* [Ch][C]   conv_match_2 (csa:419) */
    const float* b_match2;
    float slope_match2;
    const float* w_assembly;      /* [C][C]    conv_assembly (csa:420) */
    const float* b_assembly;
    float slope_assembly;
    const float* w_down;          /* [C][9C]   down / downx3 / downx4 .weight (csa:421-428) packed [co][(a*3+b)*C + ci] */
    const float* b_down;          /* [C] */
    /* optional (NULL = off): `down` weights masked per tap subset for the composed fold+down form (csattn.hip):
     * [9][C][9C], block 3r+s keeps taps a in R_r, b in S_s with R_0 = {0}, R_1 = {0,1,2}, R_2 = {1,2}; same
     * column packing as w_down.  Used on tiles of >= 4096 LR pixels, where it shrinks attn.V from 36C to 16C columns. */
    const float* w_down_masked;
    float escape_nan;             /* 1e-4 (csa:415) */
    float softmax_scale;          /* 10   (csa:408) */
} ciaosr_csattn_weights_t;

size_t ciaosr_cs_attn_workspace_bytes(int H, int W, int C);          /* scale 2 */
size_t ciaosr_cs_attn_workspace_bytes_scale(int H, int W, int C, int scale);
/* The same under opt->csa_block_mb (what a call with that option checks its workspace against; any entry's precision): equal to the
 * function above when the option is 0 or opt is NULL, else the whole-map S and P16 replaced by one band's and by the edge rows
 * [(Hp + Wp)][L] that outlive a band.  A budget below the smallest band (8 logit rows; 4 in the 16-bit entries) is not met: the size is that band's. */
size_t ciaosr_cs_attn_workspace_bytes_opt(int H, int W, int C, int scale, const ciaosr_options_t* opt /*host, may be NULL*/);
/* Padded query rows a band of ciaosr_cs_attn_<precision> produces (halo rows of the four-block route not counted): Hp = the padded map's
 * rows when the option is off or one band covers the map.  precision: 0 = _f32, 1 = _bf16, 2 = _f16; scale 2..4.  Host arithmetic only,
 * the same that drives the call (ceil(Hp / rows) bands); 0 on a bad argument. */
int ciaosr_cs_attn_block_rows(int H, int W, int C, int scale, int precision, const ciaosr_options_t* opt /*host, may be NULL*/);
/* feat_hwc [H][W][ld_feat] -> out [H][W] rows of C floats with leading dimension ld_out
 * (lets the caller write straight into the tail columns of the unfold rows, net:137). */
int ciaosr_cs_attn_f32(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w,
                       float* out, int ld_out, const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Same, with the two big contractions (correlation scores csa:497-500 and the attention-weighted patch sum csa:511)
 * on the bf16 MFMA when the composed tail applies (>= 4096 LR pixels, w_down_masked given): inputs rounded to bf16,
 * fp32 accumulation, logits and softmax in fp32, probabilities rounded to bf16.  Smaller maps: identical to _f32. */
int ciaosr_cs_attn_bf16(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w,
                        float* out, int ld_out, const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Same route with IEEE half operands (v_mfma_f32_32x32x16_f16: the bf16 MFMA's rate, 11 mantissa bits instead of 8;
 * conversions saturate at +-65504 instead of producing inf). */
int ciaosr_cs_attn_f16(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w,
                       float* out, int ld_out, const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- head ---------------------------------------------------------------------------------- */
typedef struct ciaosr_mlp {
    int n_layers;                          /* Linear layers = len(hidden_list)+1 (mlp:74-89) */
    int act;                               /* activation between the layers: CIAOSR_ACT_RELU (default; 0 is read as RELU), _SIN or _COS
                                            * (mlp:81-86).  The fused head kernels are ReLU-only: sin / cos MLPs take the staged route */
    int in_dim;                            /* fan-in of layer 0 as stored (device channel order) */
    int width[CIAOSR_MAX_LAYERS];          /* fan-out of layer i; width[n_layers-1] = out_dim */
    const float* weight[CIAOSR_MAX_LAYERS];/* layer i: [width[i]][ld[i]] row-major */
    int ld[CIAOSR_MAX_LAYERS];
    const float* bias[CIAOSR_MAX_LAYERS];  /* [width[i]] */
    /* optional: layer i pre-packed into MFMA fragment order by ciaosr_pack_fragments_f32 (NULL = not
     * packed).  With every hidden width 256, local_size 2 and fragments present the fused kernels run
     * (head_kv_fused / head_decode_fused); otherwise the staged per-layer GEMM path. */
    const float* frag[CIAOSR_MAX_LAYERS];
    /* optional: the same layers packed as 16-bit MFMA fragments: by ciaosr_pack_fragments_bf16 for the _bf16 entries, by
     * ciaosr_pack_fragments_f16 for the _f16 entries (a struct serves ONE 16-bit element type; the caller keeps one per type) */
    const void* frag16[CIAOSR_MAX_LAYERS];
    /* optional: the rounding residual w - bf16(w) of the same layers, packed by ciaosr_pack_fragments_bf16_lo (NULL = the
     * bf16 entries run with single-bf16 weights; ignored by the _f16 entries) */
    const void* frag16_lo[CIAOSR_MAX_LAYERS];
} ciaosr_mlp_t;

/* MFMA fragment packing of a Linear weight W[N][ld] (K valid columns): out[nt][j][lane][4] with
 * lane (i = lane&31, h = lane>>5) holding W[32nt+i][8j+4h .. 8j+4h+3]; zero padded. */
size_t ciaosr_fragment_floats(int N, int K);
/* Queries per workgroup of the fp32 fused decode kernel for a launch of nq queries under decode_rows (host; launches nothing): 32 or 64. */
int ciaosr_head_decode_rows(int decode_rows, int nq);
int ciaosr_pack_fragments_f32(const float* W, int ld, int N, int K, float* out, void* stream);

/* bf16 fragment packing: out[nt][ks][lane][8 bf16], lane (i = lane&31, g = lane>>5) holds
 * W[32nt+i][16ks+8g .. 16ks+8g+7] rounded to nearest-even bf16; zero padded. */
size_t ciaosr_fragment_bf16_bytes(int N, int K);
int ciaosr_pack_fragments_bf16(const float* W, int ld, int N, int K, void* out, void* stream);
/* same layout, holding bf16(W - bf16(W)): the low half of the hi + lo weight pair */
int ciaosr_pack_fragments_bf16_lo(const float* W, int ld, int N, int K, void* out, void* stream);
/* same layout and byte count with IEEE half elements (round-to-nearest-even, saturating at +-65504): the weights of the
 * _f16 entries.  Half keeps 11 mantissa bits, so ONE MFMA per product passes the PSNR gate that single bf16 weights fail
 * (DESIGN 4.3); the price is the range: activations and weights beyond 65504 are clamped, below 6e-8 flushed to 0. */
size_t ciaosr_fragment_f16_bytes(int N, int K);
int ciaosr_pack_fragments_f16(const float* W, int ld, int N, int K, void* out, void* stream);
/* Rounding residual w - half(w) of the same matrix in the same fragment order: the lo half of the pair of opt->f16_pairs. */
int ciaosr_pack_fragments_f16_lo(const float* W, int ld, int N, int K, void* out, void* stream);
/* hi and lo of a matrix in ONE launch (model-load path): out_hi = ciaosr_pack_fragments_{bf16,f16}, out_lo = ..._lo */
int ciaosr_pack_fragments_bf16_pair(const float* W, int ld, int N, int K, void* out_hi, void* out_lo, void* stream);
int ciaosr_pack_fragments_f16_pair(const float* W, int ld, int N, int K, void* out_hi, void* out_lo, void* stream);

/* Every fp32 fragment form of ONE 3x3 convolution weight in one launch (model-load path).  Element (o, a, b, c) -- output channel, kernel
 * row, kernel column, input channel -- is read at w[o * stride_o + a * stride_a + b * stride_b + c * stride_c]; N output, K input channels
 * (K a multiple of 4).  Outputs (each optional, NULL = skip): frag_direct = ciaosr_pack_fragments_f32 of the [N][(3 a + b) K + c]
 * matrix; frag_wino2 = the 16 matrices U[p] = (G g G^T)[p], p = 4 i + j, of Winograd F(2x2, 3x3), each [N][K] in
 * ciaosr_pack_fragments_f32 order, back to back (ciaosr_conv_t.frag_wino, ciaosr_head_weights_t.k_out_wino); frag_wino4 = the 36
 * matrices of F(4x4, 3x3), p = 6 i + j (frag_wino4 / k_out_wino4).  The transform is evaluated in fp64 and rounded once. */
int ciaosr_pack_conv3x3_f32(const float* w, size_t stride_o, size_t stride_a, size_t stride_b, size_t stride_c, int N, int K,
                            float* frag_direct, float* frag_wino2, float* frag_wino4, void* stream);

typedef struct ciaosr_head_weights {
    int channels;         /* C  (encoder width)                                   net:57-60 */
    int nonlocal_channels;/* Cn = C*len(multi_scale) or 0                          net:73-76 */
    int nonlocal_max_scale;/* largest entry of multi_scale (2 when 0): sizes the cs_attn scratch inside the head workspace */
    int local_size;       /* 1, 2 or 3  -> 1, 4 or 9 key samples                   net:152-155 */
    int no_unfold;        /* 0 (default): feat_unfold=True, the q/k/v maps are 3x3 unfolds, D = 9C (net:129-138);
                           * 1: feat_unfold=False, they are the feature map itself, D = C (net:139-141; unused by the configs).
                           * The dims below read with D in place of 9C */
    float softmax_scale;  /*                                                        net:215  */
    /* imnet_k: in = 9C + 4 (unfold | rel_y rel_x scale_y scale_x), out = 9C.      net:63,70
     * imnet_v: in = 9C + Cn + 4, out = 9C + Cn.                                   net:64,71,75-76
     * imnet_q: in = 9C + Cn, out = 3.                                             net:62,74
     * Layer-0 columns and last-layer rows are in device channel order. */
    ciaosr_mlp_t q, k, v;
    /* optional (C = 64, feat_unfold, 256-wide last hidden layer of imnet_k): imnet_k's OUTPUT layer W5 [9C][256] read as the 3x3
     * convolution g[n][c][a][b] = W5[(3 a + b) C + c][n] (rows in device order) in Winograd F(2x2, 3x3) form, U[p] = (G g G^T)[p], p = 4 i + j = 0..15,
     * each [256][64] matrix packed by ciaosr_pack_fragments_f32, the 16 arrays back to back.  Lets the _f32 entry build the logit
     * table of maps of 512 .. 65536 LR pixels as nine convolutions of product maps instead of a 576-deep GEMM row per
     * (pixel, key offset): 9 x 2.25 fewer multiplies (head_ops.hip qk_maps, dense_wino_f32.hip).  NULL = the GEMM */
    const float* k_out_wino;
    /* optional, same layer: the F(4x4, 3x3) form, U[p] = (G g G^T)[p] with the 6x3 G of F(4, 3), p = 6 i + j = 0..35, each [256][64] matrix
     * packed by ciaosr_pack_fragments_f32, the 36 arrays back to back (dense_wino4_f32.hip: 2.25x fewer MFMAs than the F(2x2) form);
     * preferred over k_out_wino unless head_route has CIAOSR_HEAD_TABLE_WINO2.  NULL = the F(2x2) form (or the GEMM) */
    const float* k_out_wino4;
    /* optional (16-bit entries; hidden_list = [256] * 4 for imnet_k and imnet_v): the weight stream of the weights-stationary head kernel,
     * packed by ciaosr_pack_head_chain_bf16 / _f16 with pairs = 0 (chain16: one 16-bit weight per product) and pairs = 1 (chain16_pairs:
     * every tile followed by its rounding residuals; read in the modes bf16 and f16-pairs).  ciaosr_head_chain_bytes() each (the stream of phi_k / phi_v, followed by imnet_q's where its shape allows one).
     * NULL = the kernels that read ciaosr_mlp_t.frag16 */
    const void* chain16;
    const void* chain16_pairs;
} ciaosr_head_weights_t;

/* Weight stream of the weights-stationary 16-bit head (head_chain_h16.hip): [tail fragments of imnet_k | imnet_v layer 0: 8 KB each]
 * [per 32-column tile of imnet_k layers 1-3, imnet_v layers 1-3 and imnet_v's output layer: 16 fragments [ks][lane][8 x 16 bit], lane
 * (i = lane & 31, g = lane >> 5) element e holding W[32 T + i][16 ks + 8 (e >> 2) + 4 g + (e & 3)] -- the k order in which the
 * accumulators of one layer are the operand registers of the next; pairs: + the same 16 fragments of w - h16(w)], padded to whole
 * 32-KB slots.  `w` must hold the fp32 weights (device order).  Replaces the per-layer Linear calls of mlp:87-102 at net:202-206. */
size_t ciaosr_head_chain_bytes(const ciaosr_head_weights_t* w, int pairs);
int ciaosr_pack_head_chain_bf16(const ciaosr_head_weights_t* w, int pairs, void* out, void* stream);
int ciaosr_pack_head_chain_f16(const ciaosr_head_weights_t* w, int pairs, void* out, void* stream);

/* Grid-centre coordinates and cells of an Ht x Wt target: coord[q] = (seq_y[i], seq_x[j]) with
 * seq[i] = fp32(-1 + 1/n) + fp32(2/n) * fp32(i), cell[q] = (2/Ht, 2/Wt), q = i*Wt + j
 * (mmedit make_coord, call site rest:240; cell rest:241-243). */
int ciaosr_make_coord_cell_f32(float* coord, float* cell, int Ht, int Wt, void* stream);
/* Rows [i0, i1) x columns [j0, j1) of the same grid, q = (i - i0) (j1 - j0) + (j - j0): a window render's queries, made on the device.
 * frame = NULL: the values above at (i, j), bitwise.  frame = {n_lr_y, y0, th, n_lr_x, x0, tw} (host): the grid as LR tile [y0, y0 + th) x
 * [x0, x0 + tw) of an n_lr_y x n_lr_x image sees it: coord = fp32(((g + 1) (n_lr / 2) - y0) (2 / th) - 1) with g the global value, every
 * operation a rounded fp64 one, cell = fp32((2 / n_hr) (n_lr / th)); a tile that covers its whole axis keeps the global values. */
int ciaosr_make_coord_cell_window_f32(float* coord, float* cell, int Ht, int Wt, int i0, int i1, int j0, int j1, const int* frame /*host, may be NULL*/,
                                      void* stream);

/* Index math only (test/debug): nearest LR index of every query and of its key samples.
 * q_idx [Q] (= iy*W+ix), k_idx [Q][J], rel [Q][J][2], following net:145-146,159-193. */
int ciaosr_head_indices_f32(const float* coord, const float* cell, int Q, int chunk, int H, int W,
                            int local_size, int* q_idx, int* k_idx, float* rel, void* stream);

/* Staged K4 "local attention" (net:211-216): logits_j = sum_d q[d] key_j[d] wk_j[d],
 * a = softmax(logits / softmax_scale), z = sum_j a_j value_j * wv_j.
 * unfold [HW][ld_u] rows (9C | Cn), wk [Q*J][ld_wk], wv [Q*J][ld_wv], z [Q][ld_z]. */
int ciaosr_local_attention_f32(const float* unfold, int ld_u, int C, int Cn, const int* q_idx,
                               const int* k_idx, const float* wk, int ld_wk, const float* wv, int ld_wv,
                               float* z, int ld_z, int Q, int J, float softmax_scale, void* stream);

/* The same kernel with wk, wv and z as 16-bit arrays (bf16 / IEEE half, round to nearest even, half saturating; leading dimensions in
 * ELEMENTS, multiples of 4; 8-byte aligned): the staged route's HBM-bound step at half the bytes (11 056 B per query at
 * C = 64 against 22 064).  unfold, the logits, the softmax and the sums stay fp32.  net:211-216. */
int ciaosr_local_attention_bf16(const float* unfold, int ld_u, int C, int Cn, const int* q_idx,
                                const int* k_idx, const void* wk, int ld_wk, const void* wv, int ld_wv,
                                void* z, int ld_z, int Q, int J, float softmax_scale, void* stream);
int ciaosr_local_attention_f16(const float* unfold, int ld_u, int C, int Cn, const int* q_idx,
                               const int* k_idx, const void* wk, int ld_wk, const void* wv, int ld_wv,
                               void* z, int ld_z, int Q, int J, float softmax_scale, void* stream);

/* Staged K1 "gather rows" (net:145-146,176-196), the MLP inputs exactly as the reference assembles them:
 *   q_rows [Q][ld_q]      = unfold[q_idx[q]][0:9C]                     (zeros when the query falls outside, net:145)
 *   inp_k  [Q*J][ld_k]    = [ unfold[k_idx][0:9C]      | rel_y rel_x | scale_y scale_x ]      (net:195)
 *   inp_v  [Q*J][ld_v]    = [ unfold[k_idx][0:9C+Cn]   | rel_y rel_x | scale_y scale_x ]      (net:196)
 * row r = q*J + j (the reference stacks per shift j; same rows, query-major here).  q_idx [Q], k_idx [Q*J] are
 * written for ciaosr_local_attention_f32.  unfold rows are in the library's (ki,kj,c) column order. */
int ciaosr_gather_rows_f32(const float* unfold, int ld_u, int C, int Cn, const float* coord, const float* cell, int Q,
                           int chunk, int H, int W, int local_size, float* q_rows, int ld_q, float* inp_k, int ld_k,
                           float* inp_v, int ld_v, int* q_idx, int* k_idx, void* stream);

/* Staged MLPRefiner.forward (mlp_refiner.py:87-102): y = L_n(relu(...relu(L_1 x))) on `rows` rows through the
 * fp32 MFMA GEMM, layer by layer, no hoist.  x [rows][ld_x] (in_dim columns), out [rows][ld_out];
 * n_run = 0 runs every layer; 0 < n_run < n_layers stops after layer n_run (ReLU applied) so that the
 * remaining tail can go through ciaosr_decode_residual_f32.  workspace >= ciaosr_mlp_workspace_bytes(m, rows). */
size_t ciaosr_mlp_workspace_bytes(const ciaosr_mlp_t* m, int rows);
int ciaosr_mlp_forward_f32(const float* x, int ld_x, const ciaosr_mlp_t* m, int n_run, int rows, float* out, int ld_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same MLP with every Linear on the 16-bit MFMA GEMM (bf16 / IEEE half inputs, fp32 accumulation and biases, 16-bit activations
 * between the layers, fp32 output): ReLU MLPs whose in_dim and layer widths are multiples of 4 (else CIAOSR_ERR_BAD_ARG; imnet_k / imnet_v; imnet_q's 3-wide output layer is
 * CIAOSR_ERR_UNSUPPORTED: run it up to its last hidden layer in fp32 or use the fused head).  Weights are rounded per call from
 * m->weight (single 16-bit weights: the precision of `opt->bf16_single` / the f16 mode).  workspace >= ciaosr_mlp_workspace_bytes_16(m, rows).
 * mlp_refiner.py:87-102. */
size_t ciaosr_mlp_workspace_bytes_16(const ciaosr_mlp_t* m, int rows);
int ciaosr_mlp_forward_bf16(const float* x, int ld_x, const ciaosr_mlp_t* m, int rows, float* out, int ld_out,
                            void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_mlp_forward_f16(const float* x, int ld_x, const ciaosr_mlp_t* m, int rows, float* out, int ld_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Staged decode tail (net:107-108,221): rgb[q] = W_last . h[q] + b_last + bilinear_border(x_lr_nchw; coord[q]).
 * h [Q][ld_h] (width columns), w_last [3][ld_w]; x_lr_nchw NULL = no residual. */
int ciaosr_decode_residual_f32(const float* h, int ld_h, int width, const float* w_last, int ld_w, const float* b_last,
                               const float* x_lr_nchw, const float* coord, int Q, int H, int W, float* rgb,
                               void* stream);

size_t ciaosr_head_workspace_bytes(int H, int W, const ciaosr_head_weights_t* w, int Q);
/* the same with cs_attn's share sized by ciaosr_cs_attn_workspace_bytes_opt: what ciaosr_head_forward_* checks under opt->csa_block_mb */
size_t ciaosr_head_workspace_bytes_opt(int H, int W, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt /*host, may be NULL*/);

/* query_rgb + batched_predict + bilinear residual (net:88-248) given the encoder feature map.
 *   feat_hwc   [H][W][C]                      encoder output, channels-last
 *   csattn     non-NULL iff nonlocal_channels > 0 (net:134-137): host array of nonlocal_channels / C structs, one per
 *              entry of multi_scale (net:44,85), written to consecutive C-column slices of the value rows
 *   x_lr_nchw  [3][H][W] normalised LR image for the residual (net:107-108); NULL = no residual
 *   coord/cell [Q][2] (y,x) fp32                                              (net:88-99)
 *   chunk      the reference's eval_bsize (net:238-246): only selects which query's cell feeds the
 *              shift radius (net:162-165); 0 = one chunk.  cs_attn is computed once (result-identical).
 *   rgb        [Q][3] */
int ciaosr_head_forward_f32(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w,
                            const ciaosr_csattn_weights_t* csattn, const float* x_lr_nchw,
                            const float* coord, const float* cell, int Q, int chunk, float* rgb,
                            const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Same path with bf16 MFMA inputs (fp32 accumulation) in the fused kernels' dense layers; coordinates, index
 * math, the layer-0 tables, logits, softmax and the decode output stay fp32.  Needs the bf16 fragments
 * (ciaosr_mlp_t.frag16); CIAOSR_ERR_UNSUPPORTED when the fused kernels do not apply.  Parity is PSNR-based. */
int ciaosr_head_forward_bf16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w,
                             const ciaosr_csattn_weights_t* csattn, const float* x_lr_nchw,
                             const float* coord, const float* cell, int Q, int chunk, float* rgb,
                             const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Same with IEEE half MFMA inputs (ciaosr_mlp_t.frag16 packed by ciaosr_pack_fragments_f16; one MFMA per product;
 * opt->bf16_single ignored).  opt->f16_pairs: frag16_lo (ciaosr_pack_fragments_f16_lo) is read too -- two MFMAs per product. */
int ciaosr_head_forward_f16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w,
                            const ciaosr_csattn_weights_t* csattn, const float* x_lr_nchw,
                            const float* coord, const float* cell, int Q, int chunk, float* rgb,
                            const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- a persistent head scene: encode once, query any scale or window ---------------------------------------------------------------
 * ciaosr_head_forward_* = the stages that depend on the LR image only (unfold rows, cs_attn, the layer-0 tables, the logit table)
 * followed by the per-query kernels.  The two entry-point families below run the halves apart: prepare writes what the per-query
 * kernels read into a caller-owned device buffer, the scene; query renders any Q >= 1 queries from it, any number of times.
 *   scene      U [HW][Dv] (unfold rows | non-local maps), Tk [HW][wk0], Tv [HW][wv0] and, when the route has a logit table, G
 *              [9 HW][260], each 256-byte aligned.  C = 64, hidden 256: 13 968 B per LR pixel with G, 4 608 B without.
 *   q_plan     the route is a function of the query count in two places (the logit table exists iff Q J > 9 HW; the f16 layer-0 tables
 *              ask for the room a call of Q queries has), so a scene is planned for q_plan queries -- the largest full render intended --
 *              and every query runs under the route ciaosr_head_forward_* takes at Q = q_plan, in chunks computed from its own Q.
 *              prepare + query at Q = q_plan is bitwise ciaosr_head_forward_*; so is every subset of its rows queried alone.
 *   desc       host struct written by prepare; query refuses (CIAOSR_ERR_BAD_ARG, CIAOSR_ERR_WORKSPACE for a short buffer; before its
 *              first launch) a descriptor that does not fit w, opt, the entry's precision or scene_bytes.
 * Workspaces are scratch of one call, as everywhere: prepare's holds cs_attn's workspace and the tables' operands, query's the
 * attention rows of a chunk (and the staged route's activations).  No entry allocates, synchronises or keeps state. */
typedef struct ciaosr_head_scene {
    int magic;                          /* layout tag + version */
    int H, W, C, Cn, D, Dv, J;          /* LR map, channels, non-local channels, 9C (C without unfold), D + Cn, key samples per query */
    int q_plan;
    int precision;                      /* 0 = f32, 1 = bf16, 2 = f16: the suffix of the prepare entry */
    int route;                          /* ciaosr_head_route_code of (H, W, w, q_plan, precision, opt) */
    int off_u, off_tk, off_tv, off_g;   /* carve offsets into the scene in 256-byte units; off_g = -1: no logit table */
    int total;                          /* scene bytes in 256-byte units */
} ciaosr_head_scene_t;

/* What a call of Q queries runs, packed: bit 0 fused, 1-2 layer-0 tables (h16 / small / gemm), 3-5 logit table (none / gemm32 / gemm16 /
 * wino2 / wino4), 6-7 kernel (fused32 / fused16 / wide / chain), 8 chained kv, 9 chained decode, 10 16-bit, 11 weight pairs, 12-13 wide
 * mode.  Negative: the error code the call would return.  precision: 0 | 1 | 2 as above.  Launches nothing. */
int ciaosr_head_route_code(int H, int W, const ciaosr_head_weights_t* w, int Q, int precision, const ciaosr_options_t* opt /*host, may be NULL*/);
/* Sizes for any precision of (w, opt) (the largest); 0 = bad arguments */
size_t ciaosr_head_scene_bytes(int H, int W, const ciaosr_head_weights_t* w, int q_plan, const ciaosr_options_t* opt /*host, may be NULL*/);
size_t ciaosr_head_prepare_workspace_bytes(int H, int W, const ciaosr_head_weights_t* w, int q_plan, const ciaosr_options_t* opt /*host, may be NULL*/);
size_t ciaosr_head_query_workspace_bytes(const ciaosr_head_scene_t* desc /*host*/, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt /*host, may be NULL*/);
/* Where a query of Q queries keeps the flag of the chained 16-bit kv kernel: *offset = bytes from the start of the query workspace to one
 * int32.  Each launch pair of a query (2^20 queries) clears it, and the chained kernel sets it to 1 when a row tile of 8 consecutive
 * queries does not fit its 4 x 4 window of key pixels -- the whole launch is then redone by the gated 128-row kernel.  After a query
 * the int holds the flag of its LAST launch pair only (one pair for Q <= 2^20).  Read it on the query's stream before the workspace is
 * used again.  CIAOSR_ERR_UNSUPPORTED: the scene's route has no chained kv kernel (fp32, f16x3, head_route bits), nothing is ever
 * written there; the other refusals are ciaosr_head_query_workspace_bytes' (which returns 0 for them).  Launches nothing, carves nothing. */
int ciaosr_head_query_flag_offset(const ciaosr_head_scene_t* desc /*host*/, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt /*host, may be NULL*/,
                                  size_t* offset /*host, out*/);
int ciaosr_head_prepare_f32(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, int q_plan,
                            const ciaosr_options_t* opt /*host, NULL = defaults*/, void* scene, size_t scene_bytes, ciaosr_head_scene_t* desc /*host, out*/,
                            void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_head_prepare_bf16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, int q_plan,
                             const ciaosr_options_t* opt /*host, NULL = defaults*/, void* scene, size_t scene_bytes, ciaosr_head_scene_t* desc /*host, out*/,
                             void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_head_prepare_f16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, int q_plan,
                            const ciaosr_options_t* opt /*host, NULL = defaults*/, void* scene, size_t scene_bytes, ciaosr_head_scene_t* desc /*host, out*/,
                            void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_head_query_f32(const void* scene, size_t scene_bytes, const ciaosr_head_scene_t* desc /*host*/, const ciaosr_head_weights_t* w,
                          const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb,
                          const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_head_query_bf16(const void* scene, size_t scene_bytes, const ciaosr_head_scene_t* desc /*host*/, const ciaosr_head_weights_t* w,
                           const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb,
                           const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_head_query_f16(const void* scene, size_t scene_bytes, const ciaosr_head_scene_t* desc /*host*/, const ciaosr_head_weights_t* w,
                          const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb,
                          const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- encoder trunks: gen_feature (net:321-342 RDN, net:393-408 EDSR) -------------------------- */
typedef struct ciaosr_conv {
    const float* weight; /* [cout][k*k*cin'] packed (a*k+b)*cin' + ci; cin' = cin (4 for the 3-channel first conv, zero padded) */
    const float* bias;   /* [cout] */
    int cin, cout, ksize;
    const void* frag16;  /* optional: ciaosr_pack_fragments_bf16 / _f16 (weight, ld = k*k*cin, N = cout, K = k*k*cin); used by
                          * ciaosr_rdn_forward_bf16 / _f16 for the dense layers, NULL otherwise */
    const void* frag16_lo; /* optional: ciaosr_pack_fragments_bf16_lo of the same matrix (hi + lo weight pair of the bf16 trunk) */
    const float* frag;   /* optional: ciaosr_pack_fragments_f32 of the same matrix; lets ciaosr_rdn_forward_f32 run the
                          * dense layers of maps with >= 128 tiles of 12x12 pixels through the halo-resident kernel, and any
                          * 3x3 trunk convolution of a map of <= 18432 pixels through the one-launch small-map kernel */
    const float* frag_wino; /* optional (3x3, cout = 64, cin a multiple of 64): the Winograd F(2x2, 3x3) form of the weights,
                          * U[p] = (G g G^T)[p], p = 4 i + j = 0..15, each [cout][cin] matrix packed by ciaosr_pack_fragments_f32, the 16
                          * arrays back to back; lets ciaosr_rdn_forward_f32 run the dense layers of big maps with 2.25x fewer MFMAs
                          * (dense_wino_f32.hip).  NULL = the direct halo-resident kernel (`frag`) */
    const float* frag_wino4; /* optional (same layers): the Winograd F(4x4, 3x3) form, U[p] = (G g G^T)[p], p = 6 i + j = 0..35, each
                          * [cout][cin] matrix packed by ciaosr_pack_fragments_f32, the 36 arrays back to back (dense_wino4_f32.hip: 4x fewer
                          * MFMAs than the direct form); preferred over frag_wino when given, see ciaosr_options_t.dense_direct */
} ciaosr_conv_t;

typedef struct ciaosr_rdn_weights {
    int mid_channels, growth, num_blocks, num_layers;
    ciaosr_conv_t sfe1, sfe2, gff0, gff1;
    const ciaosr_conv_t* dense; /* host array [num_blocks*num_layers]: rdbs[b].layers[l].conv */
    const ciaosr_conv_t* lff;   /* host array [num_blocks]:            rdbs[b].lff */
    /* optional "scatter form" of the dense blocks (mid_channels == growth == 64): for block b and input group s
     * (s = 0: block input, s >= 1: output of dense layer s-1) the weight slices of all later layers stacked:
     * scatter_weight[b*num_layers + s] = [64*(num_layers-s)][9*64], row (l-s)*64+co, column tap*64+ci
     *   = rdbs[b].layers[l].conv.weight[co][64*s + ci][tap];  scatter_bias = [num_blocks][num_layers][64].
     * NULL = every dense layer runs as its own (gather-form) convolution. */
    const float* const* scatter_weight; /* host array [num_blocks*num_layers] of device pointers */
    const float* scatter_bias;          /* device */
    /* optional: ciaosr_pack_fragments_f32(scatter_weight[i], ld = 576, N = 64*(num_layers-s), K = 576) per entry; maps of
     * <= 18432 pixels then run the steps through the small-map kernel (dense_scatter_f32.hip) */
    const float* const* scatter_frag;   /* host array [num_blocks*num_layers] of device pointers, or NULL */
} ciaosr_rdn_weights_t;

typedef struct ciaosr_edsr_weights {
    int mid_channels, num_blocks;
    float res_scale;
    ciaosr_conv_t conv_first, conv_after_body;
    const ciaosr_conv_t* conv1; /* host array [num_blocks]: body[b].conv1 */
    const ciaosr_conv_t* conv2; /* host array [num_blocks]: body[b].conv2 */
} ciaosr_edsr_weights_t;

size_t ciaosr_rdn_workspace_bytes(int H, int W, const ciaosr_rdn_weights_t* w);
/* x_nchw [3][H][W] normalised LR image -> feat_hwc [H][W][mid_channels] */
int ciaosr_rdn_forward_f32(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                           const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Same trunk with the dense layers (RDB.layers[l].conv) on the bf16 MFMA, fp32 accumulation, when the map has at
 * least 128 tiles of 12x12 pixels (else identical to the f32 entry); first/last convolutions, LFF/GFF and all
 * residual sums stay fp32.  Needs ciaosr_conv_t.frag16 on every dense layer.  Parity is PSNR-based. */
int ciaosr_rdn_forward_bf16(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                            const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                            void* stream);
/* Same with IEEE half operands (ciaosr_conv_t.frag16 packed by ciaosr_pack_fragments_f16; frag16_lo -- packed by
 * ciaosr_pack_fragments_f16_lo -- is read only with opt->f16_pairs). */
int ciaosr_rdn_forward_f16(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                           const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                           void* stream);
/* B images of one size through the trunk in one call: x_nchw [B][3][H][W] -> feat_hwc [B][H][W][mid_channels].  On maps big
 * enough for the halo-resident dense-layer kernels the B images share every dense-layer launch (and the f16 route's row-wise 1x1
 * kernels), so the per-launch floor of the 128 dependent launches is paid once per batch; each image's result is bitwise the
 * single-image result.  Smaller maps: the images run one after the other.  This is how clip_test's tiles (ciaosr.py:233-254,
 * independent crops of one image) are fed: `test_cfg.tile_batch` tiles per call. */
size_t ciaosr_rdn_workspace_bytes_batch(int B, int H, int W, const ciaosr_rdn_weights_t* w);
int ciaosr_rdn_forward_batch_f32(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                                 const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                                 void* stream);
int ciaosr_rdn_forward_batch_bf16(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                                  const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                                  void* stream);
int ciaosr_rdn_forward_batch_f16(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                                 const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t ciaosr_edsr_workspace_bytes(int H, int W, const ciaosr_edsr_weights_t* w);
int ciaosr_edsr_forward_f32(const float* x_nchw, int H, int W, const ciaosr_edsr_weights_t* w, float* feat_hwc,
                            void* workspace, size_t workspace_bytes, void* stream);
/* B images of one size through the EDSR trunk in one call: x_bchw [B][3][H][W] -> feat_bhwc [B][H][W][mid_channels]; fp32 in every
 * precision mode.  Two routes (ciaosr_edsr_route_code names the one a call takes and launches nothing):
 *   0, per image: the B images one after the other through ciaosr_edsr_forward_f32's launches, bitwise that entry's result.  Always with
 *      opt == NULL or opt->edsr_resident == 0.
 *   1, resident: conv_first per image; then every body convolution and conv_after_body as ONE launch of the halo-resident fp32 kernel
 *      (12x12-pixel workgroups, dense_f32.hip; profiler tag enc_edsr_resident) for the whole batch: 2 num_blocks + 1 launches per call
 *      instead of per image.  Each image is computed by the workgroups, in the order, of a B = 1 call: bitwise equal to it.  Same products
 *      as route 0 in another summation order.  Epilogues in fp32, every operation rounded on its own (no FMA): conv1 max(sum + bias, 0);
 *      conv2 x + res_scale * (sum + bias), in place on x; conv_after_body first + 1 * (sum + bias).
 * Route 1 applies iff ALL of: opt && opt->edsr_resident == 1; mid_channels == 64; num_blocks >= 1; every conv1[i], conv2[i] and
 * conv_after_body has `frag` (ciaosr_pack_fragments_f32 of its [64][9 * 64] matrix); the map has at least opt->dense_min_tiles (0 = 128)
 * tiles of 12x12 pixels; one image's [H W][128] fp32 buffer is under 4 GiB - 256 B (32-bit buffer offsets).  A batch whose [B H W][128]
 * buffer is not runs as passes of as many images as fit.
 * ciaosr_edsr_route_code: < 0 = the error the call would return for these arguments (pointers apart); else bits 0-7 = the route, and
 * bits 8.. = the images per pass when route 1 runs the batch in more than one pass (0 = one pass of B).
 * ciaosr_edsr_workspace_bytes_batch: what the call checks its workspace against (0 on a bad argument); equal to
 * ciaosr_edsr_workspace_bytes for route 0. */
size_t ciaosr_edsr_workspace_bytes_batch(int B, int H, int W, const ciaosr_edsr_weights_t* w, const ciaosr_options_t* opt /*host, may be NULL*/);
int ciaosr_edsr_route_code(int B, int H, int W, const ciaosr_edsr_weights_t* w, const ciaosr_options_t* opt /*host, may be NULL*/);
int ciaosr_edsr_forward_batch_f32(const float* x_bchw, int B, int H, int W, const ciaosr_edsr_weights_t* w, float* feat_bhwc,
                                  const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- SwinIR trunk: LocalImplicitSRSWINIR.gen_feature (net:475-525 over swinir_net.py) --------------------------
 * Token maps are [Hp*Wp][ld] with ld = embed_dim rounded up to 64 (Hp, Wp = H, W reflect-padded to window multiples,
 * net:509-512); every Linear / 3x3 convolution weight is given with its input dimension zero-padded to that ld
 * (hidden rounded up to 64 for fc2), i.e. qkv_w [3C][ld], proj_w [C][ld], fc1_w [hidden][ld], fc2_w [C][ldh],
 * group_conv / conv_after_body [C][9*ld] tap-major; conv_first as in the RDN trunk ([C][36]). */
typedef struct ciaosr_swin_block {     /* SwinTransformerBlock (swinir_net.py:149-258) */
    const float *ln1_w, *ln1_b;        /* norm1 */
    const float *qkv_w, *qkv_b;        /* attn.qkv with the q rows pre-multiplied by head_dim^-0.5 (swinir_net.py:125) */
    const float *bias;                 /* relative_position_bias_table gathered by relative_position_index: [heads][N][N] (:129-132) */
    const float *proj_w, *proj_b;      /* attn.proj */
    const float *ln2_w, *ln2_b;        /* norm2 */
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;   /* mlp (exact GELU in between) */
    int shift;                         /* 0 or window_size/2 */
    const float *mask;                 /* shifted blocks: attention mask [nW][N][N] (0 / -100) for THIS call's padded map size:
                                        * the block's attn_mask buffer when the size equals its input_resolution, else
                                        * calculate_mask(x_size) (swinir_net.py:192-213, :233-236); NULL for shift 0 */
    /* IEEE-half copies of the four Linear weights in the layouts above ([3C][ld] with the q scale folded in, [C][ld], [hidden][ld],
     * [C][ldh], pad columns zero, 16-byte aligned), read by ciaosr_swinir_forward_batch_f16 only: NULL for the fp32 entry */
    const unsigned short *qkv_w16, *proj_w16, *fc1_w16, *fc2_w16;
} ciaosr_swin_block_t;

typedef struct ciaosr_swinir_weights {
    int embed_dim, num_heads, window_size, hidden, num_groups, depth;   /* depth = blocks per RSTB (uniform) */
    ciaosr_conv_t conv_first, conv_after_body;
    const float *pe_norm_w, *pe_norm_b;        /* patch_embed.norm */
    const float *norm_w, *norm_b;              /* final norm */
    const ciaosr_swin_block_t* blocks;         /* host array [num_groups*depth] */
    const ciaosr_conv_t* group_conv;           /* host array [num_groups]: layers[g].conv ('1conv') */
} ciaosr_swinir_weights_t;

size_t ciaosr_swinir_workspace_bytes(int H, int W, const ciaosr_swinir_weights_t* w);
/* x_nchw [3][H][W] normalised LR image -> feat_hwc [H][W][embed_dim] */
int ciaosr_swinir_forward_f32(const float* x_nchw, int H, int W, const ciaosr_swinir_weights_t* w, float* feat_hwc,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same trunk with qkv / proj / fc1 / fc2 of every Swin block on the f16 MFMA (LayerNorm fused into the qkv and fc1 operand staging:
 * five launches per block instead of seven), B >= 1 equally sized images per call: x_bchw [B][3][H][W] -> feat_bhwc [B][H][W][embed_dim].
 * Every block launch is shared by the B images; image b is bitwise the B = 1 call on that image.  The residual stream, the window
 * attention (its output is rounded to half for the proj), the LayerNorm statistics, conv_first, the 3x3 convolutions and both outer norms
 * stay fp32.  Shape checks as ciaosr_swinir_forward_f32; needs the four *_w16 pointers of every block (CIAOSR_ERR_BAD_ARG without them;
 * the fp32 qkv_w / proj_w / fc1_w / fc2_w are not read).  Every refusal happens before anything is enqueued.  A batch of more than
 * 2^30 tokens (B * Hp * Wp) is refused (CIAOSR_ERR_BAD_ARG), not split into sub-batches.  Accuracy: PSNR-gated. */
size_t ciaosr_swinir_workspace_bytes_batch_f16(int B, int H, int W, const ciaosr_swinir_weights_t* w);
int ciaosr_swinir_forward_batch_f16(const float* x_bchw, int B, int H, int W, const ciaosr_swinir_weights_t* w, float* feat_bhwc,
                                    const ciaosr_options_t* opt /*host, NULL = defaults*/, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* ---- restorer plumbing (rest:142-169, :218-258) --------------------------------------------- */
/* x = (lq - mean) / std on [3][H][W] */
int ciaosr_normalize_f32(const float* lq, float* out, int H, int W, const float* mean3 /*host*/,
                         const float* std3 /*host*/, void* stream);
/* out[c][y][x] = clamp(pred[(y*W+x)*3+c] * std[c] + mean[c], 0, 1)      (rest:160-169) */
int ciaosr_denorm_clamp_f32(const float* pred_q3, float* out_chw, int H, int W, const float* mean3 /*host*/,
                            const float* std3 /*host*/, void* stream);
/* E[c][y0+y][x0+x] += tile[(y*tw+x)*3+c];  Wt[...] += 1                  (rest:247-254) */
int ciaosr_tile_blend_f32(float* E, float* Wt, int Himg, int Wimg, const float* tile_q3, int y0, int x0,
                          int th, int tw, void* stream);
/* out_q3[(y*W+x)*3+c] = E[c][y][x] / Wt[c][y][x]                          (rest:255-256) */
int ciaosr_tile_finalize_f32(const float* E, const float* Wt, float* out_q3, int Himg, int Wimg, void* stream);

/* ---- views: an encoded scene seen through an affine map (an extension, absent from the reference) ------------------------------------
 * A view is an output grid Hv x Wv and a host matrix m[6] = {m_yy, m_yx, t_y, m_xy, m_xx, t_x} (y first).  Output pixel (i, j), query
 * q = i Wv + j, has its centre at v = i + 0.5, u = j + 0.5 and maps to LR pixel units (the image is [0, h) x [0, w), LR pixel k has its
 * centre at k + 0.5):
 *     y_lr = (m_yy v + m_yx u) + t_y,   x_lr = (m_xy v + m_xx u) + t_x
 * in fp64, every operation rounded on its own (no FMA).  A frame or tile {y0, x0, th, tw} (ints, LR pixels; the whole image is
 * {0, 0, h, w}) owns the queries with y0 <= y_lr < y0 + th and x0 <= x_lr < x0 + tw, decided in fp64: tile_plan's centre membership.
 * In that frame coord = fp32(((y_lr - y0) / th) 2 - 1) (likewise x), one rounding of an fp64 value, and the cell -- constant over an
 * affine view -- is fp32(hypot(m_yy, m_yx) 2 / th), fp32(hypot(m_xy, m_xx) 2 / tw), the norms made on the host in fp64.  An
 * axis-aligned view is NOT bitwise ciaosr_make_coord_cell_window_f32's grid (three fp32 roundings there): the two differ by <= 2^-22.
 * Hv Wv <= 2^31 - 1.  No entry allocates, synchronises or keeps state; no atomics: every result is bitwise repeatable. */
/* queries per workgroup of count / select (their workspace holds one int per tile and workgroup) */
int ciaosr_view_block_queries(void);
size_t ciaosr_view_workspace_bytes(int Hv, int Wv, int n_tiles);
/* coord, cell [Hv Wv][2] of the whole grid in one frame (host ints), members or not */
int ciaosr_view_coord_cell_f32(float* coord, float* cell, const double* m /*host [6]*/, int Hv, int Wv, const int* frame /*host [4]*/,
                               void* stream);
/* count: one pass over all queries.  tiles: n_tiles x {y0, x0, th, tw} on the DEVICE, 16-byte aligned.  counts [n_tiles] (device): the
 * members of every tile.  workspace (ciaosr_view_workspace_bytes, 4-byte aligned): per tile, the exclusive scan over the workgroups of
 * their member counts -- what select places a tile's members with; valid until the next count on the same workspace. */
int ciaosr_view_count_i32(const double* m /*host [6]*/, int Hv, int Wv, const int* tiles, int n_tiles, int* counts, void* workspace,
                          size_t workspace_bytes, void* stream);
/* count for a list of views in one go: m [n_views][6] and sizes [n_views][2] = (Hv, Wv) on the host, the tiles as above.  One count
 * launch covers the workgroups of every view (the views travel by value as kernel arguments: no staging copy, nothing allocated), one
 * scan launch follows with a wave per (view, tile); a list longer than ciaosr_view_count_many_max_views() is further launch pairs on the
 * same stream, without synchronisation.  counts [n_views][n_tiles] (device).  The workspace holds every view's single-view part array
 * (the ciaosr_view_workspace_bytes layout) at ciaosr_view_many_workspace_offset(view), a multiple of 256 bytes: counts[v] and the part
 * array of view v are bitwise what ciaosr_view_count_i32 writes for that view alone, and ciaosr_view_select_f32 runs unchanged on
 * workspace + offset(view).  Sizes are 0 for a list the count refuses. */
int ciaosr_view_count_many_max_views(void);
size_t ciaosr_view_many_workspace_bytes(const int* sizes /*host [n_views][2]*/, int n_views, int n_tiles);
size_t ciaosr_view_many_workspace_offset(const int* sizes /*host [n_views][2]*/, int n_views, int n_tiles, int view);
int ciaosr_view_count_many_i32(const double* m /*host [n_views][6]*/, const int* sizes /*host [n_views][2]*/, int n_views, const int* tiles,
                               int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream);
/* select: the members of tile `tile_index` of the list count saw (`tile`: its four ints, host), in increasing q: q_index [n], coord and
 * cell [n][2] in the tile's frame, n = counts[tile_index] (nothing is written past n). */
int ciaosr_view_select_f32(const double* m /*host [6]*/, int Hv, int Wv, const int* tile /*host [4]*/, int tile_index, int n_tiles,
                           const void* workspace, size_t workspace_bytes, int n, int* q_index, float* coord, float* cell, void* stream);
/* Members in blocks.  The output grid is cut into blocks 4 wide x 2 high, row-major over ceil(Hv / 2) x ceil(Wv / 4) blocks: block
 * b = by * ceil(Wv / 4) + bx holds the output pixels (2 by + (e >> 2), 4 bx + (e & 3)), e = 0 .. 7 -- the eight queries the chained
 * 16-bit head kernel walks as one row tile on a grid.  A block with at least one member of a tile is a live block of that tile.
 * count_blocks: counts [n_tiles][2] (device) = (members, live blocks) of every tile; the member count is ciaosr_view_count_i32's.  One
 * thread per block, ciaosr_view_block_blocks() blocks per workgroup; workspace (ciaosr_view_blocks_workspace_bytes, 4-byte aligned):
 * per tile two rows of one int per workgroup, the exclusive scans of the member and of the live-block counts.  The _many form is
 * ciaosr_view_count_many_i32's scheme (views by value, groups of ciaosr_view_count_many_max_views(), counts [n_views][n_tiles][2], view
 * v's single-view workspace at ciaosr_view_blocks_many_workspace_offset).
 * select_blocks: the live blocks of tile `tile_index` in increasing b, 8 entries each, entry e of a block at list position 8 r + e
 * (r: the block's rank among the tile's live blocks): q_index [8 n_blocks], coord and cell [8 n_blocks][2], n_blocks = counts[tile][1].
 * A member entry holds its q and exactly ciaosr_view_select_f32's coord and cell for that q.  Any other entry -- a pixel that is no
 * member of the tile, or lies outside the output grid -- is a PAD: q_index = -1, coord and cell copied from the block's first member
 * in entry order (so a pad adds no key pixel to the row tile); ciaosr_view_blend_f32 skips it.  The list can be longer than Hv Wv
 * (small odd grids).  A row tile of the list fits the chained kernel's 4 x 4 window of key pixels for every translation iff
 * 3 |m_yx| + |m_yy| <= 2 and 3 |m_xx| + |m_xy| <= 2: the caller's test, nothing here depends on it. */
int ciaosr_view_block_blocks(void);
size_t ciaosr_view_blocks_workspace_bytes(int Hv, int Wv, int n_tiles);
int ciaosr_view_count_blocks_i32(const double* m /*host [6]*/, int Hv, int Wv, const int* tiles, int n_tiles, int* counts, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t ciaosr_view_blocks_many_workspace_bytes(const int* sizes /*host [n_views][2]*/, int n_views, int n_tiles);
size_t ciaosr_view_blocks_many_workspace_offset(const int* sizes /*host [n_views][2]*/, int n_views, int n_tiles, int view);
int ciaosr_view_count_blocks_many_i32(const double* m /*host [n_views][6]*/, const int* sizes /*host [n_views][2]*/, int n_views,
                                      const int* tiles, int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_view_select_blocks_f32(const double* m /*host [6]*/, int Hv, int Wv, const int* tile /*host [4]*/, int tile_index, int n_tiles,
                                  const void* workspace, size_t workspace_bytes, int n_blocks, int* q_index, float* coord, float* cell,
                                  void* stream);
/* blend: E[c][q_index[s]] += rgb[s][c], Wt[q_index[s]] += 1 for s < n; E [3][Q], Wt [Q].  q_index = NULL: s itself (a tile that owns the
 * whole view; then n <= Q).  An index may appear once per call at most; one outside [0, Q) -- a pad of a block list -- is skipped. */
int ciaosr_view_blend_f32(float* E, float* Wt, int Q, const int* q_index /*may be NULL*/, const float* rgb, int n, void* stream);
/* finalize: out_q3[q][c] = E[c][q] / Wt[q] where Wt[q] > 0 (ciaosr_denorm_clamp_f32's input layout); elsewhere the value that
 * ciaosr_denorm_clamp_f32 with mean3 / std3 turns into fill3[c] (in [0, 1], the output's space) -- exactly, whenever some fp32 value
 * near (fill - mean) / std does (always for 0 and 1, which the clamp reaches), else into the nearest value it can give. */
int ciaosr_view_finalize_f32(const float* E, const float* Wt, float* out_q3, int Q, const float* fill3 /*host*/, const float* mean3 /*host*/,
                             const float* std3 /*host*/, void* stream);

/* ---- warps: an encoded scene seen through a homography or a per-pixel coordinate map (an extension, absent from the reference) --------
 * A warp is an output grid Hv x Wv, a POINT SOURCE that gives output pixel (i, j), query q = i Wv + j, an LR position (y_lr, x_lr) in the
 * views' LR pixel units, and ONE footprint {f_y, f_x} (host doubles): the LR extent of an output pixel along each LR axis.  Every entry
 * takes exactly one point source, the other pointer NULL (else CIAOSR_ERR_BAD_ARG):
 *   h9  (host [9]) = {h00, h01, h02, h10, h11, h12, h20, h21, h22}, y first.  With v = i + 0.5, u = j + 0.5, in fp64, every operation
 *       rounded on its own (no FMA), IEEE division:
 *           Y = (h00 v + h01 u) + h02,  X = (h10 v + h11 u) + h12,  D = (h20 v + h21 u) + h22,  y_lr = Y / D,  x_lr = X / D.
 *       Finite entries, and D > 0 at the corners (v, u) = (0, 0), (Hv, 0), (0, Wv), (Hv, Wv) of the grid -- D is affine, so it is then
 *       positive on all of it: the horizon does not cross the output.  With the last row {0, 0, 1} the position is a view's, bit for bit.
 *   map (device, 16-byte aligned, [Hv Wv][2] doubles) = (y_lr, x_lr) of every query, read as one 16-byte load.  A NaN or infinite entry
 *       belongs to no tile.
 * After the position everything is the view's: membership and coord as above, cell = fp32(f_y 2 / th), fp32(f_x 2 / tw) -- constant over
 * the warp -- and blend / finalize are ciaosr_view_blend_f32 / ciaosr_view_finalize_f32.  The footprint is finite and positive.  Count,
 * workspace and select are ciaosr_view_count_i32's scheme and layout (ciaosr_view_block_queries() queries per workgroup); sizes are 0
 * for what count refuses.  Hv Wv <= 2^31 - 1.  No entry allocates, synchronises or keeps state; no atomics: bitwise repeatable. */
size_t ciaosr_warp_workspace_bytes(int Hv, int Wv, int n_tiles);
int ciaosr_warp_coord_cell_f32(float* coord, float* cell, const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/,
                               const double* footprint /*host [2]*/, int Hv, int Wv, const int* frame /*host [4]*/, void* stream);
int ciaosr_warp_count_i32(const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/, const double* footprint /*host [2]*/,
                          int Hv, int Wv, const int* tiles, int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_warp_select_f32(const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/, const double* footprint /*host [2]*/,
                           int Hv, int Wv, const int* tile /*host [4]*/, int tile_index, int n_tiles, const void* workspace,
                           size_t workspace_bytes, int n, int* q_index, float* coord, float* cell, void* stream);

/* ---- per-pixel warps: a footprint per output pixel ---------------------------------------------------------------------------------------
 * A per-pixel warp is a warp whose footprint is a function of the output pixel.  Positions, membership, frame coordinates, tile plan,
 * blend, fill, the quantised / grey / RGBA outputs and the one device-to-host copy are the existing warp's, unchanged.
 * RAW FOOTPRINT (g_y, g_x) of output pixel (i, j), in fp64, every operation rounded on its own, no FMA, from one of three sources (mode):
 *   1  Jacobian (h9 only).  v = i + 0.5, u = j + 0.5, and D, y_lr, x_lr the warp's:  g_y = sqrt(a a + b b) with a = (h00 - y_lr h20) / D,
 *      b = (h01 - y_lr h21) / D;  g_x the same with h10, h11, x_lr.  sqrt of the rounded sum, not hypot.
 *   2  Differences (map only; Hv > 1 and Wv > 1).  Per map component c and grid axis the derivative is (p[+1] - p[-1]) * 0.5 where both
 *      neighbours lie in the grid and are finite, else the one-sided difference with the one neighbour that is in the grid and finite
 *      (p[+1] - p[0] or p[0] - p[-1]), else the pixel has no footprint.  g_y = sqrt(dv_y dv_y + du_y du_y), likewise g_x.  The four
 *      neighbours are 16-byte loads like the centre's.
 *   3  Tensor (either point source): tensor (device, 16-byte aligned, [Hv Wv][2] doubles) = (g_y, g_x), one 16-byte load per query.
 * CLAMP  range = {lo, hi} (host doubles, finite, 0 < lo <= hi): f = min(max(g, lo), hi) per axis; +inf clamps to hi.  A raw footprint with
 * a NaN component, or a pixel without footprint, makes the pixel a non-member of every tile, exactly as a NaN position does.
 * CELL of a member in a th x tw frame: fp32(f_y 2 / th), fp32(f_x 2 / tw), written per member by select and coord_cell (a NaN cell in
 * coord_cell where the pixel has no footprint).  The head is queried with chunk = 1 for such a warp: the shift radius of a query comes
 * from its own cell.  A per-pixel warp whose footprints happen to be constant is the single-footprint warp of that constant, bit for bit.
 * ciaosr_ppwarp_footprints_f64 writes the clamped footprints of the whole grid, out (device, 16-byte aligned) [Hv Wv][2] doubles, NaN
 * where the pixel has none.  Workspace and layout are ciaosr_warp_workspace_bytes / ciaosr_warp_count_i32's.  CIAOSR_ERR_BAD_ARG before
 * any launch for: what the warp entries refuse, a mode that does not fit the point source, a null or misaligned tensor in mode 3,
 * lo <= 0, lo > hi, a non-finite range, a grid axis of 1 in mode 2. */
int ciaosr_ppwarp_coord_cell_f32(float* coord, float* cell, const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/,
                                 int mode, const double* range /*host [2]*/, const double* tensor /*device or NULL*/, int Hv, int Wv,
                                 const int* frame /*host [4]*/, void* stream);
int ciaosr_ppwarp_count_i32(const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/, int mode,
                            const double* range /*host [2]*/, const double* tensor /*device or NULL*/, int Hv, int Wv, const int* tiles,
                            int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_ppwarp_select_f32(const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/, int mode,
                             const double* range /*host [2]*/, const double* tensor /*device or NULL*/, int Hv, int Wv,
                             const int* tile /*host [4]*/, int tile_index, int n_tiles, const void* workspace, size_t workspace_bytes, int n,
                             int* q_index, float* coord, float* cell, void* stream);
int ciaosr_ppwarp_footprints_f64(double* out, const double* h9 /*host [9] or NULL*/, const double* map /*device or NULL*/, int mode,
                                 const double* range /*host [2]*/, const double* tensor /*device or NULL*/, int Hv, int Wv, void* stream);

/* ---- area-sampled warps: a per-pixel warp that supersamples where it minifies (version 372) -----------------------------------------------
 * A homography warp (h9; there is no map source) with the per-pixel warp's raw footprint (g_y, g_x), mode 1 (Jacobian) or 3 (tensor), and
 * N = max_samples in {1, 2, 4, 8}.  Per output pixel q = i Wv + j, fp64, every operation rounded on its own:
 *   COUNT per axis: n = 1; while n < N and g > hi n: n = 2 n (+inf: N).  A NaN component: the pixel has no samples.
 *   FOOTPRINT of its samples: f = min(max(g / n, lo), hi) per axis (where g > N hi the pixel is under-sampled, f = hi).
 *   SAMPLE s = a n_x + b (a < n_y, b < n_x) sits at v = i + (2a + 1) / (2 n_y), u = j + (2b + 1) / (2 n_x) (exact), its LR position is the
 *   warp's homography formula at (v, u); membership, coord and cell = fp32(f 2 / t) follow the warp's rules, per sample.
 *   SAMPLE ID = first[q] + s, first the exclusive prefix sum of n_y n_x in row-major q, S = first[Hv Wv] the total.
 * The accumulators are E [3][S], Wt [S]; ciaosr_view_blend_f32 blends a tile's answers with Q = S.  Hv Wv N N <= 2^31 - 1.
 * count builds the table in the workspace (per-workgroup sums of a wave-prefix scan, a one-wave scan over the workgroups, no atomics), then
 * counts and scans tile membership over SAMPLES (ciaosr_view_block_queries() consecutive sample ids per workgroup):
 *   counts [n_tiles + 2] = the samples in each tile, then S, then the number of pixels with exactly one sample (== Hv Wv: nothing is
 *   supersampled and every pixel has a footprint -- the warp is the per-pixel warp).
 * select writes the n samples of one tile in increasing sample id: s_index, coord, cell.  resolve writes the image out_chw [3][Hv][Wv]:
 * per pixel and channel the fp32 sum, in the order s = 0 .. n_y n_x - 1, of clamp(add(mul(x, std), mean), 0, 1) -- ciaosr_denorm_clamp_f32's
 * arithmetic -- of x = E / Wt where Wt > 0, else ciaosr_view_finalize_f32's fill value; times 1 / (n_y n_x); a pixel without samples holds
 * what the fill value gives.  table exports first [Hv Wv + 1] and n [Hv Wv][2] = (n_y, n_x), (0, 0) without samples.  select and resolve
 * read the workspace count (or table) filled for the same arguments.  CIAOSR_ERR_BAD_ARG before any launch for a null or misaligned pointer,
 * a bad size, mode or range, max_samples outside {1, 2, 4, 8}; CIAOSR_ERR_WORKSPACE for a short workspace; the size is 0 for what count
 * refuses.  Nothing allocates, synchronises or keeps state; bitwise repeatable. */
size_t ciaosr_areawarp_workspace_bytes(int Hv, int Wv, int n_tiles, int max_samples);
int ciaosr_areawarp_count_i32(const double* h9 /*host [9]*/, int mode, const double* range /*host [2]*/, const double* tensor /*device or NULL*/,
                              int max_samples, int Hv, int Wv, const int* tiles, int n_tiles, int* counts /*[n_tiles + 2]*/, void* workspace,
                              size_t workspace_bytes, void* stream);
int ciaosr_areawarp_select_f32(const double* h9 /*host [9]*/, int max_samples, int Hv, int Wv, const int* tile /*host [4]*/, int tile_index,
                               int n_tiles, const void* workspace, size_t workspace_bytes, int S, int n, int* s_index, float* coord,
                               float* cell, void* stream);
int ciaosr_areawarp_resolve_f32(const float* E, const float* Wt, float* out_chw, int S, int max_samples, int Hv, int Wv, int n_tiles,
                                const void* workspace, size_t workspace_bytes, const float* fill3 /*host*/, const float* mean3 /*host*/,
                                const float* std3 /*host*/, void* stream);
int ciaosr_areawarp_table_i32(int* first /*[Hv Wv + 1]*/, int* n /*[Hv Wv][2]*/, const double* h9 /*host [9]*/, int mode,
                              const double* range /*host [2]*/, const double* tensor /*device or NULL*/, int max_samples, int Hv, int Wv,
                              int n_tiles, void* workspace, size_t workspace_bytes, void* stream);

/* ---- self-ensemble: the eight flips and transposes of an image, and the mean through their inverses (an extension, absent from the
 * reference) ---------------------------------------------------------------------------------------------------------------------------
 * k in 0..7.  T_k acts on the last two axes of [planes][H][W]: k & 1: flip the columns; then k & 2: flip the rows; then k & 4: transpose
 * the two axes.  U_k is its inverse: transpose if k & 4, then flip the rows if k & 2, then flip the columns if k & 1.  T_0 is the identity.
 * Pure data movement, fp32, bitwise repeatable; nothing is allocated or synchronised.  Both entries refuse, before any launch, with
 * CIAOSR_ERR_BAD_ARG: k outside 0..7, a non-positive size, a null pointer, dst == src / acc == src, a negative or non-finite divisor
 * (and, CIAOSR_ERR_UNSUPPORTED, an image of more than 2^31 - 1 workgroups: rows x ceil(W / 1024), or 64 x 64 tiles). */
/* dst = T_k(src): src [planes][H][W], dst [planes][H][W], or [planes][W][H] when k & 4 */
int ciaosr_dihedral_f32(const float* src, float* dst, int planes, int H, int W, int k, void* stream);
/* acc = (first ? 0 : acc) + U_k(src), one correctly rounded fp32 add per element; then, with divisor > 0, acc = acc / divisor, one
 * correctly rounded division.  acc [planes][H][W] in the ORIGINAL orientation, src in member orientation ([planes][W][H] when k & 4).
 * With `first` acc is never read: the caller needs no memset.  The self-ensemble mean of members k_0 .. k_{n-1} is n calls in member
 * order, `first` on the first and divisor = n on the last. */
int ciaosr_dihedral_accum_f32(float* acc, const float* src, int planes, int H, int W, int k, int first, float divisor, void* stream);

/* ---- test data: GT -> LR degradation (configs/001_*.py, val_scale > 4) ---------------------- */
/* Pillow-exact bicubic resample of an 8-bit RGB image, PIL Image.resize((Wo, Ho), BICUBIC) -- the resize of mmedit's
 * RandomDownSampling (mmcv.imresize, backend 'pillow').  src[y * pitch + 3 x + c] (bytes), the top-left H x W of a possibly wider
 * image; pitch >= 3 W.  Tables per axis, built by the host in float64 in Pillow's order (ciaosr_amd/degrade.py):
 * bounds [n_out][2] = (first input, tap count), coef [n_out][ksize] int32 with 22 fractional bits.  Horizontal pass only if
 * Wo != W, vertical only if Ho != H (the other axis's tables may be NULL); out = clip((1 << 21 + sum src * coef) >> 22, 0, 255).
 * Writes dst_u8 [Ho][Wo][3] and / or dst_chw [3][Ho][Wo] = dst_u8 / 255 (fp32, correctly rounded); either may be NULL.
 * The source rows are read in aligned 16-byte blocks: bytes next to the image within such a block are read, never used.
 * workspace: 16-byte aligned, ciaosr_resample_u8_workspace_bytes().  H, Ho <= 65535; CIAOSR_ERR_UNSUPPORTED beyond a
 * ~4000x horizontal down-scale. */
size_t ciaosr_resample_u8_workspace_bytes(int H, int W, int Ho, int Wo);
int ciaosr_resample_u8(const unsigned char* src, size_t pitch, int H, int W, int Ho, int Wo, const int* bounds_x, const int* coef_x,
                       int ksize_x, const int* bounds_y, const int* coef_y, int ksize_y, unsigned char* dst_u8, float* dst_chw,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- evaluation on 8-bit images (mmedited/models/restorers/basic_restorer.py:101-124) -------- */
#define CIAOSR_METRIC_PSNR 1
#define CIAOSR_METRIC_SSIM 2
/* mmedit.core.tensor2img (called at basic_restorer.py:108-109; restated in ciaosr_amd/metrics.py:10-25) for min_max = (0, 1) and
 * out_type uint8: src_chw [3][H][W] fp32 RGB -> dst_hwc[y * dst_pitch + 3 x + c] bytes in BGR order, each
 * rint(clamp(v, 0, 1) * 255) with one fp32 multiply and round-half-to-even; NaN -> 0.  dst_pitch >= 3 W.  H <= 65535. */
int ciaosr_tensor2img_u8(const float* src_chw, int H, int W, unsigned char* dst_hwc, size_t dst_pitch, void* stream);
/* psnr and ssim of mmedited/core/evaluation/metrics.py:181-226 and :229-318 on two 8-bit BGR images a, b [H][W][3] with row pitches
 * in bytes (>= 3 W), in one pass.  crop_border pixels are removed on every side first.  convert_to_y = 1: both metrics on
 * Y = mmcv.bgr2ycbcr(img / 255, y_only=True) * 255 evaluated in fp32 with individually rounded operations; 0: the three channels
 * separately.  SSIM: 11-tap Gaussian (sigma 1.5), separable 'valid' filter, C1 = 6.5025, C2 = 58.5225, filtered maps and all sums in
 * fp64.  want = CIAOSR_METRIC_PSNR | CIAOSR_METRIC_SSIM (either or both; the value of one does not depend on the other being asked for).
 * result: 12 doubles on the DEVICE, [channel 0..2][sum of squared differences, pixels, sum of the SSIM map, map pixels] (channel 0
 * only with convert_to_y; unused entries 0): the host finishes with mse = sum sse / sum pixels, PSNR = 10 log10(255^2 / mse),
 * SSIM = mean over channels of (sum / map pixels).  No atomics: bitwise reproducible, independent of the pitches.
 * workspace: 8-byte aligned, ciaosr_psnr_ssim_u8_workspace_bytes() (0 = unsupported geometry); fully rewritten by every call.
 * CIAOSR_ERR_UNSUPPORTED: 2 crop_border >= H or W, a cropped side < 11 with SSIM wanted, H or W > 2^20. */
size_t ciaosr_psnr_ssim_u8_workspace_bytes(int H, int W, int crop_border, int convert_to_y);
int ciaosr_psnr_ssim_u8(const unsigned char* a, size_t pitch_a, const unsigned char* b, size_t pitch_b, int H, int W, int crop_border,
                        int convert_to_y, int want, double* result, void* workspace, size_t workspace_bytes, void* stream);

/* ---- NIQE of an 8-bit image: the image work of niqe / niqe_core (mmedited/core/evaluation/metrics.py:340-532) -----------------------
 * img [H][W][3] BGR bytes with a row pitch (>= 3 W).  Y = round_half_even(mmcv.bgr2ycbcr(img / 255, y_only=True) * 255) of the image
 * without crop_border pixels on every side, cropped to whole 96x96 blocks; per scale (1, and 2 after MATLAB's antialiased bicubic
 * imresize by 0.5) the MSCN map (x - mu) / (sqrt|filter(x^2) - mu^2| + 1) with `window` (49 doubles on the DEVICE, row-major 7x7,
 * applied as scipy's convolve(mode='nearest')); per 96x96 / 48x48 block five maps -- the block and its products with itself rolled
 * (np.roll, wrapping inside the block) by [0,1], [1,0], [1,1], [1,-1] -- each reduced to six sums.
 * moments: doubles on the DEVICE, [scale 0..1][block][map 0..4][count of v < 0, sum v^2 over v < 0, count of v > 0, sum v^2 over
 * v > 0, sum |v|, sum v^2]; blocks = floor((H - 2 crop) / 96) * floor((W - 2 crop) / 96) in the reference's order: block
 * (row i, column j) at j * rows + i.  luma_out: optional fp32 [H - 2 crop][W - 2 crop], the rounded Y plane (NULL = not wanted).
 * Maps and sums are fp64; five launches for any size, no atomics: bitwise reproducible, independent of the pitch.
 * workspace: 256-byte aligned, ciaosr_niqe_workspace_bytes() (0 = unsupported geometry); fully rewritten by every call.
 * CIAOSR_ERR_UNSUPPORTED: H or W > 65535, or no whole block after the crop. */
size_t ciaosr_niqe_workspace_bytes(int H, int W, int crop_border);
int ciaosr_niqe_moments_u8(const unsigned char* img, size_t pitch, int H, int W, int crop_border, const double* window,
                           double* moments, float* luma_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG encoding of 8-bit images (opt-in: test_cfg.gpu_png; replaces the host's PIL save on the --save-path / --out path) ---------
 * Two stages, separately callable, and their composition.  Nothing here searches for LZ77 matches: the coder emits literals and
 * end-of-block only.  Bands are coded independently, one workgroup each.  All byte offsets are 64-bit. */
#define CIAOSR_PNG_HIST_STRIDE 260   /* unsigned ints per band in a histogram array: 256 literals, end-of-block, 3 unused */
/* rows of one band for an image W pixels wide: rows_per_band if > 0, else the default -- bands of about 128 KiB of filtered bytes,
 * max(1, 131072 / (3 W + 1)) rows.  0 for an invalid W. */
int ciaosr_png_rows_per_band(int W, int rows_per_band);
/* PNG scanline filter (colour type 2, 8 bits, no interlace, 3 bytes per pixel).  src[y * pitch + 3 x + c], pitch >= 3 W (a crop view of a
 * larger image is fine); bgr = 1: the bytes of a pixel are B G R (ciaosr_tensor2img_u8's order), 0: R G B.  H, W <= 65535.
 * dst: H rows of 1 + 3 W bytes: the filter type, then the filtered bytes in RGB order.  Per row the filter in {0 None, 1 Sub, 2 Up,
 * 3 Average, 4 Paeth} whose filtered bytes have the smallest sum of (b < 128 ? b : 256 - b); ties go to the lowest number.  The
 * predecessors are raw pixels (the row above row 0 is zeros), so rows and bands are independent.
 * hist [n_bands][CIAOSR_PNG_HIST_STRIDE]: per band of rows_per_band rows (0 = default; n_bands = ceil(H / rows)) the count of every byte
 * value of its part of dst, and 1 at index 256 (one end-of-block per band).
 * adler [n_bands][2]: per band (sum of its bytes, sum over its bytes of byte * (bytes from it to the band's end)) mod 65521, i.e.
 * the Adler-32 sums of the band from a = b = 0.  No workspace; bitwise repeatable. */
int ciaosr_png_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* dst,
                         unsigned int* hist, unsigned int* adler, void* stream);
/* Raw deflate of a byte buffer, one segment per band, Huffman-coded literals only.  data: device bytes; band_offsets: HOST array of
 * n_bands + 1 ascending byte offsets into data (band i = [band_offsets[i], band_offsets[i + 1])); an empty band is refused with
 * CIAOSR_ERR_BAD_ARG before anything is launched; a band above 2^31 bytes is CIAOSR_ERR_UNSUPPORTED.  The offsets reach the device by
 * hipMemcpyAsync on `stream`: keep the array valid until the stream has passed this call.
 * A segment is ONE dynamic-Huffman block -- literal / length code lengths <= 15 (257 codes: no length symbols), code-length-code
 * lengths <= 7, HDIST = 0 with its one distance code of length 0 -- followed by an empty stored block that byte-aligns it; or, when
 * that would not be smaller, stored blocks of at most 65535 bytes (5 framing bytes each).  Only the last band's last block carries
 * BFINAL, so the concatenation of the segments is one valid deflate stream.  Code lengths are built on the device, one wave per band.
 * out: 4-byte aligned, out_capacity >= ciaosr_deflate_huff_capacity_bytes(total, n_bands) (the all-stored worst case), else
 * CIAOSR_ERR_WORKSPACE; segment i is written to out[seg_offsets[i] .. seg_offsets[i + 1]), seg_offsets: n_bands + 1 values on the
 * DEVICE, seg_offsets[0] = 0 and seg_offsets[n_bands] = the stream's size.  Segments go straight to their final place (their exact
 * sizes follow from histogram x lengths + header before a bit is packed); a byte of out is written by one workgroup only and no
 * floating point or order-dependent atomic is involved: two calls give identical bytes.  workspace: 8-byte aligned,
 * ciaosr_deflate_huff_workspace_bytes(n_bands). */
size_t ciaosr_deflate_huff_workspace_bytes(int n_bands);
size_t ciaosr_deflate_huff_capacity_bytes(size_t total_bytes, int n_bands);
int ciaosr_deflate_huff_u8(const unsigned char* data, const unsigned long long* band_offsets /*host*/, int n_bands, unsigned char* out,
                           size_t out_capacity, unsigned long long* seg_offsets, void* workspace, size_t workspace_bytes, void* stream);
/* The composition: the zlib stream of a PNG's IDAT data.  out = 78 01, the deflate segments of the filtered bands (as
 * ciaosr_png_filter_u8 and ciaosr_deflate_huff_u8 make them, with the filter's histograms), the Adler-32 of the filtered stream
 * combined from the band partials (big-endian).  *total_bytes (DEVICE) = the stream's size.  The host reads that number, then the
 * stream: two synchronising copies per image.  out 4-byte aligned with ciaosr_png_capacity_bytes(), workspace 8-byte aligned with
 * ciaosr_png_workspace_bytes() (it holds the filtered image: H (3 W + 1) bytes, plus 2.4 KB per band); 0 = unsupported geometry. */
size_t ciaosr_png_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png_capacity_bytes(int H, int W, int rows_per_band);
int ciaosr_png_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                         size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* Many crops of one image in one set of launches (tile pyramids: ciaosr_amd/pyramid.py).  rects: HOST array [n_tiles][4] = y0, x0, h, w,
 * each non-empty and inside H x W; they may overlap.  Tile t's bytes out[tile_offs[t] : tile_offs[t + 1]] are one complete zlib stream,
 * byte for byte what ciaosr_png_encode_u8 returns for the pitched crop src + y0 * pitch + 3 * x0, pitch, h, w with the same
 * rows_per_band: the pixels left of a tile's first column and above its first row count as zeros, a tile's bands are
 * ciaosr_png_rows_per_band(w, rows_per_band) of ITS rows, the stored fallback and BFINAL are decided per tile.  tile_offs (DEVICE,
 * [n_tiles + 1], 8-byte aligned): tile_offs[0] = 0, the streams lie back to back without padding, tile_offs[n_tiles] is the total.  The
 * host reads tile_offs, then the streams: two synchronising copies per call, whatever n_tiles.  The band table built from the rects
 * (per band: tile, rows, 64-bit offset in the filtered streams) reaches the device by a copy on `stream` from pageable memory.  Four
 * launches: filter, plan, a segmented scan (one workgroup; sizes, a prefix sum over tiles, every band's offset, each tile's header and
 * its Adler-32 from its own bands' partials), pack.  No two workgroups write the same byte, the output is bitwise repeatable, nothing
 * needs zeroing, nothing is allocated.  An empty rect, one that leaves the image, n_tiles < 1 or a null pointer: CIAOSR_ERR_BAD_ARG
 * before any launch; a short out (ciaosr_png_tiles_capacity_bytes) or workspace (ciaosr_png_tiles_workspace_bytes: the filtered
 * crops, 2.4 KB per band, the table): CIAOSR_ERR_WORKSPACE.  The two size functions return 0 for rects they cannot take. */
size_t ciaosr_png_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                               int rows_per_band, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- RGBA: 8-bit images with an alpha channel, and their PNG files (colour type 6; version 320) -------------------------
 * An RGBA render is a render of two batch items: the colour image, and the alpha plane copied into three channels.  The colour bytes
 * of a pixel are ciaosr_tensor2img_u8's of item 0; with (B, G, R) = ciaosr_tensor2img_u8's bytes of item 1, its alpha is
 * A = (4899 R + 9617 G + 1868 B + 8192) >> 14 in integers (the weights sum to 16384: a grey v, v, v gives v).
 * colour_chw, alpha_chw: fp32 [3][H][W] RGB -> dst[y * dst_pitch + 4 x + c] bytes in B G R A order, in one pass; every byte by
 * ciaosr_tensor2img_u8's rule (one fp32 multiply, round half to even, clamp, NaN -> 0).  dst_pitch >= 4 W (a 4-byte aligned dst and
 * pitch get one 32-bit store per pixel; any other is written in single bytes).  H <= 65535. */
int ciaosr_tensor2img_bgra_u8(const float* colour_chw, const float* alpha_chw, int H, int W, unsigned char* dst, size_t dst_pitch,
                              void* stream);
/* The same packing from two 8-bit images (the resized pyramid levels): bgr [H][W][3] B G R with `pitch` >= 3 W gives B G R, grey_bgr
 * likewise with `pitch_grey` gives A by the formula above.  dst as above. */
int ciaosr_pack_bgra_u8(const unsigned char* bgr, size_t pitch, const unsigned char* grey_bgr, size_t pitch_grey, int H, int W,
                        unsigned char* dst, size_t dst_pitch, void* stream);
/* The four-byte-per-pixel siblings of the PNG calls above, with the same arguments and contracts; where those say 3 W these say 4 W.
 * rows of one band: rows_per_band if > 0, else max(1, 131072 / (4 W + 1)).  src[y * pitch + 4 x + c], pitch >= 4 W, src and pitch
 * 4-byte ALIGNED (a pixel is one 32-bit load; a crop view of an aligned image is aligned) else CIAOSR_ERR_BAD_ARG; bgr = 1: the bytes
 * of a pixel are B G R A (ciaosr_tensor2img_bgra_u8's order), 0: R G B A.  A row of dst is 1 + 4 W bytes: the filter type, then the
 * filtered bytes in R G B A order.  The left predecessor of a byte is the same channel of the pixel before it (four bytes back), the
 * upper one the same byte of the row above; zeros stand left of column 0 and above row 0, of a crop too.  The filter choice, the
 * histogram, the Adler partials and the plan, scan and pack stages are the three-byte calls' own on the longer rows.  Tile t of
 * ciaosr_png_rgba_encode_tiles_u8 is byte for byte ciaosr_png_rgba_encode_u8 of the pitched crop src + y0 * pitch + 4 * x0: four
 * launches and two synchronising copies, whatever n_tiles.  The host wraps a stream with IHDR colour type 6. */
int ciaosr_png_rgba_rows_per_band(int W, int rows_per_band);
int ciaosr_png_rgba_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* dst,
                              unsigned int* hist, unsigned int* adler, void* stream);
size_t ciaosr_png_rgba_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png_rgba_capacity_bytes(int H, int W, int rows_per_band);
int ciaosr_png_rgba_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                              size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_png_rgba_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png_rgba_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_rgba_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                    int rows_per_band, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* ---- Grey: one byte per pixel, and its PNG (colour type 0) and JPEG (one component) files (version 340) -----------
 * The grey byte of a pixel whose three bytes are (B, G, R) is L = (19595 R + 38470 G + 7471 B + 32768) >> 16 in integers: Pillow's
 * convert('L') and libjpeg's luma.  The weights sum to 65536: a neutral v, v, v gives v.  It is NOT the alpha formula above (the two
 * differ by 1 on 39 135 of the 2^24 triples).
 * ciaosr_tensor2img_grey_u8: src_chw fp32 [3][H][W] RGB -> dst[y * dst_pitch + x] = L of ciaosr_tensor2img_u8's three bytes of the pixel
 * (one fp32 multiply, round half to even, clamp, NaN -> 0), in one pass.  dst_pitch >= W, any alignment (a 4-byte aligned dst and
 * pitch get one 32-bit store per four pixels; any other is written in single bytes).  H <= 65535.
 * ciaosr_grey_from_bgr_u8: the same reduction from an 8-bit image bgr[y * pitch + 3 x + c], pitch >= 3 W; bgr_flag = 1: the bytes of a
 * pixel are B G R, 0: R G B. */
int ciaosr_tensor2img_grey_u8(const float* src_chw, int H, int W, unsigned char* dst, size_t dst_pitch, void* stream);
int ciaosr_grey_from_bgr_u8(const unsigned char* bgr, size_t pitch, int bgr_flag, int H, int W, unsigned char* dst, size_t dst_pitch,
                            void* stream);
/* The one-byte-per-pixel siblings of the PNG calls (ciaosr_png_grey_*, colour type 0) are declared in ciaosr_hip_png_grey.h, which
 * this header includes at its end: every PNG size export declared in THIS file is one of those that tests/golden/png_sizes.json
 * records, and that record was made before the grey family existed. */
/* LZ77 matches, opt-in (version 330; png_hip `matches=True`; DESIGN 4.1i-b3 holds the contract).  The *_lz_* entry points take the
 * arguments of their namesakes above and give streams that decode to the same bytes; out needs the same capacity (stored blocks stay
 * a candidate), the workspace is larger (16 bits of token per filtered byte): ciaosr_png[_rgba]_lz_workspace_bytes and
 * ciaosr_png[_rgba]_lz_tiles_workspace_bytes, 0 = unsupported geometry.  Per band the filtered bytes are parsed greedily in chunks of
 * 4096 bytes counted from the band's start.  Candidate distances at a position, in this order: 1, 2, 3, 4, 6, 8, 12, 16, L - bpp, L,
 * L + bpp with L = 1 + bpp W the scanline length (of the tile, for tiles); one above 32768 or above the position's offset in its band
 * is skipped, so no match reads before its band and bands (and tiles) stay independent.  The length for a distance is the run of equal
 * bytes, capped at 258 and at the end of the chunk; the longest candidate wins, ties go to the earliest, and it is taken iff its length
 * is >= 8, else the byte is a literal.  A band is ONE dynamic block with a literal / length code of up to 286 symbols and a distance code
 * of up to 30 (both by the literal coder's construction, lengths <= 15, HLIT / HDIST trimmed, a single used distance symbol alone with
 * length 1), followed by the empty stored block -- where that is SMALLER than what the literal coder makes of the band (its Huffman
 * block or stored blocks), else that segment, byte for byte.  So no segment and no stream is longer than its namesake's.  The bytes
 * are bitwise repeatable.  Launches per call, whatever the number of bands or tiles: the filter, a memset of the match histograms,
 * deflate_lz_match, deflate_plan, deflate_lz_plan, the scan, deflate_pack, deflate_lz_pack; two synchronising copies as before.
 * ciaosr_deflate_lz_u8 is ciaosr_deflate_huff_u8 with matches: line = L (0: the eight near distances only) and bpp >= 1 with
 * line = 0 or line > bpp, else CIAOSR_ERR_BAD_ARG before any launch; out needs ciaosr_deflate_huff_capacity_bytes(total, n_bands),
 * the workspace ciaosr_deflate_lz_workspace_bytes(total, n_bands) with total = band_offsets[n_bands] - band_offsets[0]. */
size_t ciaosr_png_lz_workspace_bytes(int H, int W, int rows_per_band);
int ciaosr_png_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                            size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_png_lz_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                  int rows_per_band, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                  void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_png_rgba_lz_workspace_bytes(int H, int W, int rows_per_band);
int ciaosr_png_rgba_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                                 size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t ciaosr_png_rgba_lz_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_rgba_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/,
                                       int n_tiles, int rows_per_band, unsigned char* out, size_t out_capacity,
                                       unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_deflate_lz_workspace_bytes(size_t total_bytes, int n_bands);
int ciaosr_deflate_lz_u8(const unsigned char* data, const unsigned long long* band_offsets /*host*/, int n_bands, int line, int bpp,
                         unsigned char* out, size_t out_capacity, unsigned long long* seg_offsets, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- 16-bit samples: uint16 images and their PNG files of bit depth 16 (version 350) -------------------------------------
 * A 16-bit sample is q16(v) = rint(fp32(clamp(v, 0, 1) * 65535)): ciaosr_tensor2img_u8's rule with 65535 for 255 (one fp32 multiply,
 * round half to even, NaN -> 0).  An 8-bit level k / 255 becomes exactly 257 k; in general the 16-bit image is NOT the 8-bit image
 * shifted left, and its high byte is NOT ciaosr_tensor2img_u8's byte.  Samples are native (little-endian) uint16 in memory; every
 * pitch is in BYTES and, like every image pointer, EVEN (CIAOSR_ERR_BAD_ARG otherwise) -- the only alignment asked for: a crop of a
 * larger image may start at any pixel.
 * ciaosr_tensor2img_u16: src_chw fp32 [3][H][W] RGB -> the three samples of pixel (y, x) at byte y * dst_pitch + 6 x in B G R order,
 * dst_pitch >= 6 W.  ciaosr_tensor2img_grey_u16: one sample at byte y * dst_pitch + 2 x, dst_pitch >= 2 W:
 * L16 = (19595 R + 38470 G + 7471 B + 32768) >> 16 of the pixel's three 16-bit samples in unsigned 32-bit arithmetic (the largest
 * intermediate is 65535 * 65536 + 32768 < 2^32; the weights are the 8-bit grey byte's, a neutral v, v, v gives v).
 * ciaosr_grey_from_bgr_u16: the same reduction from a 16-bit image of three samples per pixel, pitch >= 6 W; bgr_flag as for the
 * 8-bit call.  H <= 65535. */
int ciaosr_tensor2img_u16(const float* src_chw, int H, int W, unsigned short* dst_hwc, size_t dst_pitch, void* stream);
int ciaosr_tensor2img_grey_u16(const float* src_chw, int H, int W, unsigned short* dst, size_t dst_pitch, void* stream);
int ciaosr_grey_from_bgr_u16(const unsigned short* bgr, size_t pitch, int bgr_flag, int H, int W, unsigned short* dst, size_t dst_pitch,
                             void* stream);
/* The PNG calls at bit depth 16, with the arguments and contracts of their 8-bit namesakes (ciaosr_png_*, ciaosr_png_lz_*):
 * ciaosr_png16_* for three samples per pixel (colour type 2; bgr = 1: B G R as ciaosr_tensor2img_u16 orders them, 0: R G B) and
 * ciaosr_png16_grey_* for one (colour type 0; bgr must be 0 or 1 and is not read).  With C = 3 or 1: pitch >= 2 C W bytes; a row of
 * the stream is 1 + 2 C W bytes, the filter type and then every sample BIG-endian, in R G B order; rows of one band: rows_per_band if
 * > 0, else max(1, 131072 / (2 C W + 1)).  The five filters work per BYTE, as the PNG specification says: the left predecessor of a
 * byte is the byte 2 C back (bpp = 6 or 2), the upper one the same byte of the row above, zeros left of column 0 and above row 0 (of a
 * crop too) -- nothing is borrowed between the two bytes of a sample.  The filter choice (smallest sum of min(b, 256 - b) over the
 * row's bytes, ties to the lowest number), the histograms, the Adler partials and the plan, scan and pack stages are the 8-bit calls'
 * own on these rows; the match candidates of the *_lz_* entries are 1, 2, 3, 4, 6, 8, 12, 16, L - 2 C, L, L + 2 C with L = 1 + 2 C W.
 * Tile t is byte for byte the single call on the pitched crop at byte y0 * pitch + 2 C x0.  The host wraps a stream with IHDR bit
 * depth 16.  (The names say png16_, not png_: the size exports whose values tests/golden/png_sizes.json records are the 8-bit ones.) */
int ciaosr_png16_rows_per_band(int W, int rows_per_band);
int ciaosr_png16_filter_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* dst,
                            unsigned int* hist, unsigned int* adler, void* stream);
size_t ciaosr_png16_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png16_lz_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png16_capacity_bytes(int H, int W, int rows_per_band);
int ciaosr_png16_encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                            size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_png16_lz_encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                               size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes,
                               void* stream);
size_t ciaosr_png16_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png16_lz_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png16_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png16_encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                  int rows_per_band, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                  void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_png16_lz_encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/,
                                     int n_tiles, int rows_per_band, unsigned char* out, size_t out_capacity,
                                     unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_png16_grey_rows_per_band(int W, int rows_per_band);
int ciaosr_png16_grey_filter_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* dst,
                                 unsigned int* hist, unsigned int* adler, void* stream);
size_t ciaosr_png16_grey_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png16_grey_lz_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png16_grey_capacity_bytes(int H, int W, int rows_per_band);
int ciaosr_png16_grey_encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                                 size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream);
int ciaosr_png16_grey_lz_encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band,
                                    unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t ciaosr_png16_grey_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png16_grey_lz_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png16_grey_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png16_grey_encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/,
                                       int n_tiles, int rows_per_band, unsigned char* out, size_t out_capacity,
                                       unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);
int ciaosr_png16_grey_lz_encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/,
                                          int n_tiles, int rows_per_band, unsigned char* out, size_t out_capacity,
                                          unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Deflate tiles of a pyramidal TIFF level (version 360; ciaosr_amd/tiff_hip.py; DESIGN 4.1i-b7 holds the format contract) ----------
 * A level is cut into T x T tiles (T a multiple of 16 in 16..4096), row-major, ceil(W / T) x ceil(H / T); a tile that reaches past the
 * image repeats its last column and row: P[r][c][k] = I[min(ty T + r, H - 1)][min(tx T + c, W - 1)][k], I the samples in stream order
 * (bgr = 1: the image holds B G R [A] and the stream R G B [A]; 0: as stored; one grey sample: bgr is checked and not read).  The
 * horizontal predictor (TIFF Predictor = 2) works per SAMPLE of S = 8 or 16 bits: D[r][0][k] = P[r][0][k],
 * D[r][c][k] = (P[r][c][k] - P[r][c - 1][k]) mod 2^S; the bytes are r, then c, then k, a 16-bit sample low byte first.  Tile t's data
 * (Compression = 8) is ONE zlib stream of those T * T * bytes_per_pixel bytes, out[tile_offs[t] : tile_offs[t + 1]], made by the PNG
 * calls' coder on lines of bytes_per_pixel * T bytes (no filter byte): the contracts of ciaosr_png_encode_tiles_u8 for out, capacity,
 * tile_offs (DEVICE, [tiles + 1], 8-byte aligned), workspace and stream hold, and the host reads tile_offs, then the bytes.
 * bytes_per_pixel: 1, 3, 4 (uint8 grey, RGB, RGBA) or 2, 6 (native uint16 grey, RGB); pitch in bytes, >= bytes_per_pixel * W; four
 * bytes per pixel are read as aligned 32-bit words, 16-bit samples as aligned 16-bit ones (image and pitch multiples of 4 / of 2).
 * Every source index is clamped: nothing is read past row H - 1 or column W - 1.  rows_per_band: tile rows per independently coded
 * band, at most T; 0 = max(1, min(T, 131072 / (bytes_per_pixel * T))).  ciaosr_tiff_lz_*: the match coder (ciaosr_png_lz_*), far
 * candidates L - bytes_per_pixel, L, L + bytes_per_pixel with L = bytes_per_pixel * T -- a padding row is a repeat at distance L; no
 * stream is longer than the literal coder's.  Launches per call, whatever the number of tiles: tiff_predict_tiles, deflate_plan,
 * png_tiles_scan, deflate_pack; the match coder adds one memset, deflate_lz_match, deflate_lz_plan and deflate_lz_pack.
 * The size functions return 0 for what the calls refuse (CIAOSR_ERR_BAD_ARG: bytes_per_pixel, T, H, W > 65535, a negative
 * rows_per_band, alignment).
 * ciaosr_halve_box_u16: uint16 [h][w][channels] (channels 1 or 3; pitches in bytes, even, >= one row) ->
 * [ceil(h / 2)][ceil(w / 2)][channels]: out[i][j][k] = (a[2i][2j] + a[2i][j1] + a[i1][2j] + a[i1][j1] + 2) >> 2 with
 * i1 = min(2i + 1, h - 1), j1 = min(2j + 1, w - 1), in unsigned 32-bit arithmetic. */
int ciaosr_tiff_rows_per_band(int bytes_per_pixel, int T, int rows_per_band);
size_t ciaosr_tiff_tiles_workspace_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band);
size_t ciaosr_tiff_lz_tiles_workspace_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band);
size_t ciaosr_tiff_tiles_capacity_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band);
int ciaosr_tiff_encode_tiles(int bytes_per_pixel, const void* image, size_t pitch, int H, int W, int bgr, int T, int rows_per_band,
                             unsigned char* out, size_t out_capacity, unsigned long long* tile_offs, void* workspace,
                             size_t workspace_bytes, void* stream);
int ciaosr_tiff_lz_encode_tiles(int bytes_per_pixel, const void* image, size_t pitch, int H, int W, int bgr, int T, int rows_per_band,
                                unsigned char* out, size_t out_capacity, unsigned long long* tile_offs, void* workspace,
                                size_t workspace_bytes, void* stream);
int ciaosr_halve_box_u16(const unsigned short* src, size_t pitch, int h, int w, int channels, unsigned short* dst, size_t dst_pitch,
                         void* stream);

/* ---- Baseline JPEG encoding of 8-bit images (ciaosr_amd/jpeg_hip.py; DESIGN 4.1i-d holds the format contract) ----------------------
 * The device makes the entropy-coded data of ONE interleaved scan of a baseline file -- libjpeg's integer pipeline as Pillow drives
 * it: 16-bit fixed-point RGB -> YCbCr, 4:4:4 or 4:2:0 with the h2v2 box filter, the "islow" forward DCT, the Annex K tables scaled by
 * `quality` (1..100), the Annex K Huffman codes, no restart markers -- with a 0x00 after every 0xFF and the last byte padded with
 * 1-bits.  The host wraps it: SOI, APP0, two DQT, SOF0, four DHT and the SOS header in front (they depend on h, w, quality and
 * subsampling only), EOI behind.  The file is then byte for byte PIL.Image.save(format='JPEG', quality=, subsampling=)'s.
 * src[y * pitch + 3 x + c], pitch >= 3 W (a crop view is fine); bgr as for the PNG entry points; H, W <= 65535.
 * mcus_per_chunk: MCUs (8 x 8 pixels in 4:4:4, 16 x 16 in 4:2:0) that one workgroup codes; 0 = the library's choice (768 blocks).
 * The bytes do not depend on it, nor on the stream, nor -- for tiles -- on what else is in the list.  All arithmetic is integer.
 * Sizes: a block takes at most 208 bytes before stuffing (64 x (16-bit code + 10 bits)) and twice that after;
 * ciaosr_jpeg_capacity_bytes returns that WORST CASE, 416 bytes per block of the scan (dummy blocks included), so that nothing can
 * ever be written at or beyond out_capacity; a shorter out, or a workspace below ciaosr_jpeg_workspace_bytes (int16 coefficients,
 * 4 bytes per block, the unstuffed stream's worst case, 52 bytes per chunk, the table: 16 per chunk, 32 per tile) is CIAOSR_ERR_WORKSPACE before any launch.
 * quality outside 1..100, a subsampling other than the two below, a null pointer, an empty rect or one that leaves the image:
 * CIAOSR_ERR_BAD_ARG before any launch.  The size functions return 0 for what they cannot take.
 * *total_bytes (DEVICE, 8-byte aligned) = the scan's size; the host reads it, then the bytes: two synchronising copies per call.
 * Eight launches per call whatever the number of tiles: coefficients, code lengths, a scan, zeroing of the unstuffed buffer, pack,
 * 0xFF count, a scan, stuffing.  The table of constants, tiles and chunks reaches the device by a copy on `stream` from pageable
 * memory.  The workspace is 8-byte aligned; nothing is allocated. */
#define CIAOSR_JPEG_444 0   /* Pillow's subsampling=0 */
#define CIAOSR_JPEG_420 2   /* Pillow's subsampling=2 */
/* One component (version 340): Pillow's mode-L file, PIL.Image.fromarray(grey, 'L').save(format='JPEG', quality=).  Accepted as
 * `subsampling` by the ciaosr_jpeg_* and ciaosr_jpeg_opt_* entries: src[y * pitch + x], pitch >= W, bgr is not read; one 8 x 8 block
 * per MCU, the luma quantisation table, Huffman tables 0, no dummy blocks (edges repeat the crop's last column and row), the DC
 * predictor chain over consecutive blocks.  Capacity: 416 bytes per block; optimised 2 x ceil(1665 x blocks / 8).  An optimised
 * call's `result` keeps its layout, the records k = 2, 3 all zero.  The host writes one DQT, SOF0 with the component (1, 0x11, 0), two
 * DHT (0x00, 0x10) and a one-component SOS.  The ciaosr_jpeg_prog_* entries refuse it: size 0, CIAOSR_ERR_UNSUPPORTED before any
 * launch.  The values 1 and 3 stay invalid. */
#define CIAOSR_JPEG_GREY 4
size_t ciaosr_jpeg_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_capacity_bytes(int H, int W, int subsampling);
int ciaosr_jpeg_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                          int mcus_per_chunk, unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Many crops of one image in one set of launches.  rects: HOST array [n_tiles][4] = y0, x0, h, w as for ciaosr_png_encode_tiles_u8.
 * A crop is an image of its own: its MCU grid starts at its origin, its edges repeat ITS last column and row whatever the image holds
 * beyond them, its DC predictors start at 0.  Tile t's scan is out[tile_offs[t] : tile_offs[t + 1]], byte for byte what
 * ciaosr_jpeg_encode_u8 gives for the pitched crop; tile_offs (DEVICE, [n_tiles + 1], 8-byte aligned): tile_offs[0] = 0, the scans lie
 * back to back, tile_offs[n_tiles] is the total.  The host reads tile_offs, then the bytes. */
size_t ciaosr_jpeg_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int subsampling);
int ciaosr_jpeg_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);
/* The same files with OPTIMISED Huffman tables (Pillow's optimize=True, libjpeg's optimize_coding): everything up to the
 * quantised coefficients and the symbols of the scan is as above; the four Huffman tables are derived per crop from the histograms
 * of the symbols its scan emits (dummy blocks count; Cb and Cr share two tables), by libjpeg's rule with its tie-breaks and its
 * limiting to 16 bits.  Ten launches per call whatever the number of tiles -- the eight above with jpeg_hist and jpeg_tables between
 * the coefficients and the code lengths -- and one memset of the histograms on `stream`.
 * `result` (DEVICE, 8-byte aligned, ciaosr_jpeg_opt_result_bytes(n_tiles) = 8 (n_tiles + 1) + 1088 n_tiles bytes) receives BOTH the
 * offsets and the tables, so that the host still reads twice per call (result, then the scans):
 *   bytes [0, 8 (n_tiles + 1))            unsigned long long tile_offs[n_tiles + 1], as above
 *   then per tile t, per table k = 0..3   one record of CIAOSR_JPEG_DHT_RECORD_BYTES = 272 bytes at 8 (n_tiles + 1) + 272 (4 t + k):
 *                                         16 bytes: the number of codes of length 1..16; 256 bytes: the symbols in code order, of which
 *                                         the first sum(counts) are valid, the rest 0.
 * k is the file's order of DHT segments: 0 DC luma (0x00), 1 AC luma (0x10), 2 DC chroma (0x01), 3 AC chroma (0x11); a segment's
 * payload is its class/id byte, the 16 counts and exactly sum(counts) symbols.  ciaosr_jpeg_opt_encode_u8 is the call for ONE rect
 * (0, 0, H, W): its result holds tile_offs[2] = {0, total} and four records, 16 + 1088 bytes.
 * Sizes: with arbitrary codes of up to 16 bits a block takes at most 16 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1665 bits (the
 * Annex K codes: 1658), so the capacity functions below return sum over the crops of 2 x ceil(1665 x blocks / 8) and the workspace
 * holds ceil(1665 x blocks / 8) bytes of unstuffed stream per crop, 4 KB of histograms and 2176 bytes of code tables per tile on top
 * of the rest.  A crop whose scan has 64 x blocks >= 1 000 000 000 (all components, dummy blocks included) is refused: the size
 * functions return 0, the calls CIAOSR_ERR_UNSUPPORTED before any launch (libjpeg's search never selects a larger frequency; below
 * the limit 32-bit counters suffice).  Every other refusal is as above. */
#define CIAOSR_JPEG_DHT_RECORD_BYTES 272
size_t ciaosr_jpeg_opt_result_bytes(int n_tiles);
size_t ciaosr_jpeg_opt_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_opt_capacity_bytes(int H, int W, int subsampling);
int ciaosr_jpeg_opt_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                              int mcus_per_chunk, unsigned char* out, size_t out_capacity, void* result, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t ciaosr_jpeg_opt_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_opt_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int subsampling);
int ciaosr_jpeg_opt_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                    int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                    void* result, void* workspace, size_t workspace_bytes, void* stream);
/* PROGRESSIVE files (Pillow's progressive=True, with or without optimize=True; csrc/jpeg_prog_u8.hip): the same
 * quantised coefficients, coded by libjpeg's progressive entropy coder in the ten scans of its default script for YCbCr, every scan
 * with a Huffman table made from its own symbols by the rule above.  The device makes the ten entropy-coded scans of every crop, each
 * stuffed and padded on its own; the host writes SOI, APP0, two DQT and SOF2, then in front of every scan its DHT segments and its
 * SOS header, and EOI behind the last.  The argument lists are those of the ciaosr_jpeg_opt_* entries.
 * `result` (DEVICE, 8-byte aligned, ciaosr_jpeg_prog_result_bytes(n_tiles) = 8 (10 n_tiles + 1) + 2720 n_tiles bytes):
 *   bytes [0, 8 (10 n_tiles + 1))         unsigned long long offs[10 n_tiles + 1]: scan s = 0..9 of crop t is
 *                                         out[offs[10 t + s] : offs[10 t + s + 1]]; offs[0] = 0, no gaps
 *   then per crop t, per table k = 0..9   one record of CIAOSR_JPEG_DHT_RECORD_BYTES as above, in the file's order of DHT segments:
 *                                         DC 0 (0x00) and DC 1 (0x01) in front of scan 1, then the AC table of scans 2, 3, 4, 5, 6,
 *                                         8, 9, 10 (0x10 for a luma scan, 0x11 for a chroma scan; scan 7 has none).
 * Scans: 1 DC of Y, Cb, Cr interleaved (Al 1); 2 Y 1..5 (Al 2); 3 Cr 1..63 (Al 1); 4 Cb 1..63 (Al 1); 5 Y 6..63 (Al 2);
 * 6 Y 1..63 (Ah 2, Al 1); 7 DC refinement of all three (Ah 1, Al 0); 8 Cr, 9 Cb, 10 Y 1..63 (Ah 1, Al 0).
 * Sizes: with arbitrary codes of up to 16 bits a block takes at most 27 bits in scan 1, 1 bit in scan 7, 26 x (Se - Ss + 1) + 60 bits in
 * a first AC scan and 17 x 63 + 60 in an AC refinement; ciaosr_jpeg_prog_capacity_bytes is twice the sum over the ten scans of
 * ceil(bits x blocks of the scan / 8) (DC scans: all blocks, dummy ones included; AC scans: the component's real blocks), so that
 * nothing can be written at or beyond out_capacity.  The workspace holds that sum once more, the coefficients, and about 29 bytes per
 * block and scan.  Thirteen launches and one memset on `stream` per call whatever the number of crops.  Refusals as above, the limit of
 * 64 x blocks < 1 000 000 000 per crop included. */
size_t ciaosr_jpeg_prog_result_bytes(int n_tiles);
size_t ciaosr_jpeg_prog_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_prog_capacity_bytes(int H, int W, int subsampling);
int ciaosr_jpeg_prog_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                               int mcus_per_chunk, unsigned char* out, size_t out_capacity, void* result, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t ciaosr_jpeg_prog_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int subsampling, int mcus_per_chunk);
size_t ciaosr_jpeg_prog_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int subsampling);
int ciaosr_jpeg_prog_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                     int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                     void* result, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#include "ciaosr_hip_png_grey.h"

#endif /* CIAOSR_HIP_H */
