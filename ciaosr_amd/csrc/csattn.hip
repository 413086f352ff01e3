// CrossScaleAttention (arch_csnln.py:430-532) as a sequence of launches on one stream.  cs_attn() checks its arguments, plans the sizes
// (csa_plan) and the band walk (csa_plan_bands), decides the route (csa_route: the only place that reads options, precision and capacities),
// carves the workspace (csa_carve: the only list of buffers; CsaBuffers names every second use of one) and calls one function per stage:
//   stage, route      launches in order (profiler tags)                                   scratch: reads -> writes
//   embed             pad_reflect, csa_conv1x1 x 2, avgpool2 | downsample, csa_conv1x1    feat -> xp -> E, M;  xp -> x2 -> R
//   scores operands   box: csa_key_norms;  gemm: csa_patch_q, csa_patch_k;                M, R -> norms (Kn) | Qp, Kn | q16, k16 (Y)
//                     16-bit: those two and cast_rows x 2
//   -- per band of query rows (one band = the whole map unless opt->csa_block_mb says otherwise) ------------------------------------------
//   scores  box       csa_scores                                                          M, R, norms -> S
//           gemm      csa_scores                                                          Qp, Kn -> S
//           16-bit    fused: softmax_gemm, or two passes: csa_scores_<h>, softmax_rows    q16, k16 -> P16 (statistics in S) | -> S -> P16
//   tail  four-block  softmax_stats, [partial_down, csa_gather_vedge], csa_attn_v4_f32    S -> stats;  E -> PE -> Pc -> vedge (Vp);
//                                                                                         S, stats, Pc -> partial4 (O)
//         16C         softmax_stats, [partial_down, csa_gather_vprime], csa_attn_v        S -> stats;  E -> PE -> Pc -> Vp;  S, stats, Vp -> O
//                     (192 x 256 or 128 x 128 tiles)
//         16-bit      [partial_down, csa_gather_vprime_t], csa_attn_v_<h>                 E -> PE -> Pc -> vpT (V);  P16, vpT -> O
//         uncomposed  softmax_rows, [csa_patch_v], csa_attn_v                             S in place;  E -> V;  S, V -> O
//         banded      csa_edge_rows x 1-2 | rows_to_f32 x 1-2                             S | P16 -> edge_rows: row 0's and column 0's pixels
//   -- behind the last band, on whole maps ----------------------------------------------------------------------------------------------
//   finish four-block edges (softmax), csa_attn_v4_combine                                S | edge_rows, stats, vedge -> Ov;  partial4, Ov -> out
//          16C        edges (softmax), gather_out                                         S | edge_rows, stats, Vp -> Ov;  O, Ov -> out
//          16-bit     csa_gather_vprime, [rows_to_f32 x 2], edges (split-K), gather_out   Pc -> Vp;  P16 -> edge_rows (S);  edges -> Ov;  O, Ov -> out
//          uncomposed fold | fold_s, csa_down                                             O -> Y -> Yp -> out
//   [..] = once, with the first band (where the whole-map call has them);  partial_down = 3x3 stride-2 patch rows of E + their GEMM with the
//   masked down weights;  edges = the three skinny contractions of the row 0 / column 0 rule (logits and stats | probability rows, and 9C
//   columns of Vp -> Ov, split-K partials in Y);  stats = (max x log2 e, 1 / sum) per query in Qp, banded in V.
//
// A C3 tile (192 x 192, C = 64) runs box + four-block in fp32 and the 16-bit forms through the _bf16 / _f16 entries; C = 180 runs gemm + 16C;
// maps below csa_composed_min pixels and scales 3, 4 run uncomposed.  The score matrix is materialised in HBM (1.36 GB at that tile), whole
// or -- opt->csa_block_mb -- one band of query rows at a time: the row softmax is over the keys of one query, so no stage needs more of S
// than a band, and the four-block kernel's item oy reads the logit rows oy - 2 .. oy + 1 only (a band carries those three halo rows).
// A row's result does not depend on the band it is computed in: every launcher derives what could change a summation order from the
// whole map's rows (ops.h: plan_rows), so banded and whole-map calls of one route are bitwise equal.
#include "ops.h"

namespace ciaosr {

struct CsaPlan {
    int H, W, C, sc, Hp, Wp, HWp, Hl, Wl, L, Lld, Lld8, Ch;
    // The band walk (opt->csa_block_mb, csa_plan_bands): bands of band_rows query rows; S (and P16) hold s_rows logit rows at a time, a
    // band's own and `up` rows above, `down` below (the four-block halo), clipped to the map.  band_rows == Hp: one band, the walk is off.
    int band_rows, up, down, s_rows;
    size_t n_V, n_S, n_Y;      // the capacities that a second use depends on or that a launch is told of (n_S: of the band)
    bool banded() const { return band_rows < Hp; }
};

static CsaPlan csa_plan(int H, int W, int C, int sc) {
    CsaPlan p;
    p.H = H; p.W = W; p.C = C; p.sc = sc; p.Ch = (int)round_up(C / 2, 4);  // zero-padded half width
    p.Hp = (int)round_up((size_t)H, sc); p.Wp = (int)round_up((size_t)W, sc);        // mod_pad to the scale (csa:438-444)
    p.HWp = p.Hp * p.Wp; p.Hl = p.Hp / sc; p.Wl = p.Wp / sc; p.L = p.Hl * p.Wl;
    p.Lld = (int)round_up(p.L, 4); p.Lld8 = (int)round_up(p.L, 8);
    p.band_rows = p.s_rows = p.Hp; p.up = p.down = 0;
    p.n_V = (size_t)p.L * 9 * sc * sc * C; p.n_S = (size_t)p.HWp * p.Lld; p.n_Y = (size_t)sc * sc * p.HWp * C;
    return p;
}

// composed tail (scale 2's) from csa_composed_min padded pixels on
static bool csa_composed(const CsaPlan& p, const ciaosr_options_t* opt) {
    const int composed_min = opt && opt->csa_composed_min ? opt->csa_composed_min : 4096;
    return p.sc == 2 && composed_min > 0 && p.HWp >= composed_min;
}
static bool csa_wants_four(const CsaPlan& p, Prec prec, const ciaosr_options_t* opt, int s_rows) {
    return prec == kF32 && !(opt && opt->csa_attn_v16) && csa_composed(p, opt) && csa_attn_v4_ok(p.Hp, p.Wp, p.C, p.Lld, s_rows);
}

// The band height under opt->csa_block_mb MiB of score storage (a logit row of S: Wp Lld floats; the 16-bit entries' P16 row with it).
// Pure arithmetic on the sizes, the precision and the options (the four-block tail is assumed wherever its size conditions hold), so
// ciaosr_cs_attn_block_rows can name the band count of a call without one.
constexpr int kCsaItemRows = 8;    // item height of the box-sum scores; the smallest fp32 band (8 logit rows, halo included)
constexpr int kCsaMinRows16 = 4;   // the smallest band of the 16-bit entries, whose GEMMs tile pixels, not rows (a row costs 1.5x the bytes)
static void csa_plan_bands(CsaPlan& p, Prec prec, const ciaosr_options_t* opt) {
    if (!opt || opt->csa_block_mb <= 0) return;
    const size_t budget = (size_t)opt->csa_block_mb << 20, row_s = (size_t)p.Wp * p.Lld * sizeof(float);
    const size_t row = row_s + (prec != kF32 ? (size_t)p.Wp * p.Lld8 * 2 : 0);
    if (budget >= row * p.Hp) return;                                   // one band covers the map
    const size_t min_rows = prec == kF32 ? kCsaItemRows : kCsaMinRows16;
    const bool four = csa_wants_four(p, prec, opt, kCsaItemRows);       // else the 16C, 16-bit or uncomposed tail: no halo
    size_t sr = budget / row;                                           // the logit rows the budget holds ...
    const size_t addr = ((four ? 0x80000000ull : 0xFFFFFF00ull) - 1) / row_s;       // ... and those the tail's kernels address (2 GiB | 4 GiB)
    if (sr > addr) sr = addr;
    if (sr >= 2 * kCsaItemRows) sr -= sr % kCsaItemRows;                // whole items of the scores kernel where that costs little
    if (sr < min_rows) sr = min_rows;                                   // a budget below the smallest band: that band
    const int halo = four ? 3 : 0;
    if (sr >= (size_t)p.Hp + halo) return;
    p.band_rows = (int)sr - halo; p.up = four ? 2 : 0; p.down = four ? 1 : 0;
    p.s_rows = (int)sr < p.Hp ? (int)sr : p.Hp;
    p.n_S = (size_t)p.s_rows * p.Wp * p.Lld;
}

// The workspace.  Each buffer is named for its first occupant (csa_carve); every later use of one is a view here, with the reason it
// fits: a capacity that always holds as a comment, one that can fail as a *_fits predicate that csa_route() consults.  Under the band
// walk S and P16 hold one band, so what outlives a band does not live in S: the edge rows have a carve-out of their own (Er) and the
// statistics move to V.
struct CsaBuffers : CsaPlan {
    float *xp, *E, *M, *x2, *R, *Qp, *Kn, *V, *S, *O, *Y, *Yp, *PE, *Pc, *Vp, *Ov, *Er;
    unsigned short* P16;
    // [HWp] (max x log2 e, 1 / sum); the patch rows are consumed or were never built.  2 HWp <= 9 Ch HWp.  Banded: the gemm scores of a later
    // band still read the patch rows, and V is free (the uncomposed tail, its user, takes no statistics).  2 HWp <= 9 HWp C at scale 2
    float* stats() const { return banded() ? V : Qp; }
    float* norms() const { return Kn; }       // [L] key norms of the box-sum scores, which build no key patch rows.  L <= 9 Ch L
    float* partial4() const { return O; }     // [4][HWp][C] four-block partial sums.  4 HWp C <= 36 HWp C at scale 2, the composed tail's only scale
    float* vedge() const { return Vp; }       // Ve [L][9C] where the 16C tails keep V' [L][25C].  9 L C <= 25 L C
    // [Wp + Hp][Lld] fp32 rows of row 0's and column 0's pixels: copies of 16-bit probability rows (no logits then; Wp + Hp <= Hp Wp from
    // 2 x 2 on) or, banded, of 16-bit probability or fp32 logit rows, each taken in the band that holds it
    float* edge_rows() const { return banded() ? Er : S; }
    float* splitk() const { return Y; }       // edges' split-K partials (no 2x map then, 16-bit Q / K consumed): the kernels split as n_Y allows
    float* softmax_scratch() const { return S; }                                   // statistics of the fused 16-bit softmax (a band's): softmax16_fits
    unsigned short* q16() const { return reinterpret_cast<unsigned short*>(Y); }   // 16-bit [HWp][9Ch] and, behind it, [L][9Ch]: qk16_fits
    unsigned short* k16() const { return q16() + round_up((size_t)HWp * 9 * Ch, 128); }
    unsigned short* vpT() const { return reinterpret_cast<unsigned short*>(V); }   // 16-bit V'^T [25C][Lld8]: vpt_fits
    float* otop() const { return Ov; }                                             // Ov = row 0 [Wp][4C], column 0 [Hp][4C], the corner pixel [C]
    float* oleft() const { return Ov + (size_t)Wp * 4 * C; }
    float* otl() const { return oleft() + (size_t)Hp * 4 * C; }
};
static bool qk16_fits(const CsaPlan& p) { return ((size_t)p.HWp + p.L) * 9 * p.Ch * 2 + 512 <= p.n_Y * sizeof(float); }   // not at C = 4
static bool vpt_fits(const CsaPlan& p) { return (size_t)25 * p.C * p.Lld8 * 2 <= p.n_V * sizeof(float); }                // not at L = 1
static bool softmax16_fits(const CsaPlan& p, const H16Ops& h) { return h.softmax_gemm_scratch((long)p.s_rows * p.Wp, p.L) <= p.n_S; }   // not at small L

// The one list of carve-outs, in carve order: take(floats) is Arena::take (256-byte aligned) for a call, a running sum for the byte count.
// p16: the call may form 16-bit probabilities (every call when the band walk is off: the carve does not depend on the entry then).
template <class Take>
static CsaBuffers csa_carve(const CsaPlan& p, bool p16, Take take) {
    const size_t HW = p.HWp, L = p.L, C = p.C, Ch = p.Ch, n_PE = (size_t)(p.Hp / 2 + 3) * (p.Wp / 2 + 3) * 9 * C;
    CsaBuffers b = {p};
    b.xp = take(HW * C);              // input, reflect-padded to Hp x Wp
    b.E = take(HW * C); b.M = take(HW * Ch);          // its assembly and match1 embeddings
    b.x2 = take(L * C); b.R = take(L * Ch);           // pooled input and its match2 embedding
    b.Qp = take(HW * 9 * Ch); b.Kn = take(L * 9 * Ch);   // 3x3 patch rows of M and, L2-normalised, of R
    b.V = take(p.n_V);                // (3s)x(3s) patch rows of E
    b.S = take(p.n_S);                // logits, then probabilities [HWp][Lld]; banded: [s_rows Wp][Lld]
    b.O = take(HW * 9 * p.sc * p.sc * C);   // attn.V [HWp][9ssC], composed tails [HWp][16C]
    b.Y = take(p.n_Y); b.Yp = take((size_t)p.H * p.W * 9 * C);   // folded s x map and its 3x3 stride-s patch rows
    b.PE = take(n_PE); b.Pc = take(n_PE);             // composed tails: stride-2 patch rows of E and their partial down-convolutions
    b.Vp = take(L * 25 * C);          // V' [L][25C]: 16C main columns, 9C edge variants
    b.Ov = take((size_t)(p.Hp + p.Wp) * 4 * C + C);   // edge outputs
    b.P16 = reinterpret_cast<unsigned short*>(take((p16 ? (size_t)p.s_rows * p.Wp * p.Lld8 / 2 : 0) + 64));   // 16-bit probabilities [HWp][Lld8]
    b.Er = p.banded() ? take((size_t)(p.Wp + p.Hp) * p.Lld) : nullptr;                                       // edge rows
    return b;
}
static size_t csa_carve_bytes(const CsaPlan& p, bool p16) {
    size_t n = 0;
    csa_carve(p, p16, [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 24 * 256;            // room for the 256-byte alignment of each carve-out
}

enum CsaScores { kScoresBox, kScoresGemm, kScores16 };
enum CsaTail { kTailUncomposed, kTail16C, kTailFour, kTail16 };
struct CsaRoute {
    CsaScores scores; CsaTail tail;
    bool tile128;         // four-block tail: its 128 x 128 kernel on request (csa_attn_tile128); 16C tail: no 192 x 256 tiles
    bool fused_softmax;   // 16-bit scores: probabilities straight from the contraction, else logits + softmax_rows
};

// What a call runs; launches nothing.  A 16-bit entry with no 16-bit route at its size takes the fp32 kernels with patch-row scores.
// Whatever depends on the size of S is asked of a band (p.s_rows logit rows), so the band walk brings back routes the whole map is too big for.
static CsaRoute csa_route(const CsaPlan& p, Prec prec, const ciaosr_options_t* opt, const ciaosr_csattn_weights_t* w) {
    CsaRoute r = {kScoresGemm, kTailUncomposed, opt && opt->csa_attn_tile128, false};
    // fp32: the scores as a 3x3 diagonal box sum of the per-pixel correlation (csa_scores_f32.hip); csa_scores_gemm = 1 keeps the patch-row GEMM
    if (prec == kF32 && !(opt && opt->csa_scores_gemm) && csa_scores_box_ok(p.Ch, p.Ch, p.Ch)) r.scores = kScoresBox;
    if (!(csa_composed(p, opt) && w->w_down_masked)) return r;
    // 16-bit modes: Q.K^T and P.V' on the bf16 / f16 MFMA (gemm_h16.hip), probabilities rounded to 16 bits; everything else stays fp32
    if (prec != kF32 && (9 * p.Ch) % 8 == 0 && (p.Lld & 3) == 0 && qk16_fits(p) && vpt_fits(p)) {
        r.scores = kScores16; r.tail = kTail16;
        // the fused form takes its pass-1 maximum on the raw accumulators, which needs a positive scale (every config has one)
        r.fused_softmax = softmax16_fits(p, h16_ops(prec)) && w->softmax_scale > 0.f;
    } else if (csa_wants_four(p, prec, opt, p.s_rows)) {
        r.tail = kTailFour;
    } else {
        r.tail = kTail16C;
    }
    return r;
}
// 16C tail, M query pixels: at a C3 tile's size (768 tiles of 192 x 256) one workgroup per CU, else -- or on request -- the 128 x 128
// kernel (bitwise equal, so a ragged last band may take the other one)
static bool csa_attn_big(const CsaPlan& p, const CsaRoute& r, int M) {
    return !r.tile128 && gemm_big_softmax_f32_ok(p.Lld, 25 * p.C, M, 16 * p.C, p.L, true) &&
           ((size_t)(M - 1) * p.Lld + p.L) * sizeof(float) < 0xFFFFFF00ull;
}

// query rows y0 <= y < y1, produced from the logit rows ya <= y < yb that S (P16) hold: S's row 0 is the map's row ya
struct CsaBand {
    int y0, y1, ya, yb;
    bool first() const { return y0 == 0; }
};

#define CSA_RUN(x) do { const int rc_ = (x); if (rc_ != CIAOSR_OK) return rc_; } while (0)
// One call: the plan, the buffers, and one function per stage.  A tail is three functions: what runs once (with the first band, where the
// whole-map call has it), what runs per band, and the finish on whole maps behind the last band.
struct CsaCall : CsaBuffers {
    const ciaosr_csattn_weights_t* w; float* out; int ld_out; hipStream_t s;

    CsaBand band(int y0) const {
        const int y1 = y0 + band_rows < Hp ? y0 + band_rows : Hp;
        return {y0, y1, y0 > up ? y0 - up : 0, y1 + down < Hp ? y1 + down : Hp};
    }
    static int npix(const CsaBand& b, int Wp_) { return (b.y1 - b.y0) * Wp_; }

    // 1x1 convolution + PReLU: the no-staging small GEMM on small maps
    int conv1x1(const float* src, const float* wgt, const float* bias, float slope, float* dst, int n_out, int rows) const {
        if (gemm_small_ok(rows, n_out, C, C, C) && rows <= 4096)
            return gemm_small_f32(src, C, wgt, C, bias, dst, n_out, nullptr, 0, nullptr, 0, rows, n_out, C, CIAOSR_ACT_PRELU, slope, 1.f, s,
                                  "csa_conv1x1");
        return gemm_f32(src, C, wgt, C, false, dst, n_out, bias, rows, n_out, C, 1.f, CIAOSR_ACT_PRELU, slope, s, "csa_conv1x1");
    }

    int embed(const float* feat_hwc, int ld_feat) const {
        CSA_RUN(pad_reflect(feat_hwc, ld_feat, H, W, C, xp, Hp, Wp, s));
        CSA_RUN(conv1x1(xp, w->w_assembly, w->b_assembly, w->slope_assembly, E, C, HWp));
        CSA_RUN(conv1x1(xp, w->w_match1, w->b_match1, w->slope_match1, M, Ch, HWp));
        CSA_RUN(sc == 2 ? avgpool2(xp, Hp, Wp, C, x2, s) : downsample(xp, Hp, Wp, C, sc, x2, s));
        return conv1x1(x2, w->w_match2, w->b_match2, w->slope_match2, R, Ch, L);
    }

    // the operands of the scores, once per call: the key norms of the box sum, or the patch rows (and their 16-bit casts)
    int scores_operands(const CsaRoute& r, Prec prec) const {
        const int Kq = 9 * Ch;
        if (r.scores == kScoresBox) return csa_key_norms(R, Ch, Hl, Wl, Ch, w->softmax_scale, w->escape_nan, norms(), s);
        CSA_RUN(patch_rows(M, Ch, Hp, Wp, Ch, 3, 1, 1, Hp, Wp, Qp, Kq, 0, 0.f, s, "csa_patch_q"));
        CSA_RUN(patch_rows(R, Ch, Hl, Wl, Ch, 3, 1, 1, Hl, Wl, Kn, Kq, 1, w->escape_nan, s, "csa_patch_k"));
        if (r.scores == kScoresGemm) return CIAOSR_OK;
        const H16Ops& h = h16_ops(prec);
        CSA_RUN(h.cast_rows(Qp, Kq, q16(), Kq, HWp, Kq, s));
        return h.cast_rows(Kn, Kq, k16(), Kq, L, Kq, s);
    }
    // a band's logits S [(yb - ya) Wp][Lld] in fp32, or its 16-bit probabilities P16 [..][Lld8] (fused: two passes over the short-K GEMM, no
    // logit matrix).  The launchers are told the whole map's rows (ops.h: plan_rows)
    int scores(const CsaRoute& r, Prec prec, const CsaBand& b) const {
        const int Kq = 9 * Ch, rows = (b.yb - b.ya) * Wp;
        const size_t q0 = (size_t)b.ya * Wp * Kq;
        if (r.scores == kScoresBox) return csa_scores_box_f32(M, Ch, Hp, Wp, R, Ch, Hl, Wl, Ch, norms(), S, Lld, b.ya, b.yb, s);
        if (r.scores == kScoresGemm)
            return gemm_f32(Qp + q0, Kq, Kn, Kq, false, S, Lld, nullptr, rows, L, Kq, w->softmax_scale, CIAOSR_ACT_NONE, 0.f, s, "csa_scores", HWp);
        const H16Ops& h = h16_ops(prec);
        const char* tag = prec == kF16 ? "csa_scores_f16" : "csa_scores_bf16";
        if (r.fused_softmax)
            return h.softmax_gemm_nt(q16() + q0, Kq, k16(), Kq, P16, Lld8, rows, L, Kq, w->softmax_scale, softmax_scratch(), n_S, s, tag, HWp);
        CSA_RUN(h.gemm_nt(q16() + q0, Kq, k16(), Kq, S, Lld, false, rows, L, Kq, w->softmax_scale, s, tag, HWp));
        return h.softmax_rows(S, rows, L, Lld, P16, Lld8, s);
    }

    // 3x3 patch rows [OH * OW][9C] of a C-channel map: the A operand of a down convolution as a GEMM
    int patch_down(const float* src, int Hs, int Ws, int stride, int pad, int OH, int OW, float* dst) const {
        return patch_rows(src, C, Hs, Ws, C, 3, stride, pad, OH, OW, dst, 9 * C, 0, 0.f, s, "csa_patch_down");
    }
    // composed fold + down (patch_ops.hip): Pc = the masked down convolution's partial products of E, from which V' / Ve / V'^T are gathered
    int partial_down() const {
        CSA_RUN(patch_down(E, Hp, Wp, 2, 3, Hl + 3, Wl + 3, PE));
        return gemm_f32(PE, 9 * C, w->w_down_masked, 9 * C, false, Pc, 9 * C, nullptr, (Hl + 3) * (Wl + 3), 9 * C, 9 * C, 1.f, CIAOSR_ACT_NONE, 0.f, s,
                        "csa_down_partial");
    }

    // Banded: the logit rows of row 0's and column 0's pixels leave the band for edge_rows(), where edges() reads them behind the last band
    int keep_edge_logits(const CsaBand& b) const {
        if (!banded()) return CIAOSR_OK;
        if (b.first()) CSA_RUN(copy_rows(S, Lld, Wp, Lld, edge_rows(), Lld, s, "csa_edge_rows"));
        return copy_rows(S + (size_t)(b.y0 - b.ya) * Wp * Lld, (long)Wp * Lld, b.y1 - b.y0, Lld, edge_rows() + (size_t)(Wp + b.y0) * Lld, Lld, s,
                         "csa_edge_rows");
    }
    // The edge rule of row 0 / column 0: three skinny contractions (Wp, Hp and 1 rows; K = L) with the 4C / 4C / C columns of Vc (row
    // stride ld) from column col0 on, split-K, into Ov.  probs == nullptr: A = row softmax of the logits (S, or banded their copies in
    // edge_rows(): the same launches on the same values), formed in the operand staging from stats(); else A = the fp32 probability rows
    // probs [Wp + Hp][Lld] (row 0's pixels, then column 0's).
    int edges(const float* Vc, int ld, int col0, const float* probs) const {
        auto edge = [&](int pix0, int pix_stride, int col, float* dst, int rows, int n) -> int {
            const float* B = Vc + col0 + col;
            if (probs)
                return gemm_f32_splitk(probs + (size_t)pix0 * Lld, Lld, B, ld, true, dst, n, nullptr, rows, n, L, 1.f, CIAOSR_ACT_NONE, 0.f, splitk(),
                                       n_Y, s, "csa_attn_v_edge");
            const float* A = !banded() ? S : edge_rows() + (size_t)pix0 * Lld;
            return gemm_f32_softmax_a(A, banded() ? Lld : pix_stride * Lld, stats(), pix_stride, B, ld, true, dst, n, rows, n, L, splitk(), n_Y, s,
                                      "csa_attn_v_edge");
        };
        CSA_RUN(edge(0, 1, 0, otop(), Wp, 4 * C));            // row 0: pixels 0 .. Wp-1
        CSA_RUN(edge(Wp, Wp, 4 * C, oleft(), Hp, 4 * C));     // column 0: pixels i * Wp (rows Wp .. of probs)
        return edge(0, 1, 8 * C, otl(), 1, C);                // the corner pixel
    }
    // the end of both 16C tails: main columns O [HWp][16C], the edge variants in columns 16C .. 25C of V'
    int finish_16c(const float* probs) const {
        CSA_RUN(edges(Vp, 25 * C, 16 * C, probs));
        return csa_gather_out(O, otop(), oleft(), otl(), w->b_down, H, W, Hp, Wp, C, out, ld_out, 16L * C, 4L * C, 4L * C, s);
    }

    // attn.V on the four diagonal tap blocks (csa_attn_v4_f32.hip): four key-row quarters of partial sums; the edge rule with the tap-0 variants,
    // subtracted in the combine.  The row softmax is applied in the operand staging (statistics-only pass over S; softmax_rows' values to rounding).
    // A band takes the statistics of its halo rows too (the neighbouring band computes the same values again) and launches its own items
    int tail_four(const CsaRoute& r, const CsaBand& b) const {
        CSA_RUN(softmax_stats_rows(S, (long)(b.yb - b.ya) * Wp, L, Lld, stats() + 2 * (size_t)b.ya * Wp, s));
        if (b.first()) {
            CSA_RUN(partial_down());
            CSA_RUN(csa_gather_vedge(Pc, Hl, Wl, C, vedge(), s));
        }
        CSA_RUN(csa_attn_v4_f32(S, Lld, stats(), Pc, partial4(), Hp, Wp, C, r.tile128, b.ya, b.yb - b.ya, b.y0, b.y1, s));
        return keep_edge_logits(b);
    }
    int finish_four() const {
        CSA_RUN(edges(vedge(), 9 * C, 0, nullptr));
        return csa_attn_v4_combine(partial4(), otop(), oleft(), otl(), w->b_down, H, W, Hp, Wp, C, out, ld_out, s);
    }

    // the same softmax-in-staging attn.V on the 16C main columns of V'; finish_16c(nullptr) ends it
    int tail_16c(const CsaRoute& r, const CsaBand& b) const {
        const int rows = npix(b, Wp);
        float* st = stats() + 2 * (size_t)b.y0 * Wp;
        float* Ob = O + (size_t)b.y0 * Wp * 16 * C;
        CSA_RUN(softmax_stats_rows(S, rows, L, Lld, st, s));
        if (b.first()) {
            CSA_RUN(partial_down());
            CSA_RUN(csa_gather_vprime(Pc, Hl, Wl, C, Vp, s));
        }
        CSA_RUN(csa_attn_big(*this, r, rows) ? gemm_big_softmax_f32(S, Lld, st, 1, Vp, 25 * C, Ob, 16 * C, rows, 16 * C, L, s, "csa_attn_v")
                                             : gemm_f32_softmax_a(S, Lld, st, 1, Vp, 25 * C, true, Ob, 16 * C, rows, 16 * C, L, nullptr, 0, s, "csa_attn_v"));
        return keep_edge_logits(b);
    }

    // main 16C columns on the 16-bit MFMA; the Wp + Hp rows that read the edge variants go back to fp32 (exact) and through the fp32 edges
    int tail_16(Prec prec, const CsaBand& b) const {
        const H16Ops& h = h16_ops(prec); const bool f16 = prec == kF16;
        if (b.first()) {
            CSA_RUN(partial_down());
            CSA_RUN(csa_gather_vprime_t_h16(Pc, Hl, Wl, C, vpT(), Lld8, f16, s));
        }
        CSA_RUN(h.gemm_nt(P16, Lld8, vpT(), Lld8, O + (size_t)b.y0 * Wp * 16 * C, 16 * C, false, npix(b, Wp), 16 * C, Lld8, 1.f, s,
                          f16 ? "csa_attn_v_f16" : "csa_attn_v_bf16", HWp));
        if (!banded()) return CIAOSR_OK;
        if (b.first()) CSA_RUN(h.rows_to_f32(P16, Lld8, 0, 1, Wp, Lld, edge_rows(), Lld, s));
        return h.rows_to_f32(P16, Lld8, 0, Wp, b.y1 - b.y0, Lld, edge_rows() + (size_t)(Wp + b.y0) * Lld, Lld, s);
    }
    int finish_16(Prec prec) const {
        const H16Ops& h = h16_ops(prec);
        CSA_RUN(csa_gather_vprime(Pc, Hl, Wl, C, Vp, s));
        if (!banded()) {
            CSA_RUN(h.rows_to_f32(P16, Lld8, 0, 1, Wp, Lld, edge_rows(), Lld, s));                             // row 0: pixels 0 .. Wp-1
            CSA_RUN(h.rows_to_f32(P16, Lld8, 0, Wp, Hp, Lld, edge_rows() + (size_t)Wp * Lld, Lld, s));         // column 0: pixels i * Wp
        }
        return finish_16c(edge_rows());
    }

    // V patches (3s)x(3s), stride s, 'same' padding = s each side (csa:462-465); attn.V; then on whole maps conv_transpose2d(stride s,
    // padding s) as a gather and the scale's down conv (3x3, stride s, pad 1: down / downx3 / downx4, csa:516-521) on the cropped H x W outputs
    int tail_uncomposed(const CsaBand& b) const {
        const int kv = 9 * sc * sc * C, rows = npix(b, Wp);
        CSA_RUN(softmax_rows(S, rows, L, Lld, s));
        if (b.first()) CSA_RUN(patch_rows(E, C, Hp, Wp, C, 3 * sc, sc, sc, Hl, Wl, V, kv, 0, 0.f, s, "csa_patch_v"));
        return gemm_f32(S, Lld, V, kv, true, O + (size_t)b.y0 * Wp * kv, kv, nullptr, rows, kv, L, 1.f, CIAOSR_ACT_NONE, 0.f, s, "csa_attn_v", HWp);
    }
    int finish_uncomposed() const {
        const int kv = 9 * sc * sc * C;
        CSA_RUN(sc == 2 ? fold(O, kv, Hp, Wp, C, Y, s) : fold_s(O, kv, Hp, Wp, C, sc, Y, s));
        CSA_RUN(patch_down(Y, sc * Hp, sc * Wp, sc, 1, H, W, Yp));
        if (gemm_small_ok(H * W, C, 9 * C, 9 * C, 9 * C) && H * W <= 4096)
            return gemm_small_f32(Yp, 9 * C, w->w_down, 9 * C, w->b_down, out, ld_out, nullptr, 0, nullptr, 0, H * W, C, 9 * C, CIAOSR_ACT_NONE, 0.f,
                                  1.0f / 6.0f, s, "csa_down");
        return gemm_f32(Yp, 9 * C, w->w_down, 9 * C, false, out, ld_out, w->b_down, H * W, C, 9 * C, 1.0f / 6.0f, CIAOSR_ACT_NONE, 0.f, s, "csa_down");
    }
};

}  // namespace ciaosr

using namespace ciaosr;

static int csa_scale(int scale) { return scale < 2 || scale > 4 ? 4 : scale; }          // callers sizing for "any scale" get the largest

extern "C" size_t ciaosr_cs_attn_workspace_bytes(int H, int W, int C) { return ciaosr_cs_attn_workspace_bytes_scale(H, W, C, 2); }
extern "C" size_t ciaosr_cs_attn_workspace_bytes_scale(int H, int W, int C, int scale) {
    return csa_carve_bytes(csa_plan(H, W, C, csa_scale(scale)), true);
}
// the larger of the fp32 and the 16-bit entries' carves (their bands differ: the 16-bit ones hold P16 rows too)
extern "C" size_t ciaosr_cs_attn_workspace_bytes_opt(int H, int W, int C, int scale, const ciaosr_options_t* opt) {
    size_t n = 0;
    for (const Prec prec : {kF32, kF16}) {
        CsaPlan p = csa_plan(H, W, C, csa_scale(scale));
        csa_plan_bands(p, prec, opt);
        const size_t m = csa_carve_bytes(p, !p.banded() || prec != kF32);
        n = m > n ? m : n;
    }
    return n;
}
extern "C" int ciaosr_cs_attn_block_rows(int H, int W, int C, int scale, int precision, const ciaosr_options_t* opt) {
    if (H < 1 || W < 1 || C < 1 || scale < 2 || scale > 4 || precision < 0 || precision > 2 || !options_ok(opt)) return 0;
    CsaPlan p = csa_plan(H, W, C, scale);
    csa_plan_bands(p, (Prec)precision, opt);
    return p.band_rows;
}

static int cs_attn(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w, float* out, int ld_out,
                   const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream, Prec prec) {
    CIAOSR_CHECK_ARG(feat_hwc && w && out && workspace && H >= 2 && W >= 2);
    CIAOSR_CHECK_ARG(options_ok(opt));
    const int C = w->channels, sc = w->scale ? w->scale : 2;
    CIAOSR_CHECK_ARG(C >= 4 && (C & 3) == 0 && ld_feat >= C && (ld_feat & 3) == 0 && (ld_out & 3) == 0);
    CIAOSR_CHECK_ARG(sc >= 2 && sc <= 4 && H >= sc && W >= sc);     // reflect padding needs pad < size
    CsaPlan p = csa_plan(H, W, C, sc);
    csa_plan_bands(p, prec, opt);
    const CsaRoute r = csa_route(p, prec, opt, w);
    if (r.tail != kTailFour) p.up = p.down = 0;     // the halo is the four-block kernel's (a call without w_down_masked planned for it)
    if (workspace_bytes < (p.banded() ? ciaosr_cs_attn_workspace_bytes_opt(H, W, C, sc, opt) : ciaosr_cs_attn_workspace_bytes_scale(H, W, C, sc)))
        return CIAOSR_ERR_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const CsaCall c = {csa_carve(p, !p.banded() || prec != kF32, [&](size_t floats) { return ar.take<float>(floats); }), w, out, ld_out,
                       (hipStream_t)stream};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    CSA_RUN(c.embed(feat_hwc, ld_feat));
    CSA_RUN(c.scores_operands(r, prec));
    for (int y0 = 0; y0 < p.Hp; y0 += p.band_rows) {                // one pass when the band walk is off
        const CsaBand b = c.band(y0);
        CSA_RUN(c.scores(r, prec, b));
        CSA_RUN(r.tail == kTailFour ? c.tail_four(r, b) : r.tail == kTail16C ? c.tail_16c(r, b) : r.tail == kTail16 ? c.tail_16(prec, b)
                                                                                                                   : c.tail_uncomposed(b));
    }
    if (r.tail == kTailFour) return c.finish_four();
    if (r.tail == kTail16C) return c.finish_16c(nullptr);
    if (r.tail == kTail16) return c.finish_16(prec);
    return c.finish_uncomposed();
}

extern "C" int ciaosr_cs_attn_f32(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w, float* out, int ld_out,
                                  const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream) {
    return cs_attn(feat_hwc, ld_feat, H, W, w, out, ld_out, opt, workspace, workspace_bytes, stream, kF32);
}
extern "C" int ciaosr_cs_attn_bf16(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w, float* out, int ld_out,
                                   const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream) {
    return cs_attn(feat_hwc, ld_feat, H, W, w, out, ld_out, opt, workspace, workspace_bytes, stream, kBF16);
}
extern "C" int ciaosr_cs_attn_f16(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w, float* out, int ld_out,
                                  const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream) {
    return cs_attn(feat_hwc, ld_feat, H, W, w, out, ld_out, opt, workspace, workspace_bytes, stream, kF16);
}
