// CrossScaleAttention (arch_csnln.py:430-532) as a sequence of launches on one stream.  cs_attn() checks its arguments, plans the sizes
// (csa_plan), decides the route (csa_route: the only place that reads options, precision and capacities), carves the workspace
// (csa_carve: the only list of buffers; CsaBuffers names every second use of one) and calls one function per stage:
//   stage, route      launches in order (profiler tags)                                   scratch: reads -> writes
//   embed             pad_reflect, csa_conv1x1 x 2, avgpool2 | downsample, csa_conv1x1    feat -> xp -> E, M;  xp -> x2 -> R
//   scores  box       csa_key_norms, csa_scores                                           M, R -> norms (Kn), S
//           gemm      csa_patch_q, csa_patch_k, csa_scores                                M -> Qp;  R -> Kn;  Qp, Kn -> S
//           16-bit    csa_patch_q, csa_patch_k, cast_rows x 2, then fused: softmax_gemm   Qp, Kn -> q16, k16 (Y) -> P16 (statistics in S)
//                     or two passes: csa_scores_<h>, softmax_rows                         q16, k16 -> S -> P16
//   tail  four-block  softmax_stats, partial_down, csa_gather_vedge, csa_attn_v4_f32,     S -> stats (Qp);  E -> PE -> Pc -> vedge (Vp);
//                     edges (softmax), csa_attn_v4_combine                                S, stats, Pc -> partial4 (O);  edges -> Ov;  -> out
//         16C         softmax_stats, partial_down, csa_gather_vprime, csa_attn_v          S -> stats (Qp);  E -> PE -> Pc -> Vp;  S, stats, Vp -> O;
//                     (192 x 256 or 128 x 128 tiles), edges (softmax), gather_out         edges -> Ov;  O, Ov -> out
//         16-bit      partial_down, csa_gather_vprime_t, csa_attn_v_<h>,                  E -> PE -> Pc -> vpT (V);  P16, vpT -> O;  Pc -> Vp;
//                     csa_gather_vprime, rows_to_f32 x 2, edges (split-K), gather_out     P16 -> edge_rows (S);  edges -> Ov;  O, Ov -> out
//         uncomposed  softmax_rows, csa_patch_v, csa_attn_v, fold | fold_s, csa_down      S in place;  E -> V;  S, V -> O -> Y -> Yp -> out
//   partial_down = 3x3 stride-2 patch rows of E + their GEMM with the masked down weights;  edges = the three skinny contractions of the
//   row 0 / column 0 rule (S, stats | edge_rows, and 9C columns of Vp -> Ov, split-K partials in Y).
//
// A C3 tile (192 x 192, C = 64) runs box + four-block in fp32 and the 16-bit forms through the _bf16 / _f16 entries; C = 180 runs gemm + 16C;
// maps below csa_composed_min pixels and scales 3, 4 run uncomposed.  The score matrix is materialised in HBM (1.36 GB at that tile).
#include "ops.h"

namespace ciaosr {

struct CsaPlan {
    int H, W, C, sc, Hp, Wp, HWp, Hl, Wl, L, Lld, Lld8, Ch;
    size_t n_V, n_S, n_Y;      // the capacities that a second use depends on or that a launch is told of
};

static CsaPlan csa_plan(int H, int W, int C, int sc) {
    CsaPlan p;
    p.H = H; p.W = W; p.C = C; p.sc = sc; p.Ch = (int)round_up(C / 2, 4);  // zero-padded half width
    p.Hp = (int)round_up((size_t)H, sc); p.Wp = (int)round_up((size_t)W, sc);        // mod_pad to the scale (csa:438-444)
    p.HWp = p.Hp * p.Wp; p.Hl = p.Hp / sc; p.Wl = p.Wp / sc; p.L = p.Hl * p.Wl;
    p.Lld = (int)round_up(p.L, 4); p.Lld8 = (int)round_up(p.L, 8);
    p.n_V = (size_t)p.L * 9 * sc * sc * C; p.n_S = (size_t)p.HWp * p.Lld; p.n_Y = (size_t)sc * sc * p.HWp * C;
    return p;
}

// The workspace.  Each buffer is named for its first occupant (csa_carve); every later use of one is a view here, with the reason it
// fits: a capacity that always holds as a comment, one that can fail as a *_fits predicate that csa_route() consults.
struct CsaBuffers : CsaPlan {
    float *xp, *E, *M, *x2, *R, *Qp, *Kn, *V, *S, *O, *Y, *Yp, *PE, *Pc, *Vp, *Ov;
    unsigned short* P16;
    float* stats() const { return Qp; }       // [HWp] (max x log2 e, 1 / sum); the patch rows are consumed or were never built.  2 HWp <= 9 Ch HWp
    float* norms() const { return Kn; }       // [L] key norms of the box-sum scores, which build no key patch rows.  L <= 9 Ch L
    float* partial4() const { return O; }     // [4][HWp][C] four-block partial sums.  4 HWp C <= 36 HWp C at scale 2, the composed tail's only scale
    float* vedge() const { return Vp; }       // Ve [L][9C] where the 16C tails keep V' [L][25C].  9 L C <= 25 L C
    float* edge_rows() const { return S; }    // [Wp + Hp][Lld] fp32 copies of 16-bit probability rows (no logits then).  Wp + Hp <= Hp Wp from 2 x 2 on
    float* splitk() const { return Y; }       // edges' split-K partials (no 2x map then, 16-bit Q / K consumed): the kernels split as n_Y allows
    float* softmax_scratch() const { return S; }                                   // statistics of the fused 16-bit softmax: softmax16_fits
    unsigned short* q16() const { return reinterpret_cast<unsigned short*>(Y); }   // 16-bit [HWp][9Ch] and, behind it, [L][9Ch]: qk16_fits
    unsigned short* k16() const { return q16() + round_up((size_t)HWp * 9 * Ch, 128); }
    unsigned short* vpT() const { return reinterpret_cast<unsigned short*>(V); }   // 16-bit V'^T [25C][Lld8]: vpt_fits
    float* otop() const { return Ov; }                                             // Ov = row 0 [Wp][4C], column 0 [Hp][4C], the corner pixel [C]
    float* oleft() const { return Ov + (size_t)Wp * 4 * C; }
    float* otl() const { return oleft() + (size_t)Hp * 4 * C; }
};
static bool qk16_fits(const CsaPlan& p) { return ((size_t)p.HWp + p.L) * 9 * p.Ch * 2 + 512 <= p.n_Y * sizeof(float); }   // not at C = 4
static bool vpt_fits(const CsaPlan& p) { return (size_t)25 * p.C * p.Lld8 * 2 <= p.n_V * sizeof(float); }                // not at L = 1
static bool softmax16_fits(const CsaPlan& p, const H16Ops& h) { return h.softmax_gemm_scratch(p.HWp, p.L) <= p.n_S; }    // not at small L

// The one list of carve-outs, in carve order: take(floats) is Arena::take (256-byte aligned) for a call, a running sum for the byte count.
template <class Take>
static CsaBuffers csa_carve(const CsaPlan& p, Take take) {
    const size_t HW = p.HWp, L = p.L, C = p.C, Ch = p.Ch, n_PE = (size_t)(p.Hp / 2 + 3) * (p.Wp / 2 + 3) * 9 * C;
    CsaBuffers b = {p};
    b.xp = take(HW * C);              // input, reflect-padded to Hp x Wp
    b.E = take(HW * C); b.M = take(HW * Ch);          // its assembly and match1 embeddings
    b.x2 = take(L * C); b.R = take(L * Ch);           // pooled input and its match2 embedding
    b.Qp = take(HW * 9 * Ch); b.Kn = take(L * 9 * Ch);   // 3x3 patch rows of M and, L2-normalised, of R
    b.V = take(p.n_V);                // (3s)x(3s) patch rows of E
    b.S = take(p.n_S);                // logits, then probabilities [HWp][Lld]
    b.O = take(HW * 9 * p.sc * p.sc * C);   // attn.V [HWp][9ssC], composed tails [HWp][16C]
    b.Y = take(p.n_Y); b.Yp = take((size_t)p.H * p.W * 9 * C);   // folded s x map and its 3x3 stride-s patch rows
    b.PE = take(n_PE); b.Pc = take(n_PE);             // composed tails: stride-2 patch rows of E and their partial down-convolutions
    b.Vp = take(L * 25 * C);          // V' [L][25C]: 16C main columns, 9C edge variants
    b.Ov = take((size_t)(p.Hp + p.Wp) * 4 * C + C);   // edge outputs
    b.P16 = reinterpret_cast<unsigned short*>(take(HW * p.Lld8 / 2 + 64));   // 16-bit probabilities [HWp][Lld8]
    return b;
}

enum CsaScores { kScoresBox, kScoresGemm, kScores16 };
enum CsaTail { kTailUncomposed, kTail16C, kTailFour, kTail16 };
struct CsaRoute {
    CsaScores scores; CsaTail tail;
    bool tile128;         // four-block tail: its 128 x 128 kernel on request (csa_attn_tile128)
    bool attn_big;        // 16C tail: attn.V with one 192 x 256 workgroup tile per CU, else the 128 x 128 kernel (bitwise equal)
    bool fused_softmax;   // 16-bit scores: probabilities straight from the contraction, else logits + softmax_rows
};

// What a call runs; launches nothing.  A 16-bit entry with no 16-bit route at its size takes the fp32 kernels with patch-row scores.
static CsaRoute csa_route(const CsaPlan& p, Prec prec, const ciaosr_options_t* opt, const ciaosr_csattn_weights_t* w) {
    CsaRoute r = {kScoresGemm, kTailUncomposed, opt && opt->csa_attn_tile128, false, false};
    // fp32: the scores as a 3x3 diagonal box sum of the per-pixel correlation (csa_scores_f32.hip); csa_scores_gemm = 1 keeps the patch-row GEMM
    if (prec == kF32 && !(opt && opt->csa_scores_gemm) && csa_scores_box_ok(p.Ch, p.Ch, p.Ch)) r.scores = kScoresBox;
    const int composed_min = opt && opt->csa_composed_min ? opt->csa_composed_min : 4096;   // composed tail (scale 2's) from this many padded pixels on
    if (!(p.sc == 2 && w->w_down_masked && composed_min > 0 && p.HWp >= composed_min)) return r;
    // 16-bit modes: Q.K^T and P.V' on the bf16 / f16 MFMA (gemm_h16.hip), probabilities rounded to 16 bits; everything else stays fp32
    if (prec != kF32 && (9 * p.Ch) % 8 == 0 && (p.Lld & 3) == 0 && qk16_fits(p) && vpt_fits(p)) {
        r.scores = kScores16; r.tail = kTail16;
        // the fused form takes its pass-1 maximum on the raw accumulators, which needs a positive scale (every config has one)
        r.fused_softmax = softmax16_fits(p, h16_ops(prec)) && w->softmax_scale > 0.f;
    } else if (prec == kF32 && !(opt && opt->csa_attn_v16) && csa_attn_v4_ok(p.Hp, p.Wp, p.C, p.Lld)) {
        r.tail = kTailFour;
    } else {
        r.tail = kTail16C;   // at a C3 tile's size (768 tiles of 192 x 256) one workgroup per CU, else -- or on request -- the 128 x 128 kernel
        r.attn_big = !r.tile128 && gemm_big_softmax_f32_ok(p.Lld, 25 * p.C, p.HWp, 16 * p.C, p.L, true) &&
                     ((size_t)(p.HWp - 1) * p.Lld + p.L) * sizeof(float) < 0xFFFFFF00ull;
    }
    return r;
}

#define CSA_RUN(x) do { const int rc_ = (x); if (rc_ != CIAOSR_OK) return rc_; } while (0)
// One call: the plan, the buffers, and one function per stage.
struct CsaCall : CsaBuffers {
    const ciaosr_csattn_weights_t* w; float* out; int ld_out; hipStream_t s;

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

    // logits S [HWp][Lld] in fp32, or 16-bit probabilities P16 [HWp][Lld8] (fused: two passes over the short-K GEMM, no logit matrix)
    int scores(const CsaRoute& r, Prec prec) const {
        const int Kq = 9 * Ch;
        if (r.scores == kScoresBox)
            return csa_scores_box_f32(M, Ch, Hp, Wp, R, Ch, Hl, Wl, Ch, w->softmax_scale, w->escape_nan, norms(), S, Lld, s);
        CSA_RUN(patch_rows(M, Ch, Hp, Wp, Ch, 3, 1, 1, Hp, Wp, Qp, Kq, 0, 0.f, s, "csa_patch_q"));
        CSA_RUN(patch_rows(R, Ch, Hl, Wl, Ch, 3, 1, 1, Hl, Wl, Kn, Kq, 1, w->escape_nan, s, "csa_patch_k"));
        if (r.scores == kScoresGemm)
            return gemm_f32(Qp, Kq, Kn, Kq, false, S, Lld, nullptr, HWp, L, Kq, w->softmax_scale, CIAOSR_ACT_NONE, 0.f, s, "csa_scores");
        const H16Ops& h = h16_ops(prec);
        const char* tag = prec == kF16 ? "csa_scores_f16" : "csa_scores_bf16";
        CSA_RUN(h.cast_rows(Qp, Kq, q16(), Kq, HWp, Kq, s));
        CSA_RUN(h.cast_rows(Kn, Kq, k16(), Kq, L, Kq, s));
        if (r.fused_softmax) return h.softmax_gemm_nt(q16(), Kq, k16(), Kq, P16, Lld8, HWp, L, Kq, w->softmax_scale, softmax_scratch(), n_S, s, tag);
        CSA_RUN(h.gemm_nt(q16(), Kq, k16(), Kq, S, Lld, false, HWp, L, Kq, w->softmax_scale, s, tag));
        return h.softmax_rows(S, HWp, L, Lld, P16, Lld8, s);
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

    // The edge rule of row 0 / column 0: three skinny contractions (Wp, Hp and 1 rows; K = L) with the 4C / 4C / C columns of Vc (row
    // stride ld) from column col0 on, split-K, into Ov.  probs == nullptr: A = row softmax of the logits S, formed in the operand staging
    // from stats(); else A = the fp32 probability rows probs [Wp + Hp][Lld] (row 0's pixels, then column 0's).
    int edges(const float* Vc, int ld, int col0, const float* probs) const {
        auto edge = [&](int pix0, int pix_stride, int col, float* dst, int rows, int n) -> int {
            const float* B = Vc + col0 + col;
            if (probs)
                return gemm_f32_splitk(probs + (size_t)pix0 * Lld, Lld, B, ld, true, dst, n, nullptr, rows, n, L, 1.f, CIAOSR_ACT_NONE, 0.f, splitk(),
                                       n_Y, s, "csa_attn_v_edge");
            return gemm_f32_softmax_a(S, pix_stride * Lld, stats(), pix_stride, B, ld, true, dst, n, rows, n, L, splitk(), n_Y, s, "csa_attn_v_edge");
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
    // subtracted in the combine.  The row softmax is applied in the operand staging (statistics-only pass over S; softmax_rows' values to rounding)
    int tail_four(bool tile128) const {
        CSA_RUN(softmax_stats_rows(S, HWp, L, Lld, stats(), s));
        CSA_RUN(partial_down());
        CSA_RUN(csa_gather_vedge(Pc, Hl, Wl, C, vedge(), s));
        CSA_RUN(csa_attn_v4_f32(S, Lld, stats(), Pc, partial4(), Hp, Wp, C, tile128, s));
        CSA_RUN(edges(vedge(), 9 * C, 0, nullptr));
        return csa_attn_v4_combine(partial4(), otop(), oleft(), otl(), w->b_down, H, W, Hp, Wp, C, out, ld_out, s);
    }

    // the same softmax-in-staging attn.V on the 16C main columns of V'
    int tail_16c(bool big) const {
        CSA_RUN(softmax_stats_rows(S, HWp, L, Lld, stats(), s));
        CSA_RUN(partial_down());
        CSA_RUN(csa_gather_vprime(Pc, Hl, Wl, C, Vp, s));
        CSA_RUN(big ? gemm_big_softmax_f32(S, Lld, stats(), 1, Vp, 25 * C, O, 16 * C, HWp, 16 * C, L, s, "csa_attn_v")
                    : gemm_f32_softmax_a(S, Lld, stats(), 1, Vp, 25 * C, true, O, 16 * C, HWp, 16 * C, L, nullptr, 0, s, "csa_attn_v"));
        return finish_16c(nullptr);
    }

    // main 16C columns on the 16-bit MFMA; the Wp + Hp rows that read the edge variants go back to fp32 (exact) and through the fp32 edges
    int tail_16(Prec prec) const {
        const H16Ops& h = h16_ops(prec); const bool f16 = prec == kF16;
        CSA_RUN(partial_down());
        CSA_RUN(csa_gather_vprime_t_h16(Pc, Hl, Wl, C, vpT(), Lld8, f16, s));
        CSA_RUN(h.gemm_nt(P16, Lld8, vpT(), Lld8, O, 16 * C, false, HWp, 16 * C, Lld8, 1.f, s, f16 ? "csa_attn_v_f16" : "csa_attn_v_bf16"));
        CSA_RUN(csa_gather_vprime(Pc, Hl, Wl, C, Vp, s));
        CSA_RUN(h.rows_to_f32(P16, Lld8, 0, 1, Wp, Lld, edge_rows(), Lld, s));                             // row 0: pixels 0 .. Wp-1
        CSA_RUN(h.rows_to_f32(P16, Lld8, 0, Wp, Hp, Lld, edge_rows() + (size_t)Wp * Lld, Lld, s));         // column 0: pixels i * Wp
        return finish_16c(edge_rows());
    }

    // V patches (3s)x(3s), stride s, 'same' padding = s each side (csa:462-465); attn.V; conv_transpose2d(stride s, padding s) as a
    // gather; the scale's down conv (3x3, stride s, pad 1: down / downx3 / downx4, csa:516-521) on the cropped H x W outputs
    int tail_uncomposed() const {
        const int kv = 9 * sc * sc * C;
        CSA_RUN(softmax_rows(S, HWp, L, Lld, s));
        CSA_RUN(patch_rows(E, C, Hp, Wp, C, 3 * sc, sc, sc, Hl, Wl, V, kv, 0, 0.f, s, "csa_patch_v"));
        CSA_RUN(gemm_f32(S, Lld, V, kv, true, O, kv, nullptr, HWp, kv, L, 1.f, CIAOSR_ACT_NONE, 0.f, s, "csa_attn_v"));
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

extern "C" size_t ciaosr_cs_attn_workspace_bytes(int H, int W, int C) { return ciaosr_cs_attn_workspace_bytes_scale(H, W, C, 2); }
extern "C" size_t ciaosr_cs_attn_workspace_bytes_scale(int H, int W, int C, int scale) {
    if (scale < 2 || scale > 4) scale = 4;          // callers sizing for "any scale" get the largest
    size_t n = 0;
    csa_carve(csa_plan(H, W, C, scale), [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 24 * 256;            // room for the 256-byte alignment of each carve-out
}

static int cs_attn(const float* feat_hwc, int ld_feat, int H, int W, const ciaosr_csattn_weights_t* w, float* out, int ld_out,
                   const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream, Prec prec) {
    CIAOSR_CHECK_ARG(feat_hwc && w && out && workspace && H >= 2 && W >= 2);
    CIAOSR_CHECK_ARG(options_ok(opt));
    const int C = w->channels, sc = w->scale ? w->scale : 2;
    CIAOSR_CHECK_ARG(C >= 4 && (C & 3) == 0 && ld_feat >= C && (ld_feat & 3) == 0 && (ld_out & 3) == 0);
    CIAOSR_CHECK_ARG(sc >= 2 && sc <= 4 && H >= sc && W >= sc);     // reflect padding needs pad < size
    const CsaPlan p = csa_plan(H, W, C, sc);
    const CsaRoute r = csa_route(p, prec, opt, w);
    if (workspace_bytes < ciaosr_cs_attn_workspace_bytes_scale(H, W, C, sc)) return CIAOSR_ERR_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const CsaCall c = {csa_carve(p, [&](size_t floats) { return ar.take<float>(floats); }), w, out, ld_out, (hipStream_t)stream};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    CSA_RUN(c.embed(feat_hwc, ld_feat));
    CSA_RUN(c.scores(r, prec));
    if (r.tail == kTailFour) return c.tail_four(r.tile128);
    if (r.tail == kTail16C) return c.tail_16c(r.attn_big);
    if (r.tail == kTail16) return c.tail_16(prec);
    return c.tail_uncomposed();
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
