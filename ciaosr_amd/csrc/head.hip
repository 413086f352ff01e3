// LocalImplicitSRNet.forward minus the encoder (ciaosr_net.py:88-248) as a sequence of launches on one stream.  head_forward() checks its
// arguments, plans the sizes (head_plan), carves the workspace (head_carve: the only list of buffers; HeadBuffers names every second use
// of one), decides the route (head_route: the only place that reads options, the precision mode, the weights' presence and the
// capacities; it launches nothing, so a call it refuses has enqueued nothing) and calls one function per stage:
//   stage, route          launches in order (profiler tags)                                  scratch: reads -> writes
//   unfold                head_unfold                                                        feat -> U[:, :D]
//   cs_attn               one cs_attn call per scale (csattn.hip)                            feat -> U[:, D + i C ..);  its own workspace csa_ws
//   layer0_tables  h16    cast_rows x 3, head_table_f16 x 2                                  U, W0k, W0v -> u16, wk16, wv16 (bufA) -> Tk, Tv
//                  small  head_table x 2 (the no-staging GEMM)                               U -> Tk, Tv
//                  gemm   head_table x 2                                                     U -> Tk, Tv
//   logit_table    none   --
//                  wino4  head_qk_maps, head_logit_table_w4, head_qk_rows (bias term)        feat -> qk_maps (QK) -> G;  U -> G[:, 256]
//                  wino2  head_qk_maps, head_logit_table_w2, head_qk_rows                    the same
//                  gemm32 per 65 536 rows: head_qk_rows, head_logit_table                    U -> QK -> G
//                  gemm16 transpose_cast_h16, per 65 536 rows: head_qk_rows,                 W5k -> W5T;  U -> qk16 (QK);  qk16, W5T -> G
//                         head_logit_table_<h>
//   -- per chunk of queries (fused: plan.qcf, one chunk up to 2^20 queries;  staged: plan.qc = 65 536) ------------------------------------
//   kv      fused32       head_kv_fused                                                      U, Tk, Tv, [G] -> Z
//           fused16       head_kv_fused_<h>                                                  the same
//           wide          head_kv_fused_wide (its mode: f16, f16 pairs, x3)                  the same
//           chain         memset, head_kv_chain[_pairs]_<h>, then fused16 gated on the flag  U, Tk, Tv, G -> Z, chain_flag
//   decode  fused32 | fused16 | wide | chain                                                 Z -> rgb
//                         head_decode_fused[_<h>] | .._wide | head_decode_chain[_pairs]_<h>
//   staged_chunk          head_rows, mlp_hidden x n, mlp_out_k, mlp_hidden x n, mlp_out_v,   Tk, Tv -> bufA (Hk), Hv, q_idx, k_idx -> bufB <-> bufA -> WK;
//                         local_attention, mlp_in_q, mlp_hidden_q x n, decode_residual       Hv -> bufA <-> bufB -> WV;  U, WK, WV -> Z -> bufA <-> bufB -> rgb
// The fused routes need local_size 2, ReLU chains of 256-wide layers and packed fragments; everything else, and head_route bit 0, runs staged
// (fp32 only: a 16-bit entry without a fused route is refused).  Staged form: every stage is its own kernel with a clean roofline.
// The stages above the dashed line depend on the LR image only (HeadCall::per_image), those below on the queries (per_query).
// ciaosr_head_prepare_* runs the first half into a caller-owned scene (U, Tk, Tv, [G]), ciaosr_head_query_* the second half from it, any
// number of times: the same stage functions, the same route (planned for q_plan queries), the same carve list with an owner per buffer.
#include "ops.h"

namespace ciaosr {

struct HeadPlan {
    int H, W, C, Cn, D, Dv, J, HW;
    long Q;
    int wk0, wv0;            // layer-0 widths
    int wmax;                // widest hidden activation among k / v / q chains
    int qc;                  // queries per work-chunk of the STAGED route (its [4 qc][..] intermediates are the big buffers)
    int qcf;                 // queries per launch pair of the FUSED route: only Z [qcf][Dv] scales with it, so a whole 192x192
                             // tile (589 824 queries) is ONE launch pair instead of nine -- every launch ends with a drain phase
                             // in which the 4-workgroups-per-CU overlap that the kernels live on decays (probe: a workgroup lives
                             // 685k cycles, a 65 536-query launch 3.0M, so ~1/4 of every launch ran under-occupied)
    size_t csa_bytes;
    size_t R() const { return (size_t)qc * J; }      // key / value rows of a staged chunk
};

constexpr int kLdG = 260;        // logit-table row: 256 coefficients + the bias term + pad
constexpr int kQkChunk = 65536;  // rows of (q*key) products materialised at a time

static int n_samples(int local_size) { return local_size == 1 ? 1 : (local_size == 2 ? 4 : 9); }

static HeadPlan head_plan(int H, int W, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt) {
    HeadPlan p;
    p.H = H; p.W = W; p.C = w->channels; p.Cn = w->nonlocal_channels; p.Q = Q;
    p.D = (w->no_unfold ? 1 : 9) * p.C; p.Dv = p.D + p.Cn; p.J = n_samples(w->local_size); p.HW = H * W;
    p.wk0 = w->k.width[0];
    p.wv0 = w->v.width[0];
    int wm = 4;
    for (int i = 0; i + 1 < w->k.n_layers; ++i) wm = wm > w->k.width[i] ? wm : w->k.width[i];
    for (int i = 0; i + 1 < w->v.n_layers; ++i) wm = wm > w->v.width[i] ? wm : w->v.width[i];
    for (int i = 0; i + 1 < w->q.n_layers; ++i) wm = wm > w->q.width[i] ? wm : w->q.width[i];
    p.wmax = wm;
    p.qc = Q < 65536 ? Q : 65536;
    p.qcf = Q < (1 << 20) ? Q : (1 << 20);
    const long zcap = (long)(0xE0000000ull / ((size_t)p.Dv * sizeof(float)));      // Z is addressed through a 32-bit buffer descriptor
    if (p.qcf > zcap) p.qcf = (int)zcap;
    const int max_sc = w->nonlocal_max_scale ? w->nonlocal_max_scale : 2;
    p.csa_bytes = p.Cn > 0 ? ciaosr_cs_attn_workspace_bytes_scale(H, W, p.C, max_sc) : 0;
    if (p.Cn > 0 && opt && opt->csa_block_mb > 0) {         // cs_attn in bands: the largest of the scales' sizes (a band's S does not grow with the scale)
        p.csa_bytes = 0;
        for (int sc = 2; sc <= (max_sc < 2 || max_sc > 4 ? 4 : max_sc); ++sc) {
            const size_t n = ciaosr_cs_attn_workspace_bytes_opt(H, W, p.C, sc, opt);
            p.csa_bytes = n > p.csa_bytes ? n : p.csa_bytes;
        }
    }
    return p;
}

// The workspace.  Each buffer is named for its first occupant (head_carve); every later use of one is a view here, with the reason it
// fits: a capacity that always holds as a comment, one that can fail as a *_fits predicate that head_route() consults.
struct HeadBuffers : HeadPlan {
    float *U, *Tk, *Tv, *bufA, *bufB, *Hv, *WK, *WV, *Z, *G, *QK, *csa_ws;
    int *q_idx, *k_idx, *chain_flag;
    unsigned short *W5T, *H16;
    // h16 layer-0 tables: 16-bit copies of U [HW][Dv] and of both layer-0 weights [wk0][D], [wv0][Dv].  One call: where the staged route
    // keeps its activations (H16 = bufA, free on the fused routes, the only ones with a 16-bit mode): u16_fits.  A scene: their own buffer
    unsigned short* u16() const { return H16; }
    unsigned short* wk16() const { return u16() + round_up((size_t)HW * Dv, 128); }
    unsigned short* wv16() const { return wk16() + round_up((size_t)wk0 * D, 128); }
    // the nine product maps [9][HW][C] of the Winograd logit table, where the GEMM forms keep a chunk of rows [kQkChunk][9C]: qk_maps_fits
    float* qk_maps() const { return QK; }
    // the same chunk of rows in 16 bits for the 16-bit table GEMM.  2 kQkChunk D <= 4 kQkChunk D
    unsigned short* qk16() const { return reinterpret_cast<unsigned short*>(QK); }
};
static bool u16_fits(const HeadPlan& p) {                                                              // not at small Q
    return (size_t)p.HW * p.Dv * 2 + 256 + (size_t)(p.wk0 + p.wv0) * p.Dv * 2 + 512 <= p.R() * p.wmax * sizeof(float);
}
static bool qk_maps_fits(const HeadPlan& p) { return p.HW <= kQkChunk; }                               // not above 256 x 256 pixels
static size_t h16_floats(const HeadPlan& p) {                                                          // u16 | wk16 | wv16, as floats
    return (round_up((size_t)p.HW * p.Dv, 128) + round_up((size_t)p.wk0 * p.D, 128) + (size_t)p.wv0 * p.Dv + 1) / 2;
}

// Who owns a buffer when the head runs as prepare + query (ciaosr_head_prepare_* / ciaosr_head_query_*): the scene holds what the per-image
// stages write and the per-query kernels read, the two workspaces what only one side touches.  ciaosr_head_forward_* carves all of them
// from its one workspace.
enum Owner { kScene, kPrepare, kQuery };
struct SceneLayout { bool logit, h16; };      // what of the scene's optional buffers its route needs

// The one list of carve-outs, in carve order: take(owner, floats) is Arena::take (256-byte aligned) on the owner's arena for a call, a
// running sum for a byte count.  scene = nullptr: the one-call layout (every buffer, the 16-bit copies inside bufA).
template <class Take>
static HeadBuffers head_carve(const HeadPlan& p, const SceneLayout* scene, Take take) {
    const size_t HW = p.HW, R = p.R();
    HeadBuffers b = {p};
    b.U = take(kScene, HW * p.Dv);                    // unfold rows [HW][D] and, behind them, the non-local maps [HW][Cn]
    b.Tk = take(kScene, HW * p.wk0); b.Tv = take(kScene, HW * p.wv0);       // layer-0 tables
    b.bufA = take(kQuery, R * p.wmax); b.bufB = take(kQuery, R * p.wmax);   // staged: ping-pong activations
    b.Hv = take(kQuery, R * p.wv0);                   // staged: layer-0 rows of the value chain, kept while the key chain runs
    b.WK = take(kQuery, R * p.D); b.WV = take(kQuery, R * p.Dv);            // staged: the chains' outputs
    b.Z = take(kQuery, (size_t)p.qcf * p.Dv);         // attention output of a chunk (sized for the fused routes' chunk)
    b.q_idx = reinterpret_cast<int*>(take(kQuery, p.qc)); b.k_idx = reinterpret_cast<int*>(take(kQuery, R));
    b.G = take(kScene, !scene || scene->logit ? HW * 9 * kLdG : 0);         // logit table
    b.QK = take(kPrepare, (size_t)kQkChunk * p.D);    // one chunk of its GEMM rows
    b.W5T = reinterpret_cast<unsigned short*>(take(kPrepare, (size_t)128 * p.D + 64));   // 16-bit modes: transposed 16-bit copy [256][D] of imnet_k's output layer
    b.chain_flag = reinterpret_cast<int*>(take(kQuery, 64));  // 16-bit chained kernel: its "redo with the 128-row kernel" flag
    b.csa_ws = take(kPrepare, p.csa_bytes / sizeof(float));   // cs_attn's workspace (a whole number of floats: csa_carve_bytes)
    b.H16 = reinterpret_cast<unsigned short*>(scene ? take(kPrepare, scene->h16 ? h16_floats(p) : 0) : b.bufA);
    return b;
}
static size_t head_ws_bytes(const HeadPlan& p) {
    size_t n = 0;
    head_carve(p, nullptr, [&](Owner, size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 32 * 256;              // room for the 256-byte alignment of each carve-out
}
// prepare + query: each owner's buffers from its own arena (nullptr: not this side's), at the offsets the same takes give every time
static HeadBuffers head_carve_split(const HeadPlan& p, const SceneLayout& lay, Arena* const (&ar)[3]) {
    return head_carve(p, &lay, [&](Owner o, size_t floats) { return ar[o] ? ar[o]->take<float>(floats) : (float*)nullptr; });
}
struct SplitBytes { size_t n[3]; };                   // by Owner
static SplitBytes head_split_bytes(const HeadPlan& p, const SceneLayout& lay) {
    Arena a[3] = {Arena(nullptr, ~(size_t)0), Arena(nullptr, ~(size_t)0), Arena(nullptr, ~(size_t)0)};
    Arena* const ar[3] = {&a[0], &a[1], &a[2]};
    head_carve_split(p, lay, ar);
    return {{round_up(a[0].off, 256), round_up(a[1].off, 256), round_up(a[2].off, 256)}};
}

static int mlp_act(const ciaosr_mlp_t& m) { return m.act == CIAOSR_ACT_SIN || m.act == CIAOSR_ACT_COS ? m.act : CIAOSR_ACT_RELU; }

static bool mlp_ok(const ciaosr_mlp_t& m) {
    if (m.n_layers < 1 || m.n_layers > CIAOSR_MAX_LAYERS) return false;
    for (int i = 0; i < m.n_layers; ++i)
        if (!m.weight[i] || !m.bias[i] || (m.ld[i] & 3) != 0 || m.width[i] <= 0) return false;
    return true;
}

// fused kernels: hidden width 256 everywhere, fragments packed, 4 key samples
static bool chain_fused_ok(const ciaosr_mlp_t& m, bool is_q, bool h16) {
    if (m.n_layers < 2 || mlp_act(m) != CIAOSR_ACT_RELU) return false;
    for (int i = 0; i + 1 < m.n_layers; ++i)
        if (m.width[i] != 256) return false;
    for (int i = is_q ? 0 : 1; i < m.n_layers - (is_q ? 1 : 0); ++i)
        if (!(h16 ? m.frag16[i] : (const void*)m.frag[i])) return false;
    return true;
}

enum HeadTables { kTablesH16, kTablesSmall, kTablesGemm };
enum HeadLogit { kLogitNone, kLogitGemm32, kLogitGemm16, kLogitWino2, kLogitWino4 };
enum HeadKernel { kHeadFused32, kHeadFused16, kHeadWide, kHeadChain };
struct HeadRoute {
    int refusal;            // CIAOSR_OK, or what the call returns before its first launch
    bool fused;             // else staged: one kernel per stage (fp32 only)
    bool h16, lo;           // fused: 16-bit fragments; their hi + lo weight pairs
    HeadTables tables;
    HeadLogit logit;
    HeadKernel kernel;      // kv and decode of the fused routes; behind the chained kv kernel it runs gated
    int wide_mode;          // kHeadWide: 0 = f16, 1 = f16 pairs, 2 = x3
    bool chain, decode_chain;   // the chained kernels, as far as it does not depend on the chunk
    // The chained kv kernel addresses a chunk's 16-bit Z rows with 32-bit offsets: the one condition asked per chunk of queries.
    HeadKernel kv(const HeadPlan& p, int nq) const { return chain && (size_t)nq * p.Dv * 2 < 0xFFFFFF00ull ? kHeadChain : kernel; }
    HeadKernel decode(const HeadPlan& p, int nq) const { return decode_chain && kv(p, nq) == kHeadChain ? kHeadChain : kernel; }
};

// What a call runs; launches nothing.
static HeadRoute head_route(const HeadPlan& p, Prec prec, const Mode& m, const ciaosr_options_t* opt, const ciaosr_head_weights_t* w) {
    const int bits = opt ? opt->head_route : 0;
    HeadRoute r = {CIAOSR_OK, false, prec != kF32, m.lo, kTablesGemm, kLogitNone, kHeadFused32, m.x3 ? 2 : (m.lo ? 1 : 0), false, false};
    r.fused = !(bits & CIAOSR_HEAD_STAGED) && w->local_size == 2 && chain_fused_ok(w->k, false, r.h16) && chain_fused_ok(w->v, false, r.h16) &&
              chain_fused_ok(w->q, true, r.h16) && (p.Dv & 7) == 0;
    if (r.h16 && !r.fused) r.refusal = CIAOSR_ERR_UNSUPPORTED;        // the 16-bit modes exist for the fused kernels only
    if (m.x3 && r.refusal == CIAOSR_OK) {                              // the pair kernels read every lo fragment unconditionally
        bool all = true;
        for (int i = 1; i < w->k.n_layers; ++i) all = all && w->k.frag16_lo[i];
        for (int i = 1; i < w->v.n_layers; ++i) all = all && w->v.frag16_lo[i];
        for (int i = 0; i + 1 < w->q.n_layers; ++i) all = all && w->q.frag16_lo[i];
        if (!all) r.refusal = CIAOSR_ERR_BAD_ARG;
    }
    // exact layer-1 hoist: T = U . W1[:, :fan]^T + b1, one row per LR pixel.  f16 mode: on the 16-bit GEMM from a half copy of U
    if (m.hoist16 && (p.D & 7) == 0 && (p.Dv & 7) == 0 && u16_fits(p)) r.tables = kTablesH16;
    else if (gemm_small_ok(p.HW, p.wk0, p.D, p.Dv, w->k.ld[0]) && gemm_small_ok(p.HW, p.wv0, p.Dv, p.Dv, w->v.ld[0]) && p.HW <= 4096)
        r.tables = kTablesSmall;
    // logit table of imnet_k's output layer (exact fold, head_ops.hip): pays off when queries outnumber LR pixels
    const int last = w->k.n_layers - 1;
    if (r.fused && !(bits & CIAOSR_HEAD_NO_LOGIT_TABLE) && w->k.width[last] == p.D && w->k.width[last - 1] == 256 && p.Q * p.J > (long)p.HW * 9 &&
        (size_t)p.HW * 9 * kLdG * sizeof(float) < 0xFFFFFF00ull) {
        // 16-bit modes: the table GEMM on the 16-bit MFMA (fp32 table out).  (Half-pairs mode: the exact-fp32 GEMM here was measured
        // and changes nothing -- max |delta| 1.04e-3 -> 1.14e-3 on the full-tile vector, +0.9 ms: W5's rounding is not what limits it.)
        r.logit = m.table16 && (p.D & 7) == 0 ? kLogitGemm16 : kLogitGemm32;
        // fp32, C = 64: nine Winograd convolutions of the product maps Pi_o = F . shift_o(F) (same sums as the GEMM rows, re-associated
        // through the transform; 2.25x fewer multiplies, F(4x4): 4x), the maps where the GEMM would keep its row chunk
        if (!m.table16 && w->k_out_wino && !(bits & CIAOSR_HEAD_TABLE_GEMM) && p.C == 64 && !w->no_unfold && p.HW >= 512 && qk_maps_fits(p))
            r.logit = w->k_out_wino4 && !(bits & CIAOSR_HEAD_TABLE_WINO2) ? kLogitWino4 : kLogitWino2;
    }
    if (!r.fused) return r;
    // f16x3 runs the wide-workgroup kernels (head_fused_wide.hip: its two activation arrays leave room for one workgroup per CU);
    // f16 / f16-pairs keep the 128-row kernels with two workgroups per CU (head_fused_h16.hip) and take the wide form -- 256 rows, half
    // the weight stream per MFMA, measured equal in time: one workgroup per CU exposes its gather phases -- only with head_route bit 3
    const bool wide = m.x3 || (prec == kF16 && (bits & CIAOSR_HEAD_WIDE_WG));
    r.kernel = wide ? kHeadWide : r.h16 ? kHeadFused16 : kHeadFused32;
    // 16-bit default: the weights-stationary, register-chained kernel (head_chain_h16.hip) where its weight stream is given and the
    // logit table exists; imnet_q through the same form where the blob carries its stream (Dv a multiple of 128, 256-wide layers)
    r.chain = r.kernel == kHeadFused16 && r.logit != kLogitNone && (m.lo ? w->chain16_pairs : w->chain16) && !(bits & CIAOSR_HEAD_NO_CHAIN) &&
              h16_ops(prec).head_chain_ok(w);
    r.decode_chain = r.chain && !(bits & CIAOSR_HEAD_NO_DECODE_CHAIN) && h16_ops(prec).head_decode_chain_ok(w);
    return r;
}

// The fp32 ping-pong loop of the staged route: layers i0 <= i < i1 of m on `rows` rows, from cur [rows][ld_cur] (K = k_cur), hidden
// activations packed (ld = width) alternately into pp0, pp1; the MLP's last layer, when in range, writes last_out (ld_last) without
// activation under tag_out.  *end = the rows the last launch wrote.
static int mlp_layers_f32(const ciaosr_mlp_t& m, int i0, int i1, const float* cur, int ld_cur, int k_cur, float* pp0, float* pp1, float* last_out,
                          int ld_last, long rows, hipStream_t s, const char* tag_first, const char* tag_hidden, const char* tag_out,
                          const float** end = nullptr) {
    float* pp[2] = {pp0, pp1};
    for (int i = i0; i < i1; ++i) {
        const bool last = i == m.n_layers - 1;
        float* dst = last ? last_out : pp[(i - i0) & 1];
        const int ldd = last ? ld_last : m.width[i];
        const int rc = gemm_f32(cur, ld_cur, m.weight[i], m.ld[i], false, dst, ldd, m.bias[i], (int)rows, m.width[i], k_cur, 1.f,
                                last ? CIAOSR_ACT_NONE : mlp_act(m), 0.f, s, last ? tag_out : i == i0 ? tag_first : tag_hidden);
        if (rc != CIAOSR_OK) return rc;
        cur = dst; ld_cur = ldd; k_cur = m.width[i];
    }
    if (end) *end = cur;
    return CIAOSR_OK;
}

// the fields FusedChain (imnet_k, imnet_v) and FusedQP (imnet_q) share: the hidden layers 1 .. n - 2
template <class P>
static void fill_hidden(P& c, const ciaosr_mlp_t& m, const HeadRoute& r) {
    c.n_hidden = m.n_layers - 2;
    for (int i = 0; i < c.n_hidden; ++i) {
        c.frag_hidden[i] = r.h16 ? m.frag16[i + 1] : (const void*)m.frag[i + 1];
        c.frag_hidden_lo[i] = (r.h16 && r.lo) ? m.frag16_lo[i + 1] : nullptr;
        c.bias_hidden[i] = m.bias[i + 1];
    }
}
static void fill_chain(FusedChain& c, const ciaosr_mlp_t& m, const float* table, int fan, const HeadRoute& r) {
    const int last = m.n_layers - 1;
    c.table = table;
    c.tail = m.weight[0] + fan;
    c.ld_tail = m.ld[0];
    fill_hidden(c, m, r);
    c.frag_out = r.h16 ? m.frag16[last] : (const void*)m.frag[last];
    c.frag_out_lo = (r.h16 && r.lo) ? m.frag16_lo[last] : nullptr;
    c.bias_out = m.bias[last];
    c.n_out = m.width[last];
}

static const decltype(&ciaosr_cs_attn_f32) kCsAttnEntry[3] = {ciaosr_cs_attn_f32, ciaosr_cs_attn_bf16, ciaosr_cs_attn_f16};   // by Prec
static const char* const kLogitTableTag16[3] = {nullptr, "head_logit_table_bf16", "head_logit_table_f16"};

#define HEAD_RUN(x) do { const int rc_ = (x); if (rc_ != CIAOSR_OK) return rc_; } while (0)
// One call: the plan, the buffers, the route and one function per stage.
struct HeadCall : HeadBuffers {
    HeadRoute r; Prec prec;
    const float* feat; const ciaosr_head_weights_t* w; const ciaosr_csattn_weights_t* csattn;
    const float *x_lr, *coord, *cell; int chunk; float* rgb; const ciaosr_options_t* opt; hipStream_t s;

    // unfold rows U[:, :9C] (net:132-136); feat_unfold=False (net:139-141): the "unfold" row is the pixel's C features (a 1x1 patch)
    int unfold() const {
        const int k = w->no_unfold ? 1 : 3;
        return patch_rows(feat, C, H, W, C, k, 1, k / 2, H, W, U, Dv, 0, 0.f, s, "head_unfold");
    }
    // the non-local maps into U[:, 9C:] (net:134-137): one C-column slice per scale, in the order of multi_scale (csa:528 torch.cat(res_y, dim=1))
    int cs_attn(int n_scales) const {
        for (int i = 0; i < n_scales; ++i)
            HEAD_RUN(kCsAttnEntry[prec](feat, C, H, W, csattn + i, U + D + (size_t)i * C, Dv, opt, csa_ws, csa_bytes, s));
        return CIAOSR_OK;
    }
    int layer0_tables() const {
        const struct { const ciaosr_mlp_t& m; float* T; int n, fan; } kv[2] = {{w->k, Tk, wk0, D}, {w->v, Tv, wv0, Dv}};
        if (r.tables == kTablesH16) {
            const H16Ops& h = h16_ops(prec);
            unsigned short* const w16[2] = {wk16(), wv16()};
            HEAD_RUN(h.cast_rows(U, Dv, u16(), Dv, HW, Dv, s));
            for (int i = 0; i < 2; ++i) HEAD_RUN(h.cast_rows(kv[i].m.weight[0], kv[i].m.ld[0], w16[i], kv[i].fan, kv[i].n, kv[i].fan, s));
            for (int i = 0; i < 2; ++i)
                HEAD_RUN(h.conv1x1(u16(), Dv, w16[i], kv[i].fan, kv[i].m.bias[0], nullptr, 0, kv[i].T, kv[i].n, nullptr, 0, nullptr, 0, HW, kv[i].n, kv[i].fan, s,
                                   "head_table_f16"));
            return CIAOSR_OK;
        }
        for (const auto& t : kv)
            HEAD_RUN(r.tables == kTablesSmall ? gemm_small_f32(U, Dv, t.m.weight[0], t.m.ld[0], t.m.bias[0], t.T, t.n, nullptr, 0, nullptr, 0, HW, t.n, t.fan,
                                                               CIAOSR_ACT_NONE, 0.f, 1.f, s, "head_table")
                                              : gemm_f32(U, Dv, t.m.weight[0], t.m.ld[0], false, t.T, t.n, t.m.bias[0], HW, t.n, t.fan, 1.f, CIAOSR_ACT_NONE, 0.f, s,
                                                         "head_table"));
        return CIAOSR_OK;
    }
    int logit_table() const {
        if (r.logit == kLogitNone) return CIAOSR_OK;
        const int last = w->k.n_layers - 1;
        const long total = (long)HW * 9;
        const float *w5 = w->k.weight[last], *b5 = w->k.bias[last];
        if (r.logit == kLogitWino4 || r.logit == kLogitWino2) {
            HEAD_RUN(ciaosr::qk_maps(feat, C, C, H, W, qk_maps(), s));
            HEAD_RUN(r.logit == kLogitWino4 ? wino4_table_f32(qk_maps(), H, W, w->k_out_wino4, 4, G, kLdG, s)
                                            : wino_table_f32(qk_maps(), H, W, w->k_out_wino, 4, G, kLdG, s));
            return qk_rows(U, Dv, D, H, W, 0, (int)total, b5, nullptr, G, kLdG, 3, s);
        }
        const bool t16 = r.logit == kLogitGemm16;
        if (t16) HEAD_RUN(transpose_cast_h16(w5, w->k.ld[last], D, 256, W5T, prec == kF16, s));
        for (long r0 = 0; r0 < total; r0 += kQkChunk) {
            const int nr = (int)((total - r0) < kQkChunk ? (total - r0) : kQkChunk);
            HEAD_RUN(qk_rows(U, Dv, D, H, W, r0, nr, b5, QK, G, kLdG, t16 ? (int)prec : 0, s));
            // G[r][n] = sum_d QK[r][d] * W5k[d][n]: the Linear weight [D][256] is the [K][N] operand as stored
            HEAD_RUN(t16 ? h16_ops(prec).gemm_nt(qk16(), D, W5T, D, G + (size_t)r0 * kLdG, kLdG, false, nr, 256, D, 1.f, s, kLogitTableTag16[prec], 0)
                         : gemm_f32(QK, D, w5, w->k.ld[last], true, G + (size_t)r0 * kLdG, kLdG, nullptr, nr, 256, D, 1.f, CIAOSR_ACT_NONE, 0.f, s,
                                    "head_logit_table"));
        }
        return CIAOSR_OK;
    }

    const void* chain_blob() const { return r.lo ? w->chain16_pairs : w->chain16; }
    // imnet_k, imnet_v and the local attention of nq queries into Z.  Chained: the 128-row kernel is launched behind the chained one, gated
    // on the flag that one raises when a key leaves its query's 3x3 neighbourhood (cannot happen for 0 < cell < 1): it then redoes the
    // launch, else it returns at once
    int kv(long q0, int nq) const {
        FusedKVP kp;
        kp.coord = coord; kp.cell = cell; kp.q0 = q0; kp.nq = nq; kp.chunk = chunk; kp.H = H; kp.W = W;
        kp.U = U; kp.ldu = Dv; kp.D = D; kp.Dv = Dv;
        kp.u_bytes = (unsigned)((size_t)HW * Dv * sizeof(float));
        fill_chain(kp.k, w->k, Tk, D, r);
        fill_chain(kp.v, w->v, Tv, Dv, r);
        kp.softmax_scale = w->softmax_scale;
        kp.Z = Z; kp.ldz = Dv;
        kp.rows_per_wg = opt ? opt->kv_rows : 0;
        kp.G = r.logit != kLogitNone ? G : nullptr; kp.ldg = kLdG; kp.g_bytes = (unsigned)((size_t)HW * 9 * kLdG * sizeof(float));
        kp.gate = nullptr;
        if (r.kv(*this, nq) == kHeadChain) {
            if (hipMemsetAsync(chain_flag, 0, sizeof(int), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
            HEAD_RUN(h16_ops(prec).head_kv_chain(kp, w, chain_blob(), r.lo ? 1 : 0, opt ? opt->query_grid_w : 0, chain_flag, s));
            kp.gate = chain_flag;
        }
        if (r.kernel == kHeadWide) return h16_ops(prec).head_kv_fused_wide(kp, r.wide_mode, s);
        return r.kernel == kHeadFused16 ? h16_ops(prec).head_kv_fused(kp, s) : head_kv_fused(kp, s);
    }
    // imnet_q on Z with the bilinear residual of the last layer, into rgb
    int decode(long q0, int nq) const {
        const ciaosr_mlp_t& mq = w->q;
        const int last = mq.n_layers - 1;
        FusedQP qp;
        qp.Z = Z; qp.ldz = Dv; qp.Dv = Dv;
        qp.frag_in = r.h16 ? mq.frag16[0] : (const void*)mq.frag[0]; qp.bias_in = mq.bias[0];
        qp.frag_in_lo = (r.h16 && r.lo) ? mq.frag16_lo[0] : nullptr;
        qp.nj_in = r.h16 ? (Dv + 15) / 16 : (Dv + 7) / 8;
        fill_hidden(qp, mq, r);
        qp.w_last = mq.weight[last]; qp.ld_last = mq.ld[last]; qp.b_last = mq.bias[last];
        qp.rows_per_wg = opt ? opt->decode_rows : 0;
        qp.x_lr = x_lr; qp.coord = coord; qp.q0 = q0; qp.nq = nq; qp.H = H; qp.W = W; qp.rgb = rgb;
        if (r.decode(*this, nq) == kHeadChain) {
            const H16Ops& h = h16_ops(prec);
            return h.head_decode_chain(qp, w, reinterpret_cast<const unsigned char*>(chain_blob()) + h.head_kv_chain_bytes(w, r.lo ? 1 : 0), r.lo ? 1 : 0, s);
        }
        if (r.kernel == kHeadWide) return h16_ops(prec).head_decode_fused_wide(qp, r.wide_mode, s);
        return r.kernel == kHeadFused16 ? h16_ops(prec).head_decode_fused(qp, s) : head_decode_fused(qp, s);
    }
    int staged_chunk(long q0, int nq) const {
        const long rows = (long)nq * J;
        HeadRowsP hp;
        hp.coord = coord; hp.cell = cell; hp.q0 = q0; hp.nq = nq; hp.chunk = chunk; hp.H = H; hp.W = W;
        hp.local_size = w->local_size; hp.J = J;
        hp.Tk = Tk; hp.Tv = Tv;
        hp.tailK = w->k.weight[0] + D;      // columns [9C, 9C+4) of layer 0, stride ld -> packed copy below
        hp.tailV = w->v.weight[0] + Dv;
        hp.wk0 = wk0; hp.wv0 = wv0; hp.relu_k = mlp_act(w->k); hp.relu_v = mlp_act(w->v);
        hp.Hk = bufA; hp.Hv = Hv; hp.q_idx = q_idx; hp.k_idx = k_idx;
        hp.ld_tail_k = w->k.ld[0]; hp.ld_tail_v = w->v.ld[0];
        HEAD_RUN(head_rows(hp, s));
        // imnet_k layers 1..n-1 -> WK   (bufA holds layer-0 rows; ping-pong through bufB/bufA)
        HEAD_RUN(mlp_layers_f32(w->k, 1, w->k.n_layers, bufA, wk0, wk0, bufB, bufA, WK, D, rows, s, "mlp_hidden", "mlp_hidden", "mlp_out_k"));
        // imnet_v: layer-0 rows are in Hv
        HEAD_RUN(mlp_layers_f32(w->v, 1, w->v.n_layers, Hv, wv0, wv0, bufA, bufB, WV, Dv, rows, s, "mlp_hidden", "mlp_hidden", "mlp_out_v"));
        LocalAttnP lp{U, Dv, D, Dv, q_idx, k_idx, WK, D, WV, Dv, Z, Dv, nq, J, w->softmax_scale};
        HEAD_RUN(local_attention(lp, s));
        // imnet_q: layer 0 on Z, hidden layers, last layer fused with the bilinear residual
        const ciaosr_mlp_t& mq = w->q;
        const int last = mq.n_layers - 1;
        const float* h;
        HEAD_RUN(mlp_layers_f32(mq, 0, last, Z, Dv, Dv, bufA, bufB, nullptr, 0, nq, s, "mlp_in_q", "mlp_hidden_q", nullptr, &h));
        DecodeP dp{h, mq.width[last - 1], mq.width[last - 1], mq.weight[last], mq.ld[last], mq.bias[last], x_lr, coord, q0, nq, H, W, rgb};
        return decode_residual(dp, s);
    }
    // The two halves of a call.  per_image: what depends on the LR image only (writes the scene's buffers); per_query: the Q queries of
    // coord / cell in chunks of the route's step (reads them)
    int per_image(int n_scales) const {
        HEAD_RUN(unfold());
        HEAD_RUN(cs_attn(n_scales));
        HEAD_RUN(layer0_tables());
        return logit_table();
    }
    int per_query(long Q) const {
        const int step = r.fused ? qcf : qc;
        for (long q0 = 0; q0 < Q; q0 += step) {
            const int nq = (int)((Q - q0) < step ? (Q - q0) : step);
            if (r.fused) {
                HEAD_RUN(kv(q0, nq));
                HEAD_RUN(decode(q0, nq));
            } else {
                HEAD_RUN(staged_chunk(q0, nq));
            }
        }
        return CIAOSR_OK;
    }
};

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_head_workspace_bytes(int H, int W, const ciaosr_head_weights_t* w, int Q) {
    if (!w || H <= 0 || W <= 0 || Q <= 0) return 0;
    return head_ws_bytes(head_plan(H, W, w, Q, nullptr));
}
extern "C" size_t ciaosr_head_workspace_bytes_opt(int H, int W, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt) {
    if (!w || H <= 0 || W <= 0 || Q <= 0 || !options_ok(opt)) return 0;
    return head_ws_bytes(head_plan(H, W, w, Q, opt));
}

// The argument checks the head's entry points share, in the order head_forward has always made them
static int head_check_weights(int H, int W, const ciaosr_head_weights_t* w, const ciaosr_options_t* opt) {
    CIAOSR_CHECK_ARG(w && H >= 1 && W >= 1);
    CIAOSR_CHECK_ARG(options_ok(opt));
    CIAOSR_CHECK_ARG(w->channels >= 4 && (w->channels & 3) == 0 && (w->nonlocal_channels & 3) == 0);
    CIAOSR_CHECK_ARG(w->local_size >= 1 && w->local_size <= 3 && w->softmax_scale != 0.f);
    CIAOSR_CHECK_ARG(mlp_ok(w->q) && mlp_ok(w->k) && mlp_ok(w->v));
    return CIAOSR_OK;
}
static int head_check_dims(const HeadPlan& p, const ciaosr_head_weights_t* w) {
    // dims wiring of LocalImplicitSRNet.__init__ (ciaosr_net.py:61-76)
    CIAOSR_CHECK_ARG(w->k.in_dim == p.D + 4 && w->k.width[w->k.n_layers - 1] == p.D);
    CIAOSR_CHECK_ARG(w->v.in_dim == p.Dv + 4 && w->v.width[w->v.n_layers - 1] == p.Dv);
    CIAOSR_CHECK_ARG(w->q.in_dim == p.Dv && w->q.width[w->q.n_layers - 1] == 3);
    CIAOSR_CHECK_ARG(w->k.n_layers >= 2 && w->v.n_layers >= 2 && w->q.n_layers >= 2);
    CIAOSR_CHECK_ARG((p.wk0 & 3) == 0 && (p.wv0 & 3) == 0);
    return CIAOSR_OK;
}
static int head_check_csattn(const HeadPlan& p, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, int* n_scales) {
    CIAOSR_CHECK_ARG((w->nonlocal_channels > 0) == (csattn != nullptr));
    *n_scales = csattn ? p.Cn / p.C : 0;                     // csattn = host array, one struct per entry of multi_scale
    if (csattn) {
        CIAOSR_CHECK_ARG(p.Cn == *n_scales * p.C && *n_scales >= 1 && *n_scales <= 3);
        for (int i = 0; i < *n_scales; ++i) {
            const int sc = csattn[i].scale ? csattn[i].scale : 2;
            CIAOSR_CHECK_ARG(csattn[i].channels == p.C && sc <= (w->nonlocal_max_scale ? w->nonlocal_max_scale : 2));
        }
    }
    return CIAOSR_OK;
}
static int head_route_refusal(const HeadRoute& r) {          // the route's refusals: before the first launch
    if (r.refusal == CIAOSR_ERR_UNSUPPORTED) return CIAOSR_ERR_UNSUPPORTED;
    CIAOSR_CHECK_ARG(r.refusal == CIAOSR_OK);                // x3 without every lo fragment
    return CIAOSR_OK;
}

static int head_forward(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn,
                        const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb, const ciaosr_options_t* opt,
                        void* workspace, size_t workspace_bytes, void* stream_, Prec prec) {
    CIAOSR_CHECK_ARG(feat_hwc && w && coord && cell && rgb && workspace && H >= 1 && W >= 1 && Q >= 1);
    HEAD_RUN(head_check_weights(H, W, w, opt));
    const HeadPlan p = head_plan(H, W, w, Q, opt);
    HEAD_RUN(head_check_dims(p, w));
    int n_scales;
    HEAD_RUN(head_check_csattn(p, w, csattn, &n_scales));
    if (workspace_bytes < head_ws_bytes(p)) return CIAOSR_ERR_WORKSPACE;
    CIAOSR_CHECK_ARG((size_t)p.HW * p.Dv * sizeof(float) < 0xFFFFFF00ull);   // 32-bit buffer offsets into U (and into its 16-bit copy)
    Arena ar(workspace, workspace_bytes);
    const HeadCall c = {head_carve(p, nullptr, [&](Owner, size_t floats) { return ar.take<float>(floats); }), head_route(p, prec, resolve_mode(prec, opt), opt, w),
                        prec, feat_hwc, w, csattn, x_lr_nchw, coord, cell, chunk, rgb, opt, (hipStream_t)stream_};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    HEAD_RUN(head_route_refusal(c.r));
    HEAD_RUN(c.per_image(n_scales));
    return c.per_query(Q);
}

extern "C" int ciaosr_head_forward_f32(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn,
                                       const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb, const ciaosr_options_t* opt,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return head_forward(feat_hwc, H, W, w, csattn, x_lr_nchw, coord, cell, Q, chunk, rgb, opt, workspace, workspace_bytes, stream, kF32);
}

extern "C" int ciaosr_head_forward_bf16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn,
                                        const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb, const ciaosr_options_t* opt,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return head_forward(feat_hwc, H, W, w, csattn, x_lr_nchw, coord, cell, Q, chunk, rgb, opt, workspace, workspace_bytes, stream, kBF16);
}

extern "C" int ciaosr_head_forward_f16(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn,
                                       const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb, const ciaosr_options_t* opt,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return head_forward(feat_hwc, H, W, w, csattn, x_lr_nchw, coord, cell, Q, chunk, rgb, opt, workspace, workspace_bytes, stream, kF16);
}

// ---- a persistent scene: the per-image half once (prepare), the per-query half any number of times (query) -----------------------------
// The route is planned for q_plan queries (head_route reads Q in the logit-table threshold and in u16_fits); a query of any Q runs under
// it, in chunks computed from its own Q.  The descriptor records what the scene was built as; query checks it before its first launch.
constexpr int kSceneMagic = 0x43530001;               // 'CS', layout version 1

static int route_code(const HeadRoute& r) {
    if (r.refusal != CIAOSR_OK) return r.refusal;
    return (r.fused ? 1 : 0) | (int)r.tables << 1 | (int)r.logit << 3 | (int)r.kernel << 6 | (r.chain ? 1 : 0) << 8 | (r.decode_chain ? 1 : 0) << 9 |
           (r.h16 ? 1 : 0) << 10 | (r.lo ? 1 : 0) << 11 | r.wide_mode << 12;
}
static SceneLayout scene_layout(const HeadRoute& r) { return {r.logit != kLogitNone, r.tables == kTablesH16}; }

// plan + route of a scene for q_plan queries, after every check that needs no pointer but w
static int scene_route(int H, int W, const ciaosr_head_weights_t* w, int q_plan, Prec prec, const ciaosr_options_t* opt, HeadPlan* p, HeadRoute* r) {
    CIAOSR_CHECK_ARG(q_plan >= 1);
    HEAD_RUN(head_check_weights(H, W, w, opt));
    *p = head_plan(H, W, w, q_plan, opt);
    HEAD_RUN(head_check_dims(*p, w));
    CIAOSR_CHECK_ARG((size_t)p->HW * p->Dv * sizeof(float) < 0xFFFFFF00ull);
    *r = head_route(*p, prec, resolve_mode(prec, opt), opt, w);
    return head_route_refusal(*r);
}

extern "C" int ciaosr_head_route_code(int H, int W, const ciaosr_head_weights_t* w, int Q, int precision, const ciaosr_options_t* opt) {
    CIAOSR_CHECK_ARG(precision >= kF32 && precision <= kF16);
    HeadPlan p; HeadRoute r;
    HEAD_RUN(scene_route(H, W, w, Q, (Prec)precision, opt, &p, &r));
    return route_code(r);
}

// the entry points that size a scene take no precision: the largest over the precisions that have a route
static size_t scene_bytes_max(int H, int W, const ciaosr_head_weights_t* w, int q_plan, const ciaosr_options_t* opt, Owner o) {
    size_t n = 0;
    for (int prec = kF32; prec <= kF16; ++prec) {
        HeadPlan p; HeadRoute r;
        if (scene_route(H, W, w, q_plan, (Prec)prec, opt, &p, &r) != CIAOSR_OK) continue;
        const size_t m = head_split_bytes(p, scene_layout(r)).n[o];
        n = m > n ? m : n;
    }
    return n;
}
extern "C" size_t ciaosr_head_scene_bytes(int H, int W, const ciaosr_head_weights_t* w, int q_plan, const ciaosr_options_t* opt) {
    return scene_bytes_max(H, W, w, q_plan, opt, kScene);
}
extern "C" size_t ciaosr_head_prepare_workspace_bytes(int H, int W, const ciaosr_head_weights_t* w, int q_plan, const ciaosr_options_t* opt) {
    return scene_bytes_max(H, W, w, q_plan, opt, kPrepare);
}

static int off256(const void* p, const void* base) { return p ? (int)(((const char*)p - (const char*)base) >> 8) : -1; }

static int head_prepare(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, int q_plan,
                        const ciaosr_options_t* opt, void* scene, size_t scene_bytes, ciaosr_head_scene_t* desc, void* workspace,
                        size_t workspace_bytes, void* stream_, Prec prec) {
    CIAOSR_CHECK_ARG(feat_hwc && scene && desc && workspace);
    HeadPlan p; HeadRoute r;
    HEAD_RUN(scene_route(H, W, w, q_plan, prec, opt, &p, &r));
    int n_scales;
    HEAD_RUN(head_check_csattn(p, w, csattn, &n_scales));
    const SceneLayout lay = scene_layout(r);
    const SplitBytes need = head_split_bytes(p, lay);
    CIAOSR_CHECK_ARG(need.n[kScene] >> 8 < 0x7FFFFFFFull);                        // the descriptor counts 256-byte units in an int
    if (scene_bytes < need.n[kScene] || workspace_bytes < need.n[kPrepare]) return CIAOSR_ERR_WORKSPACE;
    Arena sc(scene, scene_bytes), ws(workspace, workspace_bytes);
    Arena* const ar[3] = {&sc, &ws, nullptr};
    const HeadCall c = {head_carve_split(p, lay, ar), r, prec, feat_hwc, w, csattn, nullptr, nullptr, nullptr, 0, nullptr, opt, (hipStream_t)stream_};
    if (!sc.ok || !ws.ok) return CIAOSR_ERR_WORKSPACE;
    *desc = {kSceneMagic, p.H, p.W, p.C, p.Cn, p.D, p.Dv, p.J, q_plan, (int)prec, route_code(r),
             off256(c.U, scene), off256(c.Tk, scene), off256(c.Tv, scene), lay.logit ? off256(c.G, scene) : -1, (int)(need.n[kScene] >> 8)};
    return c.per_image(n_scales);
}

// What query (and its size function) make of a descriptor: the plan for Q queries and the route the scene was planned under, or the
// refusal.  prec < 0: the descriptor's own.
static int scene_open(const ciaosr_head_scene_t* d, const ciaosr_head_weights_t* w, int Q, int prec, const ciaosr_options_t* opt, HeadPlan* p,
                      HeadRoute* r) {
    CIAOSR_CHECK_ARG(d && d->magic == kSceneMagic && Q >= 1 && d->precision >= kF32 && d->precision <= kF16);
    CIAOSR_CHECK_ARG(prec < 0 || prec == d->precision);
    HeadPlan pp;
    HEAD_RUN(scene_route(d->H, d->W, w, d->q_plan, (Prec)d->precision, opt, &pp, r));
    CIAOSR_CHECK_ARG(pp.C == d->C && pp.Cn == d->Cn && pp.D == d->D && pp.Dv == d->Dv && pp.J == d->J);
    CIAOSR_CHECK_ARG(route_code(*r) == d->route);                                  // a route-changing option, other weights
    *p = head_plan(d->H, d->W, w, Q, opt);
    return CIAOSR_OK;
}

extern "C" size_t ciaosr_head_query_workspace_bytes(const ciaosr_head_scene_t* desc, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt) {
    HeadPlan p; HeadRoute r;
    if (scene_open(desc, w, Q, -1, opt, &p, &r) != CIAOSR_OK) return 0;
    return head_split_bytes(p, scene_layout(r)).n[kQuery];
}

// Where head_carve puts chain_flag in the query workspace of this call: the same takes on an arena that starts at address 0
extern "C" int ciaosr_head_query_flag_offset(const ciaosr_head_scene_t* desc, const ciaosr_head_weights_t* w, int Q, const ciaosr_options_t* opt,
                                             size_t* offset) {
    CIAOSR_CHECK_ARG(offset);
    HeadPlan p; HeadRoute r;
    HEAD_RUN(scene_open(desc, w, Q, -1, opt, &p, &r));
    const int step = r.fused ? p.qcf : p.qc;
    const int nq_last = (int)(Q - ((long)(Q - 1) / step) * step);                 // the launch pair whose flag is left behind
    if (!r.fused || r.kv(p, nq_last) != kHeadChain) return CIAOSR_ERR_UNSUPPORTED;
    Arena ws(nullptr, ~(size_t)0);
    Arena* const ar[3] = {nullptr, nullptr, &ws};
    const HeadBuffers b = head_carve_split(p, scene_layout(r), ar);
    *offset = (size_t)reinterpret_cast<uintptr_t>(b.chain_flag);
    return CIAOSR_OK;
}

static int head_query(const void* scene, size_t scene_bytes, const ciaosr_head_scene_t* desc, const ciaosr_head_weights_t* w, const float* x_lr_nchw,
                      const float* coord, const float* cell, int Q, int chunk, float* rgb, const ciaosr_options_t* opt, void* workspace,
                      size_t workspace_bytes, void* stream_, Prec prec) {
    CIAOSR_CHECK_ARG(scene && coord && cell && rgb && workspace);
    HeadPlan p; HeadRoute r;
    HEAD_RUN(scene_open(desc, w, Q, (int)prec, opt, &p, &r));
    const SceneLayout lay = scene_layout(r);
    const SplitBytes need = head_split_bytes(p, lay);
    CIAOSR_CHECK_ARG((int)(need.n[kScene] >> 8) == desc->total);
    if (scene_bytes < need.n[kScene] || workspace_bytes < need.n[kQuery]) return CIAOSR_ERR_WORKSPACE;
    Arena sc(const_cast<void*>(scene), scene_bytes), ws(workspace, workspace_bytes);
    Arena* const ar[3] = {&sc, nullptr, &ws};
    const HeadCall c = {head_carve_split(p, lay, ar), r, prec, nullptr, w, nullptr, x_lr_nchw, coord, cell, chunk, rgb, opt, (hipStream_t)stream_};
    if (!sc.ok || !ws.ok) return CIAOSR_ERR_WORKSPACE;
    CIAOSR_CHECK_ARG(off256(c.U, scene) == desc->off_u && off256(c.Tk, scene) == desc->off_tk && off256(c.Tv, scene) == desc->off_tv &&
                     (lay.logit ? off256(c.G, scene) : -1) == desc->off_g);
    return c.per_query(Q);
}

#define CIAOSR_HEAD_SCENE_ENTRIES(sfx, prec)                                                                                                          \
    extern "C" int ciaosr_head_prepare_##sfx(const float* feat_hwc, int H, int W, const ciaosr_head_weights_t* w, const ciaosr_csattn_weights_t* csattn, \
                                             int q_plan, const ciaosr_options_t* opt, void* scene, size_t scene_bytes, ciaosr_head_scene_t* desc,   \
                                             void* workspace, size_t workspace_bytes, void* stream) {                                                \
        return head_prepare(feat_hwc, H, W, w, csattn, q_plan, opt, scene, scene_bytes, desc, workspace, workspace_bytes, stream, prec);            \
    }                                                                                                                                                 \
    extern "C" int ciaosr_head_query_##sfx(const void* scene, size_t scene_bytes, const ciaosr_head_scene_t* desc, const ciaosr_head_weights_t* w,   \
                                           const float* x_lr_nchw, const float* coord, const float* cell, int Q, int chunk, float* rgb,             \
                                           const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream) {                    \
        return head_query(scene, scene_bytes, desc, w, x_lr_nchw, coord, cell, Q, chunk, rgb, opt, workspace, workspace_bytes, stream, prec);       \
    }
CIAOSR_HEAD_SCENE_ENTRIES(f32, kF32)
CIAOSR_HEAD_SCENE_ENTRIES(bf16, kBF16)
CIAOSR_HEAD_SCENE_ENTRIES(f16, kF16)
#undef CIAOSR_HEAD_SCENE_ENTRIES

// ---- staged MLPRefiner (mlp_refiner.py:87-102), layer by layer, no hoist -------------------------------------
static int mlp_wmax(const ciaosr_mlp_t* m) {
    int w = 0;
    for (int i = 0; i + 1 < m->n_layers; ++i) w = m->width[i] > w ? m->width[i] : w;
    return (w + 3) & ~3;
}

extern "C" size_t ciaosr_mlp_workspace_bytes(const ciaosr_mlp_t* m, int rows) {
    if (!m || rows <= 0 || m->n_layers < 1 || m->n_layers > CIAOSR_MAX_LAYERS) return 0;
    return 2 * ((size_t)rows * mlp_wmax(m) * sizeof(float) + 256);
}

extern "C" int ciaosr_mlp_forward_f32(const float* x, int ld_x, const ciaosr_mlp_t* m, int n_run, int rows, float* out,
                                      int ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(x && m && out && rows > 0 && mlp_ok(*m) && ld_x >= m->in_dim);
    CIAOSR_CHECK_ARG(n_run >= 0 && n_run <= m->n_layers);
    const int n = n_run ? n_run : m->n_layers;
    if (workspace_bytes < ciaosr_mlp_workspace_bytes(m, rows)) return CIAOSR_ERR_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const int wmax = mlp_wmax(m);
    float* pp[2] = {ar.take<float>((size_t)rows * wmax), ar.take<float>((size_t)rows * wmax)};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    const float* cur = x;
    int ld_cur = ld_x, k_cur = m->in_dim;
    // Not mlp_layers_f32: these hidden rows have one stride (wmax) and the last layer RUN writes `out`, activated unless it is the MLP's last
    for (int i = 0; i < n; ++i) {
        const bool last = i + 1 == n;
        float* dst = last ? out : pp[i & 1];
        const int ldd = last ? ld_out : wmax;
        int rc = gemm_f32(cur, ld_cur, m->weight[i], m->ld[i], false, dst, ldd, m->bias[i], rows, m->width[i], k_cur, 1.f,
                          i + 1 == m->n_layers ? CIAOSR_ACT_NONE : mlp_act(*m), 0.f, (hipStream_t)stream, "mlp_layer");
        if (rc != CIAOSR_OK) return rc;
        cur = dst; ld_cur = ldd; k_cur = m->width[i];
    }
    return CIAOSR_OK;
}

// ---- staged MLP with 16-bit operands (SURVEY 8(b-2) "ciaosr_mlp5_bf16"): every Linear on the 16-bit MFMA GEMM, activations 16-bit between layers,
// fp32 accumulation, biases and the last layer's output fp32.  ReLU MLPs only (what the 16-bit modes are defined for).
static size_t round8(size_t v) { return (v + 7) & ~(size_t)7; }
// Row lengths in 16-bit elements, each padded to a multiple of 8: x (k0), the widest layer output (wmax: an activation row, and the rows
// of the widest weight matrix) and the widest contraction (kmax: a weight row)
struct Mlp16Sizes { size_t k0, wmax, kmax; };
static Mlp16Sizes mlp16_sizes(const ciaosr_mlp_t* m) {
    Mlp16Sizes z = {round8((size_t)m->in_dim), 0, round8((size_t)m->in_dim)};
    for (int i = 0; i < m->n_layers; ++i) {
        z.wmax = std::max(z.wmax, round8((size_t)m->width[i]));
        if (i + 1 < m->n_layers) z.kmax = std::max(z.kmax, round8((size_t)m->width[i]));
    }
    return z;
}
extern "C" size_t ciaosr_mlp_workspace_bytes_16(const ciaosr_mlp_t* m, int rows) {
    if (!m || rows <= 0 || !mlp_ok(*m)) return 0;
    const Mlp16Sizes z = mlp16_sizes(m);
    // x as 16 bits, two ping-pong activation buffers, one layer's weights as 16 bits; 256 B of slack per buffer for alignment
    return ((size_t)rows * z.k0 + 2 * (size_t)rows * z.wmax + z.wmax * z.kmax) * 2 + 4 * 256;
}

template <typename CastFn, typename LinFn>
static int mlp_forward_16(CastFn cast_rows, LinFn linear, const float* x, int ld_x, const ciaosr_mlp_t* m, int rows, float* out, int ld_out,
                          void* workspace, size_t workspace_bytes, hipStream_t s) {
    CIAOSR_CHECK_ARG(x && m && out && rows > 0 && mlp_ok(*m) && ld_x >= m->in_dim && (ld_x & 3) == 0 && (ld_out & 3) == 0);
    CIAOSR_CHECK_ARG(m->n_layers == 1 || mlp_act(*m) == CIAOSR_ACT_RELU);
    // cast_rows converts whole 4-column groups: with in_dim % 4 != 0 the group past in_dim would carry x padding / the next weight row
    // into the contraction (the model's own in_dim is 9C + 4 or 10C + 4 with C % 4 == 0)
    CIAOSR_CHECK_ARG((m->in_dim & 3) == 0);
    for (int i = 0; i < m->n_layers; ++i) CIAOSR_CHECK_ARG((m->width[i] & 3) == 0 || i + 1 == m->n_layers);
    if (workspace_bytes < ciaosr_mlp_workspace_bytes_16(m, rows)) return CIAOSR_ERR_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const Mlp16Sizes z = mlp16_sizes(m);
    const int k0 = (int)z.k0;
    unsigned short* x16 = ar.take<unsigned short>((size_t)rows * z.k0);
    unsigned short* pp[2] = {ar.take<unsigned short>((size_t)rows * z.wmax), ar.take<unsigned short>((size_t)rows * z.wmax)};
    unsigned short* w16 = ar.take<unsigned short>(z.wmax * z.kmax);
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    // cast_rows zeroes the pad columns [cols, ld_dst): K is padded to a multiple of 8 on both operands
    int rc = cast_rows(x, ld_x, x16, k0, (long)rows, (m->in_dim + 3) & ~3, s);
    if (rc != CIAOSR_OK) return rc;
    const unsigned short* cur = x16;
    int ld_cur = k0, k_cur = k0, k_real = m->in_dim;
    for (int i = 0; i < m->n_layers; ++i) {
        const bool last = i + 1 == m->n_layers;
        const int N = m->width[i];
        rc = cast_rows(m->weight[i], m->ld[i], w16, k_cur, (long)N, (k_real + 3) & ~3, s);
        if (rc != CIAOSR_OK) return rc;
        if (last) {
            // an output width that is no multiple of 4 (imnet_q: 3) goes through a padded scratch row in the free ping-pong buffer
            if ((N & 3) == 0) rc = linear(cur, ld_cur, w16, k_cur, m->bias[i], false, out, ld_out, false, rows, N, k_cur, s, "mlp_layer_16");
            else return CIAOSR_ERR_UNSUPPORTED;
        } else {
            const int ldn = (int)round8((size_t)N);
            unsigned short* dst = pp[i & 1];
            if (ldn != N && hipMemsetAsync(dst, 0, (size_t)rows * ldn * 2, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
            rc = linear(cur, ld_cur, w16, k_cur, m->bias[i], true, dst, ldn, true, rows, N, k_cur, s, "mlp_layer_16");
            cur = dst; ld_cur = ldn; k_cur = ldn; k_real = N;
        }
        if (rc != CIAOSR_OK) return rc;
    }
    return CIAOSR_OK;
}

extern "C" int ciaosr_mlp_forward_bf16(const float* x, int ld_x, const ciaosr_mlp_t* m, int rows, float* out, int ld_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return mlp_forward_16(b16::cast_rows_h16, b16::linear_h16, x, ld_x, m, rows, out, ld_out, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int ciaosr_mlp_forward_f16(const float* x, int ld_x, const ciaosr_mlp_t* m, int rows, float* out, int ld_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return mlp_forward_16(f16::cast_rows_h16, f16::linear_h16, x, ld_x, m, rows, out, ld_out, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- weight stream of the weights-stationary 16-bit head (head_chain_h16.hip) ---------------------------------------------------------
static bool chain_weights_ok(const ciaosr_head_weights_t* w) {
    if (!w || !mlp_ok(w->k) || !mlp_ok(w->v)) return false;
    return b16::head_chain_ok(w);
}

extern "C" size_t ciaosr_head_chain_bytes(const ciaosr_head_weights_t* w, int pairs) {
    if (!chain_weights_ok(w)) return 0;
    return b16::head_chain_bytes(w, pairs ? 1 : 0);
}

extern "C" int ciaosr_pack_head_chain_bf16(const ciaosr_head_weights_t* w, int pairs, void* out, void* stream) {
    CIAOSR_CHECK_ARG(out && (pairs == 0 || pairs == 1));
    if (!chain_weights_ok(w)) return CIAOSR_ERR_UNSUPPORTED;
    return b16::pack_head_chain(w, pairs, out, (hipStream_t)stream);
}

extern "C" int ciaosr_pack_head_chain_f16(const ciaosr_head_weights_t* w, int pairs, void* out, void* stream) {
    CIAOSR_CHECK_ARG(out && (pairs == 0 || pairs == 1));
    if (!chain_weights_ok(w)) return CIAOSR_ERR_UNSUPPORTED;
    return f16::pack_head_chain(w, pairs, out, (hipStream_t)stream);
}
