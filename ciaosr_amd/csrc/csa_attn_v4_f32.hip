// attn.V of CrossScaleAttention's composed fold + down tail (scale 2, fp32) on FOUR diagonal tap blocks instead of 16 offsets.
//
// The 16C route (csattn.hip, patch_ops.hip "Composed fold + down") computes
//   out[o] = ( b + sum_{d in {-2..1}^2} (P @ V'_d)[o + d] ) / 6,   V'_d[l] = Pc_{R(dy),R(dx)}[l - d]
// with R(-2) = {0}, R(-1) = R(0) = {0,1,2}, R(1) = {1,2}: a [HpWp x L] @ [L x 16C] contraction.  Write A = {1,2}, B = {0}: every R(d) is
// A, B or A + B, and Pc is linear in its tap set, so with g = l - d + 1 (an index of Pc's (Hh+3) x (Wh+3) grid)
//   out[o] = ( b + sum_{beta in {A,B}^2} sum_g Pbeta[o][g] U_beta[g] ) / 6,    U_beta = Pc_{beta_y, beta_x}  (4 of csa_down_partial's 9 blocks)
//   Pbeta[o][g] = sum_{dy in D(beta_y)} sum_{dx in D(beta_x)} P[o + d][g - 1 + d],   D(A) = {-1,0,1}, D(B) = {-2,-1,0}
// (P = 0 outside the query grid and outside the key grid).  K = 4 (Hh+3)(Wh+3) instead of 16 L: 3.8x fewer MACs at a C3 tile
// (36 864 x 64 x 4 x 99 x 100 against 36 864 x 1024 x 9216).  The edge rule of row 0 / column 0 (there the dy = 0 / dx = 0 blocks must
// not see the cropped row -1 of the 2x map) is NOT applied here: the caller subtracts it with three skinny contractions (csattn.hip).
//
// The A operand is generated from the logits S and the row statistics st = (max x log2 e, 1 / sum): P = exp2(x log2 e - m'),
// m' = max log2 e - log2(1 / sum), then the x-stencils per dy on diagonals and the combination over dy:
//   XA = (P[dx=-1] + P[dx=0]) + P[dx=1],  XB = (P[dx=-1] + P[dx=0]) + P[dx=-2]             (the pair is shared)
//   P(A,.) = (X[dy=-1] + X[dy=0]) + X[dy=1],  P(B,.) = (X[dy=-1] + X[dy=0]) + X[dy=-2]
// Every sum is of non-negative probabilities; the operation order depends on (o, g) only.
//
// Work item: one query row oy, QW (= 192, or 96 for csa_attn_tile128) queries of it, one quarter of the padded key rows; the four
// quarters write fixed-order partial outputs part[q][o][0..64) that csa_attn_v4_combine sums.  A step = one padded key row gy and
// SW = 20 padded key columns gx0 .. gx0+19 in two halves of KW = 10, all four blocks (K = 40 per half).  The workgroup is
// wave-specialised (as csa_scores_box_f32_kernel), three roles with one wave of each on every SIMD, one A and one U tile per half in
// LDS, three barriers per step:
//   stagers (waves 0-3)    X: exp2 of the four logit blocks (query row oy+dy) x (key row gy-1+dy), (QW+3) x 23 each with the halos,
//                          into LDS.  Y0, Y1: the next step's logit loads, two blocks each.  These waves spend Y0 and Y1 waiting on
//                          the memory pipeline (72 dword loads of 92-byte row pieces per thread: the probe shows ~4 500 cycles per
//                          half), which is why the loads have waves of their own: nothing else waits with them.
//   diagonals (waves 4-7)  X: U loads of the step.  Y0: U's 40 x 64 tile of half 0; one thread per diagonal o - k of the QW x 10
//                          tile reads its 13 probabilities per dy, forms the four A values of 10 (o, k) and writes them to the
//                          [k][o] A tile 0.  Y1: the same for half 1.
//   consumers (waves 8-11; two for QW = 96)  half 0 of step n during Y1(n) and X(n+1), half 1 during X(n+1) and Y0(n+1): each
//                          tile is rewritten one phase after its last read.  A wave owns 96 x 32 outputs (3 MFMA tiles,
//                          v_mfma_f32_32x32x2f32, 20 k-pairs per half), carries no staging registers and reads its fragments
//                          AV_PF k-pairs ahead.
// The fp32 MFMA and the VALU are the same lanes of a SIMD, so a step costs the sum of the three roles' issue cycles, not
// their maximum; what the split removes is every wait: on the loads, on the LDS round trips of fragments and diagonals, on barriers.
// Key rows are walked as gy = base + (t + oy) mod n, so the four items oy = qy - dy that need the logit block (qy, ly) read it in the
// same step; the XCD-aware remap keeps consecutive query rows on one XCD (its L2 serves the three re-reads).
// The K order of an output (gy walk, gx0 ascending, half, block, k ascending) depends on (oy, quarter) only: both tile widths give
// bitwise the same result.
#include "ops.h"

namespace ciaosr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int AV_KW = 10;                  // padded key columns per half step and block
constexpr int AV_SW = 2 * AV_KW;           // padded key columns per step
constexpr int AV_RS = AV_SW + 3;           // staged logit columns per row (x-halo -3 .. +2 around the step)
constexpr int AV_C = 64;                   // channels (N)
constexpr int AV_NCOL = 4 * AV_KW;         // K per half
constexpr int AV_BT = AV_NCOL * AV_C;      // U tile: [40][64]
constexpr int AV_KP = AV_NCOL / 2;         // k-pairs (MFMA k = 2) per half
constexpr int AV_SA = 14;                  // k-pairs of half 0 the consumers run in Y1 (the others in X)
constexpr int AV_SB = 8;                   // k-pairs of half 1 the consumers run in X (the others in Y0)
constexpr int AV_PF = 4;                   // k-pairs of fragments a consumer reads ahead
static_assert(AV_SA % 2 == 0 && AV_SB % 2 == 0 && AV_PF % 2 == 0 && AV_KP % 2 == 0 && AV_SA > 0 && AV_SA + AV_PF <= AV_KP && AV_SB > 0 &&
              AV_SB < AV_KP, "k-pair groups; half 1 is not read before the barrier that completes it");

template <int QW>
struct AvCfg {
    static constexpr int NP = 256;                             // threads of the staging role and of the diagonal role (4 waves each)
    static constexpr int NT = 2 * NP + 64 * (QW / 48);         // and 4 or 2 consumer waves of 96 x 32
    static constexpr int TR = NP / AV_RS;                      // staging: threads per column of the logit block (11)
    static constexpr int NI = (QW + 3 + TR - 1) / TR;         // staged rows per thread and block (18 or 9)
    static constexpr int NRB = TR * NI;                        // rows per staged block (>= QW + 3)
    static constexpr int PST = 4 * NRB * AV_RS;                // staged probabilities
    static constexpr int AT = AV_NCOL * QW;                    // A tile [40][QW]
    static constexpr size_t LDS = (size_t)(2 * AV_BT + PST + 2 * AT) * sizeof(float);
};
static_assert(AvCfg<192>::LDS <= 163840 && AvCfg<96>::LDS <= 163840, "LDS");
static_assert(AvCfg<192>::NP >= 192 + AV_KW - 1 && AvCfg<96>::NP >= 96 + AV_KW - 1, "one thread per diagonal");
static_assert(AvCfg<192>::NRB >= 192 + 3 && AvCfg<96>::NRB >= 96 + 3, "staged rows");
// the diagonal reads of rows -(KW-1) .. QW + KW + 1 of a block stay inside the allocation: U tiles before, A tiles after the staged blocks
static_assert(2 * AV_BT >= (AV_KW - 1) * AV_RS && 2 * AvCfg<96>::AT >= (AV_KW + 2) * AV_RS + AV_RS, "diagonal read guard");

#ifdef CIAOSR_PROBE      // developer probe build (make probe; tools/csattn_v4_probe.py): cycle sums of the last <192> launch's workgroups
__device__ unsigned long long g_avprobe[1024 * 48];
#define AVPROBE_T() __builtin_readcyclecounter()
#else
#define AVPROBE_T() 0ull
#endif

struct CsaAv4P {
    const float* S; const float2* st; const float* Pc; float* part;
    int Hp, Wp, Hh, Wh, Lld, nseg, nch, n_wg;
    int ys, oy0, noy;          // S holds the logit rows ys .. (s_bytes worth) of the map; the launch's items are the query rows oy0 .. oy0 + noy - 1
    unsigned s_bytes, pc_bytes;
};

// s_barrier that no memory access is moved across by the compiler, without the waits of a fence: for the consumer waves, whose reads
// in flight at such a barrier are of tiles that stay unwritten through the next phase
__device__ __forceinline__ void av_phase_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int QW>
__global__ __launch_bounds__(AvCfg<QW>::NT) void csa_attn_v4_kernel(CsaAv4P p) {
    using Cfg = AvCfg<QW>;
    constexpr int NP = Cfg::NP, TR = Cfg::TR, NI = Cfg::NI, NRB = Cfg::NRB;
    constexpr int NB = (AV_BT / 4 + NP - 1) / NP;              // float4 of a U tile per producer thread (3, the last one partial)
    extern __shared__ __attribute__((aligned(16))) float avs[];
    float* Bt = avs;                                            // [2][40][64]
    float* Pst = avs + 2 * AV_BT;
    float* At = Pst + Cfg::PST;                                 // [2][40][QW]

    // XCD-aware bijective remap (as gemm_big_softmax_f32_kernel): an XCD walks a contiguous run of items, consecutive query rows
    const int bid = blockIdx.x;
    const int q8 = p.n_wg >> 3, r8 = p.n_wg & 7;
    const int xcd = bid & 7, slot0 = bid >> 3;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot0;
    const int oy = p.oy0 + lid % p.noy, rest = lid / p.noy;     // the global query row: the key-row walk below does not depend on the band
    const int seg = rest % p.nseg, quarter = rest / p.nseg;
    const int x0 = seg * QW, nq = min(QW, p.Wp - x0);
    const int ngy = p.Hh + 3, gyb = quarter * ngy / 4, nr = (quarter + 1) * ngy / 4 - gyb;
    const int HWp = p.Hp * p.Wp;
    const int nsteps = nr * p.nch;

    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
#ifdef CIAOSR_PROBE
    const bool stamp = QW == 192 && lane == 0 && (w & 3) == 0 && bid < 1024;
    unsigned long long pacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long pstart = AVPROBE_T();
#define AVPROBE_ADD(slot, t0) do { const unsigned long long now_ = AVPROBE_T(); pacc[slot] += now_ - (t0); (t0) = now_; } while (0)
#define AVPROBE_OUT(role) do { if (stamp) { for (int i_ = 0; i_ < 10; ++i_) g_avprobe[bid * 48 + 16 * (role) + i_] = pacc[i_];                \
        g_avprobe[bid * 48 + 16 * (role) + 14] = AVPROBE_T() - pstart; g_avprobe[bid * 48 + 16 * (role) + 15] = (unsigned long long)nsteps; } } while (0)
#else
#define AVPROBE_ADD(slot, t0) do { } while (0)
#define AVPROBE_OUT(role) do { } while (0)
#endif

    int trow = 0, ch = 0;
    int gy = gyb + oy % nr, gx0 = 0;
    auto next_step = [&]() __attribute__((always_inline)) {
        if (++ch == p.nch) { ch = 0; ++trow; }
        gy = gyb + (trow + oy) % nr; gx0 = ch * AV_SW;
    };

    if (w < NP / 64) {
        // ================= stagers: logits -> probabilities in LDS =================
        const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.S), 0, p.s_bytes, 0x00020000);
        // staging coordinates: column j of the block, rows r0 + TR i.  Query pixel (oy + dy, x0 + r - 2), key (gy - 1 + dy, gx0 - 3 + j).
        const bool stager = t < TR * AV_RS;
        const int sj = t % AV_RS, sr0 = t / AV_RS;
        float negm[4][NI];                                      // -m' per staged element; -inf outside the query grid (P = 0)
#pragma unroll
        for (int dyi = 0; dyi < 4; ++dyi) {
            const int qy = oy + dyi - 2;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int qx = x0 + sr0 + TR * i - 2;
                float v = -__builtin_inff();
                if (stager && qy >= 0 && qy < p.Hp && qx >= 0 && qx < p.Wp) {
                    const float2 s2 = p.st[(size_t)qy * p.Wp + qx];
                    v = -(s2.x - __builtin_amdgcn_logf(s2.y));    // exp2(x l2e - mx) / sum = exp2(x l2e - (mx - log2(1 / sum)))
                }
                negm[dyi][i] = v;
            }
        }
        const int s_thread = sr0 * p.Lld + sj;                  // element offset of (r0, j) relative to the block's (r = 0, j = 0)
        const int s_istep = TR * p.Lld;
        float ra[4][NI];
        auto issue_logits = [&](auto dy0_c) __attribute__((always_inline)) {
            constexpr int DY0 = decltype(dy0_c)::value;
#pragma unroll
            for (int dyi = DY0; dyi < DY0 + 2; ++dyi) {
                const int dy = dyi - 2;
                // may be negative (rows above the grid or the band, x-halo left of column 0): as unsigned it is past s_bytes (< 2 GiB) and
                // reads 0.  A band holds every row of the map among oy - 2 .. oy + 1; the others have P = 0 (negm = -inf) whatever is read
                const int base = ((oy + dy - p.ys) * p.Wp + x0 - 2) * p.Lld + (gy - 1 + dy) * p.Wh + gx0 - 3 + s_thread;
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    ra[dyi][i] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_s, (base + i * s_istep) * 4, 0, 0));
            }
        };
        // probabilities into the staged blocks.  EDGE: some key of the step lies outside the key grid (its logit may be anything, the
        // pad columns of S included): those elements are replaced by 0.
        auto stage = [&](auto edge_c) __attribute__((always_inline)) {
            constexpr bool EDGE = decltype(edge_c)::value;
            constexpr float kL2e = 1.4426950408889634f;
            const bool kx = (unsigned)(gx0 - 3 + sj) < (unsigned)p.Wh;
#pragma unroll
            for (int dyi = 0; dyi < 4; ++dyi) {
                const bool ok = kx && (unsigned)(gy - 3 + dyi) < (unsigned)p.Hh;
                float* dst = Pst + dyi * NRB * AV_RS + sr0 * AV_RS + sj;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    float v = __builtin_amdgcn_exp2f(__builtin_fmaf(ra[dyi][i], kL2e, negm[dyi][i]));
                    if (EDGE) v = ok ? v : 0.f;
                    if (stager) dst[i * TR * AV_RS] = v;
                }
                __builtin_amdgcn_sched_barrier(0);              // block by block: each waits only for its own loads, the later ones still land
            }
        };
        issue_logits(std::integral_constant<int, 0>{});
        issue_logits(std::integral_constant<int, 2>{});
        [[maybe_unused]] unsigned long long pt0 = AVPROBE_T();
#pragma unroll 1
        for (int step = 0; step < nsteps; ++step) {
            // ---- X ----
            const bool edge = gy < 3 || gy >= p.Hh || gx0 < 3 || gx0 + AV_SW - 1 >= p.Wh;
            if (edge) stage(std::true_type{});
            else stage(std::false_type{});
            AVPROBE_ADD(0, pt0);
            __syncthreads();
            AVPROBE_ADD(1, pt0);
            // ---- Y0, Y1 ----  the next step's logits: the wave waits here on the memory pipeline, beside the diagonal waves' work
            next_step();
            const bool more = step + 1 < nsteps;
            if (more) issue_logits(std::integral_constant<int, 0>{});
            AVPROBE_ADD(2, pt0);
            __syncthreads();
            AVPROBE_ADD(3, pt0);
            if (more) issue_logits(std::integral_constant<int, 2>{});
            AVPROBE_ADD(4, pt0);
            __syncthreads();
            AVPROBE_ADD(5, pt0);
        }
        AVPROBE_OUT(0);
        return;
    }

    if (w < 2 * NP / 64) {
        // ================= diagonal waves: probabilities -> A tiles, U tiles =================
        const int td = t - NP;
        const __amdgpu_buffer_rsrc_t rs_pc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Pc), 0, p.pc_bytes, 0x00020000);
        // U tiles: float4 s of the thread = (kk = idx / 16, c4 = idx % 16); kk = block * KW + k, half h at key column gx0 + KW h + k
        int b_rel[NB], b_k[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int idx = td + NP * s, kk = idx >> 4, c4 = idx & 15;
            const int blk = kk / AV_KW, k = kk - blk * AV_KW;
            const int pcb = blk == 0 ? 8 : blk == 1 ? 6 : blk == 2 ? 2 : 0;     // (A,A) (A,B) (B,A) (B,B): 3 r + s with {0} = 0, {1,2} = 2
            b_rel[s] = k * 9 * AV_C + pcb * AV_C + 4 * c4;
            b_k[s] = idx < AV_BT / 4 ? k : 0x40000000;          // past the tile: never in range, never written
        }
        float4 rb[2][NB];
        auto issue_u = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int brow = (gy * (p.Wh + 3) + gx0 + AV_KW * h) * 9 * AV_C;
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    const unsigned off = gx0 + AV_KW * h + b_k[s] < p.Wh + 3 ? (unsigned)(brow + b_rel[s]) * 4u : 0x80000000u;
                    const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_pc, off, 0, 0);
                    rb[h][s] = make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
                }
            }
        };
        // diagonal of this thread in either half: outputs (o = c + k, k), k = 0 .. KW-1, 0 <= o < nq
        const int c = td - (AV_KW - 1);
        const bool diag = td < QW + AV_KW - 1;
        const float* dsrc = Pst + c * AV_RS;                    // half h: row c + j, column KW h + j: + KW h + j (RS + 1)
        float* adst0 = At + c;                                  // A[h][kk][o]: + h AT + kk QW + k
        auto half = [&](auto h_c) __attribute__((always_inline)) {
            constexpr int H = decltype(h_c)::value;
#pragma unroll
            for (int s = 0; s < NB; ++s)
                if (NP * (s + 1) <= AV_BT / 4 || td + NP * s < AV_BT / 4)
                    *reinterpret_cast<float4*>(Bt + H * AV_BT + 4 * (td + NP * s)) = rb[H][s];
            if (diag) {
                float* adst = adst0 + H * Cfg::AT;
                float xa2[AV_KW], xb2[AV_KW], ya[AV_KW], yb[AV_KW];
#pragma unroll
                for (int dyi = 0; dyi < 4; ++dyi) {
                    float d[AV_KW + 3];
#pragma unroll
                    for (int j = 0; j < AV_KW + 3; ++j) d[j] = dsrc[dyi * NRB * AV_RS + AV_KW * H + j * (AV_RS + 1)];
#pragma unroll
                    for (int k = 0; k < AV_KW; ++k) {
                        const float pr = d[k + 1] + d[k + 2];
                        const float xa = pr + d[k + 3], xb = pr + d[k];
                        if (dyi == 0) { xa2[k] = xa; xb2[k] = xb; }
                        else if (dyi == 1) { ya[k] = xa; yb[k] = xb; }
                        else if (dyi == 2) {
                            ya[k] = ya[k] + xa; yb[k] = yb[k] + xb;
                            if ((unsigned)(c + k) < (unsigned)nq) {
                                adst[(2 * AV_KW + k) * QW + k] = ya[k] + xa2[k];     // (B, A)
                                adst[(3 * AV_KW + k) * QW + k] = yb[k] + xb2[k];     // (B, B)
                            }
                        } else if ((unsigned)(c + k) < (unsigned)nq) {
                            adst[(0 * AV_KW + k) * QW + k] = ya[k] + xa;              // (A, A)
                            adst[(1 * AV_KW + k) * QW + k] = yb[k] + xb;              // (A, B)
                        }
                    }
                }
            }
        };
        [[maybe_unused]] unsigned long long pt0 = AVPROBE_T();
#pragma unroll 1
        for (int step = 0; step < nsteps; ++step) {
            issue_u();                                          // X: these waves' only work; the tiles are written in Y0 and Y1
            __syncthreads();                                    // X | Y0: the staged blocks of this step are complete
            AVPROBE_ADD(0, pt0);
            half(std::integral_constant<int, 0>{});
            AVPROBE_ADD(1, pt0);
            __syncthreads();
            AVPROBE_ADD(2, pt0);
            half(std::integral_constant<int, 1>{});
            next_step();
            AVPROBE_ADD(3, pt0);
            __syncthreads();
            AVPROBE_ADD(4, pt0);
        }
        AVPROBE_OUT(1);
        return;
    }

    // ================= consumers =================
    const int cw = w - 2 * NP / 64, wm = cw >> 1, wn = cw & 1, li = lane & 31, lh = lane >> 5;
    f32x16 acc[3];
#pragma unroll
    for (int mi = 0; mi < 3; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
    // fragments: lane (li, lh) reads A[h][kk = 2 s + lh][o = wm 96 + mi 32 + li], U[h][kk][wn 32 + li]
    const float* fa = At + lh * QW + wm * 96 + li;
    const float* fb = Bt + lh * AV_C + wn * 32 + li;
    [[maybe_unused]] unsigned long long ct0 = AVPROBE_T();
    // One step: the 2 x 20 k-pairs (entry e = half * 20 + k-pair) with the fragments read AV_PF entries ahead of their MFMAs, in fenced
    // groups of two (the scheduler otherwise sinks every read to just in front of its MFMA and waits for it there).  NBAR barriers on
    // the way: behind entry SA - 1 (Y1 | X: completes half 1, which is first read behind it) and behind entry 20 + SB - 1 (X | Y0).
    auto mma_step = [&](auto nbar_c) __attribute__((always_inline)) {
        constexpr int NBAR = decltype(nbar_c)::value, NE = 2 * AV_KP;
        float a[NE][3], b[NE];
        auto ld = [&](int e) __attribute__((always_inline)) {
            const int h = e / AV_KP, kp = e - h * AV_KP;
            b[e] = fb[h * AV_BT + 2 * kp * AV_C];
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) a[e][mi] = fa[h * Cfg::AT + 2 * kp * QW + mi * 32];
        };
#pragma unroll
        for (int e = 0; e < AV_PF; ++e) ld(e);
#pragma unroll
        for (int e = 0; e < NE; e += 2) {
            if (e + AV_PF < NE) { ld(e + AV_PF); ld(e + AV_PF + 1); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int mi = 0; mi < 3; ++mi)
                    acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e + u][mi], b[e + u], acc[mi], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (NBAR >= 1 && e + 2 == AV_SA) {
                AVPROBE_ADD(0, ct0);
                av_phase_barrier();
                AVPROBE_ADD(1, ct0);
            }
            if (NBAR >= 2 && e + 2 == AV_KP + AV_SB) {
                AVPROBE_ADD(2, ct0);
                av_phase_barrier();
                AVPROBE_ADD(3, ct0);
            }
        }
    };
    if (nsteps > 0) {                                           // X and Y0 of step 0: nothing to consume yet
        av_phase_barrier();
        __syncthreads();
    }
    ct0 = AVPROBE_T();
#pragma unroll 1
    for (int step = 0; step + 1 < nsteps; ++step) {
        mma_step(std::integral_constant<int, 2>{});
        AVPROBE_ADD(4, ct0);
        __syncthreads();                                        // Y0 | Y1: tiles 0 of the next step are complete, tiles 1 are free
        AVPROBE_ADD(5, ct0);
    }
    if (nsteps > 0) mma_step(std::integral_constant<int, 1>{}); // the last step: the producers leave behind their Y1
    AVPROBE_OUT(2);

    // part[quarter][o][col]: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* dst = p.part + ((size_t)quarter * HWp + (size_t)oy * p.Wp + x0) * AV_C + wn * 32 + li;
#pragma unroll
    for (int mi = 0; mi < 3; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 96 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (row < nq) dst[(size_t)row * AV_C] = acc[mi][r];
        }
}
#undef AVPROBE_ADD
#undef AVPROBE_OUT


// V columns of the edge-rule contractions, Ve[l][blk * C + co]: blk 0..3 top (dy = 0, dx = blk - 2, tap rows {0}, columns R(dx)),
// 4..7 left (dy = blk - 6, dx = 0, rows R(dy), columns {0}), 8 corner ({0} x {0})
__device__ __forceinline__ int av_subset(int d) { return d == -2 ? 0 : (d == 1 ? 2 : 1); }   // {0} / {0,1,2} / {1,2}

__global__ void csa_gather_vedge_kernel(const float* __restrict__ Pc, int Hh, int Wh, int C, float* __restrict__ Ve) {
    const int c4n = C >> 2;
    const long n = (long)Hh * Wh * 9 * c4n;
    const int We = Wh + 3;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % c4n);
        const long t = idx / c4n;
        const int blk = (int)(t % 9);
        const int l = (int)(t / 9);
        const int ly = l / Wh, lx = l - ly * Wh;
        int dy, dx, r, sct;
        if (blk < 4) { dy = 0; dx = blk - 2; r = 0; sct = av_subset(dx); }
        else if (blk < 8) { dy = blk - 6; dx = 0; r = av_subset(dy); sct = 0; }
        else { dy = 0; dx = 0; r = 0; sct = 0; }
        const size_t src = ((size_t)(ly - dy + 1) * We + (lx - dx + 1)) * (9 * C) + (size_t)(3 * r + sct) * C + 4 * c4;
        reinterpret_cast<float4*>(Ve)[idx] = *reinterpret_cast<const float4*>(Pc + src);
    }
}

// out[(y,x)][co] = (bd[co] + ((part0 + part1) + part2) + part3 - E) / 6 with the edge-rule terms
//   E = [y == 0] sum_dx Otop[x + dx][dx] + [x == 0] sum_dy Oleft[y + dy][dy] - [y == 0 && x == 0] Otl      (inclusion-exclusion)
__global__ void csa_attn_v4_combine_kernel(const float* __restrict__ part, const float* __restrict__ Otop, const float* __restrict__ Oleft,
                                           const float* __restrict__ Otl, const float* __restrict__ bd, int H, int W, int Hp, int Wp,
                                           int C, float* __restrict__ out, int ld_out) {
    const int c4n = C >> 2;
    const long n = (long)H * W * c4n;
    const size_t qs = (size_t)Hp * Wp * C;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % c4n);
        const long pix = idx / c4n;
        const int x = (int)(pix % W), y = (int)(pix / W);
        const size_t o = ((size_t)y * Wp + x) * C + 4 * c4;
        float4 acc = *reinterpret_cast<const float4*>(part + o);
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(part + q * qs + o);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        if (y == 0 || x == 0) {
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y == 0)
                for (int dx = -2; dx <= 1; ++dx) {
                    if (x + dx < 0 || x + dx >= Wp) continue;
                    const float4 v = *reinterpret_cast<const float4*>(Otop + (size_t)(x + dx) * 4 * C + (size_t)(dx + 2) * C + 4 * c4);
                    e.x += v.x; e.y += v.y; e.z += v.z; e.w += v.w;
                }
            if (x == 0)
                for (int dy = -2; dy <= 1; ++dy) {
                    if (y + dy < 0 || y + dy >= Hp) continue;
                    const float4 v = *reinterpret_cast<const float4*>(Oleft + (size_t)(y + dy) * 4 * C + (size_t)(dy + 2) * C + 4 * c4);
                    e.x += v.x; e.y += v.y; e.z += v.z; e.w += v.w;
                }
            if (y == 0 && x == 0) {
                const float4 v = *reinterpret_cast<const float4*>(Otl + 4 * c4);
                e.x -= v.x; e.y -= v.y; e.z -= v.z; e.w -= v.w;
            }
            acc.x -= e.x; acc.y -= e.y; acc.z -= e.z; acc.w -= e.w;
        }
        const float4 b = *reinterpret_cast<const float4*>(bd + 4 * c4);
        acc.x = (b.x + acc.x) / 6.f; acc.y = (b.y + acc.y) / 6.f; acc.z = (b.z + acc.z) / 6.f; acc.w = (b.w + acc.w) / 6.f;
        *reinterpret_cast<float4*>(out + (size_t)pix * ld_out + 4 * c4) = acc;
    }
}

static inline int av_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// s_rows: the logit rows S holds at a time (Hp, or a band of query rows with its halo)
bool csa_attn_v4_ok(int Hp, int Wp, int C, int Lld, int s_rows) {
    return C == AV_C && Hp >= 4 && Wp >= 4 && (Hp & 1) == 0 && (Wp & 1) == 0 && (Lld & 3) == 0 && s_rows >= 1 &&
           (size_t)s_rows * Wp * Lld * sizeof(float) < 0x80000000ull;     // every offset the kernel forms (negative ones included) is < 2^32
}

// The items of query rows oy0 <= oy < oy1 from S = the logit rows ys .. ys + s_rows - 1 (every row of the map among oy0 - 2 .. oy1);
// stats2 and part are whole-map arrays.  The whole map in one launch: ys = 0, s_rows = Hp, oy0 = 0, oy1 = Hp.
int csa_attn_v4_f32(const float* S, int Lld, const float* stats2, const float* Pc, float* part, int Hp, int Wp, int C, bool tile128,
                    int ys, int s_rows, int oy0, int oy1, hipStream_t s) {
    CIAOSR_CHECK_ARG(S && stats2 && Pc && part && csa_attn_v4_ok(Hp, Wp, C, Lld, s_rows) && aligned16(Pc) && aligned16(part));
    CIAOSR_CHECK_ARG(0 <= oy0 && oy0 < oy1 && oy1 <= Hp && ys >= 0 && ys + s_rows <= Hp && ys <= (oy0 > 2 ? oy0 - 2 : 0) &&
                     ys + s_rows >= (oy1 < Hp ? oy1 + 1 : Hp));
    CsaAv4P p;
    p.S = S; p.st = reinterpret_cast<const float2*>(stats2); p.Pc = Pc; p.part = part;
    p.Hp = Hp; p.Wp = Wp; p.Hh = Hp / 2; p.Wh = Wp / 2; p.Lld = Lld;
    const int qw = tile128 ? 96 : 192;
    p.nseg = ceil_div(Wp, qw);
    p.nch = ceil_div(p.Wh + 3, AV_SW);
    p.ys = ys; p.oy0 = oy0; p.noy = oy1 - oy0;
    p.n_wg = p.noy * p.nseg * 4;
    p.s_bytes = (unsigned)((size_t)s_rows * Wp * Lld * sizeof(float));
    p.pc_bytes = (unsigned)((size_t)(p.Hh + 3) * (p.Wh + 3) * 9 * C * sizeof(float));
    ProfScope prof("csa_attn_v", s);
    if (tile128) {
        CIAOSR_BIG_LDS(csa_attn_v4_kernel<96>, AvCfg<96>::LDS);
        hipLaunchKernelGGL(csa_attn_v4_kernel<96>, dim3(p.n_wg), dim3(AvCfg<96>::NT), AvCfg<96>::LDS, s, p);
    } else {
        CIAOSR_BIG_LDS(csa_attn_v4_kernel<192>, AvCfg<192>::LDS);
        hipLaunchKernelGGL(csa_attn_v4_kernel<192>, dim3(p.n_wg), dim3(AvCfg<192>::NT), AvCfg<192>::LDS, s, p);
    }
    return launch_status("csa_attn_v4_f32");
}

int csa_gather_vedge(const float* Pc, int Hh, int Wh, int C, float* Ve, hipStream_t s) {
    ProfScope prof("csa_gather_vedge", s);
    hipLaunchKernelGGL(csa_gather_vedge_kernel, dim3(av_grid((long)Hh * Wh * 9 * C / 4)), dim3(256), 0, s, Pc, Hh, Wh, C, Ve);
    return launch_status("csa_gather_vedge");
}

int csa_attn_v4_combine(const float* part, const float* Otop, const float* Oleft, const float* Otl, const float* bd, int H, int W, int Hp,
                        int Wp, int C, float* out, int ld_out, hipStream_t s) {
    ProfScope prof("csa_gather_out", s);
    hipLaunchKernelGGL(csa_attn_v4_combine_kernel, dim3(av_grid((long)H * W * C / 4)), dim3(256), 0, s, part, Otop, Oleft, Otl, bd, H, W,
                       Hp, Wp, C, out, ld_out);
    return launch_status("csa_attn_v4_combine");
}

}  // namespace ciaosr

#ifdef CIAOSR_PROBE
extern "C" int ciaosr_debug_probe_av4_read(unsigned long long* host, int n_words) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(ciaosr::g_avprobe), (size_t)n_words * 8) == hipSuccess ? 0 : -1;
}
#endif
