// SwinIR trunk with the four linears of every Swin block on the f16 MFMA, B equally sized images per call
// (ciaosr_swinir_forward_batch_f16; opt-in above the ABI through ciaosr_options_t.swin_h16).  IEEE half only: built with CIAOSR_F16=1.
//
// Token map [B * Hp * Wp][ld], ld = C rounded up to 64: the fp32 trunk's layout (swinir.hip) with the B images stacked along the rows.
// The residual stream T stays fp32.  Per Swin block FIVE launches over all B images (the fp32 trunk: seven per image):
//   swin_qkv_f16           LayerNorm-1 in the A staging (fp32 statistics, layernorm_kernel's formula; rounded to half on the way to LDS),
//                          f16 weights [3C][ld] (q scale folded in), + bias -> QKV fp32
//   swin_window_attention  the fp32 kernel's device code (swin_window.h: exact-fp32 MFMA, bias, mask, row softmax) on a grid of
//                          B x windows x heads; the mask is indexed by the window within its image; output as half = proj's A operand
//   swin_proj_f16          f16 A, f16 weights, + bias + fp32 residual, in place in T
//   swin_fc1_f16           LayerNorm-2 in the A staging, + bias, exact GELU (erf, CIAOSR_ACT_GELU) -> hidden activations as half [rows][ldh]
//   swin_fc2_f16           f16 A, + bias + fp32 residual, in place in T
// conv_first, the PatchEmbed norm, the group 3x3 convolutions, the final norm, conv_after_body and the crop are the fp32 trunk's kernels:
// the two norms in one launch over all rows, the convolutions per image (their routes and split decisions see one image: each image is
// bitwise its B = 1 result).
//
// The GEMM: one workgroup (4 waves, 2 x 2) per 64 x 128 output tile, two workgroups per CU.  K <= 192 (ld of C = 180) is staged whole:
// A [64][K] and W [128][K] as half in LDS (row pitch 2 K + 16 B: the 32 rows of a ds_read_b128 land on distinct bank quads), then
// K / 16 steps of one A and two W fragments for two v_mfma_f32_32x32x16_f16 per wave; deeper K (fc2: 384) runs in chunks of 192 through
// the same buffers.  Every output element is ONE dot product over K in a fixed order and the tile shape is a constant, so nothing
// depends on the number of rows: image b of a batch is bitwise the B = 1 call on that image (the plan_rows convention of ops.h holds
// trivially).  Rows and row offsets are 64-bit in these kernels; the per-image fp32 stages keep their 32-bit buffer offsets.
// Offsets past 32 bits: REFUSED -- a batch of more than 2^30 tokens is CIAOSR_ERR_BAD_ARG (no sub-batching).
//
// Pad columns: [C, ld) of the half attention output and [hid, ldh) of the half hidden activations are zeroed once per call and never
// written (the epilogues stop at N); the LayerNorm staging writes zeros into LDS for [C, ld).
//
// Driver (the shape of encoder.hip / csattn.hip): one plan, one carve list walked by the byte-count export and by the call, a route
// function that launches nothing and does every refusal, one function per stage.  The plan, the refusals both trunks share and the
// stages outside the blocks (swin_embed, swin_conv3x3_image, swin_tail) are the fp32 trunk's (swin_window.h, swinir.hip).
#include "h16_util.h"
#include "ops.h"
#include "swin_window.h"

#if !CIAOSR_F16
#error "swinir_h16.hip is the IEEE-half trunk: compile with -DCIAOSR_F16=1"
#endif

namespace ciaosr {

namespace CIAOSR_H16_NS {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LBM = 64, LBN = 128;                       // workgroup tile
constexpr int LKC = 192;                                 // K staged per pass
constexpr int LPITCH = LKC * 2 + 16;                     // LDS row pitch in bytes
constexpr size_t kLinLds = (size_t)(LBM + LBN) * LPITCH; // 76 800 B: two workgroups per CU

enum { kEpiF32 = 0, kEpiRes = 1, kEpiGelu16 = 2 };

struct SwinLinP {
    const float* X; int ldx, C;            // LN kernels: A = LayerNorm(X[:, :C]) * g + b, pad columns [C, K) zero
    const float* g; const float* b;
    const unsigned short* A16; int lda;    // other kernels: A as half [M][lda]
    const unsigned short* W; int ldw;      // [N][ldw] half
    const float* bias;                     // [N]
    float* out; int ldo;                   // kEpiF32: destination; kEpiRes: residual and destination (in place)
    unsigned short* out16; int ldo16;      // kEpiGelu16
    long M; int N, K, tiles_n;
};

template <bool LN, int EPI>
__global__ __launch_bounds__(256, 2) void swin_linear_f16_kernel(SwinLinP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_lin[];      // A [LBM][LPITCH], W [LBN][LPITCH]
    unsigned char* la = lds_lin;
    unsigned char* lw = lds_lin + LBM * LPITCH;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
    const long rt = blockIdx.x / p.tiles_n;
    const int ntile = (int)(blockIdx.x - rt * p.tiles_n);
    const long m0 = rt * LBM;
    const int n0 = ntile * LBN;
    const int wm = w >> 1, wn = w & 1;
    f32x16 acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += LKC) {
        const int kc = p.K - k0 < LKC ? p.K - k0 : LKC;                          // a multiple of 64
        const int cpr = kc >> 3;                                                  // 16-byte chunks per row
        if (k0) __syncthreads();                                                  // everyone is done reading the previous chunk
        for (int c = t; c < LBN * cpr; c += 256) {
            const int r = c / cpr, k8 = c - r * cpr;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (n0 + r < p.N) v = *reinterpret_cast<const uint4*>(p.W + (size_t)(n0 + r) * p.ldw + k0 + k8 * 8);
            *reinterpret_cast<uint4*>(lw + r * LPITCH + k8 * 16) = v;
        }
        if constexpr (LN) {
            // wave w normalises rows 16 w .. 16 w + 15 of the tile, four at a time (eight loads in flight per lane); a lane holds
            // columns 4 lane .. + 3 and 256 + 4 lane .. + 3 of the token (C <= 512), exactly as layernorm_kernel does
            const int n4 = p.C >> 2;
            const float4* g4 = reinterpret_cast<const float4*>(p.g);
            const float4* b4 = reinterpret_cast<const float4*>(p.b);
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 ga = lane < n4 ? g4[lane] : z4, ba = lane < n4 ? b4[lane] : z4;
            const float4 gb = lane + 64 < n4 ? g4[lane + 64] : z4, bb = lane + 64 < n4 ? b4[lane + 64] : z4;
            for (int r4 = 0; r4 < 16; r4 += 4) {
                float4 v[4], v2[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long row = m0 + 16 * w + r4 + j;
                    const float4* x = reinterpret_cast<const float4*>(p.X + (size_t)(row < p.M ? row : 0) * p.ldx);
                    v[j] = (row < p.M && lane < n4) ? x[lane] : z4;
                    v2[j] = (row < p.M && lane + 64 < n4) ? x[lane + 64] : z4;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 a = v[j], c2 = v2[j];
                    const float mean = wsum64((a.x + a.y) + (a.z + a.w) + (c2.x + c2.y) + (c2.z + c2.w)) / (float)p.C;
                    float sq = 0.f;
                    if (lane < n4) sq += (a.x - mean) * (a.x - mean) + (a.y - mean) * (a.y - mean) + (a.z - mean) * (a.z - mean) + (a.w - mean) * (a.w - mean);
                    if (lane + 64 < n4) sq += (c2.x - mean) * (c2.x - mean) + (c2.y - mean) * (c2.y - mean) + (c2.z - mean) * (c2.z - mean) + (c2.w - mean) * (c2.w - mean);
                    const float rstd = 1.0f / sqrtf(wsum64(sq) / (float)p.C + 1e-5f);
                    unsigned char* dst = la + (16 * w + r4 + j) * LPITCH;
                    const int ca = 4 * lane - k0, cb = 4 * (lane + 64) - k0;      // column within the staged chunk
                    if (ca >= 0 && ca < kc) {
                        uint2 o = make_uint2(0u, 0u);
                        if (lane < n4)
                            o = pack_h16x4<true>((a.x - mean) * rstd * ga.x + ba.x, (a.y - mean) * rstd * ga.y + ba.y,
                                                 (a.z - mean) * rstd * ga.z + ba.z, (a.w - mean) * rstd * ga.w + ba.w);
                        *reinterpret_cast<uint2*>(dst + ca * 2) = o;
                    }
                    if (cb >= 0 && cb < kc) {
                        uint2 o = make_uint2(0u, 0u);
                        if (lane + 64 < n4)
                            o = pack_h16x4<true>((c2.x - mean) * rstd * gb.x + bb.x, (c2.y - mean) * rstd * gb.y + bb.y,
                                                 (c2.z - mean) * rstd * gb.z + bb.z, (c2.w - mean) * rstd * gb.w + bb.w);
                        *reinterpret_cast<uint2*>(dst + cb * 2) = o;
                    }
                }
            }
        } else {
            for (int c = t; c < LBM * cpr; c += 256) {
                const int r = c / cpr, k8 = c - r * cpr;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (m0 + r < p.M) v = *reinterpret_cast<const uint4*>(p.A16 + (size_t)(m0 + r) * p.lda + k0 + k8 * 8);
                *reinterpret_cast<uint4*>(la + r * LPITCH + k8 * 16) = v;
            }
        }
        __syncthreads();
        // fragment ks of lane (li, lh): row li of the operand, k = 16 ks + 8 lh .. + 7.  Swapped operands (W rows first): a lane owns ONE
        // output row and four consecutive columns per accumulator quad
        const unsigned char* ar = la + (32 * wm + li) * LPITCH + lh * 16;
        const unsigned char* wr = lw + (64 * wn + li) * LPITCH + lh * 16;
        const int nks = kc >> 4;
#pragma unroll
        for (int ks = 0; ks < LKC / 16; ++ks) {
            if (ks < nks) {                                                       // uniform
                const uint4 a = *reinterpret_cast<const uint4*>(ar + ks * 32);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const uint4 wf = *reinterpret_cast<const uint4*>(wr + nt * 32 * LPITCH + ks * 32);
                    acc[nt] = mfma_h16<true>(wf, a, acc[nt]);
                }
            }
        }
    }
    const long row = m0 + 32 * wm + li;
    if (row >= p.M) return;
    // accumulator quad q of tile nt: columns n0 + 64 wn + 32 nt + 8 q + 4 lh .. + 3 (N a multiple of 4: whole quads).  Every load of the
    // epilogue first, then the stores
    float4 bq[2][4], rq[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + 64 * wn + 32 * nt + 8 * q + 4 * lh;
            bq[nt][q] = make_float4(0.f, 0.f, 0.f, 0.f);
            rq[nt][q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < p.N) {
                bq[nt][q] = *reinterpret_cast<const float4*>(p.bias + n);
                if constexpr (EPI == kEpiRes) rq[nt][q] = *reinterpret_cast<const float4*>(p.out + (size_t)row * p.ldo + n);
            }
        }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + 64 * wn + 32 * nt + 8 * q + 4 * lh;
            if (n >= p.N) continue;
            const float4 b = bq[nt][q];
            float v0 = acc[nt][4 * q] + b.x, v1 = acc[nt][4 * q + 1] + b.y, v2 = acc[nt][4 * q + 2] + b.z, v3 = acc[nt][4 * q + 3] + b.w;
            if constexpr (EPI == kEpiRes) {
                const float4 r = rq[nt][q];
                v0 += r.x; v1 += r.y; v2 += r.z; v3 += r.w;
            }
            if constexpr (EPI == kEpiGelu16) {
                v0 = 0.5f * v0 * (1.f + erff(v0 * 0.70710678118654752f));
                v1 = 0.5f * v1 * (1.f + erff(v1 * 0.70710678118654752f));
                v2 = 0.5f * v2 * (1.f + erff(v2 * 0.70710678118654752f));
                v3 = 0.5f * v3 * (1.f + erff(v3 * 0.70710678118654752f));
                *reinterpret_cast<uint2*>(p.out16 + (size_t)row * p.ldo16 + n) = pack_h16x4<true>(v0, v1, v2, v3);
            } else {
                *reinterpret_cast<float4*>(p.out + (size_t)row * p.ldo + n) = make_float4(v0, v1, v2, v3);
            }
        }
}

// B images per launch: workgroup = (image, window, head); the image's QKV rows and output rows by 64-bit strides, the mask by the
// window within the image
struct WinAttnBatchP {
    WinAttnP a;
    unsigned short* out16;
    size_t qkv_img, out_img;       // elements per image
    int wg_per_img;
};
__global__ __launch_bounds__(256) void window_attention_f16_kernel(WinAttnBatchP p) {
    const int img = blockIdx.x / p.wg_per_img, r = blockIdx.x - img * p.wg_per_img;
    window_attention_body<unsigned short>(p.a, r / p.a.heads, r % p.a.heads, p.a.qkv + (size_t)img * p.qkv_img, p.out16 + (size_t)img * p.out_img);
}

template <bool LN, int EPI>
static int launch_linear(SwinLinP& p, hipStream_t s, const char* tag) {
    p.tiles_n = ceil_div(p.N, LBN);
    const long wgs = (long)ceil_div(p.M, LBM) * p.tiles_n;
    CIAOSR_BIG_LDS((swin_linear_f16_kernel<LN, EPI>), kLinLds);
    {
        ProfScope prof(tag, s);
        hipLaunchKernelGGL((swin_linear_f16_kernel<LN, EPI>), dim3((unsigned)wgs), dim3(256), kLinLds, s, p);
    }
    return launch_status(tag);
}

// ---- carve list, route (the plan, SwinBufs and the refusals both trunks share: swin_window.h) ---------------------------------------
// THE list of workspace buffers: walked with base == nullptr by the byte count, with the workspace by the call
static size_t swin_carve(const SwinPlan& p, char* base, SwinBufs* b) {
    size_t off = 0;
    auto take = [&](size_t bytes) -> char* {
        off = (off + 255) & ~(size_t)255;
        char* r = base ? base + off : nullptr;
        off += bytes;
        return r;
    };
    SwinBufs t = {};
    t.img4 = (float*)take(p.HW * 4 * sizeof(float));                  // one image at a time
    t.rows36 = (float*)take(p.HW * 36 * sizeof(float));               // one image at a time
    t.x0 = (float*)take(p.rows * p.ld * sizeof(float));               // conv_first of every image: the last residual
    t.T = (float*)take(p.rows * p.ld * sizeof(float));                // group input / output
    t.Y = t.Tn = (float*)take(p.rows * p.ld * sizeof(float));         // residual stream of the group's blocks; final norm
    t.F = (float*)take(p.HW * p.ld * sizeof(float));                  // conv_after_body of one image
    t.QKV = (float*)take(p.rows * p.ldq * sizeof(float));
    t.A16 = (unsigned short*)take(p.rows * p.ld * sizeof(unsigned short));     // attention output
    t.Hb16 = (unsigned short*)take(p.rows * p.ldh * sizeof(unsigned short));   // hidden activations
    t.part_floats = 16 * p.HW * p.ld;                                 // split-K slabs of the per-image 3x3 convolutions
    t.part = (float*)take(t.part_floats * sizeof(float));
    if (b) *b = t;
    return off + 256;
}

// every refusal, nothing enqueued
static int swin_route(const float* x, int B, int H, int W, const ciaosr_swinir_weights_t* w, float* feat, const ciaosr_options_t* opt,
                      void* workspace, size_t workspace_bytes, SwinPlan* plan) {
    CIAOSR_CHECK_ARG(options_ok(opt));
    SWIN_RUN(swin_args_ok(x, B, H, W, w, feat, workspace, plan));
    const SwinPlan& p = *plan;
    CIAOSR_CHECK_ARG(p.rows <= ((size_t)1 << 30));                     // refused, not sub-batched (header)
    CIAOSR_CHECK_ARG(p.HW * (size_t)p.ldq * 4 < 0xFFFFFF00ull);       // one image's QKV under a buffer descriptor
    for (int i = 0; i < w->num_groups * w->depth; ++i) {
        const ciaosr_swin_block_t& b = w->blocks[i];
        CIAOSR_CHECK_ARG(b.qkv_w16 && b.proj_w16 && b.fc1_w16 && b.fc2_w16);
        CIAOSR_CHECK_ARG(aligned16(b.qkv_w16) && aligned16(b.proj_w16) && aligned16(b.fc1_w16) && aligned16(b.fc2_w16));
        CIAOSR_CHECK_ARG(aligned16(b.ln1_w) && aligned16(b.ln1_b) && aligned16(b.ln2_w) && aligned16(b.ln2_b));
        CIAOSR_CHECK_ARG(aligned16(b.qkv_b) && aligned16(b.proj_b) && aligned16(b.fc1_b) && aligned16(b.fc2_b));
    }
    if (workspace_bytes < swin_carve(p, nullptr, nullptr)) return CIAOSR_ERR_WORKSPACE;
    return CIAOSR_OK;
}

// ---- stages (swin_embed, swin_conv3x3_image and swin_tail are the fp32 trunk's: swinir.hip) ------------------------------------------
// the padded maps are zeroed once: their pad columns are never written afterwards
static int zero_pads(const SwinPlan& p, const SwinBufs& b, hipStream_t s) {
    if (hipMemsetAsync(b.x0, 0, p.rows * p.ld * sizeof(float), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if (hipMemsetAsync(b.F, 0, p.HW * p.ld * sizeof(float), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if (hipMemsetAsync(b.A16, 0, p.rows * p.ld * sizeof(unsigned short), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if (hipMemsetAsync(b.Hb16, 0, p.rows * p.ldh * sizeof(unsigned short), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    return CIAOSR_OK;
}

// one Swin block on the residual stream Tn, all images: five launches
static int stage_block(const SwinPlan& p, const SwinBufs& b, const ciaosr_swin_block_t& k, hipStream_t s) {
    SwinLinP q{};
    q.M = (long)p.rows;
    q.X = b.Tn; q.ldx = p.ld; q.C = p.C; q.g = k.ln1_w; q.b = k.ln1_b;
    q.W = k.qkv_w16; q.ldw = p.ld; q.bias = k.qkv_b; q.out = b.QKV; q.ldo = p.ldq; q.N = 3 * p.C; q.K = p.ld;
    SWIN_RUN((launch_linear<true, kEpiF32>(q, s, "swin_qkv_f16")));
    {
        WinAttnBatchP ap;
        ap.a = WinAttnP{b.QKV, p.ldq, (unsigned)(p.HW * (size_t)p.ldq * 4), nullptr, p.ld, k.bias, k.shift ? k.mask : nullptr,
                        p.Hp, p.Wp, p.C, p.heads, p.d, p.ws, k.shift};
        ap.out16 = b.A16; ap.qkv_img = p.HW * (size_t)p.ldq; ap.out_img = p.HW * (size_t)p.ld;
        ap.wg_per_img = (p.Hp / p.ws) * (p.Wp / p.ws) * p.heads;
        {
            ProfScope prof("swin_window_attention", s);
            hipLaunchKernelGGL(window_attention_f16_kernel, dim3((unsigned)ap.wg_per_img * (unsigned)p.B), dim3(256), 0, s, ap);
        }
        SWIN_RUN(launch_status("window_attention_f16"));
    }
    SwinLinP r{};
    r.M = (long)p.rows;
    r.A16 = b.A16; r.lda = p.ld; r.W = k.proj_w16; r.ldw = p.ld; r.bias = k.proj_b; r.out = b.Tn; r.ldo = p.ld; r.N = p.C; r.K = p.ld;
    SWIN_RUN((launch_linear<false, kEpiRes>(r, s, "swin_proj_f16")));
    SwinLinP f{};
    f.M = (long)p.rows;
    f.X = b.Tn; f.ldx = p.ld; f.C = p.C; f.g = k.ln2_w; f.b = k.ln2_b;
    f.W = k.fc1_w16; f.ldw = p.ld; f.bias = k.fc1_b; f.out16 = b.Hb16; f.ldo16 = p.ldh; f.N = p.hid; f.K = p.ld;
    SWIN_RUN((launch_linear<true, kEpiGelu16>(f, s, "swin_fc1_f16")));
    SwinLinP g{};
    g.M = (long)p.rows;
    g.A16 = b.Hb16; g.lda = p.ldh; g.W = k.fc2_w16; g.ldw = p.ldh; g.bias = k.fc2_b; g.out = b.Tn; g.ldo = p.ld; g.N = p.C; g.K = p.ldh;
    return launch_linear<false, kEpiRes>(g, s, "swin_fc2_f16");
}

// one RSTB: blocks on a copy of the group input, then conv3x3 + the group input, in place over it (per image)
static int stage_group(const SwinPlan& p, const SwinBufs& b, const ciaosr_swinir_weights_t* w, int g, hipStream_t s) {
    if (hipMemcpyAsync(b.Tn, b.T, p.rows * p.ld * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    for (int l = 0; l < w->depth; ++l) SWIN_RUN(stage_block(p, b, w->blocks[g * w->depth + l], s));
    for (int i = 0; i < p.B; ++i) {
        const size_t o = (size_t)i * p.HW * p.ld;
        SWIN_RUN(swin_conv3x3_image(p, b, w->group_conv[g], b.Tn + o, b.T + o, b.T + o, s, "swin_group_conv"));
    }
    return CIAOSR_OK;
}

}  // namespace CIAOSR_H16_NS
}  // namespace ciaosr

using namespace ciaosr;
using namespace ciaosr::CIAOSR_H16_NS;

extern "C" size_t ciaosr_swinir_workspace_bytes_batch_f16(int B, int H, int W, const ciaosr_swinir_weights_t* w) {
    SwinPlan p;
    if (!swin_plan(B, H, W, w, &p) || p.C <= 0 || p.hid <= 0 || p.heads <= 0) return 0;
    return swin_carve(p, nullptr, nullptr);
}

extern "C" int ciaosr_swinir_forward_batch_f16(const float* x_bchw, int B, int H, int W, const ciaosr_swinir_weights_t* w, float* feat_bhwc,
                                               const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream_) {
    SwinPlan p;
    SWIN_RUN(swin_route(x_bchw, B, H, W, w, feat_bhwc, opt, workspace, workspace_bytes, &p));
    hipStream_t s = (hipStream_t)stream_;
    SwinBufs b;
    swin_carve(p, (char*)workspace, &b);
    SWIN_RUN(zero_pads(p, b, s));
    SWIN_RUN(swin_embed(p, b, x_bchw, w, s));
    for (int g = 0; g < w->num_groups; ++g) SWIN_RUN(stage_group(p, b, w, g, s));
    return swin_tail(p, b, w, feat_bhwc, s);
}
