// SwinIR trunk of LocalImplicitSRSWINIR.gen_feature (ciaosr_net.py:475-525 over swinir_net.py: conv_first :710,
// PatchEmbed norm :553-557, RSTB :420-460 = 6 x SwinTransformerBlock :149-258 + conv + residual, final norm :718,
// conv_after_body :777) on channels-last token maps.
//
// Token map T [Hp*Wp][ld] fp32, ld = C rounded up to 64 (180 -> 192), pad columns kept at zero so that every linear
// layer and 3x3 convolution runs through the implicit-GEMM convolution of conv_f32.hip with Cin = ld (weights are
// zero-padded on the host).  Per Swin block: LayerNorm -> qkv (1x1 conv) -> window attention -> proj (+ residual,
// in place) -> LayerNorm -> fc1 (+ exact GELU) -> fc2 (+ residual, in place): 7 launches instead of PyTorch's ~30.
//
// Window attention (swinir_net.py:66-146): one workgroup per (window, head); the cyclic shift (torch.roll :228-231,
// :247-250) is folded into the token index, the relative-position bias arrives pre-gathered per layer
// [heads][N][N] and the shifted-window mask [nW][N][N] (calculate_mask :192-213) per map size, both built once on the
// host.  Everything fp32 (exact-fp32 MFMA for q k^T and P v).
//
// Driver (the shape of encoder.hip / swinir_h16.hip): ciaosr_swinir_forward_f32 is the plan (swin_plan, B = 1), the route (swin_route_f32:
// every refusal, nothing enqueued), the carve list (swin_carve_f32: the only list of buffers, walked by the byte count too) and one
// function per stage.  swin_embed, swin_conv3x3_image and swin_tail are the f16-linear trunk's stages too (swin_window.h).
//   stage          launches in order (profiler tags)                                               scratch: reads -> writes
//   zero_pads      memset pad5, memset Hb (pad columns [C, ld) / [hid, ldh): never written after)  -> x0 | T | Tn | Y | F, Hb
//   swin_embed     per image: image_to_hwc4, enc_patch_first, enc_conv_first;                      x -> img4 -> rows36 -> x0
//                  swin_layernorm over all rows (PatchEmbed norm)                                  x0 -> T
//   group g        copy T -> Tn, then depth x block, then swin_group_conv (+ T, in place)          T -> Tn;  Tn, T -> T (partials in part)
//     block        swin_layernorm, swin_qkv, swin_window_attention, swin_proj (+ Tn, in place),    Tn -> Y -> QKV -> F -> Tn
//                  swin_layernorm, swin_fc1 (GELU), swin_fc2 (+ Tn, in place): seven launches      Tn -> Y -> Hb -> Tn
//   swin_tail      swin_layernorm over all rows (final norm);                                      T -> Y
//                  per image: swin_conv_after_body (+ x0), swin_crop                               Y, x0 -> F -> feat
// A linear is the no-staging small GEMM for maps of <= 16384 tokens, else the implicit-GEMM 1x1 convolution (partials in part); a 3x3
// convolution is the one-launch small-map kernel where the layer has fragments and the map fits, else the split-K convolution.
#include "h16_util.h"
#include "ops.h"
#include "swin_window.h"

namespace ciaosr {

// [3][H][W] -> [Hp*Wp][4], bottom/right reflect padding (F.pad(..., 'reflect'), ciaosr_net.py:509-512), zero 4th channel
__global__ void image_to_hwc4_reflect_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int Hp, int Wp) {
    const long n = (long)Hp * Wp;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int y = (int)(i / Wp), xx = (int)(i - (long)y * Wp);
        if (y >= H) y = 2 * (H - 1) - y;
        if (xx >= W) xx = 2 * (W - 1) - xx;
        const long s = (long)y * W + xx, HW = (long)H * W;
        reinterpret_cast<float4*>(out)[i] = make_float4(x[s], x[HW + s], x[2 * HW + s], 0.f);
    }
}

// LayerNorm over the first C of ld columns of each token (eps 1e-5, biased variance: nn.LayerNorm); pad columns -> 0.
// One wavefront per token, float4 lanes.
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ X, int ldx, float* __restrict__ Y, int ldy,
                                                        const float* __restrict__ g, const float* __restrict__ b, long rows, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* x = reinterpret_cast<const float4*>(X + row * ldx);
    const int n4 = C >> 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < n4) v = x[lane];
    float4 v2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane + 64 < n4) v2 = x[lane + 64];                       // C <= 512
    const float mean = wsum64((v.x + v.y) + (v.z + v.w) + (v2.x + v2.y) + (v2.z + v2.w)) / (float)C;
    float sq = 0.f;
    if (lane < n4) sq += (v.x - mean) * (v.x - mean) + (v.y - mean) * (v.y - mean) + (v.z - mean) * (v.z - mean) + (v.w - mean) * (v.w - mean);
    if (lane + 64 < n4) sq += (v2.x - mean) * (v2.x - mean) + (v2.y - mean) * (v2.y - mean) + (v2.z - mean) * (v2.z - mean) + (v2.w - mean) * (v2.w - mean);
    const float rstd = 1.0f / sqrtf(wsum64(sq) / (float)C + 1e-5f);
    float4* y = reinterpret_cast<float4*>(Y + row * ldy);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    for (int t = lane; t < (ldy >> 2); t += 64) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < n4) {
            const float4 xv = t < 64 ? v : v2, gv = g4[t], bv = b4[t];
            o = make_float4((xv.x - mean) * rstd * gv.x + bv.x, (xv.y - mean) * rstd * gv.y + bv.y,
                            (xv.z - mean) * rstd * gv.z + bv.z, (xv.w - mean) * rstd * gv.w + bv.w);
        }
        y[t] = o;
    }
}

// ---- window attention: swin_window.h (one workgroup per (window, head) of the image) --------------------------------
__global__ __launch_bounds__(256) void window_attention_kernel(WinAttnP p) {
    window_attention_body<float>(p, blockIdx.x / p.heads, blockIdx.x % p.heads, p.qkv, p.out);
}

// F [Hp*Wp][ld] -> feat [H][W][C] (crop of the reflect padding, ciaosr_net.py:523, and repack to C columns)
__global__ void crop_repack_kernel(const float* __restrict__ F, int ld, int Wp, float* __restrict__ out, int H, int W, int C) {
    const int c4n = C >> 2;
    const long n = (long)H * W * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const long pix = i / c4n;
        const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
        reinterpret_cast<float4*>(out)[i] = *reinterpret_cast<const float4*>(F + ((size_t)y * Wp + x) * ld + 4 * c4);
    }
}

// ---- what both trunks run (declared in swin_window.h) ---------------------------------------------------------------------------
int swin_args_ok(const float* x, int B, int H, int W, const ciaosr_swinir_weights_t* w, const float* feat, const void* workspace, SwinPlan* plan) {
    CIAOSR_CHECK_ARG(x && w && feat && workspace && B >= 1 && H > 0 && W > 0);
    const int C = w->embed_dim, heads = w->num_heads, ws = w->window_size, hid = w->hidden;
    CIAOSR_CHECK_ARG(C > 0 && (C & 3) == 0 && heads > 0 && C % heads == 0 && C / heads <= WMAXD && ws > 0 && ws * ws <= WMAXN);
    CIAOSR_CHECK_ARG(((C / heads) & 1) == 0);                        // 8-byte q/k/v loads in the window-attention kernel
    CIAOSR_CHECK_ARG(C <= 512);                                      // a token's values in one wave's registers (LayerNorm)
    CIAOSR_CHECK_ARG(hid > 0 && (hid & 3) == 0 && w->num_groups >= 1 && w->depth >= 1 && w->blocks && w->group_conv);
    CIAOSR_CHECK_ARG(w->pe_norm_w && w->pe_norm_b && w->norm_w && w->norm_b);
    CIAOSR_CHECK_ARG(swin_plan(B, H, W, w, plan));
    const SwinPlan& p = *plan;
    CIAOSR_CHECK_ARG(p.Hp - H < H && p.Wp - W < W);                  // reflect padding needs pad < size
    CIAOSR_CHECK_ARG(conv_ok(w->conv_first, 3, C, 3) && conv_ok(w->conv_after_body, p.ld, C, 3));
    for (int i = 0; i < w->num_groups * w->depth; ++i) {
        const ciaosr_swin_block_t& b = w->blocks[i];
        CIAOSR_CHECK_ARG(b.ln1_w && b.ln1_b && b.qkv_b && b.bias && b.proj_b && b.ln2_w && b.ln2_b && b.fc1_b && b.fc2_b);
        // shift is fixed at construction from the CONFIGURED input_resolution (:170-173), not the map size
        CIAOSR_CHECK_ARG(b.shift == 0 || b.mask);
    }
    for (int g = 0; g < w->num_groups; ++g) CIAOSR_CHECK_ARG(conv_ok(w->group_conv[g], p.ld, C, 3));
    return CIAOSR_OK;
}

int swin_layernorm(const float* X, int ldx, float* Y, int ldy, const float* g, const float* b, long rows, int C, hipStream_t s) {
    CIAOSR_CHECK_ARG(X && Y && g && b && (C & 3) == 0 && C <= 512 && (ldx & 3) == 0 && (ldy & 3) == 0);
    ProfScope prof("swin_layernorm", s);
    hipLaunchKernelGGL(layernorm_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, X, ldx, Y, ldy, g, b, rows, C);
    return launch_status("layernorm");
}

int swin_embed(const SwinPlan& p, const SwinBufs& b, const float* x, const ciaosr_swinir_weights_t* w, hipStream_t s) {
    for (int i = 0; i < p.B; ++i) {
        {
            ProfScope prof("image_to_hwc4", s);
            const int grid = (int)((p.HW + 255) / 256);
            hipLaunchKernelGGL(image_to_hwc4_reflect_kernel, dim3(grid > 2048 ? 2048 : grid), dim3(256), 0, s, x + (size_t)i * 3 * p.H * p.W, b.img4, p.H,
                               p.W, p.Hp, p.Wp);
        }
        SWIN_RUN(launch_status("image_to_hwc4_reflect"));
        SWIN_RUN(patch_rows(b.img4, 4, p.Hp, p.Wp, 4, 3, 1, 1, p.Hp, p.Wp, b.rows36, 36, 0, 0.f, s, "enc_patch_first"));
        SWIN_RUN(gemm_f32(b.rows36, 36, w->conv_first.weight, 36, false, b.x0 + (size_t)i * p.HW * p.ld, p.ld, w->conv_first.bias, (int)p.HW, p.C,
                          36, 1.f, CIAOSR_ACT_NONE, 0.f, s, "enc_conv_first"));
    }
    // PatchEmbed: flatten (free in channels-last) + LayerNorm
    return swin_layernorm(b.x0, p.ld, b.T, p.ld, w->pe_norm_w, w->pe_norm_b, (long)p.rows, p.C, s);
}

int swin_conv3x3_image(const SwinPlan& p, const SwinBufs& b, const ciaosr_conv_t& c, const float* src, float* dst, const float* res, hipStream_t s,
                       const char* tag) {
    if (c.frag && conv3x3_small_ok(p.Hp, p.Wp, p.ld, p.C, p.ld, CIAOSR_ACT_NONE))
        return conv3x3_small(src, p.ld, p.Hp, p.Wp, p.ld, c.frag, c.bias, p.C, dst, p.ld, nullptr, 0, res, p.ld, CIAOSR_ACT_NONE, 1.f, s, tag);
    return conv2d_hwc(src, p.ld, p.Hp, p.Wp, p.ld, c.weight, 9 * p.ld, c.bias, p.C, 3, dst, p.ld, nullptr, 0, res, p.ld, CIAOSR_ACT_NONE, 1.f, b.part,
                      b.part_floats, s, tag);
}

int swin_tail(const SwinPlan& p, const SwinBufs& b, const ciaosr_swinir_weights_t* w, float* feat, hipStream_t s) {
    SWIN_RUN(swin_layernorm(b.T, p.ld, b.Y, p.ld, w->norm_w, w->norm_b, (long)p.rows, p.C, s));
    for (int i = 0; i < p.B; ++i) {
        const size_t o = (size_t)i * p.HW * p.ld;
        SWIN_RUN(swin_conv3x3_image(p, b, w->conv_after_body, b.Y + o, b.F, b.x0 + o, s, "swin_conv_after_body"));
        {   // crop of the reflect padding and repack to C columns
            ProfScope prof("swin_crop", s);
            const long n = (long)p.H * p.W * (p.C >> 2);
            const int grid = (int)((n + 255) / 256);
            hipLaunchKernelGGL(crop_repack_kernel, dim3(grid > 4096 ? 4096 : grid), dim3(256), 0, s, b.F, p.ld, p.Wp, feat + (size_t)i * p.H * p.W * p.C,
                               p.H, p.W, p.C);
        }
        SWIN_RUN(launch_status("crop_repack"));
    }
    return CIAOSR_OK;
}

// ---- the fp32 driver: carve list, route, its own stages ---------------------------------------------------------------------------
// THE list of workspace buffers, in carve order: take(floats) is Arena::take (256-byte aligned) for a call, a running sum for the byte
// count.  pad5 is sliced, not carved five times: ld is a multiple of 64, so the five maps are the 256-byte aligned carve-outs they were.
template <class Take>
static SwinBufs swin_carve_f32(const SwinPlan& p, Take take) {
    SwinBufs b = {};
    const size_t map = p.HW * p.ld;
    b.img4 = take(p.HW * 4); b.rows36 = take(p.HW * 36);
    b.pad5 = take(5 * map);
    b.x0 = b.pad5; b.T = b.x0 + map; b.Tn = b.T + map; b.Y = b.Tn + map; b.F = b.Y + map;
    b.QKV = take(p.HW * (size_t)p.ldq);
    b.Hb = take(p.HW * p.ldh);
    b.part_floats = 16 * map;
    b.part = take(b.part_floats);
    return b;
}

// every refusal, nothing enqueued
static int swin_route_f32(const float* x, int H, int W, const ciaosr_swinir_weights_t* w, const float* feat, const void* workspace,
                          size_t workspace_bytes, SwinPlan* plan) {
    SWIN_RUN(swin_args_ok(x, 1, H, W, w, feat, workspace, plan));
    for (int i = 0; i < w->num_groups * w->depth; ++i) {
        const ciaosr_swin_block_t& b = w->blocks[i];
        CIAOSR_CHECK_ARG(b.qkv_w && b.proj_w && b.fc1_w && b.fc2_w);
    }
    if (workspace_bytes < ciaosr_swinir_workspace_bytes(H, W, w)) return CIAOSR_ERR_WORKSPACE;
    return CIAOSR_OK;
}

// the padded maps are zeroed once: their pad columns [C, ld) / [hid, ldh) are never written afterwards
static int zero_pads(const SwinPlan& p, const SwinBufs& b, hipStream_t s) {
    if (hipMemsetAsync(b.pad5, 0, 5 * p.HW * p.ld * sizeof(float), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if (hipMemsetAsync(b.Hb, 0, p.HW * p.ldh * sizeof(float), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    return CIAOSR_OK;
}

// Linear on the token map, dst = act(src W^T + bias) + res
static int linear(const SwinPlan& p, const SwinBufs& b, const float* src, int ld_src, const float* wgt, const float* bias, int N, float* dst, int ld_dst,
                  const float* res, int act, hipStream_t s, const char* tag) {
    const int M = (int)p.HW, K = ld_src, ld_res = res ? p.ld : 0;
    if (gemm_small_ok(M, N, K, ld_src, K)) return gemm_small_f32(src, ld_src, wgt, K, bias, dst, ld_dst, nullptr, 0, res, ld_res, M, N, K, act, 0.f, 1.f, s, tag);
    return conv2d_hwc(src, ld_src, p.Hp, p.Wp, K, wgt, K, bias, N, 1, dst, ld_dst, nullptr, 0, res, ld_res, act, 1.f, b.part, b.part_floats, s, tag);
}

// one Swin block on the residual stream Tn: seven launches
static int stage_block(const SwinPlan& p, const SwinBufs& b, const ciaosr_swin_block_t& k, hipStream_t s) {
    SWIN_RUN(swin_layernorm(b.Tn, p.ld, b.Y, p.ld, k.ln1_w, k.ln1_b, (long)p.HW, p.C, s));
    SWIN_RUN(linear(p, b, b.Y, p.ld, k.qkv_w, k.qkv_b, 3 * p.C, b.QKV, p.ldq, nullptr, CIAOSR_ACT_NONE, s, "swin_qkv"));
    {
        WinAttnP ap{b.QKV, p.ldq, (unsigned)(p.HW * (size_t)p.ldq * 4), b.F, p.ld, k.bias, k.shift ? k.mask : nullptr, p.Hp, p.Wp, p.C, p.heads, p.d, p.ws, k.shift};
        ProfScope prof("swin_window_attention", s);
        hipLaunchKernelGGL(window_attention_kernel, dim3((p.Hp / p.ws) * (p.Wp / p.ws) * p.heads), dim3(256), 0, s, ap);
    }
    SWIN_RUN(launch_status("window_attention"));
    SWIN_RUN(linear(p, b, b.F, p.ld, k.proj_w, k.proj_b, p.C, b.Tn, p.ld, b.Tn, CIAOSR_ACT_NONE, s, "swin_proj"));
    SWIN_RUN(swin_layernorm(b.Tn, p.ld, b.Y, p.ld, k.ln2_w, k.ln2_b, (long)p.HW, p.C, s));
    SWIN_RUN(linear(p, b, b.Y, p.ld, k.fc1_w, k.fc1_b, p.hid, b.Hb, p.ldh, nullptr, CIAOSR_ACT_GELU, s, "swin_fc1"));
    return linear(p, b, b.Hb, p.ldh, k.fc2_w, k.fc2_b, p.C, b.Tn, p.ld, b.Tn, CIAOSR_ACT_NONE, s, "swin_fc2");
}

// one RSTB: the blocks on a copy of the group input (the residual needs it), then conv3x3 + the group input, in place over it: the
// epilogue reads res[row][col] and writes dst[row][col] from the same lane
static int stage_group(const SwinPlan& p, const SwinBufs& b, const ciaosr_swinir_weights_t* w, int g, hipStream_t s) {
    if (hipMemcpyAsync(b.Tn, b.T, p.HW * p.ld * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    for (int l = 0; l < w->depth; ++l) SWIN_RUN(stage_block(p, b, w->blocks[g * w->depth + l], s));
    return swin_conv3x3_image(p, b, w->group_conv[g], b.Tn, b.T, b.T, s, "swin_group_conv");
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_swinir_workspace_bytes(int H, int W, const ciaosr_swinir_weights_t* w) {
    SwinPlan p;
    if (!swin_plan(1, H, W, w, &p)) return 0;
    size_t n = 0;
    swin_carve_f32(p, [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 16 * 256;              // room for the 256-byte alignment of each carve-out
}

extern "C" int ciaosr_swinir_forward_f32(const float* x_nchw, int H, int W, const ciaosr_swinir_weights_t* w, float* feat_hwc,
                                         void* workspace, size_t workspace_bytes, void* stream_) {
    SwinPlan p;
    SWIN_RUN(swin_route_f32(x_nchw, H, W, w, feat_hwc, workspace, workspace_bytes, &p));
    hipStream_t s = (hipStream_t)stream_;
    Arena ar(workspace, workspace_bytes);
    const SwinBufs b = swin_carve_f32(p, [&](size_t floats) { return ar.take<float>(floats); });
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    SWIN_RUN(zero_pads(p, b, s));
    SWIN_RUN(swin_embed(p, b, x_nchw, w, s));
    for (int g = 0; g < w->num_groups; ++g) SWIN_RUN(stage_group(p, b, w, g, s));
    return swin_tail(p, b, w, feat_hwc, s);
}

