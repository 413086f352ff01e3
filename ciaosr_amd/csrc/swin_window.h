// Window attention of the SwinIR trunks (swinir_net.py:66-146), shared by the fp32 trunk (swinir.hip: one image, fp32 output) and the
// f16-linear trunk (swinir_h16.hip: B images per launch, output as IEEE half = the A operand of the proj GEMM): one device function,
// templated on the element type of the store; the caller passes the window, the head and the image's QKV / output rows.
#pragma once
#include "h16_util.h"
#include "ops.h"

namespace ciaosr {

__device__ __forceinline__ void swin_store(float* o, float v) { *o = v; }
__device__ __forceinline__ void swin_store(unsigned short* o, float v) { *o = to_h16<true>(v); }

struct WinAttnP {
    const float* qkv; int ld_qkv; unsigned qkv_bytes;   // [HW][3C]: q | k | v, each [heads][d]  (q already scaled: the scale is folded into the weights)
    float* out; int ld_out;           // [HW][ld]: column h*d + e
    const float* bias;                // [heads][N][N] relative-position bias of this layer
    const float* mask;                // [nW][N][N] or null (unshifted layer)
    int Hp, Wp, C, heads, d, ws, shift;
};

constexpr int WMAXN = 64, WMAXD = 32;   // window 8x8, head dim <= 32
typedef float f32x16w __attribute__((ext_vector_type(16)));

// One workgroup per (window, head), 4 waves.  q, k, v of the window's 64 tokens go to LDS (head dim zero-padded to 32);
// S = q k^T as four 32x32 MFMA tiles (one per wave, exact-fp32 v_mfma_f32_32x32x2_f32), + bias + mask, row softmax,
// O = P v as two 32x32 tiles.  N < 64 (smaller windows) runs with zero rows and -inf columns.
template <typename OutT>
__device__ __forceinline__ void window_attention_body(const WinAttnP& p, const int win, const int head, const float* qkv_img, OutT* out_img) {
    __shared__ float sq[WMAXN][WMAXD + 2], sk[WMAXN][WMAXD + 2], sv[WMAXN][WMAXD + 2];
    __shared__ float sp[WMAXN][WMAXN + 1];
    __shared__ int stok[WMAXN];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
    const int N = p.ws * p.ws, nwx = p.Wp / p.ws;
    const int wy = win / nwx, wx = win - wy * nwx;
    if (t < WMAXN) {
        // window-local (ly, lx) of the ROLLED map -> original token: rolled[y'] = x[(y' + shift) mod Hp]  (roll by -shift)
        int tok = 0;
        if (t < N) {
            const int ly = t / p.ws, lx = t - ly * p.ws;
            int y = wy * p.ws + ly + p.shift, x = wx * p.ws + lx + p.shift;
            if (y >= p.Hp) y -= p.Hp;
            if (x >= p.Wp) x -= p.Wp;
            tok = y * p.Wp + x;
        }
        stok[t] = tok;
    }
    __syncthreads();
    {   // q, k, v of the window's tokens -> LDS.  All 12 loads of a thread are issued before the first LDS store (a
        // load-store loop makes hipcc wait for every load in turn: 8 dependent HBM round trips, ~16 us)
        // (buffer loads with an out-of-range offset for the padding: no branch around a load)
        const __amdgpu_buffer_rsrc_t rs_q = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qkv_img), 0, p.qkv_bytes, 0x00020000);
        typedef int i32x2w __attribute__((ext_vector_type(2)));
        float2 vq[4], vk[4], vv[4];
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) {
            const int i = t + 256 * sI, n = i >> 4, e = 2 * (i & 15);
            const unsigned off = (n < N && e < p.d) ? ((unsigned)stok[n] * (unsigned)p.ld_qkv + (unsigned)(head * p.d + e)) * 4u : 0xFFFFFFF0u;
            const unsigned offk = off == 0xFFFFFFF0u ? off : off + (unsigned)p.C * 4u;
            const unsigned offv = off == 0xFFFFFFF0u ? off : off + (unsigned)p.C * 8u;
            const i32x2w a = __builtin_amdgcn_raw_buffer_load_b64(rs_q, (int)off, 0, 0);
            const i32x2w b = __builtin_amdgcn_raw_buffer_load_b64(rs_q, (int)offk, 0, 0);
            const i32x2w c = __builtin_amdgcn_raw_buffer_load_b64(rs_q, (int)offv, 0, 0);
            vq[sI] = make_float2(__int_as_float(a.x), __int_as_float(a.y));
            vk[sI] = make_float2(__int_as_float(b.x), __int_as_float(b.y));
            vv[sI] = make_float2(__int_as_float(c.x), __int_as_float(c.y));
        }
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) {
            const int i = t + 256 * sI, n = i >> 4, e = 2 * (i & 15);
            sq[n][e] = vq[sI].x; sq[n][e + 1] = vq[sI].y;
            sk[n][e] = vk[sI].x; sk[n][e + 1] = vk[sI].y;
            sv[n][e] = vv[sI].x; sv[n][e + 1] = vv[sI].y;
        }
    }
    __syncthreads();
    {   // scores tile (mi, ni) of this wave: D[m][n], lane holds column j = 32 ni + li, rows 8 (r >> 2) + 4 lh + (r & 3)
        const int mi = w >> 1, ni = w & 1;
        f32x16w acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < WMAXD / 2; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sq[32 * mi + li][2 * ks + lh], sk[32 * ni + li][2 * ks + lh], acc, 0, 0, 0);
        const int j = 32 * ni + li;
        float bb[16], mm[16];                              // bias and mask of the 16 rows: all requested before use
        const unsigned nn4 = (unsigned)N * (unsigned)N * 4u;
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias) + (size_t)head * N * N, 0, nn4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_m =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.mask ? p.mask + (size_t)win * N * N : p.bias), 0, p.mask ? nn4 : 0u, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * mi + 8 * (r >> 2) + 4 * lh + (r & 3);
            const unsigned off = (i < N && j < N) ? (unsigned)(i * N + j) * 4u : 0xFFFFFFF0u;
            bb[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_b, (int)off, 0, 0));
            mm[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_m, (int)off, 0, 0));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * mi + 8 * (r >> 2) + 4 * lh + (r & 3);
            sp[i][j] = (i < N && j < N) ? acc[r] + bb[r] + mm[r] : -INFINITY;
        }
    }
    __syncthreads();
    {   // softmax: 4 adjacent lanes per row (16 columns each), quad reductions through DPP
        const int i = t >> 2, c0 = (t & 3) * 16;
        float v[16];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) { v[c] = sp[i][c0 + c]; m = fmaxf(m, v[c]); }
        m = fmaxf(m, quad_xor1(m));
        m = fmaxf(m, quad_xor2(m));
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) { v[c] = (i < N && c0 + c < N) ? expf(v[c] - m) : 0.f; sum += v[c]; }
        sum += quad_xor1(sum);
        sum += quad_xor2(sum);
        const float inv = i < N ? 1.0f / sum : 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) sp[i][c0 + c] = v[c] * inv;
    }
    __syncthreads();
    if (w < 2) {                                          // O tile mi = w: D[m][e], lane holds channel e = li
        f32x16w acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
        for (int ks = 0; ks < WMAXN / 2; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sp[32 * w + li][2 * ks + lh], sv[2 * ks + lh][li], acc, 0, 0, 0);
        if (li < p.d) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
                if (i < N) swin_store(out_img + (size_t)stok[i] * p.ld_out + head * p.d + li, acc[r]);
            }
        }
    }
}

// sum over the wavefront (the LayerNorm statistics of both trunks)
__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- host side shared by the two drivers: the plan, the buffers, the common refusals and the fp32 stages both run (swinir.hip) ------
struct SwinPlan {
    int B, H, W, Hp, Wp, C, heads, d, ws, hid, ld, ldh, ldq;   // the fp32 entry: B = 1
    size_t HW, rows;               // tokens of one image, of the batch
};
// ld = C rounded up to 64; ldq: the convolution kernels store whole 32-column tiles, so a QKV row has room up to the next multiple of 32
inline bool swin_plan(int B, int H, int W, const ciaosr_swinir_weights_t* w, SwinPlan* p) {
    if (!w || B <= 0 || H <= 0 || W <= 0 || w->window_size <= 0) return false;
    p->B = B; p->H = H; p->W = W; p->ws = w->window_size;
    p->Hp = (int)round_up((size_t)H, p->ws); p->Wp = (int)round_up((size_t)W, p->ws);
    p->C = w->embed_dim; p->heads = w->num_heads; p->d = p->heads > 0 ? p->C / p->heads : 0; p->hid = w->hidden;
    p->ld = (int)round_up((size_t)p->C, 64); p->ldh = (int)round_up((size_t)p->hid, 64);
    p->ldq = (int)round_up((size_t)3 * p->C, 32);
    p->HW = (size_t)p->Hp * p->Wp; p->rows = p->HW * (size_t)B;
    return true;
}
// What the shared stages touch, and each driver's own buffers beside them (a driver leaves the other's null)
struct SwinBufs {
    float *img4, *rows36;          // conv_first temporaries, one image at a time
    float *x0, *T, *Tn;            // conv_first of every image (the last residual); group input / output; residual stream of the group's blocks
    float *Y, *F;                  // normed map (f16: Tn again); conv_after_body of one image (fp32: the blocks' attention output too)
    float *QKV, *part;
    size_t part_floats;            // split-K slabs of the per-image 3x3 convolutions
    float *pad5, *Hb;              // fp32: x0 | T | Tn | Y | F as ONE carve-out, zeroed whole; hidden activations
    unsigned short *A16, *Hb16;    // f16: attention output, hidden activations
};

#define SWIN_RUN(x) do { const int rc_ = (x); if (rc_ != CIAOSR_OK) return rc_; } while (0)

// every refusal the two entries share (shapes, the plan, the pointers and convolutions both read); enqueues nothing
int swin_args_ok(const float* x, int B, int H, int W, const ciaosr_swinir_weights_t* w, const float* feat, const void* workspace, SwinPlan* plan);
int swin_layernorm(const float* X, int ldx, float* Y, int ldy, const float* g, const float* b, long rows, int C, hipStream_t s);
// per image conv_first, then the PatchEmbed norm over all rows: x -> img4 -> rows36 -> x0 -> T
int swin_embed(const SwinPlan& p, const SwinBufs& b, const float* x, const ciaosr_swinir_weights_t* w, hipStream_t s);
// 3x3 convolution of ONE image, dst = conv(src) + res: the small-map kernel where the layer has fragments and the map fits, else split-K
int swin_conv3x3_image(const SwinPlan& p, const SwinBufs& b, const ciaosr_conv_t& c, const float* src, float* dst, const float* res, hipStream_t s,
                       const char* tag);
// final norm over all rows, then per image conv_after_body + conv_first's output, crop and repack: T -> Y -> F (+ x0) -> feat
int swin_tail(const SwinPlan& p, const SwinBufs& b, const ciaosr_swinir_weights_t* w, float* feat, hipStream_t s);

}  // namespace ciaosr
