// Pillow-exact bicubic resample of an 8-bit RGB image (HWC), the GT -> LR step of the reference's GT-only test data
// (configs/001_*.py, val_scale > 4: RandomDownSampling -> mmcv.imresize(..., 'bicubic', backend='pillow') -> PIL Image.resize).
// Pillow's 8-bit resample (Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc) is integer arithmetic once the coefficient
// tables are fixed: acc = 1 << 21 + sum_t src[xmin + t] * coef[t] in int32, out = clip(acc >> 22, 0, 255).  With 8-bit inputs
// |acc| < 255 sum |coef| < 2^31, so the sum is exact in any order and the result is bitwise Pillow's.  The tables are built by the
// host in float64 (ciaosr_amd/degrade.py); nothing here evaluates the filter.
//
// Two passes, as Pillow runs them: horizontal (only if Wo != W) into a uint8 [H][Wo][3] workspace with a 16-byte row pitch, clipped
// to uint8; vertical (only if Ho != H) from the workspace into dst_u8 [Ho][Wo][3] and / or dst_chw [3][Ho][Wo] = u8 / 255 (the
// RescaleToZeroOne + ImageToTensor of the test pipeline).  A skipped pass is a copy.
#include "ops.h"

namespace ciaosr {

struct ResampleP {
    const unsigned char* src;
    size_t pitch;                 // bytes between source rows
    int H, W, Ho, Wo;
    const int* bx;                // horizontal (xmin, count) per output column, or null = no horizontal pass
    const int* kx;                // [Wo][ksx] fixed-point coefficients
    int ksx;
    const int* by;                // vertical (ymin, count) per output row, or null = no vertical pass
    const int* ky;                // [Ho][ksy]
    int ksy;
    unsigned char* ws;            // [H][wsp] uint8
    int wsp;                      // workspace row pitch, a multiple of 16
    unsigned char* dst;           // [Ho][Wo][3] or null
    float* chw;                   // [3][Ho][Wo] or null
    int ob;                       // horizontal pass: output columns per workgroup
    int cap;                      // horizontal pass: LDS words (input pixels) per workgroup
};

constexpr int kHThreads = 128;
constexpr int kVThreads = 64;
constexpr int kLdsBudget = 32 * 1024;     // bytes of staged row per workgroup the column blocking aims for
constexpr int kLdsMax = 64 * 1024;

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> 22, 0), 255); }

// One workgroup = one input row y x `ob` output columns.  The input pixels those columns read, [lo, hi), are staged in LDS one 32-bit
// word per pixel (bytes R, G, B, unused) through 16-byte loads of the aligned blocks that cover them: an aligned 16-byte block that
// holds a byte of the image never crosses a page, so the bytes around the row that such a block also reads cannot fault.
__global__ __launch_bounds__(kHThreads) void resample_h_u8_kernel(ResampleP p) {
    extern __shared__ unsigned int row[];
    const int y = blockIdx.y;
    const int o0 = blockIdx.x * p.ob, o1 = min(o0 + p.ob, p.Wo);
    const bool copy = p.bx == nullptr;
    int lo = copy ? o0 : p.bx[2 * o0];
    int hi = copy ? o1 : p.bx[2 * (o1 - 1)] + p.bx[2 * (o1 - 1) + 1];
    lo = min(max(lo, 0), p.W);                     // tables come from the host: clamp them to the row and the LDS anyway
    hi = min(max(hi, lo), min(p.W, lo + p.cap));

    const unsigned char* rowp = p.src + (size_t)y * p.pitch;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(rowp + 3 * lo), nbytes = 3u * (unsigned)(hi - lo);
    const uintptr_t a0 = b0 & ~uintptr_t(15);
    const int nblk = nbytes ? (int)((b0 + nbytes - a0 + 15) >> 4) : 0;
    unsigned char* rb = reinterpret_cast<unsigned char*>(row);
    for (int j = threadIdx.x; j < nblk; j += kHThreads) {
        const uint4 v = *reinterpret_cast<const uint4*>(a0 + 16 * (uintptr_t)j);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long rel = (long)(a0 + 16 * (uintptr_t)j + k) - (long)b0;
            if (rel >= 0 && rel < (long)nbytes) {
                const int px = (int)(rel / 3), ch = (int)(rel - 3 * px);
                rb[4 * px + ch] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    __syncthreads();

    for (int o = o0 + threadIdx.x; o < o1; o += kHThreads) {
        unsigned char* out = p.ws + (size_t)y * p.wsp + 3 * o;
        if (copy) {
            const unsigned int w = row[min(o - lo, p.cap - 1)];
            out[0] = (unsigned char)w;
            out[1] = (unsigned char)(w >> 8);
            out[2] = (unsigned char)(w >> 16);
            continue;
        }
        const int xmin = p.bx[2 * o], n = min(p.bx[2 * o + 1], p.ksx);
        const int* k = p.kx + (size_t)o * p.ksx;
        int a_r = 1 << 21, a_g = 1 << 21, a_b = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const unsigned int w = row[min(max(xmin - lo + t, 0), p.cap - 1)];
            const int c = k[t];
            a_r += (int)(w & 255u) * c;
            a_g += (int)((w >> 8) & 255u) * c;
            a_b += (int)((w >> 16) & 255u) * c;
        }
        out[0] = (unsigned char)clip8(a_r);
        out[1] = (unsigned char)clip8(a_g);
        out[2] = (unsigned char)clip8(a_b);
    }
}

// One lane = 16 consecutive bytes of one output row (a 16-byte load per tap from the workspace); the row's coefficients are uniform
// over the workgroup.
__global__ __launch_bounds__(kVThreads) void resample_v_u8_kernel(ResampleP p) {
    const int oy = blockIdx.y;
    const int j = blockIdx.x * kVThreads + threadIdx.x;
    const int rowbytes = 3 * p.Wo;
    if (16 * j >= rowbytes) return;
    int acc[16];
    if (p.by == nullptr) {
        const uint4 v = *reinterpret_cast<const uint4*>(p.ws + (size_t)oy * p.wsp + 16 * j);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
    } else {
        const int ymin = p.by[2 * oy], n = min(p.by[2 * oy + 1], p.ksy);
        const int* kk = p.ky + (size_t)oy * p.ksy;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 1 << 21;
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const int yy = min(max(ymin + t, 0), p.H - 1);
            const uint4 v = *reinterpret_cast<const uint4*>(p.ws + (size_t)yy * p.wsp + 16 * j);
            const unsigned int w[4] = {v.x, v.y, v.z, v.w};
            const int c = kk[t];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += (int)((w[k >> 2] >> (8 * (k & 3))) & 255u) * c;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = clip8(acc[k]);
    }
    const size_t plane = (size_t)p.Ho * p.Wo;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int b = 16 * j + k;
        if (b < rowbytes) {
            if (p.dst) p.dst[(size_t)oy * rowbytes + b] = (unsigned char)acc[k];
            if (p.chw) {
                const int x = b / 3, c = b - 3 * x;
                p.chw[c * plane + (size_t)oy * p.Wo + x] = (float)acc[k] / 255.0f;   // correctly rounded, as numpy's u8 / 255.
            }
        }
    }
}

static inline int ws_pitch(int Wo) { return (3 * Wo + 15) & ~15; }

// input pixels the columns [o, o + ob) of an n_in -> n_out axis can read: (ob - 1) * scale + 1 + ksize (degrade.py's tables)
static inline long h_span(int ob, int n_in, int n_out, int ksize) {
    return (long)std::ceil((ob - 1) * ((double)n_in / n_out)) + ksize + 2;
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_resample_u8_workspace_bytes(int H, int W, int Ho, int Wo) {
    if (H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || Wo > (1 << 28)) return 0;
    return (size_t)H * (size_t)ws_pitch(Wo);
}

extern "C" int ciaosr_resample_u8(const unsigned char* src, size_t pitch, int H, int W, int Ho, int Wo, const int* bounds_x,
                                  const int* coef_x, int ksize_x, const int* bounds_y, const int* coef_y, int ksize_y,
                                  unsigned char* dst_u8, float* dst_chw, void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(src && H > 0 && W > 0 && Ho > 0 && Wo > 0 && W <= (1 << 28) && Wo <= (1 << 28) && pitch >= 3 * (size_t)W);
    CIAOSR_CHECK_ARG(Wo == W || (bounds_x && coef_x && ksize_x > 0));
    CIAOSR_CHECK_ARG(Ho == H || (bounds_y && coef_y && ksize_y > 0));
    CIAOSR_CHECK_ARG(workspace && aligned16(workspace));
    if (H > 65535 || Ho > 65535) return CIAOSR_ERR_UNSUPPORTED;     // one grid row per image row
    if (workspace_bytes < ciaosr_resample_u8_workspace_bytes(H, W, Ho, Wo)) return CIAOSR_ERR_WORKSPACE;
    if (!dst_u8 && !dst_chw) return CIAOSR_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool need_h = Wo != W, need_v = Ho != H;
    ResampleP p{src, pitch, H, W, Ho, Wo, need_h ? bounds_x : nullptr, coef_x, ksize_x, need_v ? bounds_y : nullptr, coef_y, ksize_y,
                (unsigned char*)workspace, ws_pitch(Wo), dst_u8, dst_chw, kHThreads, 0};
    const int ks = need_h ? ksize_x : 1;
    while (p.ob > 1 && h_span(p.ob, W, Wo, ks) * 4 > kLdsBudget) p.ob >>= 1;
    const long cap = h_span(p.ob, W, Wo, ks);
    if (cap * 4 > kLdsMax) return CIAOSR_ERR_UNSUPPORTED;               // a down-scale factor beyond ~4000
    p.cap = (int)cap;
    {
        ProfScope prof("resample_h_u8", s);
        hipLaunchKernelGGL(resample_h_u8_kernel, dim3(ceil_div(Wo, p.ob), H), dim3(kHThreads), (size_t)cap * 4, s, p);
        int rc = launch_status("resample_h_u8");
        if (rc) return rc;
    }
    ProfScope prof("resample_v_u8", s);
    hipLaunchKernelGGL(resample_v_u8_kernel, dim3(ceil_div(ceil_div(3L * Wo, 16), kVThreads), Ho), dim3(kVThreads), 0, s, p);
    return launch_status("resample_v_u8");
}
