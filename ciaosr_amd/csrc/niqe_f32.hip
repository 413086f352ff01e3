// NIQE on the device: the image work of mmedited/core/evaluation/metrics.py:340-532 (niqe, niqe_core, compute_feature,
// estimate_aggd_param) for an 8-bit BGR image, down to six sums per map and block.  The host finishes (ciaosr_amd/niqe_hip.py):
// AGGD parameters from the sums, the mean and covariance over blocks, the distance to the pristine model.
//
// Five launches for any image size, no atomics, every result bitwise repeatable and independent of the row pitch:
//   niqe_luma     Y = round_half_even(mmcv.bgr2ycbcr(img / 255, y_only=True) * 255) of the cropped image, fp32 (y_of_bgr, shared
//                 with psnr_ssim_u8; the values are integers)
//   niqe_mscn     (x - mu) / (sqrt|filter(x^2) - mu^2| + 1), the 7x7 window with a replicated border: a 32x32 tile with a
//                 3-pixel halo in LDS, one launch per scale
//   niqe_half     MATLAB imresize(x / 255, 0.5) * 255: bicubic (a = -0.5), antialiased, symmetric border, rows first and then columns.
//                 For even sizes every output has the same eight taps [-3 -9 29 111 111 29 -9 -3] / 256 on inputs 2o-3 .. 2o+4
//   niqe_moments  one workgroup per 96x96 (scale 1) or 48x48 (scale 2) block: the block and its products with itself rolled by
//                 [0,1], [1,0], [1,1], [1,-1] -- wrapping INSIDE the block, as np.roll of the block does -- each reduced to (count and
//                 sum of squares of the negatives, the same of the positives, sum of |v|, sum of v^2) by a fixed tree
//
// Every map is fp64 and every operation individually rounded, in the order the float64 host restatement (tests/niqe_ref.py) and
// scipy's `convolve` use: the 49 window taps are added one after the other in raster order, the eight resample taps from the lowest
// index up.  The maps then follow the restatement operation for operation (IEEE fp64, no FMA), so the SIGN of a sample -- which decides the side of the AGGD it is
// counted on, and whether a flat block has no sample on a side at all (a NaN row) -- never depends on the device; only the block
// sums are added in another order.  The kernels are bound by memory; the fp64 maps cost 16 bytes per pixel of workspace.
#include "ops.h"
#include "index_math.h"

namespace ciaosr {

constexpr int kNThreads = 256;
constexpr int kBlock = 96;                  // block side at scale 1 (48 at scale 2)
constexpr int kWin = 7, kRad = 3;
constexpr int kTile = 32;                   // MSCN outputs per workgroup: 32 x 32
constexpr int kTileIn = kTile + 2 * kRad;   // 38
constexpr int kNiqeMaxDim = 65535;          // H, W: one grid row per image row
constexpr int kMaps = 5, kSums = 6;

struct NiqeGeom {
    int Hc, Wc;         // after crop_border
    int nbh, nbw;       // blocks
    int Hb, Wb;         // after the block crop
    int H2, W2;         // second scale
    long blocks;
};

static inline bool niqe_geometry(int H, int W, int crop, NiqeGeom* g) {
    if (H <= 0 || W <= 0 || H > kNiqeMaxDim || W > kNiqeMaxDim || crop < 0 || crop > kNiqeMaxDim) return false;
    g->Hc = H - 2 * crop;
    g->Wc = W - 2 * crop;
    if (g->Hc < kBlock || g->Wc < kBlock) return false;
    g->nbh = g->Hc / kBlock;
    g->nbw = g->Wc / kBlock;
    g->Hb = g->nbh * kBlock;
    g->Wb = g->nbw * kBlock;
    g->H2 = g->Hb / 2;
    g->W2 = g->Wb / 2;
    g->blocks = (long)g->nbh * g->nbw;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNThreads) void niqe_luma_kernel(const unsigned char* img, size_t pitch, int crop, int Hc, int Wc,
                                                              float* luma, float* luma_out) {
    const int r = blockIdx.y, c = blockIdx.x * kNThreads + threadIdx.x;
    if (c >= Wc) return;
    const unsigned char* q = img + (size_t)(crop + r) * pitch + 3 * (size_t)(crop + c);
    const float y = __builtin_rintf(y_of_bgr((unsigned int)q[0] | (unsigned int)q[1] << 8 | (unsigned int)q[2] << 16));
    luma[(size_t)r * Wc + c] = y;
    if (luma_out) luma_out[(size_t)r * Wc + c] = y;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// src [Hs][pitch] (the top-left Hs x Ws of it), dst [Hs][Ws]
template <typename T>
__global__ __launch_bounds__(kNThreads) void niqe_mscn_kernel(const T* src, size_t pitch, int Hs, int Ws, const double* window,
                                                              double* dst) {
#pragma clang fp contract(off)
    __shared__ double tile[kTileIn][kTileIn + 1];
    __shared__ double wf[kWin * kWin];
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    // `convolve` flips the window: tap (a, b) of the raster walk multiplies window[6 - a][6 - b]
    if (threadIdx.x < kWin * kWin) wf[threadIdx.x] = window[kWin * kWin - 1 - threadIdx.x];
    for (int e = threadIdx.x; e < kTileIn * kTileIn; e += kNThreads) {
        const int tr = e / kTileIn, tc = e % kTileIn;
        const int r = min(max(r0 + tr - kRad, 0), Hs - 1), c = min(max(c0 + tc - kRad, 0), Ws - 1);      // replicated border
        tile[tr][tc] = (double)src[(size_t)r * pitch + c];
    }
    __syncthreads();
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < kTile / 8; ++k) {
        const int lr = ty + 8 * k;
        const int r = r0 + lr, c = c0 + tx;
        if (r >= Hs || c >= Ws) continue;
        double mu = 0.0, sq = 0.0;
#pragma unroll
        for (int a = 0; a < kWin; ++a)
#pragma unroll
            for (int b = 0; b < kWin; ++b) {
                const double x = tile[lr + a][tx + b], w = wf[a * kWin + b];
                mu = mu + x * w;
                sq = sq + (x * x) * w;
            }
        const double x = tile[lr + kRad][tx + kRad];
        const double sigma = sqrt(fabs(sq - mu * mu));
        dst[(size_t)r * Ws + c] = (x - mu) / (sigma + 1.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_sym(int i, int n) {      // MATLAB's symmetric padding: ... 1 0 | 0 1 .. n-1 | n-1 n-2 ...
    return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
}

// luma [Hb][pitch] -> half [Hb / 2][Wb / 2]
__global__ __launch_bounds__(kNThreads) void niqe_half_kernel(const float* luma, size_t pitch, int Hb, int Wb, double* half) {
#pragma clang fp contract(off)
    const double w[8] = {-3.0 / 256, -9.0 / 256, 29.0 / 256, 111.0 / 256, 111.0 / 256, 29.0 / 256, -9.0 / 256, -3.0 / 256};
    const int H2 = Hb / 2, W2 = Wb / 2;
    const int orow = blockIdx.y, ocol = blockIdx.x * kNThreads + threadIdx.x;
    if (ocol >= W2 || orow >= H2) return;
    int rows[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) rows[j] = reflect_sym(2 * orow - 3 + j, Hb);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = reflect_sym(2 * ocol - 3 + k, Wb);
        double t = 0.0;                                   // the row pass (along the height) of column c
#pragma unroll
        for (int j = 0; j < 8; ++j) t = t + w[j] * ((double)luma[(size_t)rows[j] * pitch + c] / 255.0);
        acc = acc + w[k] * t;
    }
    half[(size_t)orow * W2 + ocol] = acc * 255.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double niqe_wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;                       // complete in lane 0
}

__device__ __forceinline__ void aggd_add(double v, double* s) {
    const double vv = v * v;
    if (v < 0.0) {
        s[0] += 1.0;
        s[1] += vv;
    }
    if (v > 0.0) {
        s[2] += 1.0;
        s[3] += vv;
    }
    s[4] += fabs(v);
    s[5] += vv;
}

// grid (blocks, 2 scales); moments [2][blocks][5][6], blocks in the reference's order (column of blocks outer)
__global__ __launch_bounds__(kNThreads) void niqe_moments_kernel(const double* mscn1, const double* mscn2, int nbh, int Wb, long blocks,
                                                                 double* moments) {
    __shared__ double red[kNThreads / kWave][kMaps * kSums];
    const int scale = blockIdx.y;
    const int bs = kBlock >> scale;
    const size_t pitch = (size_t)(Wb >> scale);
    const long bi = blockIdx.x;
    const int bw = (int)(bi / nbh), bh = (int)(bi % nbh);
    const double* m = (scale ? mscn2 : mscn1) + (size_t)bh * bs * pitch + (size_t)bw * bs;

    double s[kMaps][kSums];
#pragma unroll
    for (int a = 0; a < kMaps; ++a)
#pragma unroll
        for (int q = 0; q < kSums; ++q) s[a][q] = 0.0;

    for (int e = threadIdx.x; e < bs * bs; e += kNThreads) {
        const int r = e / bs, c = e % bs;
        const int rm = r == 0 ? bs - 1 : r - 1, cm = c == 0 ? bs - 1 : c - 1, cp = c == bs - 1 ? 0 : c + 1;
        const double v = m[r * pitch + c];
        aggd_add(v, s[0]);
        aggd_add(v * m[r * pitch + cm], s[1]);          // np.roll(block, [0, 1]): [r][c - 1]
        aggd_add(v * m[rm * pitch + c], s[2]);          // [1, 0]: [r - 1][c]
        aggd_add(v * m[rm * pitch + cm], s[3]);         // [1, 1]: [r - 1][c - 1]
        aggd_add(v * m[rm * pitch + cp], s[4]);         // [1, -1]: [r - 1][c + 1]
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < kMaps; ++a)
#pragma unroll
        for (int q = 0; q < kSums; ++q) {
            const double t = niqe_wave_sum(s[a][q]);
            if (lane == 0) red[wave][a * kSums + q] = t;
        }
    __syncthreads();
    if (threadIdx.x < kMaps * kSums) {
        const int i = threadIdx.x;
        const double t = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        moments[((size_t)scale * blocks + bi) * (kMaps * kSums) + i] = t;
    }
}

struct NiqeWs {
    float* luma;
    double *mscn1, *half, *mscn2;
    size_t bytes;
    bool ok;
};

static inline NiqeWs niqe_carve(const NiqeGeom& g, void* base, size_t size) {
    Arena ar(base, size);
    NiqeWs w;
    w.luma = ar.take<float>((size_t)g.Hc * g.Wc);
    w.mscn1 = ar.take<double>((size_t)g.Hb * g.Wb);
    w.half = ar.take<double>((size_t)g.H2 * g.W2);
    w.mscn2 = ar.take<double>((size_t)g.H2 * g.W2);
    w.bytes = ar.off;
    w.ok = ar.ok;
    return w;
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_niqe_workspace_bytes(int H, int W, int crop_border) {
    NiqeGeom g;
    if (!niqe_geometry(H, W, crop_border, &g)) return 0;
    return niqe_carve(g, nullptr, ~(size_t)0).bytes;
}

extern "C" int ciaosr_niqe_moments_u8(const unsigned char* img, size_t pitch, int H, int W, int crop_border, const double* window,
                                      double* moments, float* luma_out, void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(img && window && moments && H > 0 && W > 0 && crop_border >= 0);
    CIAOSR_CHECK_ARG(W <= kNiqeMaxDim && pitch >= 3 * (size_t)W);
    CIAOSR_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(window) & 7u) == 0 && (reinterpret_cast<uintptr_t>(moments) & 7u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(luma_out) & 3u) == 0);
    NiqeGeom g;
    if (!niqe_geometry(H, W, crop_border, &g)) return CIAOSR_ERR_UNSUPPORTED;       // beyond the index range, or no 96x96 block
    const NiqeWs w = niqe_carve(g, workspace, workspace_bytes);
    if (!w.ok) return CIAOSR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    {
        ProfScope prof("niqe_luma", s);
        hipLaunchKernelGGL(niqe_luma_kernel, dim3(ceil_div(g.Wc, kNThreads), g.Hc), dim3(kNThreads), 0, s, img, pitch, crop_border, g.Hc,
                           g.Wc, w.luma, luma_out);
        if ((rc = launch_status("niqe_luma"))) return rc;
    }
    {
        ProfScope prof("niqe_mscn", s);
        hipLaunchKernelGGL(niqe_mscn_kernel<float>, dim3(ceil_div(g.Wb, kTile), ceil_div(g.Hb, kTile)), dim3(kNThreads), 0, s,
                           (const float*)w.luma, (size_t)g.Wc, g.Hb, g.Wb, window, w.mscn1);
        if ((rc = launch_status("niqe_mscn"))) return rc;
    }
    {
        ProfScope prof("niqe_half", s);
        hipLaunchKernelGGL(niqe_half_kernel, dim3(ceil_div(g.W2, kNThreads), g.H2), dim3(kNThreads), 0, s, (const float*)w.luma,
                           (size_t)g.Wc, g.Hb, g.Wb, w.half);
        if ((rc = launch_status("niqe_half"))) return rc;
    }
    {
        ProfScope prof("niqe_mscn", s);
        hipLaunchKernelGGL(niqe_mscn_kernel<double>, dim3(ceil_div(g.W2, kTile), ceil_div(g.H2, kTile)), dim3(kNThreads), 0, s,
                           (const double*)w.half, (size_t)g.W2, g.H2, g.W2, window, w.mscn2);
        if ((rc = launch_status("niqe_mscn"))) return rc;
    }
    ProfScope prof("niqe_moments", s);
    hipLaunchKernelGGL(niqe_moments_kernel, dim3((unsigned)g.blocks, 2), dim3(kNThreads), 0, s, (const double*)w.mscn1,
                       (const double*)w.mscn2, g.nbh, g.Wb, g.blocks, moments);
    return launch_status("niqe_moments");
}
