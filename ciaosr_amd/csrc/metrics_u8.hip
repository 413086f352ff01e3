// Evaluation on the device: the 8-bit quantiser of mmedit's tensor2img and PSNR / SSIM of two 8-bit BGR images
// (basic_restorer.py:101-124 -> mmedited/core/evaluation/metrics.py:181-226 psnr, :229-318 ssim; restated in ciaosr_amd/metrics.py).
//
// tensor2img_u8: clamp to [0, 1], ONE fp32 multiply by 255, round half to even, RGB planes -> BGR bytes.
//
// psnr_ssim_u8: one wave owns a strip of 64 columns x kTileH rows of the cropped image and walks it top to bottom.  Per row it loads
// its 74 pixels of both images (64 + the 10-pixel halo to the right), converts them to the evaluated channel in fp32 exactly as the
// host does (Y = ((b/255 * 24.966 + g/255 * 128.553 + r/255 * 65.481 + 16) / 255) * 255, every operation individually rounded), and
// exchanges them through a per-wave LDS row.  Lane c then runs the 11-tap Gaussian row pass of x, y, xx, yy, xy at column c in fp64
// and feeds the result into 11 pending fp64 column sums per quantity held in registers (the loop is unrolled by 11, so the ring index
// is static): no fp64 map ever reaches LDS or memory.  A finished column sum gives one value of the SSIM map.  The squared differences
// of PSNR come from the same fp32 values (each cropped pixel once: the halo rows and columns belong to the neighbouring strip).
// Every sum over pixels is fp64.  No atomics: each wave stores its two partial sums, one fixed-order pass adds them, so a result is
// bitwise reproducible and independent of the row pitch.
#include "ops.h"
#include "index_math.h"

namespace ciaosr {

constexpr int kQThreads = 256;
constexpr int kTaps = 11;
constexpr int kHalo = kTaps - 1;
constexpr int kTileH = 64;                 // rows of the cropped image per strip
constexpr int kStripW = kWave;             // columns per wave
constexpr int kWaves = 4;                  // strips (side by side) per workgroup
constexpr int kRowLds = kStripW + kHalo + 6;    // floats per staged row (74 used)
constexpr int kMaxDim = 1 << 20;           // H, W the index arithmetic is checked for

// ---------------------------------------------------------------------------------------------------------------------------------
struct QuantP {
    const float* src;             // [3][H][W] RGB
    unsigned char* dst;           // [H][pitch] BGR bytes
    size_t pitch;
    int H, W;
    int vec;                      // 4 pixels per lane (W % 4 == 0, planes 16-byte aligned, rows 4-byte aligned)
};

__device__ __forceinline__ unsigned int quant8(float v) {
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (unsigned int)(int)__builtin_rintf(mul_rn(v, 255.0f));
}

__global__ __launch_bounds__(kQThreads) void tensor2img_u8_kernel(QuantP p) {
    const int y = blockIdx.y;
    const size_t plane = (size_t)p.H * p.W;
    const float* row = p.src + (size_t)y * p.W;
    unsigned char* out = p.dst + (size_t)y * p.pitch;
    const int j = blockIdx.x * kQThreads + threadIdx.x;
    if (p.vec) {
        const int x = 4 * j;
        if (x >= p.W) return;
        const float4 r = *reinterpret_cast<const float4*>(row + x);
        const float4 g = *reinterpret_cast<const float4*>(row + plane + x);
        const float4 b = *reinterpret_cast<const float4*>(row + 2 * plane + x);
        // bytes b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
        const unsigned int w0 = quant8(b.x) | quant8(g.x) << 8 | quant8(r.x) << 16 | quant8(b.y) << 24;
        const unsigned int w1 = quant8(g.y) | quant8(r.y) << 8 | quant8(b.z) << 16 | quant8(g.z) << 24;
        const unsigned int w2 = quant8(r.z) | quant8(b.w) << 8 | quant8(g.w) << 16 | quant8(r.w) << 24;
        unsigned int* o = reinterpret_cast<unsigned int*>(out + 3 * (size_t)x);
        o[0] = w0;
        o[1] = w1;
        o[2] = w2;
    } else {
        if (j >= p.W) return;
        out[3 * (size_t)j + 0] = (unsigned char)quant8(row[2 * plane + j]);
        out[3 * (size_t)j + 1] = (unsigned char)quant8(row[plane + j]);
        out[3 * (size_t)j + 2] = (unsigned char)quant8(row[j]);
    }
}

// RGBA: the colour bytes of item 0 and, as alpha, the integer luma of item 1's bytes.  The weights sum to 2^14, so a grey v, v, v is v.
__device__ __forceinline__ unsigned int alpha_of_bgr(unsigned int b, unsigned int g, unsigned int r) {
    return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

__device__ __forceinline__ void store_bgra(unsigned char* out, int x, unsigned int word, int vec) {
    if (vec) {
        reinterpret_cast<unsigned int*>(out)[x] = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[4 * (size_t)x + k] = (unsigned char)(word >> (8 * k));
    }
}

struct QuantAP {
    const float* colour;          // [3][H][W] RGB
    const float* alpha;           // [3][H][W] RGB: the alpha plane as the model rendered it, three times
    unsigned char* dst;           // [H][pitch] B G R A bytes
    size_t pitch;
    int H, W;
    int vec;                      // one 32-bit store per pixel (dst and pitch 4-byte aligned)
};

__global__ __launch_bounds__(kQThreads) void tensor2img_bgra_u8_kernel(QuantAP p) {
    const int y = blockIdx.y, x = blockIdx.x * kQThreads + threadIdx.x;
    if (x >= p.W) return;
    const size_t plane = (size_t)p.H * p.W, i = (size_t)y * p.W + x;
    const unsigned int b = quant8(p.colour[2 * plane + i]), g = quant8(p.colour[plane + i]), r = quant8(p.colour[i]);
    const unsigned int a = alpha_of_bgr(quant8(p.alpha[2 * plane + i]), quant8(p.alpha[plane + i]), quant8(p.alpha[i]));
    store_bgra(p.dst + (size_t)y * p.pitch, x, b | g << 8 | r << 16 | a << 24, p.vec);
}

struct PackAP {
    const unsigned char* bgr;     // [H][pitch_bgr] B G R
    const unsigned char* grey;    // [H][pitch_grey] B G R of the alpha image
    size_t pitch_bgr, pitch_grey;
    unsigned char* dst;           // [H][pitch] B G R A
    size_t pitch;
    int H, W;
    int vec;
};

__global__ __launch_bounds__(kQThreads) void pack_bgra_u8_kernel(PackAP p) {
    const int y = blockIdx.y, x = blockIdx.x * kQThreads + threadIdx.x;
    if (x >= p.W) return;
    const unsigned char* c = p.bgr + (size_t)y * p.pitch_bgr + 3 * (size_t)x;
    const unsigned char* q = p.grey + (size_t)y * p.pitch_grey + 3 * (size_t)x;
    const unsigned int a = alpha_of_bgr(q[0], q[1], q[2]);
    store_bgra(p.dst + (size_t)y * p.pitch, x, (unsigned int)c[0] | (unsigned int)c[1] << 8 | (unsigned int)c[2] << 16 | a << 24, p.vec);
}

// Grey: ONE byte per pixel, the integer luma of the pixel's three bytes -- Pillow's convert('L') and libjpeg's Y (ycc(.., 0) in
// jpeg_u8.hip).  The weights sum to 2^16, so a neutral v, v, v is v.  Not alpha_of_bgr: the two differ by 1 on 39 135 triples.
__device__ __forceinline__ unsigned int grey_of_bgr(unsigned int b, unsigned int g, unsigned int r) {
    return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

constexpr int kGreyPer = 4;       // consecutive output bytes per lane: one 32-bit store where dst and its pitch allow

// bytes [x, x + n) of a row, n <= kGreyPer, packed little-endian in `word`
__device__ __forceinline__ void store_grey(unsigned char* out, int x, int n, unsigned int word, int vec) {
    if (vec && n == kGreyPer) {
        *reinterpret_cast<unsigned int*>(out + x) = word;
    } else {
        for (int k = 0; k < n; ++k) out[x + k] = (unsigned char)(word >> (8 * k));
    }
}

struct QuantGP {
    const float* src;             // [3][H][W] RGB
    unsigned char* dst;           // [H][pitch], one byte per pixel
    size_t pitch;
    int H, W;
    int vec_in;                   // float4 loads (W % 4 == 0, planes 16-byte aligned)
    int vec_out;                  // 32-bit stores (dst and pitch 4-byte aligned)
};

__global__ __launch_bounds__(kQThreads) void tensor2img_grey_u8_kernel(QuantGP p) {
    const int y = blockIdx.y, x = kGreyPer * (blockIdx.x * kQThreads + threadIdx.x);
    if (x >= p.W) return;
    const int n = min(kGreyPer, p.W - x);
    const size_t plane = (size_t)p.H * p.W;
    const float* row = p.src + (size_t)y * p.W + x;
    float c[3][kGreyPer];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (p.vec_in) {
            const float4 v = *reinterpret_cast<const float4*>(row + ch * plane);
            c[ch][0] = v.x, c[ch][1] = v.y, c[ch][2] = v.z, c[ch][3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < kGreyPer; ++k) c[ch][k] = k < n ? row[ch * plane + k] : 0.0f;
        }
    }
    unsigned int word = 0u;
#pragma unroll
    for (int k = 0; k < kGreyPer; ++k) word |= grey_of_bgr(quant8(c[2][k]), quant8(c[1][k]), quant8(c[0][k])) << (8 * k);
    store_grey(p.dst + (size_t)y * p.pitch, x, n, word, p.vec_out);
}

struct GreyP {
    const unsigned char* src;     // [H][pitch_src], 3 bytes per pixel
    size_t pitch_src;
    int bgr;                      // the bytes of a pixel are B G R, else R G B
    unsigned char* dst;           // [H][pitch]
    size_t pitch;
    int H, W;
    int vec_in;                   // three 32-bit loads per lane (src and its pitch 4-byte aligned)
    int vec_out;
};

__global__ __launch_bounds__(kQThreads) void grey_from_bgr_u8_kernel(GreyP p) {
    const int y = blockIdx.y, x = kGreyPer * (blockIdx.x * kQThreads + threadIdx.x);
    if (x >= p.W) return;
    const int n = min(kGreyPer, p.W - x);
    const unsigned char* q = p.src + (size_t)y * p.pitch_src + 3 * (size_t)x;
    unsigned int b12[3 * kGreyPer];
    if (p.vec_in && n == kGreyPer) {                      // 12 bytes from a 4-byte aligned address
        const unsigned int* w = reinterpret_cast<const unsigned int*>(q);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned int v = w[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) b12[4 * i + k] = v >> (8 * k) & 255u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * kGreyPer; ++i) b12[i] = i < 3 * n ? q[i] : 0u;
    }
    unsigned int word = 0u;
#pragma unroll
    for (int k = 0; k < kGreyPer; ++k) {
        const unsigned int c0 = b12[3 * k], g = b12[3 * k + 1], c2 = b12[3 * k + 2];
        word |= grey_of_bgr(p.bgr ? c0 : c2, g, p.bgr ? c2 : c0) << (8 * k);
    }
    store_grey(p.dst + (size_t)y * p.pitch, x, n, word, p.vec_out);
}

// 16-bit samples: tensor2img_u8's rule with 65535 for 255 -- clamp, ONE fp32 multiply, round half to even -- into native uint16.
// It is its own quantiser, not the 8-bit one widened: k / 255 gives 257 k, and the high byte of a sample is not tensor2img_u8's byte.
__device__ __forceinline__ unsigned int quant16(float v) {
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (unsigned int)(int)__builtin_rintf(mul_rn(v, 65535.0f));
}
// the grey weights on three 16-bit values, in unsigned 32 bits: at most 65535 * 65536 + 32768 < 2^32; a neutral v, v, v gives v
__device__ __forceinline__ unsigned int grey16_of_bgr(unsigned int b, unsigned int g, unsigned int r) {
    return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

struct Quant16P {
    const float* src;             // [3][H][W] RGB
    unsigned short* dst;          // rows `pitch` BYTES apart (even): [H][W][3] B G R samples, or [H][W] grey ones
    size_t pitch;
    int H, W;
};

template <bool kGrey>
__global__ __launch_bounds__(kQThreads) void tensor2img_u16_kernel(Quant16P p) {
    const int y = blockIdx.y, x = blockIdx.x * kQThreads + threadIdx.x;
    if (x >= p.W) return;
    const size_t plane = (size_t)p.H * p.W, i = (size_t)y * p.W + x;
    const unsigned int r = quant16(p.src[i]), g = quant16(p.src[plane + i]), b = quant16(p.src[2 * plane + i]);
    unsigned short* out = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(p.dst) + (size_t)y * p.pitch);
    if constexpr (kGrey) {
        out[x] = (unsigned short)grey16_of_bgr(b, g, r);
    } else {
        out[3 * (size_t)x + 0] = (unsigned short)b;
        out[3 * (size_t)x + 1] = (unsigned short)g;
        out[3 * (size_t)x + 2] = (unsigned short)r;
    }
}

struct Grey16P {
    const unsigned short* src;    // rows pitch_src BYTES apart, three samples per pixel
    size_t pitch_src;
    int bgr;                      // the samples of a pixel are B G R, else R G B
    unsigned short* dst;          // rows `pitch` BYTES apart
    size_t pitch;
    int H, W;
};

__global__ __launch_bounds__(kQThreads) void grey_from_bgr_u16_kernel(Grey16P p) {
    const int y = blockIdx.y, x = blockIdx.x * kQThreads + threadIdx.x;
    if (x >= p.W) return;
    const unsigned short* q =
        reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.src) + (size_t)y * p.pitch_src) + 3 * (size_t)x;
    unsigned short* out = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(p.dst) + (size_t)y * p.pitch);
    const unsigned int c0 = q[0], g = q[1], c2 = q[2];
    out[x] = (unsigned short)grey16_of_bgr(p.bgr ? c0 : c2, g, p.bgr ? c2 : c0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct MetricsP {
    const unsigned char* a;
    const unsigned char* b;
    size_t pitch_a, pitch_b;
    int crop;                     // pixels removed on every side
    int Hc, Wc;                   // cropped size
    int ssim;                     // SSIM wanted (else the strips stop at their own rows and skip the filter)
    int gx, gy, nch;              // grid: strips of 4 x 64 columns, tiles of kTileH rows, evaluated channels
    double k[kTaps];              // normalised Gaussian window, sigma 1.5
    double* partial;              // [nch][gy][gx][kWaves][2] = (sum of squared differences, sum of the SSIM map)
    double* result;               // [3][4]
};

// y_of_bgr (index_math.h): mmcv.bgr2ycbcr(img / 255, y_only=True) * 255 in fp32, shared with niqe_f32.hip

// pixel (row, col) of the CROPPED image: the three bytes packed b | g << 8 | r << 16 (kY) or the byte of channel ch; 0 outside
template <bool kY>
__device__ __forceinline__ unsigned int load_px(const unsigned char* img, size_t pitch, int crop, int row, int col, int Wc, int ch) {
    if (col >= Wc) return 0u;
    const unsigned char* q = img + (size_t)(crop + row) * pitch + 3 * (size_t)(crop + col);
    if (kY) return (unsigned int)q[0] | (unsigned int)q[1] << 8 | (unsigned int)q[2] << 16;
    return (unsigned int)q[ch];
}

template <bool kY>
__device__ __forceinline__ float value_of(unsigned int raw) {
    return kY ? y_of_bgr(raw) : (float)raw;
}

__device__ __forceinline__ double ssim_value(double mx, double my, double xx, double yy, double xy) {
#pragma clang fp contract(off)
    const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
    const double sxx = xx - mx * mx, syy = yy - my * my, sxy = xy - mx * my;
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;                       // complete in lane 0
}

template <bool kY>
__global__ __launch_bounds__(kQThreads) void psnr_ssim_u8_kernel(MetricsP p) {
    __shared__ float rows[kWaves][2][kRowLds];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ch = blockIdx.z;
    const int c0 = (blockIdx.x * kWaves + wave) * kStripW, r0 = blockIdx.y * kTileH;
    const size_t slot = ((((size_t)ch * p.gy + blockIdx.y) * p.gx + blockIdx.x) * kWaves + wave) * 2;
    if (c0 >= p.Wc) {               // a strip right of the image: its slot is still written (nothing reads unwritten workspace)
        if (lane == 0) {
            p.partial[slot] = 0.0;
            p.partial[slot + 1] = 0.0;
        }
        return;
    }
    const int rows_own = min(kTileH, p.Hc - r0);
    const int rows_all = p.ssim ? min(kTileH + kHalo, p.Hc - r0) : rows_own;
    const int col = c0 + lane;
    const bool own_col = col < p.Wc, map_col = col < p.Wc - kHalo;
    float* rx = rows[wave][0];
    float* ry = rows[wave][1];

    double sse = 0.0, ssum = 0.0;
    double acc[5][kTaps];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < kTaps; ++j) acc[q][j] = 0.0;

    // lane l holds pixel c0 + l of the row, lanes 0..9 also pixel c0 + 64 + l; the next row is in flight while this one is filtered
    const int col2 = lane < kHalo ? c0 + kStripW + lane : p.Wc;
    unsigned int na0 = load_px<kY>(p.a, p.pitch_a, p.crop, r0, col, p.Wc, ch);
    unsigned int nb0 = load_px<kY>(p.b, p.pitch_b, p.crop, r0, col, p.Wc, ch);
    unsigned int na1 = load_px<kY>(p.a, p.pitch_a, p.crop, r0, col2, p.Wc, ch);
    unsigned int nb1 = load_px<kY>(p.b, p.pitch_b, p.crop, r0, col2, p.Wc, ch);

    for (int i0 = 0; i0 < rows_all; i0 += kTaps) {
#pragma unroll
        for (int u = 0; u < kTaps; ++u) {
            const int i = i0 + u;                       // row of the strip; i % 11 == u
            if (i >= rows_all) break;
            const float vx = value_of<kY>(na0), vy = value_of<kY>(nb0);
            const float vx2 = value_of<kY>(na1), vy2 = value_of<kY>(nb1);
            if (i + 1 < rows_all) {
                na0 = load_px<kY>(p.a, p.pitch_a, p.crop, r0 + i + 1, col, p.Wc, ch);
                nb0 = load_px<kY>(p.b, p.pitch_b, p.crop, r0 + i + 1, col, p.Wc, ch);
                na1 = load_px<kY>(p.a, p.pitch_a, p.crop, r0 + i + 1, col2, p.Wc, ch);
                nb1 = load_px<kY>(p.b, p.pitch_b, p.crop, r0 + i + 1, col2, p.Wc, ch);
            }
            if (i < rows_own && own_col) {
                const double d = (double)sub_rn(vx, vy);
                sse += d * d;
            }
            if (!p.ssim) continue;

            wave_lds_sync();                            // the previous row's reads are done
            rx[lane] = vx;
            ry[lane] = vy;
            if (lane < kHalo) {
                rx[kStripW + lane] = vx2;
                ry[kStripW + lane] = vy2;
            }
            wave_lds_sync();

            double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const double x = (double)rx[lane + t], y = (double)ry[lane + t], w = p.k[t];
                hx += w * x;
                hy += w * y;
                hxx += w * (x * x);
                hyy += w * (y * y);
                hxy += w * (x * y);
            }
            // row i is tap t of the map row i - t, whose sums live in ring slot (i - t) mod 11; tap 0 opens a slot
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const int s = (u - t + kTaps) % kTaps;
                const double w = p.k[t];
                if (t == 0) {
                    acc[0][s] = w * hx;
                    acc[1][s] = w * hy;
                    acc[2][s] = w * hxx;
                    acc[3][s] = w * hyy;
                    acc[4][s] = w * hxy;
                } else {
                    acc[0][s] += w * hx;
                    acc[1][s] += w * hy;
                    acc[2][s] += w * hxx;
                    acc[3][s] += w * hyy;
                    acc[4][s] += w * hxy;
                }
            }
            if (i >= kHalo && map_col) {                // map row i - 10 is complete (slot (u + 1) mod 11)
                const int s = (u + 1) % kTaps;
                ssum += ssim_value(acc[0][s], acc[1][s], acc[2][s], acc[3][s], acc[4][s]);
            }
        }
    }
    sse = wave_sum(sse);
    ssum = wave_sum(ssum);
    if (lane == 0) {
        p.partial[slot] = sse;
        p.partial[slot + 1] = ssum;
    }
}

// one workgroup: lane t adds the partials t, t + 256, ... of each channel in order, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(kQThreads) void psnr_ssim_finalize_kernel(MetricsP p) {
    __shared__ double red[2][kQThreads];
    const long per_ch = (long)p.gy * p.gx * kWaves;
    for (int ch = 0; ch < 3; ++ch) {
        double s0 = 0.0, s1 = 0.0;
        if (ch < p.nch)
            for (long i = threadIdx.x; i < per_ch; i += kQThreads) {
                s0 += p.partial[2 * ((size_t)ch * per_ch + i)];
                s1 += p.partial[2 * ((size_t)ch * per_ch + i) + 1];
            }
        red[0][threadIdx.x] = s0;
        red[1][threadIdx.x] = s1;
        __syncthreads();
        for (int off = kQThreads / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) {
                red[0][threadIdx.x] += red[0][threadIdx.x + off];
                red[1][threadIdx.x] += red[1][threadIdx.x + off];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const bool on = ch < p.nch;
            p.result[4 * ch + 0] = red[0][0];
            p.result[4 * ch + 1] = on ? (double)p.Hc * (double)p.Wc : 0.0;
            p.result[4 * ch + 2] = red[1][0];
            p.result[4 * ch + 3] = (on && p.ssim) ? (double)(p.Hc - kHalo) * (double)(p.Wc - kHalo) : 0.0;
        }
        __syncthreads();
    }
}

static inline bool metrics_geometry(int H, int W, int crop_border, int convert_to_y, int* Hc, int* Wc, int* gx, int* gy, int* nch) {
    if (H <= 0 || W <= 0 || H > kMaxDim || W > kMaxDim || crop_border < 0 || crop_border > kMaxDim) return false;
    *Hc = H - 2 * crop_border;
    *Wc = W - 2 * crop_border;
    if (*Hc <= 0 || *Wc <= 0) return false;
    *gx = ceil_div(*Wc, kWaves * kStripW);
    *gy = ceil_div(*Hc, kTileH);
    *nch = convert_to_y ? 1 : 3;
    return true;
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" int ciaosr_tensor2img_u8(const float* src_chw, int H, int W, unsigned char* dst_hwc, size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(src_chw && dst_hwc && H > 0 && W > 0 && dst_pitch >= 3 * (size_t)W);
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    QuantP p{src_chw, dst_hwc, dst_pitch, H, W, 0};
    p.vec = (W % 4 == 0) && aligned16(src_chw) && (reinterpret_cast<uintptr_t>(dst_hwc) & 3u) == 0 && (dst_pitch & 3u) == 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("tensor2img_u8", s);
    hipLaunchKernelGGL(tensor2img_u8_kernel, dim3(ceil_div(p.vec ? W / 4 : W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("tensor2img_u8");
}

static inline int bgra_vec(const unsigned char* dst, size_t pitch) {
    return (reinterpret_cast<uintptr_t>(dst) & 3u) == 0 && (pitch & 3u) == 0;
}

extern "C" int ciaosr_tensor2img_bgra_u8(const float* colour_chw, const float* alpha_chw, int H, int W, unsigned char* dst,
                                         size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(colour_chw && alpha_chw && dst && H > 0 && W > 0 && dst_pitch >= 4 * (size_t)W);
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    QuantAP p{colour_chw, alpha_chw, dst, dst_pitch, H, W, bgra_vec(dst, dst_pitch)};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("tensor2img_bgra_u8", s);
    hipLaunchKernelGGL(tensor2img_bgra_u8_kernel, dim3(ceil_div(W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("tensor2img_bgra_u8");
}

extern "C" int ciaosr_pack_bgra_u8(const unsigned char* bgr, size_t pitch, const unsigned char* grey_bgr, size_t pitch_grey, int H, int W,
                                   unsigned char* dst, size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(bgr && grey_bgr && dst && H > 0 && W > 0);
    CIAOSR_CHECK_ARG(pitch >= 3 * (size_t)W && pitch_grey >= 3 * (size_t)W && dst_pitch >= 4 * (size_t)W);
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    PackAP p{bgr, grey_bgr, pitch, pitch_grey, dst, dst_pitch, H, W, bgra_vec(dst, dst_pitch)};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("pack_bgra_u8", s);
    hipLaunchKernelGGL(pack_bgra_u8_kernel, dim3(ceil_div(W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("pack_bgra_u8");
}

extern "C" int ciaosr_tensor2img_grey_u8(const float* src_chw, int H, int W, unsigned char* dst, size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(src_chw && dst && H > 0 && W > 0 && dst_pitch >= (size_t)W);
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    QuantGP p{src_chw, dst, dst_pitch, H, W, (W % 4 == 0) && aligned16(src_chw), bgra_vec(dst, dst_pitch)};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("tensor2img_grey_u8", s);
    hipLaunchKernelGGL(tensor2img_grey_u8_kernel, dim3(ceil_div(ceil_div(W, kGreyPer), kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("tensor2img_grey_u8");
}

extern "C" int ciaosr_grey_from_bgr_u8(const unsigned char* bgr, size_t pitch, int bgr_flag, int H, int W, unsigned char* dst,
                                       size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(bgr && dst && H > 0 && W > 0 && pitch >= 3 * (size_t)W && dst_pitch >= (size_t)W && (bgr_flag == 0 || bgr_flag == 1));
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    GreyP p{bgr, pitch, bgr_flag, dst, dst_pitch, H, W, bgra_vec(bgr, pitch), bgra_vec(dst, dst_pitch)};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("grey_from_bgr_u8", s);
    hipLaunchKernelGGL(grey_from_bgr_u8_kernel, dim3(ceil_div(ceil_div(W, kGreyPer), kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("grey_from_bgr_u8");
}

static inline bool even2(const void* p, size_t pitch) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0 && (pitch & 1u) == 0; }

extern "C" int ciaosr_tensor2img_u16(const float* src_chw, int H, int W, unsigned short* dst_hwc, size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(src_chw && dst_hwc && H > 0 && W > 0 && dst_pitch >= 6 * (size_t)W && even2(dst_hwc, dst_pitch));
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    Quant16P p{src_chw, dst_hwc, dst_pitch, H, W};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("tensor2img_u16", s);
    hipLaunchKernelGGL(tensor2img_u16_kernel<false>, dim3(ceil_div(W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("tensor2img_u16");
}

extern "C" int ciaosr_tensor2img_grey_u16(const float* src_chw, int H, int W, unsigned short* dst, size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(src_chw && dst && H > 0 && W > 0 && dst_pitch >= 2 * (size_t)W && even2(dst, dst_pitch));
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    Quant16P p{src_chw, dst, dst_pitch, H, W};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("tensor2img_grey_u16", s);
    hipLaunchKernelGGL(tensor2img_u16_kernel<true>, dim3(ceil_div(W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("tensor2img_grey_u16");
}

extern "C" int ciaosr_grey_from_bgr_u16(const unsigned short* bgr, size_t pitch, int bgr_flag, int H, int W, unsigned short* dst,
                                        size_t dst_pitch, void* stream) {
    CIAOSR_CHECK_ARG(bgr && dst && H > 0 && W > 0 && pitch >= 6 * (size_t)W && dst_pitch >= 2 * (size_t)W && (bgr_flag == 0 || bgr_flag == 1));
    CIAOSR_CHECK_ARG(even2(bgr, pitch) && even2(dst, dst_pitch));
    if (H > 65535 || W > kMaxDim) return CIAOSR_ERR_UNSUPPORTED;        // one grid row per image row
    Grey16P p{bgr, pitch, bgr_flag, dst, dst_pitch, H, W};
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("grey_from_bgr_u16", s);
    hipLaunchKernelGGL(grey_from_bgr_u16_kernel, dim3(ceil_div(W, kQThreads), H), dim3(kQThreads), 0, s, p);
    return launch_status("grey_from_bgr_u16");
}

extern "C" size_t ciaosr_psnr_ssim_u8_workspace_bytes(int H, int W, int crop_border, int convert_to_y) {
    int Hc, Wc, gx, gy, nch;
    if (!metrics_geometry(H, W, crop_border, convert_to_y, &Hc, &Wc, &gx, &gy, &nch)) return 0;
    return (size_t)nch * gy * gx * kWaves * 2 * sizeof(double);
}

extern "C" int ciaosr_psnr_ssim_u8(const unsigned char* a, size_t pitch_a, const unsigned char* b, size_t pitch_b, int H, int W,
                                   int crop_border, int convert_to_y, int want, double* result, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(a && b && result && H > 0 && W > 0 && crop_border >= 0);
    CIAOSR_CHECK_ARG(want >= 1 && want <= 3 && (convert_to_y == 0 || convert_to_y == 1));
    CIAOSR_CHECK_ARG(W <= kMaxDim && pitch_a >= 3 * (size_t)W && pitch_b >= 3 * (size_t)W);
    CIAOSR_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(result) & 7u) == 0);
    int Hc, Wc, gx, gy, nch;
    if (!metrics_geometry(H, W, crop_border, convert_to_y, &Hc, &Wc, &gx, &gy, &nch)) return CIAOSR_ERR_UNSUPPORTED;
    const int ssim = (want & CIAOSR_METRIC_SSIM) ? 1 : 0;
    if (ssim && (Hc < kTaps || Wc < kTaps)) return CIAOSR_ERR_UNSUPPORTED;     // no 11 x 11 window fits
    if (gy > 65535) return CIAOSR_ERR_UNSUPPORTED;
    if (workspace_bytes < ciaosr_psnr_ssim_u8_workspace_bytes(H, W, crop_border, convert_to_y)) return CIAOSR_ERR_WORKSPACE;
    MetricsP p{a, b, pitch_a, pitch_b, crop_border, Hc, Wc, ssim, gx, gy, nch, {}, (double*)workspace, result};
    double sum = 0.0;
    for (int t = 0; t < kTaps; ++t) {
        p.k[t] = std::exp(-((t - 5.0) * (t - 5.0)) / (2 * 1.5 * 1.5));
        sum += p.k[t];
    }
    for (int t = 0; t < kTaps; ++t) p.k[t] /= sum;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope prof("psnr_ssim_u8", s);
        if (convert_to_y)
            hipLaunchKernelGGL(psnr_ssim_u8_kernel<true>, dim3(gx, gy, nch), dim3(kQThreads), 0, s, p);
        else
            hipLaunchKernelGGL(psnr_ssim_u8_kernel<false>, dim3(gx, gy, nch), dim3(kQThreads), 0, s, p);
        int rc = launch_status("psnr_ssim_u8");
        if (rc) return rc;
    }
    ProfScope prof("psnr_ssim_finalize", s);
    hipLaunchKernelGGL(psnr_ssim_finalize_kernel, dim3(1), dim3(kQThreads), 0, s, p);
    return launch_status("psnr_ssim_finalize");
}
