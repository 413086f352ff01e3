// The eight symmetries of the square on [planes][H][W] fp32 images, and the self-ensemble accumulation through their inverses
// (include/ciaosr_hip.h, "self-ensemble").  Pure data movement.  One index map serves both entries: element (y, x) of the image in the
// ORIGINAL orientation [H][W] and element (yf, xf) -- yf = k & 2 ? H - 1 - y : y, xf = k & 1 ? W - 1 - x : x -- of the image in MEMBER
// orientation are the same pixel; the member image is [H][W] and holds it at [yf][xf] for k < 4, and is [W][H] and holds it at [xf][yf]
// for k >= 4.  ciaosr_dihedral_f32 reads the original side and writes the member side (T_k), ciaosr_dihedral_accum_f32 reads the member
// side and adds into the original side (U_k); a flip is its own inverse, so no second map exists.
//   k < 4:  one workgroup per row segment of 1024 elements; a wave reads 64 consecutive floats and writes 64 consecutive floats
//           (backwards under a column flip).  32-bit accesses only: results cannot depend on W % 4.
//   k >= 4: 64 x 64 tiles through LDS with a row pitch of 65 dwords.  Both global sides run along rows: the original side 64 lanes
//           along x, the member side 64 lanes along y (its row direction); the LDS side of the latter is a column access, lane l at
//           dword 65 l + c -> bank (l + c) % 64, conflict-free (at pitch 64 it would be 64-way).
// The workgroups of a launch are flattened into blockIdx.x (planes x rows x segments, planes x tile rows x tile columns), counted in
// size_t and refused beyond 2^31 - 1; every element offset is size_t.
#include <climits>
#include <cmath>

#include "common.h"

namespace ciaosr {

constexpr int kDihThreads = 256;
constexpr int kDihSeg = 4 * kDihThreads;      // elements of a row one workgroup of the flip kernels moves
constexpr int kDihTile = 64, kDihPitch = kDihTile + 1;

struct DihP { int H, W, fy, fx; unsigned segs, tiles_x, tiles_y; };

// the value the original side ends with: `v` is the member's pixel
template <bool kAccum>
__device__ __forceinline__ void dih_put(float* __restrict__ orig, size_t at, float v, int first, float divisor) {
    if (kAccum) {
        if (!first) v = orig[at] + v;             // one rounded add; `first`: acc is not read
        if (divisor > 0.0f) v = __fdiv_rn(v, divisor);
    }
    orig[at] = v;
}

// k < 4.  kAccum = false: member[yf][xf] = orig[y][x].  kAccum = true: orig[y][x] = (first ? 0 : orig[y][x]) + member[yf][xf].
template <bool kAccum>
__global__ __launch_bounds__(kDihThreads) void dihedral_flip_kernel(DihP p, float* __restrict__ orig, float* __restrict__ member, int first,
                                                                     float divisor) {
    const unsigned row = blockIdx.x / p.segs, seg = blockIdx.x - row * p.segs;          // uniform over the workgroup
    const unsigned plane = row / (unsigned)p.H;
    const int y = (int)(row - plane * (unsigned)p.H);
    const int yf = p.fy ? p.H - 1 - y : y;
    const size_t o_row = ((size_t)plane * p.H + y) * p.W, m_row = ((size_t)plane * p.H + yf) * p.W;
#pragma unroll
    for (int i = 0; i < kDihSeg / kDihThreads; ++i) {
        const long x = (long)seg * kDihSeg + i * kDihThreads + threadIdx.x;
        if (x < p.W) {
            const long xf = p.fx ? p.W - 1 - x : x;
            if (kAccum)
                dih_put<true>(orig, o_row + x, member[m_row + xf], first, divisor);
            else
                member[m_row + xf] = orig[o_row + x];
        }
    }
}

// k >= 4: the member image is [W][H], member[xf][yf] is orig[y][x].  Workgroup = one 64 x 64 tile of the original image.
template <bool kAccum>
__global__ __launch_bounds__(kDihThreads) void dihedral_transpose_kernel(DihP p, float* __restrict__ orig, float* __restrict__ member,
                                                                          int first, float divisor) {
    __shared__ float s[kDihTile * kDihPitch];                                           // s[r * pitch + c]: pixel (y0 + r, x0 + c)
    const unsigned per_plane = p.tiles_y * p.tiles_x;
    const unsigned plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;   // uniform over the workgroup
    const unsigned ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int y0 = (int)ty * kDihTile, x0 = (int)tx * kDihTile;
    const int lane = threadIdx.x & (kDihTile - 1), w = threadIdx.x / kDihTile;           // 4 waves, each a line of 64 per step
    const size_t base = (size_t)plane * p.H * p.W;
    // the member side: lane along y (the member's row direction), one member row xf per step
    const int ym = y0 + lane;
    const int yf = p.fy ? p.H - 1 - ym : ym;
    if (kAccum) {
        for (int c = w; c < kDihTile; c += kDihThreads / kDihTile) {
            const int x = x0 + c;
            if (x < p.W && ym < p.H) s[lane * kDihPitch + c] = member[base + (size_t)(p.fx ? p.W - 1 - x : x) * p.H + yf];
        }
    } else {
        for (int r = w; r < kDihTile; r += kDihThreads / kDihTile) {
            const int y = y0 + r, x = x0 + lane;
            if (y < p.H && x < p.W) s[r * kDihPitch + lane] = orig[base + (size_t)y * p.W + x];
        }
    }
    __syncthreads();
    if (kAccum) {
        for (int r = w; r < kDihTile; r += kDihThreads / kDihTile) {
            const int y = y0 + r, x = x0 + lane;
            if (y < p.H && x < p.W) dih_put<true>(orig, base + (size_t)y * p.W + x, s[r * kDihPitch + lane], first, divisor);
        }
    } else {
        for (int c = w; c < kDihTile; c += kDihThreads / kDihTile) {
            const int x = x0 + c;
            if (x < p.W && ym < p.H) member[base + (size_t)(p.fx ? p.W - 1 - x : x) * p.H + yf] = s[lane * kDihPitch + c];
        }
    }
}

template <bool kAccum>
static int dihedral_launch(float* orig, float* member, int planes, int H, int W, int k, int first, float divisor, hipStream_t s) {
    DihP p{H, W, (k >> 1) & 1, k & 1, (unsigned)ceil_div(W, kDihSeg), (unsigned)ceil_div(W, kDihTile), (unsigned)ceil_div(H, kDihTile)};
    const bool tr = (k & 4) != 0;
    const size_t blocks = tr ? (size_t)planes * p.tiles_y * p.tiles_x : (size_t)planes * (size_t)H * p.segs;
    if (blocks > (size_t)INT_MAX) return CIAOSR_ERR_UNSUPPORTED;
    ProfScope prof(kAccum ? (tr ? "dihedral_accum_t" : "dihedral_accum") : (tr ? "dihedral_t" : "dihedral"), s);
    if (tr)
        hipLaunchKernelGGL(dihedral_transpose_kernel<kAccum>, dim3((unsigned)blocks), dim3(kDihThreads), 0, s, p, orig, member, first, divisor);
    else
        hipLaunchKernelGGL(dihedral_flip_kernel<kAccum>, dim3((unsigned)blocks), dim3(kDihThreads), 0, s, p, orig, member, first, divisor);
    return launch_status(kAccum ? "dihedral_accum" : "dihedral");
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" int ciaosr_dihedral_f32(const float* src, float* dst, int planes, int H, int W, int k, void* stream) {
    CIAOSR_CHECK_ARG(src && dst && src != dst && planes > 0 && H > 0 && W > 0 && k >= 0 && k <= 7);
    return dihedral_launch<false>(const_cast<float*>(src), dst, planes, H, W, k, 0, 0.0f, (hipStream_t)stream);
}

extern "C" int ciaosr_dihedral_accum_f32(float* acc, const float* src, int planes, int H, int W, int k, int first, float divisor,
                                         void* stream) {
    CIAOSR_CHECK_ARG(acc && src && acc != src && planes > 0 && H > 0 && W > 0 && k >= 0 && k <= 7);
    CIAOSR_CHECK_ARG(std::isfinite(divisor) && divisor >= 0.0f);
    return dihedral_launch<true>(acc, const_cast<float*>(src), planes, H, W, k, first != 0, divisor, (hipStream_t)stream);
}
