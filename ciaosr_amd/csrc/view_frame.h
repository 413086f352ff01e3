// What view_ops.hip (affine views) and warp_ops.hip (homographies and coordinate maps) share: everything that follows the LR position of a
// query -- the frame a query is sorted into, its membership test and its coordinate in the frame, the geometry of the count / select
// workgroups, the scan of a tile's per-workgroup counts -- the host checks of a frame, and the fill value both files' finishing kernels
// write where no tile claimed a query.  Where the position comes from is each file's own.
#pragma once
#include <climits>
#include <cmath>

#include "common.h"

namespace ciaosr {

// A block of kViewThreads threads owns kViewChunk consecutive queries, in kViewRounds rounds of one query per thread: query
// q = block * kViewChunk + round * kViewThreads + thread, so (round, wave, lane) in lexicographic order is increasing q.
constexpr int kViewThreads = 256, kViewRounds = 4, kViewChunk = kViewThreads * kViewRounds, kViewWaves = kViewThreads / kWave;
constexpr int kViewTileBatch = 256;        // tiles whose per-wave counts one pass of the count kernel keeps in LDS

struct ViewFrame { double y0, x0, y1, x1, th, tw; };       // [y0, y1) x [x0, x1) in LR pixel units, y1 = y0 + th (exact: integers)

__device__ __forceinline__ bool view_member(double y, double x, const ViewFrame& f) {
    return y >= f.y0 && y < f.y1 && x >= f.x0 && x < f.x1;           // NaN: no member
}
__device__ __forceinline__ float2 view_coord(double y, double x, const ViewFrame& f) {
#pragma clang fp contract(off)
    return make_float2((float)(((y - f.y0) / f.th) * 2.0 - 1.0), (float)(((x - f.x0) / f.tw) * 2.0 - 1.0));
}
__device__ __forceinline__ ViewFrame view_frame(int y0, int x0, int th, int tw) {
    return ViewFrame{(double)y0, (double)x0, (double)y0 + (double)th, (double)x0 + (double)tw, (double)th, (double)tw};
}

// One wave: row[*] (a tile's per-block counts) becomes its exclusive scan over the blocks, *total their sum
__device__ __forceinline__ void view_scan_row(int* __restrict__ row, int n_blocks, int* __restrict__ total) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += kWave) {
        const int b = b0 + lane;
        const int v = b < n_blocks ? row[b] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += up;
        }
        if (b < n_blocks) row[b] = carry + incl - v;
        carry += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) *total = carry;
}

static inline int view_grid(long n) {
    const long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

static inline bool frame_ok(const int* f) { return f && f[0] >= 0 && f[1] >= 0 && f[2] > 0 && f[3] > 0 && f[0] <= INT_MAX - f[2] && f[1] <= INT_MAX - f[3]; }
static inline ViewFrame frame_of(const int* f) {
    return ViewFrame{(double)f[0], (double)f[1], (double)f[0] + (double)f[2], (double)f[1] + (double)f[3], (double)f[2], (double)f[3]};
}
static inline int view_blocks(long Q) { return (int)((Q + kViewChunk - 1) / kViewChunk); }

struct Fill3 { float v[3]; };

// The value v with clamp(v * std + mean, 0, 1) == fill in ciaosr_denorm_clamp_f32's arithmetic (two rounded fp32 operations), searched
// among the neighbours of (fill - mean) / std; where no fp32 value maps onto fill, the one that comes nearest
static inline float fill_preimage(float fill, float mean, float std_) {
#pragma clang fp contract(off)
    float best = (float)(((double)fill - (double)mean) / (double)std_);
    float lo = best, hi = best;
    double best_err = HUGE_VAL;
    float pick = best;
    for (int k = 0; k <= 8; ++k) {
        const float cand[2] = {lo, hi};
        for (int s = 0; s < 2; ++s) {
            volatile float prod = cand[s] * std_;
            volatile float sum = prod + mean;
            const float got = fminf(fmaxf(sum, 0.f), 1.f);
            const double err = std::fabs((double)got - (double)fill);
            if (err < best_err) { best_err = err; pick = cand[s]; }
        }
        if (best_err == 0.0) break;
        lo = std::nextafterf(lo, -HUGE_VALF);
        hi = std::nextafterf(hi, HUGE_VALF);
    }
    return pick;
}

}  // namespace ciaosr
