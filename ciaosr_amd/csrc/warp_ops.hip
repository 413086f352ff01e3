// Warps of an encoded scene (include/ciaosr_hip.h, "warps"): the queries of an Hv x Wv output grid whose LR positions come from a
// homography (nine doubles, by value) or from a coordinate map (one (y_lr, x_lr) pair of doubles per output pixel, on the device), sorted
// into the LR tiles exactly as a view's are.  Three roles -- count, select, the whole grid's coordinates in one frame -- in view_ops.hip's
// scheme: tile membership is counted with wave ballots, a block's members are placed at (exclusive scan of the per-block counts) + (rank
// inside the block), no atomics, every result bitwise repeatable.  Everything after the LR position is view_frame.h's, shared with the
// views; blend and finalize are the views' own entries.  The second half of the file is the per-pixel warps: the same roles with a
// footprint, and hence a cell, per output pixel (Jacobian of the homography, differences of the map, or a device tensor), and the entry
// that writes the footprints themselves.  The last part is the area-sampled warps: a per-pixel homography warp that gives a pixel whose
// raw footprint exceeds the range n_y x n_x samples -- a per-pixel sample table, count and select over the samples, and the resolve that
// averages a pixel's finished samples.
#include <climits>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "index_math.h"
#include "view_frame.h"

namespace ciaosr {

// map == nullptr: the homography h (y first); else map[q] = (y_lr, x_lr), 16-byte aligned
struct WarpP { double h[9]; const double* map; int Hv, Wv; long Q; };

// LR position of the centre of output pixel q.  Homography: fp64, every operation rounded on its own, IEEE division -- with the last row
// (0, 0, 1) the denominator is exactly 1 and the point is view_point's, bit for bit.  Map: one aligned 16-byte load.
template <bool kMap>
__device__ __forceinline__ void warp_point(const WarpP& p, long q, double& y, double& x) {
#pragma clang fp contract(off)
    if constexpr (kMap) {
        const double2 yx = reinterpret_cast<const double2*>(p.map)[q];
        y = yx.x;
        x = yx.y;
    } else {
        const int i = (int)(q / p.Wv), j = (int)(q - (long)i * p.Wv);
        const double v = (double)i + 0.5, u = (double)j + 0.5;
        const double Y = (p.h[0] * v + p.h[1] * u) + p.h[2];
        const double X = (p.h[3] * v + p.h[4] * u) + p.h[5];
        const double D = (p.h[6] * v + p.h[7] * u) + p.h[8];
        y = Y / D;
        x = X / D;
    }
}

// part[t * n_blocks + b] = members of tile t among block b's queries.  Per tile one ballot per round and wave; lane 0 of each wave owns
// its LDS slot, so nothing is added concurrently.
template <bool kMap>
__global__ __launch_bounds__(kViewThreads) void warp_count_kernel(WarpP p, const int* __restrict__ tiles, int n_tiles, int n_blocks,
                                                                  int* __restrict__ part) {
    __shared__ int s_cnt[kViewTileBatch][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, block = (int)blockIdx.x;
    const long q0 = (long)block * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds];
    bool live[kViewRounds];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        live[r] = q < p.Q;
        y[r] = x[r] = 0.0;
        if (live[r]) warp_point<kMap>(p, q, y[r], x[r]);
    }
    for (int t0 = 0; t0 < n_tiles; t0 += kViewTileBatch) {
        const int nt = min(kViewTileBatch, n_tiles - t0);
        for (int t = 0; t < nt; ++t) {
            const int4 tl = reinterpret_cast<const int4*>(tiles)[t0 + t];          // (y0, x0, th, tw): the same for every lane
            const ViewFrame f = view_frame(tl.x, tl.y, tl.z, tl.w);
            int c = 0;
#pragma unroll
            for (int r = 0; r < kViewRounds; ++r) c += __popcll(__ballot(live[r] && view_member(y[r], x[r], f)));
            if (lane == 0) s_cnt[t][wave] = c;
        }
        __syncthreads();
        for (int t = tid; t < nt; t += kViewThreads) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < kViewWaves; ++w) c += s_cnt[t][w];
            part[(size_t)(t0 + t) * n_blocks + block] = c;
        }
        __syncthreads();
    }
}

// One wave per tile: part[t][*] becomes its exclusive scan over the blocks, counts[t] the total
__global__ __launch_bounds__(kWave) void warp_scan_kernel(int* __restrict__ part, int n_blocks, int* __restrict__ counts) {
    view_scan_row(part + (size_t)blockIdx.x * n_blocks, n_blocks, counts + blockIdx.x);
}

// The members of one tile in increasing q: position = offs[block] + members of the block before this one
template <bool kMap>
__global__ __launch_bounds__(kViewThreads) void warp_select_kernel(WarpP p, ViewFrame f, float2 cellv, const int* __restrict__ offs, long n,
                                                                   int* __restrict__ q_index, float* __restrict__ coord,
                                                                   float* __restrict__ cell) {
    __shared__ int s_cnt[kViewRounds][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long q0 = (long)blockIdx.x * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds];
    int rank[kViewRounds];                     // among the members of the same round and wave, -1: no member
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        bool m = false;
        y[r] = x[r] = 0.0;
        if (q < p.Q) {
            warp_point<kMap>(p, q, y[r], x[r]);
            m = view_member(y[r], x[r], f);
        }
        const unsigned long long mask = __ballot(m);
        rank[r] = m ? __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        if (lane == 0) s_cnt[r][wave] = __popcll(mask);
    }
    __syncthreads();
    long pos = offs[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
#pragma unroll
        for (int w = 0; w < kViewWaves; ++w) {
            if (w == wave && rank[r] >= 0) {
                const long o = pos + rank[r];
                if (o >= 0 && o < n) {         // holds whenever offs / n come from the count of the same warp and tile
                    q_index[o] = (int)(q0 + (long)r * kViewThreads);
                    reinterpret_cast<float2*>(coord)[o] = view_coord(y[r], x[r], f);
                    reinterpret_cast<float2*>(cell)[o] = cellv;
                }
            }
            pos += s_cnt[r][w];
        }
    }
}

// The whole grid in one frame, members or not (a non-finite map entry gives a non-finite coordinate: the caller walks a grid only where
// the count says that the frame owns every query)
template <bool kMap>
__global__ void warp_coord_cell_kernel(WarpP p, ViewFrame f, float2 cellv, float* __restrict__ coord, float* __restrict__ cell) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < p.Q; q += (long)gridDim.x * blockDim.x) {
        double y, x;
        warp_point<kMap>(p, q, y, x);
        reinterpret_cast<float2*>(coord)[q] = view_coord(y, x, f);
        reinterpret_cast<float2*>(cell)[q] = cellv;
    }
}

// exactly one point source; a finite homography whose denominator is positive at the four corners of the output grid (it is affine in
// (v, u), so it is positive on all of it), or a 16-byte aligned map; a finite, positive footprint
static inline bool warp_ok(const double* h9, const double* map, const double* fp, int Hv, int Wv) {
    if ((h9 != nullptr) == (map != nullptr) || !fp || Hv <= 0 || Wv <= 0 || (long)Hv * Wv > (long)INT_MAX) return false;
    if (!(std::isfinite(fp[0]) && std::isfinite(fp[1]) && fp[0] > 0.0 && fp[1] > 0.0)) return false;
    if (map) return aligned16(map);
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(h9[i])) return false;
    for (int c = 0; c < 4; ++c) {
        const double v = (c & 1) ? (double)Hv : 0.0, u = (c & 2) ? (double)Wv : 0.0;
        if (!((h9[6] * v + h9[7] * u) + h9[8] > 0.0)) return false;
    }
    return true;
}
static inline WarpP warp_p(const double* h9, const double* map, int Hv, int Wv) {
    WarpP p = {};
    if (h9)
        for (int i = 0; i < 9; ++i) p.h[i] = h9[i];
    p.map = map;
    p.Hv = Hv;
    p.Wv = Wv;
    p.Q = (long)Hv * Wv;
    return p;
}
// the warp's cell in a th x tw frame: view_cell's operations on the footprint
static inline float2 warp_cell(const double* fp, const int* f) {
    return make_float2((float)(fp[0] * 2.0 / (double)f[2]), (float)(fp[1] * 2.0 / (double)f[3]));
}

// ---- per-pixel warps (include/ciaosr_hip.h, "per-pixel warps"): the footprint is a function of the output pixel ----------------------
// The same three roles with the same workgroups, scan and layout; membership is the warp's AND "has a footprint", and select and the
// whole grid write one cell per query.  kMode: 1 the Jacobian of the homography, 2 differences of the map, 3 a device tensor.
constexpr int kFpJacobian = 1, kFpDifferences = 2, kFpTensor = 3;
struct WarpFp { double lo, hi; const double* tensor; };

// d(p)/d(grid step) from the neighbours `m` (before) and `n` (after) of the centre value `c`; a neighbour outside the grid arrives as NaN
__device__ __forceinline__ bool warp_diff(double m, double c, double n, double& d) {
#pragma clang fp contract(off)
    const bool fm = isfinite(m), fn = isfinite(n);
    if (fm && fn) d = (n - m) * 0.5;
    else if (fn) d = n - c;
    else if (fm) d = c - m;
    else return false;
    return true;
}

// The raw footprint (g_y, g_x) of query q, whose LR position is (y, x); false: the pixel has none, or a component is NaN.  fp64, every
// operation rounded on its own; sqrt of the rounded sum, IEEE.
template <bool kMap, int kMode>
__device__ __forceinline__ bool warp_raw_footprint(const WarpP& p, const WarpFp& s, long q, double y, double x, double& gy, double& gx) {
#pragma clang fp contract(off)
    if constexpr (kMode == kFpJacobian) {
        const int i = (int)(q / p.Wv), j = (int)(q - (long)i * p.Wv);
        const double v = (double)i + 0.5, u = (double)j + 0.5;
        const double D = (p.h[6] * v + p.h[7] * u) + p.h[8];
        const double ay = (p.h[0] - y * p.h[6]) / D, by = (p.h[1] - y * p.h[7]) / D;
        const double ax = (p.h[3] - x * p.h[6]) / D, bx = (p.h[4] - x * p.h[7]) / D;
        gy = sqrt(ay * ay + by * by);
        gx = sqrt(ax * ax + bx * bx);
    } else if constexpr (kMode == kFpDifferences) {
        const int i = (int)(q / p.Wv), j = (int)(q - (long)i * p.Wv);
        const double2* m = reinterpret_cast<const double2*>(p.map);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double2 none = make_double2(nan, nan);
        const double2 up = i > 0 ? m[q - p.Wv] : none, down = i + 1 < p.Hv ? m[q + p.Wv] : none;         // inside [0, Q): guarded
        const double2 left = j > 0 ? m[q - 1] : none, right = j + 1 < p.Wv ? m[q + 1] : none;
        double dvy, duy, dvx, dux;
        if (!warp_diff(up.x, y, down.x, dvy) || !warp_diff(left.x, y, right.x, duy)) return false;
        if (!warp_diff(up.y, x, down.y, dvx) || !warp_diff(left.y, x, right.y, dux)) return false;
        gy = sqrt(dvy * dvy + duy * duy);
        gx = sqrt(dvx * dvx + dux * dux);
    } else {
        const double2 g = reinterpret_cast<const double2*>(s.tensor)[q];
        gy = g.x;
        gx = g.y;
    }
    return !(gy != gy || gx != gx);
}

// The clamped footprint (f_y, f_x) of query q, whose LR position is (y, x); false: the pixel has none
template <bool kMap, int kMode>
__device__ __forceinline__ bool warp_footprint(const WarpP& p, const WarpFp& s, long q, double y, double x, double& fy, double& fx) {
    double gy, gx;
    if (!warp_raw_footprint<kMap, kMode>(p, s, q, y, x, gy, gx)) return false;
    fy = gy < s.lo ? s.lo : (gy > s.hi ? s.hi : gy);
    fx = gx < s.lo ? s.lo : (gx > s.hi ? s.hi : gx);
    return true;
}

// the cell of a member with footprint (fy, fx) in the frame: warp_cell's operations
__device__ __forceinline__ float2 warp_cell_of(double fy, double fx, const ViewFrame& f) {
#pragma clang fp contract(off)
    return make_float2((float)(fy * 2.0 / f.th), (float)(fx * 2.0 / f.tw));
}

// warp_count_kernel with the footprint in the membership
template <bool kMap, int kMode>
__global__ __launch_bounds__(kViewThreads) void warp_pp_count_kernel(WarpP p, WarpFp s, const int* __restrict__ tiles, int n_tiles,
                                                                     int n_blocks, int* __restrict__ part) {
    __shared__ int s_cnt[kViewTileBatch][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, block = (int)blockIdx.x;
    const long q0 = (long)block * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds];
    bool live[kViewRounds];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        live[r] = q < p.Q;
        y[r] = x[r] = 0.0;
        if (live[r]) {
            double fy, fx;
            warp_point<kMap>(p, q, y[r], x[r]);
            live[r] = warp_footprint<kMap, kMode>(p, s, q, y[r], x[r], fy, fx);
        }
    }
    for (int t0 = 0; t0 < n_tiles; t0 += kViewTileBatch) {
        const int nt = min(kViewTileBatch, n_tiles - t0);
        for (int t = 0; t < nt; ++t) {
            const int4 tl = reinterpret_cast<const int4*>(tiles)[t0 + t];
            const ViewFrame f = view_frame(tl.x, tl.y, tl.z, tl.w);
            int c = 0;
#pragma unroll
            for (int r = 0; r < kViewRounds; ++r) c += __popcll(__ballot(live[r] && view_member(y[r], x[r], f)));
            if (lane == 0) s_cnt[t][wave] = c;
        }
        __syncthreads();
        for (int t = tid; t < nt; t += kViewThreads) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < kViewWaves; ++w) c += s_cnt[t][w];
            part[(size_t)(t0 + t) * n_blocks + block] = c;
        }
        __syncthreads();
    }
}

// warp_select_kernel with the footprint in the membership and the member's own cell
template <bool kMap, int kMode>
__global__ __launch_bounds__(kViewThreads) void warp_pp_select_kernel(WarpP p, WarpFp s, ViewFrame f, const int* __restrict__ offs, long n,
                                                                      int* __restrict__ q_index, float* __restrict__ coord,
                                                                      float* __restrict__ cell) {
    __shared__ int s_cnt[kViewRounds][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long q0 = (long)blockIdx.x * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds], fy[kViewRounds], fx[kViewRounds];
    int rank[kViewRounds];                     // among the members of the same round and wave, -1: no member
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        bool m = false;
        y[r] = x[r] = fy[r] = fx[r] = 0.0;
        if (q < p.Q) {
            warp_point<kMap>(p, q, y[r], x[r]);
            m = view_member(y[r], x[r], f) && warp_footprint<kMap, kMode>(p, s, q, y[r], x[r], fy[r], fx[r]);
        }
        const unsigned long long mask = __ballot(m);
        rank[r] = m ? __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        if (lane == 0) s_cnt[r][wave] = __popcll(mask);
    }
    __syncthreads();
    long pos = offs[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
#pragma unroll
        for (int w = 0; w < kViewWaves; ++w) {
            if (w == wave && rank[r] >= 0) {
                const long o = pos + rank[r];
                if (o >= 0 && o < n) {         // holds whenever offs / n come from the count of the same warp and tile
                    q_index[o] = (int)(q0 + (long)r * kViewThreads);
                    reinterpret_cast<float2*>(coord)[o] = view_coord(y[r], x[r], f);
                    reinterpret_cast<float2*>(cell)[o] = warp_cell_of(fy[r], fx[r], f);
                }
            }
            pos += s_cnt[r][w];
        }
    }
}

// The whole grid in one frame, members or not: a query without a footprint gets a NaN cell (the caller walks a grid only where the count
// says that the frame owns every query, and then every query has one)
template <bool kMap, int kMode>
__global__ void warp_pp_coord_cell_kernel(WarpP p, WarpFp s, ViewFrame f, float* __restrict__ coord, float* __restrict__ cell) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < p.Q; q += (long)gridDim.x * blockDim.x) {
        double y, x, fy, fx;
        warp_point<kMap>(p, q, y, x);
        const bool has = warp_footprint<kMap, kMode>(p, s, q, y, x, fy, fx);
        const float nan = __int_as_float(0x7fc00000);
        reinterpret_cast<float2*>(coord)[q] = view_coord(y, x, f);
        reinterpret_cast<float2*>(cell)[q] = has ? warp_cell_of(fy, fx, f) : make_float2(nan, nan);
    }
}

// out[q] = the clamped (f_y, f_x), NaN where the pixel has none: one 16-byte store per query
template <bool kMap, int kMode>
__global__ void warp_footprints_kernel(WarpP p, WarpFp s, double* __restrict__ out) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < p.Q; q += (long)gridDim.x * blockDim.x) {
        double y = 0.0, x = 0.0, fy, fx;
        if constexpr (kMode != kFpTensor) warp_point<kMap>(p, q, y, x);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (!warp_footprint<kMap, kMode>(p, s, q, y, x, fy, fx)) fy = fx = nan;
        reinterpret_cast<double2*>(out)[q] = make_double2(fy, fx);
    }
}

// a point source as warp_ok has it; a mode that fits the source (the Jacobian needs the homography, differences the map and two pixels
// along each grid axis, a tensor its aligned pointer); a finite range 0 < lo <= hi
static inline bool warp_pp_ok(const double* h9, const double* map, int mode, const double* range, const double* tensor, int Hv, int Wv) {
    const double one[2] = {1.0, 1.0};
    if (!warp_ok(h9, map, one, Hv, Wv) || !range) return false;
    if (!(std::isfinite(range[0]) && std::isfinite(range[1]) && range[0] > 0.0 && range[0] <= range[1])) return false;
    if (mode == kFpJacobian) return h9 != nullptr;
    if (mode == kFpDifferences) return map != nullptr && Hv > 1 && Wv > 1;
    return mode == kFpTensor && tensor && aligned16(tensor);
}
static inline WarpFp warp_fp(const double* range, const double* tensor) { return WarpFp{range[0], range[1], tensor}; }

// f(kMap, kMode) as compile-time constants, for the combinations warp_pp_ok lets through
template <class F>
static inline void warp_pp_dispatch(bool map, int mode, F&& f) {
    if (mode == kFpJacobian) f(std::false_type{}, std::integral_constant<int, kFpJacobian>{});
    else if (mode == kFpDifferences) f(std::true_type{}, std::integral_constant<int, kFpDifferences>{});
    else if (map) f(std::true_type{}, std::integral_constant<int, kFpTensor>{});
    else f(std::false_type{}, std::integral_constant<int, kFpTensor>{});
}

// ---- area-sampled warps (include/ciaosr_hip.h, "area-sampled warps"): n_y x n_x samples per output pixel where the warp minifies ----------
// Two steps.  The TABLE, one thread per output pixel: the sample count of each axis, the footprint its samples share, and `first`, the
// exclusive prefix sum of n_y n_x over the pixels -- counts are not 0 / 1 here, so a wave scans them with shuffles, a block adds its waves'
// totals in (round, wave) order, and one wave scans the blocks' sums.  Then count and select are the file's own kernels with the SAMPLE in
// the place of the query: a block owns kViewChunk consecutive sample ids, a sample finds its pixel by bisection of `first`, membership is
// one bit per thread, so the ballot ranks and the per-block partials serve unchanged and a tile's list comes out in increasing sample id.
// S is only known on the device when the count is launched: it launches the blocks of the largest possible S, and those past S leave.
struct AreaT { const double2* fp; const int* first; const int* nn; };          // per pixel: (f_y, f_x); first [Q + 1]; n_y | n_x << 8

__device__ __forceinline__ int area_n(double g, double hi, int N) {
#pragma clang fp contract(off)
    int n = 1;
    while (n < N && g > hi * (double)n) n *= 2;       // hi * n and g / n are exact: n is a power of two
    return n;
}

// block-relative `first`, the samples' footprint and the packed counts of every pixel of the block; blk[block] = the block's samples,
// blk[n_blocks + block] = its pixels with exactly one sample
template <int kMode>
__global__ __launch_bounds__(kViewThreads) void area_table_kernel(WarpP p, WarpFp s, int N, double2* __restrict__ fp, int* __restrict__ first,
                                                                  int* __restrict__ nn, int* __restrict__ blk, int n_blocks) {
#pragma clang fp contract(off)
    __shared__ int s_tot[kViewRounds][kViewWaves], s_one[kViewRounds][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long q0 = (long)blockIdx.x * kViewChunk + tid;
    int excl[kViewRounds];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        int cnt = 0;
        if (q < p.Q) {
            double y = 0.0, x = 0.0, gy, gx;
            if constexpr (kMode != kFpTensor) warp_point<false>(p, q, y, x);
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            double2 f = make_double2(nan, nan);
            int pk = 0;
            if (warp_raw_footprint<false, kMode>(p, s, q, y, x, gy, gx)) {
                const int ny = area_n(gy, s.hi, N), nx = area_n(gx, s.hi, N);
                const double fy = gy / (double)ny, fx = gx / (double)nx;
                f = make_double2(fy < s.lo ? s.lo : (fy > s.hi ? s.hi : fy), fx < s.lo ? s.lo : (fx > s.hi ? s.hi : fx));
                cnt = ny * nx;
                pk = ny | (nx << 8);
            }
            fp[q] = f;
            nn[q] = pk;
        }
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += up;
        }
        excl[r] = incl - cnt;
        const int ones = __popcll(__ballot(cnt == 1));
        if (lane == kWave - 1) s_tot[r][wave] = incl;
        if (lane == 0) s_one[r][wave] = ones;
    }
    __syncthreads();
    int run = 0, ones = 0;
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
#pragma unroll
        for (int w = 0; w < kViewWaves; ++w) {
            if (w == wave) {
                const long q = q0 + (long)r * kViewThreads;
                if (q < p.Q) first[q] = run + excl[r];
            }
            run += s_tot[r][w];
            ones += s_one[r][w];
        }
    }
    if (tid == 0) {
        blk[blockIdx.x] = run;
        blk[n_blocks + blockIdx.x] = ones;
    }
}

// two waves: blk[0][*] and blk[1][*] become their exclusive scans over the blocks, tot[0] = S, tot[1] = the pixels with one sample
__global__ __launch_bounds__(kWave) void area_scan_kernel(int* __restrict__ blk, int n_blocks, int* __restrict__ tot) {
    view_scan_row(blk + (size_t)blockIdx.x * n_blocks, n_blocks, tot + blockIdx.x);
}

// first[q] becomes absolute, first[Q] = S
__global__ __launch_bounds__(kViewThreads) void area_offset_kernel(int* __restrict__ first, const int* __restrict__ blk,
                                                                   const int* __restrict__ tot, long Q) {
    const int base = blk[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = (long)blockIdx.x * kViewChunk + (long)r * kViewThreads + threadIdx.x;
        if (q < Q) first[q] += base;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) first[Q] = tot[0];
}

// Sample `sid` < S: its LR position and the footprint of its pixel.  The pixel is the last q with first[q] <= sid (first[0] = 0 and
// first[Q] = S > sid bracket it; a pixel without samples is never the last one).
__device__ __forceinline__ void area_sample(const WarpP& p, const AreaT& t, long sid, double& y, double& x, double& fy, double& fx) {
#pragma clang fp contract(off)
    long lo = 0, hi = p.Q;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if ((long)t.first[mid] <= sid) lo = mid;
        else hi = mid;
    }
    const int s = (int)(sid - (long)t.first[lo]), pk = t.nn[lo];
    const int ny = pk & 255, nx = pk >> 8;
    const int a = s / nx, b = s - a * nx;
    const int i = (int)(lo / p.Wv), j = (int)(lo - (long)i * p.Wv);
    const double v = (double)i + (double)(2 * a + 1) / (double)(2 * ny), u = (double)j + (double)(2 * b + 1) / (double)(2 * nx);
    const double Y = (p.h[0] * v + p.h[1] * u) + p.h[2];
    const double X = (p.h[3] * v + p.h[4] * u) + p.h[5];
    const double D = (p.h[6] * v + p.h[7] * u) + p.h[8];
    y = Y / D;
    x = X / D;
    const double2 f = t.fp[lo];
    fy = f.x;
    fx = f.y;
}

// warp_count_kernel over the samples; part rows are `stride` apart, a block past S leaves its entries alone (the scan does not read them)
__global__ __launch_bounds__(kViewThreads) void area_count_kernel(WarpP p, AreaT t, const int* __restrict__ tiles, int n_tiles, int stride,
                                                                  int* __restrict__ part) {
    __shared__ int s_cnt[kViewTileBatch][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, block = (int)blockIdx.x;
    const long S = t.first[p.Q];
    if ((long)block * kViewChunk >= S) return;                      // uniform over the block
    const long s0 = (long)block * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds];
    bool live[kViewRounds];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long sid = s0 + (long)r * kViewThreads;
        live[r] = sid < S;
        y[r] = x[r] = 0.0;
        double fy, fx;
        if (live[r]) area_sample(p, t, sid, y[r], x[r], fy, fx);
    }
    for (int t0 = 0; t0 < n_tiles; t0 += kViewTileBatch) {
        const int nt = min(kViewTileBatch, n_tiles - t0);
        for (int k = 0; k < nt; ++k) {
            const int4 tl = reinterpret_cast<const int4*>(tiles)[t0 + k];
            const ViewFrame f = view_frame(tl.x, tl.y, tl.z, tl.w);
            int c = 0;
#pragma unroll
            for (int r = 0; r < kViewRounds; ++r) c += __popcll(__ballot(live[r] && view_member(y[r], x[r], f)));
            if (lane == 0) s_cnt[k][wave] = c;
        }
        __syncthreads();
        for (int k = tid; k < nt; k += kViewThreads) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < kViewWaves; ++w) c += s_cnt[k][w];
            part[(size_t)(t0 + k) * stride + block] = c;
        }
        __syncthreads();
    }
}

// One wave per tile over the blocks that hold a sample; the wave after the last tile appends S and the one-sample pixels to the counts
__global__ __launch_bounds__(kWave) void area_tile_scan_kernel(int* __restrict__ part, int stride, const int* __restrict__ tot, int n_tiles,
                                                               int* __restrict__ counts) {
    if ((int)blockIdx.x == n_tiles) {
        if (threadIdx.x < 2) counts[n_tiles + threadIdx.x] = tot[threadIdx.x];
        return;
    }
    view_scan_row(part + (size_t)blockIdx.x * stride, (int)(((long)tot[0] + kViewChunk - 1) / kViewChunk), counts + blockIdx.x);
}

// warp_pp_select_kernel over the samples: the members of one tile in increasing sample id
__global__ __launch_bounds__(kViewThreads) void area_select_kernel(WarpP p, AreaT t, ViewFrame f, const int* __restrict__ offs, long S, long n,
                                                                   int* __restrict__ s_index, float* __restrict__ coord,
                                                                   float* __restrict__ cell) {
    __shared__ int s_cnt[kViewRounds][kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long s0 = (long)blockIdx.x * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds], fy[kViewRounds], fx[kViewRounds];
    int rank[kViewRounds];                     // among the members of the same round and wave, -1: no member
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long sid = s0 + (long)r * kViewThreads;
        bool m = false;
        y[r] = x[r] = fy[r] = fx[r] = 0.0;
        if (sid < S) {
            area_sample(p, t, sid, y[r], x[r], fy[r], fx[r]);
            m = view_member(y[r], x[r], f);
        }
        const unsigned long long mask = __ballot(m);
        rank[r] = m ? __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        if (lane == 0) s_cnt[r][wave] = __popcll(mask);
    }
    __syncthreads();
    long pos = offs[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
#pragma unroll
        for (int w = 0; w < kViewWaves; ++w) {
            if (w == wave && rank[r] >= 0) {
                const long o = pos + rank[r];
                if (o >= 0 && o < n) {         // holds whenever offs / n come from the count of the same warp and tile
                    s_index[o] = (int)(s0 + (long)r * kViewThreads);
                    reinterpret_cast<float2*>(coord)[o] = view_coord(y[r], x[r], f);
                    reinterpret_cast<float2*>(cell)[o] = warp_cell_of(fy[r], fx[r], f);
                }
            }
            pos += s_cnt[r][w];
        }
    }
}

// The image: per pixel and channel the mean of its samples' finished values, added in sample order.  A sample's value is
// view_finalize_kernel's pushed through denorm_clamp_kernel's two rounded operations and clamp; 1 / (n_y n_x) is a power of two.
__global__ void area_resolve_kernel(const float* __restrict__ E, const float* __restrict__ Wt, float* __restrict__ out,
                                    const int* __restrict__ first, long Q, long S, Fill3 fill, Fill3 mean, Fill3 std_) {
    const long n = 3 * Q;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i / Q);
        const long q = i - (long)c * Q;
        const int c0 = first[q], cnt = first[q + 1] - c0;
        if (cnt <= 0) {
            out[i] = fminf(fmaxf(add_rn(mul_rn(fill.v[c], std_.v[c]), mean.v[c]), 0.f), 1.f);
            continue;
        }
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) {
            const long sid = (long)c0 + k;
            if (sid >= S) break;               // E and Wt are S wide: a caller whose S is not the table's reads nothing past them
            const float w = Wt[sid];
            const float v = w > 0.f ? E[(long)c * S + sid] / w : fill.v[c];
            acc = add_rn(acc, fminf(fmaxf(add_rn(mul_rn(v, std_.v[c]), mean.v[c]), 0.f), 1.f));
        }
        out[i] = mul_rn(acc, 1.f / (float)cnt);
    }
}

// the table as the tests read it: first [Q + 1], n [Q][2] = (n_y, n_x)
__global__ void area_export_kernel(AreaT t, long Q, int* __restrict__ first, int* __restrict__ n) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q <= Q; q += (long)gridDim.x * blockDim.x) {
        first[q] = t.first[q];
        if (q < Q) {
            const int pk = t.nn[q];
            n[2 * q] = pk & 255;
            n[2 * q + 1] = pk >> 8;
        }
    }
}

// The workspace: per pixel the samples' footprint, first [Q + 1], the packed counts; the table's per-block sums (two rows) and their
// totals; the per-tile partials over the blocks of the largest possible S.  Every part starts on a 16-byte boundary.
struct AreaWs { size_t fp, first, nn, blk, tot, part, bytes; int tb, sb; };
static inline size_t area_up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline bool area_layout(int Hv, int Wv, int n_tiles, int N, AreaWs& w) {
    if (Hv <= 0 || Wv <= 0 || n_tiles <= 0 || !(N == 1 || N == 2 || N == 4 || N == 8)) return false;
    const long Q = (long)Hv * Wv;
    if (Q > (long)INT_MAX / ((long)N * N)) return false;
    w.tb = view_blocks(Q);
    w.sb = view_blocks(Q * N * N);
    size_t o = 0;
    w.fp = o;    o += (size_t)Q * sizeof(double2);
    w.first = o; o += area_up16((size_t)(Q + 1) * sizeof(int));
    w.nn = o;    o += area_up16((size_t)Q * sizeof(int));
    w.blk = o;   o += area_up16((size_t)2 * w.tb * sizeof(int));
    w.tot = o;   o += 16;
    w.part = o;  o += (size_t)n_tiles * (size_t)w.sb * sizeof(int);
    w.bytes = o;
    return true;
}
static inline AreaT area_t(const void* ws, const AreaWs& w) {
    const char* b = (const char*)ws;
    return AreaT{(const double2*)(b + w.fp), (const int*)(b + w.first), (const int*)(b + w.nn)};
}
// a homography with the Jacobian or a tensor as the raw footprint, a per-pixel warp's range
static inline bool area_ok(const double* h9, int mode, const double* range, const double* tensor, int Hv, int Wv) {
    return h9 && (mode == kFpJacobian || mode == kFpTensor) && warp_pp_ok(h9, nullptr, mode, range, tensor, Hv, Wv);
}
// the three launches of the table
static inline void area_table(const WarpP& p, const WarpFp& s, int mode, int N, void* ws, const AreaWs& w, hipStream_t stream) {
    char* b = (char*)ws;
    double2* fp = (double2*)(b + w.fp);
    int *first = (int*)(b + w.first), *nn = (int*)(b + w.nn), *blk = (int*)(b + w.blk), *tot = (int*)(b + w.tot);
    if (mode == kFpJacobian)
        hipLaunchKernelGGL(area_table_kernel<kFpJacobian>, dim3(w.tb), dim3(kViewThreads), 0, stream, p, s, N, fp, first, nn, blk, w.tb);
    else
        hipLaunchKernelGGL(area_table_kernel<kFpTensor>, dim3(w.tb), dim3(kViewThreads), 0, stream, p, s, N, fp, first, nn, blk, w.tb);
    hipLaunchKernelGGL(area_scan_kernel, dim3(2), dim3(kWave), 0, stream, blk, w.tb, tot);
    hipLaunchKernelGGL(area_offset_kernel, dim3(w.tb), dim3(kViewThreads), 0, stream, first, blk, tot, p.Q);
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_warp_workspace_bytes(int Hv, int Wv, int n_tiles) {
    if (Hv <= 0 || Wv <= 0 || n_tiles <= 0 || (long)Hv * Wv > (long)INT_MAX) return 0;
    return (size_t)n_tiles * (size_t)view_blocks((long)Hv * Wv) * sizeof(int);
}

extern "C" int ciaosr_warp_coord_cell_f32(float* coord, float* cell, const double* h9, const double* map, const double* footprint, int Hv,
                                          int Wv, const int* frame, void* stream) {
    CIAOSR_CHECK_ARG(coord && cell && warp_ok(h9, map, footprint, Hv, Wv) && frame_ok(frame));
    ProfScope prof("warp_coord_cell", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    if (map)
        hipLaunchKernelGGL(warp_coord_cell_kernel<true>, dim3(view_grid(p.Q)), dim3(256), 0, (hipStream_t)stream, p, frame_of(frame),
                           warp_cell(footprint, frame), coord, cell);
    else
        hipLaunchKernelGGL(warp_coord_cell_kernel<false>, dim3(view_grid(p.Q)), dim3(256), 0, (hipStream_t)stream, p, frame_of(frame),
                           warp_cell(footprint, frame), coord, cell);
    return launch_status("warp_coord_cell");
}

extern "C" int ciaosr_warp_count_i32(const double* h9, const double* map, const double* footprint, int Hv, int Wv, const int* tiles,
                                     int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(warp_ok(h9, map, footprint, Hv, Wv) && tiles && n_tiles > 0 && counts && workspace && aligned16(tiles));
    CIAOSR_CHECK_ARG(((size_t)workspace & 3) == 0);
    if (workspace_bytes < ciaosr_warp_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_count", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const int n_blocks = view_blocks(p.Q);
    if (map)
        hipLaunchKernelGGL(warp_count_kernel<true>, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, tiles, n_tiles, n_blocks,
                           (int*)workspace);
    else
        hipLaunchKernelGGL(warp_count_kernel<false>, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, tiles, n_tiles, n_blocks,
                           (int*)workspace);
    hipLaunchKernelGGL(warp_scan_kernel, dim3(n_tiles), dim3(kWave), 0, (hipStream_t)stream, (int*)workspace, n_blocks, counts);
    return launch_status("warp_count");
}

extern "C" int ciaosr_warp_select_f32(const double* h9, const double* map, const double* footprint, int Hv, int Wv, const int* tile,
                                      int tile_index, int n_tiles, const void* workspace, size_t workspace_bytes, int n, int* q_index,
                                      float* coord, float* cell, void* stream) {
    CIAOSR_CHECK_ARG(warp_ok(h9, map, footprint, Hv, Wv) && frame_ok(tile) && n_tiles > 0 && tile_index >= 0 && tile_index < n_tiles && workspace);
    CIAOSR_CHECK_ARG(n > 0 && (long)n <= (long)Hv * Wv && q_index && coord && cell && ((size_t)workspace & 3) == 0);
    if (workspace_bytes < ciaosr_warp_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_select", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const int n_blocks = view_blocks(p.Q);
    const int* offs = (const int*)workspace + (size_t)tile_index * n_blocks;
    if (map)
        hipLaunchKernelGGL(warp_select_kernel<true>, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, frame_of(tile),
                           warp_cell(footprint, tile), offs, (long)n, q_index, coord, cell);
    else
        hipLaunchKernelGGL(warp_select_kernel<false>, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, frame_of(tile),
                           warp_cell(footprint, tile), offs, (long)n, q_index, coord, cell);
    return launch_status("warp_select");
}

// ---- per-pixel warps: the same entries with a footprint per output pixel, and the footprints themselves ------------------------------
extern "C" int ciaosr_ppwarp_coord_cell_f32(float* coord, float* cell, const double* h9, const double* map, int mode, const double* range,
                                            const double* tensor, int Hv, int Wv, const int* frame, void* stream) {
    CIAOSR_CHECK_ARG(coord && cell && warp_pp_ok(h9, map, mode, range, tensor, Hv, Wv) && frame_ok(frame));
    ProfScope prof("warp_pp_coord_cell", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const WarpFp s = warp_fp(range, tensor);
    warp_pp_dispatch(map != nullptr, mode, [&](auto m, auto k) {
        hipLaunchKernelGGL((warp_pp_coord_cell_kernel<decltype(m)::value, decltype(k)::value>), dim3(view_grid(p.Q)), dim3(256), 0,
                           (hipStream_t)stream, p, s, frame_of(frame), coord, cell);
    });
    return launch_status("warp_pp_coord_cell");
}

extern "C" int ciaosr_ppwarp_count_i32(const double* h9, const double* map, int mode, const double* range, const double* tensor, int Hv,
                                       int Wv, const int* tiles, int n_tiles, int* counts, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    CIAOSR_CHECK_ARG(warp_pp_ok(h9, map, mode, range, tensor, Hv, Wv) && tiles && n_tiles > 0 && counts && workspace && aligned16(tiles));
    CIAOSR_CHECK_ARG(((size_t)workspace & 3) == 0);
    if (workspace_bytes < ciaosr_warp_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_pp_count", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const WarpFp s = warp_fp(range, tensor);
    const int n_blocks = view_blocks(p.Q);
    warp_pp_dispatch(map != nullptr, mode, [&](auto m, auto k) {
        hipLaunchKernelGGL((warp_pp_count_kernel<decltype(m)::value, decltype(k)::value>), dim3(n_blocks), dim3(kViewThreads), 0,
                           (hipStream_t)stream, p, s, tiles, n_tiles, n_blocks, (int*)workspace);
    });
    hipLaunchKernelGGL(warp_scan_kernel, dim3(n_tiles), dim3(kWave), 0, (hipStream_t)stream, (int*)workspace, n_blocks, counts);
    return launch_status("warp_pp_count");
}

extern "C" int ciaosr_ppwarp_select_f32(const double* h9, const double* map, int mode, const double* range, const double* tensor, int Hv,
                                        int Wv, const int* tile, int tile_index, int n_tiles, const void* workspace, size_t workspace_bytes,
                                        int n, int* q_index, float* coord, float* cell, void* stream) {
    CIAOSR_CHECK_ARG(warp_pp_ok(h9, map, mode, range, tensor, Hv, Wv) && frame_ok(tile) && n_tiles > 0 && tile_index >= 0 &&
                     tile_index < n_tiles && workspace);
    CIAOSR_CHECK_ARG(n > 0 && (long)n <= (long)Hv * Wv && q_index && coord && cell && ((size_t)workspace & 3) == 0);
    if (workspace_bytes < ciaosr_warp_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_pp_select", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const WarpFp s = warp_fp(range, tensor);
    const int n_blocks = view_blocks(p.Q);
    const int* offs = (const int*)workspace + (size_t)tile_index * n_blocks;
    warp_pp_dispatch(map != nullptr, mode, [&](auto m, auto k) {
        hipLaunchKernelGGL((warp_pp_select_kernel<decltype(m)::value, decltype(k)::value>), dim3(n_blocks), dim3(kViewThreads), 0,
                           (hipStream_t)stream, p, s, frame_of(tile), offs, (long)n, q_index, coord, cell);
    });
    return launch_status("warp_pp_select");
}

extern "C" int ciaosr_ppwarp_footprints_f64(double* out, const double* h9, const double* map, int mode, const double* range,
                                            const double* tensor, int Hv, int Wv, void* stream) {
    CIAOSR_CHECK_ARG(out && aligned16(out) && warp_pp_ok(h9, map, mode, range, tensor, Hv, Wv));
    ProfScope prof("warp_footprints", (hipStream_t)stream);
    const WarpP p = warp_p(h9, map, Hv, Wv);
    const WarpFp s = warp_fp(range, tensor);
    warp_pp_dispatch(map != nullptr, mode, [&](auto m, auto k) {
        hipLaunchKernelGGL((warp_footprints_kernel<decltype(m)::value, decltype(k)::value>), dim3(view_grid(p.Q)), dim3(256), 0,
                           (hipStream_t)stream, p, s, out);
    });
    return launch_status("warp_footprints");
}

// ---- area-sampled warps: the table, count and select over the samples, the resolve, the table's export ---------------------------------
extern "C" size_t ciaosr_areawarp_workspace_bytes(int Hv, int Wv, int n_tiles, int max_samples) {
    AreaWs w;
    return area_layout(Hv, Wv, n_tiles, max_samples, w) ? w.bytes : 0;
}

extern "C" int ciaosr_areawarp_count_i32(const double* h9, int mode, const double* range, const double* tensor, int max_samples, int Hv, int Wv,
                                         const int* tiles, int n_tiles, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
    AreaWs w;
    CIAOSR_CHECK_ARG(area_ok(h9, mode, range, tensor, Hv, Wv) && area_layout(Hv, Wv, n_tiles, max_samples, w));
    CIAOSR_CHECK_ARG(tiles && aligned16(tiles) && counts && workspace && aligned16(workspace));
    if (workspace_bytes < w.bytes) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_area_count", (hipStream_t)stream);
    const WarpP p = warp_p(h9, nullptr, Hv, Wv);
    area_table(p, warp_fp(range, tensor), mode, max_samples, workspace, w, (hipStream_t)stream);
    int* part = (int*)((char*)workspace + w.part);
    const int* tot = (const int*)((const char*)workspace + w.tot);
    hipLaunchKernelGGL(area_count_kernel, dim3(w.sb), dim3(kViewThreads), 0, (hipStream_t)stream, p, area_t(workspace, w), tiles, n_tiles, w.sb,
                       part);
    hipLaunchKernelGGL(area_tile_scan_kernel, dim3(n_tiles + 1), dim3(kWave), 0, (hipStream_t)stream, part, w.sb, tot, n_tiles, counts);
    return launch_status("warp_area_count");
}

extern "C" int ciaosr_areawarp_select_f32(const double* h9, int max_samples, int Hv, int Wv, const int* tile, int tile_index, int n_tiles,
                                          const void* workspace, size_t workspace_bytes, int S, int n, int* s_index, float* coord, float* cell,
                                          void* stream) {
    AreaWs w;
    const double one[2] = {1.0, 1.0};
    CIAOSR_CHECK_ARG(h9 && warp_ok(h9, nullptr, one, Hv, Wv) && area_layout(Hv, Wv, n_tiles, max_samples, w) && frame_ok(tile));
    CIAOSR_CHECK_ARG(tile_index >= 0 && tile_index < n_tiles && workspace && aligned16(workspace));
    CIAOSR_CHECK_ARG(S > 0 && (long)S <= (long)Hv * Wv * max_samples * max_samples && n > 0 && n <= S && s_index && coord && cell);
    if (workspace_bytes < w.bytes) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_area_select", (hipStream_t)stream);
    const WarpP p = warp_p(h9, nullptr, Hv, Wv);
    const int* offs = (const int*)((const char*)workspace + w.part) + (size_t)tile_index * w.sb;
    hipLaunchKernelGGL(area_select_kernel, dim3(view_blocks(S)), dim3(kViewThreads), 0, (hipStream_t)stream, p, area_t(workspace, w),
                       frame_of(tile), offs, (long)S, (long)n, s_index, coord, cell);
    return launch_status("warp_area_select");
}

extern "C" int ciaosr_areawarp_resolve_f32(const float* E, const float* Wt, float* out_chw, int S, int max_samples, int Hv, int Wv, int n_tiles,
                                           const void* workspace, size_t workspace_bytes, const float* fill3, const float* mean3,
                                           const float* std3, void* stream) {
    AreaWs w;
    CIAOSR_CHECK_ARG(E && Wt && out_chw && area_layout(Hv, Wv, n_tiles, max_samples, w) && workspace && aligned16(workspace));
    CIAOSR_CHECK_ARG(S >= 0 && (long)S <= (long)Hv * Wv * max_samples * max_samples && fill3 && mean3 && std3);
    if (workspace_bytes < w.bytes) return CIAOSR_ERR_WORKSPACE;
    Fill3 fill, mean, std_;
    for (int c = 0; c < 3; ++c) {
        CIAOSR_CHECK_ARG(fill3[c] >= 0.f && fill3[c] <= 1.f && std::isfinite(mean3[c]) && std::isfinite(std3[c]) && std3[c] != 0.f);
        fill.v[c] = fill_preimage(fill3[c], mean3[c], std3[c]);
        mean.v[c] = mean3[c];
        std_.v[c] = std3[c];
    }
    ProfScope prof("warp_area_resolve", (hipStream_t)stream);
    const long Q = (long)Hv * Wv;
    hipLaunchKernelGGL(area_resolve_kernel, dim3(view_grid(3 * Q)), dim3(256), 0, (hipStream_t)stream, E, Wt, out_chw,
                       area_t(workspace, w).first, Q, (long)S, fill, mean, std_);
    return launch_status("warp_area_resolve");
}

extern "C" int ciaosr_areawarp_table_i32(int* first, int* n, const double* h9, int mode, const double* range, const double* tensor,
                                         int max_samples, int Hv, int Wv, int n_tiles, void* workspace, size_t workspace_bytes, void* stream) {
    AreaWs w;
    CIAOSR_CHECK_ARG(first && n && area_ok(h9, mode, range, tensor, Hv, Wv) && area_layout(Hv, Wv, n_tiles, max_samples, w));
    CIAOSR_CHECK_ARG(workspace && aligned16(workspace));
    if (workspace_bytes < w.bytes) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("warp_area_table", (hipStream_t)stream);
    const WarpP p = warp_p(h9, nullptr, Hv, Wv);
    area_table(p, warp_fp(range, tensor), mode, max_samples, workspace, w, (hipStream_t)stream);
    hipLaunchKernelGGL(area_export_kernel, dim3(view_grid(p.Q + 1)), dim3(256), 0, (hipStream_t)stream, area_t(workspace, w), p.Q, first, n);
    return launch_status("warp_area_table");
}
