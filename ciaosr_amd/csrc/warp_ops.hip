// Warps of an encoded scene (include/ciaosr_hip.h, "warps"): the queries of an Hv x Wv output grid whose LR positions come from a
// homography (nine doubles, by value) or from a coordinate map (one (y_lr, x_lr) pair of doubles per output pixel, on the device), sorted
// into the LR tiles exactly as a view's are.  Three roles -- count, select, the whole grid's coordinates in one frame -- in view_ops.hip's
// scheme: tile membership is counted with wave ballots, a block's members are placed at (exclusive scan of the per-block counts) + (rank
// inside the block), no atomics, every result bitwise repeatable.  Everything after the LR position is view_frame.h's, shared with the
// views; blend and finalize are the views' own entries.  The second half of the file is the per-pixel warps: the same roles with a
// footprint, and hence a cell, per output pixel (Jacobian of the homography, differences of the map, or a device tensor), and the entry
// that writes the footprints themselves.
#include <climits>
#include <cmath>
#include <type_traits>

#include "common.h"
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

// The clamped footprint (f_y, f_x) of query q, whose LR position is (y, x); false: the pixel has none.  fp64, every operation rounded on
// its own; sqrt of the rounded sum, IEEE.
template <bool kMap, int kMode>
__device__ __forceinline__ bool warp_footprint(const WarpP& p, const WarpFp& s, long q, double y, double x, double& fy, double& fx) {
#pragma clang fp contract(off)
    double gy, gx;
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
    if (gy != gy || gx != gx) return false;
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
