// Affine views of an encoded scene (include/ciaosr_hip.h, "views"): the queries of an Hv x Wv output grid under a 2 x 3 matrix into LR
// pixel units, sorted into the LR tiles of the reference's tiling and blended back.  Four roles -- count, select, blend, finalize -- and
// the whole grid's coordinates in one frame.  No atomics: tile membership is counted with wave ballots, a block's members are placed at
// (exclusive scan of the per-block counts) + (rank inside the block), so every result is bitwise repeatable.  A second count / select
// pair lists a tile's members as blocks of 4 x 2 output pixels padded to 8 entries: the row tiles of the chained 16-bit head kernel.
#include <climits>
#include <cmath>

#include "common.h"
#include "view_frame.h"

namespace ciaosr {

// (the workgroup geometry kViewThreads / kViewRounds / kViewChunk, ViewFrame and what follows a query's LR position: view_frame.h)
struct ViewP { double myy, myx, ty, mxy, mxx, tx; int Hv, Wv; long Q; };

// LR position of the centre of output pixel q, fp64, every operation rounded on its own (an FMA would change the value that the
// membership tests and the fp32 rounding of the coordinate see)
__device__ __forceinline__ void view_point(const ViewP& p, long q, double& y, double& x) {
#pragma clang fp contract(off)
    const int i = (int)(q / p.Wv), j = (int)(q - (long)i * p.Wv);
    const double v = (double)i + 0.5, u = (double)j + 0.5;
    y = (p.myy * v + p.myx * u) + p.ty;
    x = (p.mxy * v + p.mxx * u) + p.tx;
}

// part[t * n_blocks + b] = members of tile t among block b's queries.  Per tile one ballot per round and wave; lane 0 of each wave owns
// its LDS slot, so nothing is added concurrently.  `block` is the block's number within ITS view (blockIdx.x for a single view).
__device__ __forceinline__ void view_count_block(const ViewP& p, const int* __restrict__ tiles, int n_tiles, int n_blocks, int block,
                                                 int* __restrict__ part, int (*s_cnt)[kViewWaves]) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long q0 = (long)block * kViewChunk + tid;
    double y[kViewRounds], x[kViewRounds];
    bool live[kViewRounds];
#pragma unroll
    for (int r = 0; r < kViewRounds; ++r) {
        const long q = q0 + (long)r * kViewThreads;
        live[r] = q < p.Q;
        y[r] = x[r] = 0.0;
        if (live[r]) view_point(p, q, y[r], x[r]);
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

__global__ __launch_bounds__(kViewThreads) void view_count_kernel(ViewP p, const int* __restrict__ tiles, int n_tiles, int n_blocks,
                                                                  int* __restrict__ part) {
    __shared__ int s_cnt[kViewTileBatch][kViewWaves];
    view_count_block(p, tiles, n_tiles, n_blocks, (int)blockIdx.x, part, s_cnt);
}

// One wave per tile: part[t][*] becomes its exclusive scan over the blocks, counts[t] the total
__global__ __launch_bounds__(kWave) void view_scan_kernel(int* __restrict__ part, int n_blocks, int* __restrict__ counts) {
    view_scan_row(part + (size_t)blockIdx.x * n_blocks, n_blocks, counts + blockIdx.x);
}

// ---- the members of several views in one launch pair --------------------------------------------------------------------------------
// Up to kViewMany views travel BY VALUE as kernel arguments (no staging copy): their parameters, the prefix table first[] over their
// workgroup counts (workgroup b of the launch is workgroup b - first[v] of the view v with first[v] <= b < first[v + 1]) and the offset
// of each view's part array in the workspace, in ints.  Every view's part array and counts are what the single-view kernels write.
constexpr int kViewMany = 32;             // 32 x 64 + 33 x 4 + 32 x 8 + 8 bytes of arguments: well inside the 4 KiB kernel-argument limit
struct ViewManyP {
    ViewP p[kViewMany];
    int first[kViewMany + 1];
    int n_views;
    unsigned long part[kViewMany];
};

__global__ __launch_bounds__(kViewThreads) void view_count_many_kernel(ViewManyP a, const int* __restrict__ tiles, int n_tiles,
                                                                       int* __restrict__ ws) {
    __shared__ int s_cnt[kViewTileBatch][kViewWaves];
    const int b = (int)blockIdx.x;
    int v = 0;                                   // uniform over the workgroup: a scalar search of the prefix table
    while (v + 1 < a.n_views && b >= a.first[v + 1]) ++v;
    view_count_block(a.p[v], tiles, n_tiles, a.first[v + 1] - a.first[v], b - a.first[v], ws + a.part[v], s_cnt);
}

// One wave per (view, tile): workgroup v * n_tiles + t
__global__ __launch_bounds__(kWave) void view_scan_many_kernel(ViewManyP a, int n_tiles, int* __restrict__ ws, int* __restrict__ counts) {
    const int v = (int)blockIdx.x / n_tiles, t = (int)blockIdx.x - v * n_tiles;
    const int n_blocks = a.first[v + 1] - a.first[v];
    view_scan_row(ws + a.part[v] + (size_t)t * n_blocks, n_blocks, counts + blockIdx.x);
}

// The members of one tile in increasing q: position = offs[block] + members of the block before this one
__global__ __launch_bounds__(kViewThreads) void view_select_kernel(ViewP p, ViewFrame f, float2 cellv, const int* __restrict__ offs, long n,
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
            view_point(p, q, y[r], x[r]);
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
                if (o >= 0 && o < n) {         // holds whenever offs / n come from the count of the same view and tile
                    q_index[o] = (int)(q0 + (long)r * kViewThreads);
                    reinterpret_cast<float2*>(coord)[o] = view_coord(y[r], x[r], f);
                    reinterpret_cast<float2*>(cell)[o] = cellv;
                }
            }
            pos += s_cnt[r][w];
        }
    }
}

// ---- members in blocks of 4 x 2 output pixels (include/ciaosr_hip.h, "Members in blocks") ------------------------------------------------
// One thread owns one block; a workgroup kViewThreads consecutive blocks, so (wave, lane) in lexicographic order is increasing block
// index.  The eight points of a block are view_point's values of its pixels: the membership tests and coordinates are bit for bit those of
// the per-query kernels above.
constexpr int kViewBlockQ = 8;             // entries of a block: entry e is pixel (row e >> 2, column e & 3)

__device__ __forceinline__ int view_nbx(const ViewP& p) { return (int)(((long)p.Wv + 3) >> 2); }
__device__ __forceinline__ long view_n_blocks(const ViewP& p) { return (long)view_nbx(p) * (((long)p.Hv + 1) >> 1); }

// y[e], x[e] and q[e] of block b's pixels; -> the mask of the entries that lie inside the output grid (0 for b past the last block)
__device__ __forceinline__ unsigned view_block_points(const ViewP& p, long b, double (&y)[kViewBlockQ], double (&x)[kViewBlockQ],
                                                      int (&q)[kViewBlockQ]) {
    unsigned valid = 0;
    const int nbx = view_nbx(p);
    const bool in = b < view_n_blocks(p);
    const int by = in ? (int)(b / nbx) : 0, bx = in ? (int)(b - (long)by * nbx) : 0;
#pragma unroll
    for (int e = 0; e < kViewBlockQ; ++e) {
        const int i = 2 * by + (e >> 2), j = 4 * bx + (e & 3);
        y[e] = x[e] = 0.0;
        q[e] = -1;
        if (in && i < p.Hv && j < p.Wv) {
            q[e] = i * p.Wv + j;               // <= Hv Wv - 1 <= INT_MAX - 1
            view_point(p, (long)q[e], y[e], x[e]);
            valid |= 1u << e;
        }
    }
    return valid;
}

// part[(2 t) * n_wg + wg] = members of tile t among workgroup wg's blocks, part[(2 t + 1) * n_wg + wg] = its live blocks among them.
// Ballots and one LDS slot per wave as view_count_block; `wg` is the workgroup's number within ITS view.
__device__ __forceinline__ void view_count_blocks_wg(const ViewP& p, const int* __restrict__ tiles, int n_tiles, int n_wg, int wg,
                                                     int* __restrict__ part, int (*s_cnt)[2][kViewWaves]) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    double y[kViewBlockQ], x[kViewBlockQ];
    int q[kViewBlockQ];
    const unsigned valid = view_block_points(p, (long)wg * kViewThreads + tid, y, x, q);
    for (int t0 = 0; t0 < n_tiles; t0 += kViewTileBatch) {
        const int nt = min(kViewTileBatch, n_tiles - t0);
        for (int t = 0; t < nt; ++t) {
            const int4 tl = reinterpret_cast<const int4*>(tiles)[t0 + t];
            const ViewFrame f = view_frame(tl.x, tl.y, tl.z, tl.w);
            int c = 0;
            bool live = false;
#pragma unroll
            for (int e = 0; e < kViewBlockQ; ++e) {
                const bool m = ((valid >> e) & 1u) && view_member(y[e], x[e], f);
                c += __popcll(__ballot(m));
                live = live || m;
            }
            const int nb = __popcll(__ballot(live));
            if (lane == 0) { s_cnt[t][0][wave] = c; s_cnt[t][1][wave] = nb; }
        }
        __syncthreads();
        for (int i = tid; i < 2 * nt; i += kViewThreads) {
            const int t = i >> 1, k = i & 1;
            int c = 0;
#pragma unroll
            for (int w = 0; w < kViewWaves; ++w) c += s_cnt[t][k][w];
            part[((size_t)(t0 + t) * 2 + k) * n_wg + wg] = c;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kViewThreads) void view_count_blocks_kernel(ViewP p, const int* __restrict__ tiles, int n_tiles, int n_wg,
                                                                         int* __restrict__ part) {
    __shared__ int s_cnt[kViewTileBatch][2][kViewWaves];
    view_count_blocks_wg(p, tiles, n_tiles, n_wg, (int)blockIdx.x, part, s_cnt);
}

__global__ __launch_bounds__(kViewThreads) void view_count_blocks_many_kernel(ViewManyP a, const int* __restrict__ tiles, int n_tiles,
                                                                              int* __restrict__ ws) {
    __shared__ int s_cnt[kViewTileBatch][2][kViewWaves];
    const int b = (int)blockIdx.x;
    int v = 0;
    while (v + 1 < a.n_views && b >= a.first[v + 1]) ++v;
    view_count_blocks_wg(a.p[v], tiles, n_tiles, a.first[v + 1] - a.first[v], b - a.first[v], ws + a.part[v], s_cnt);
}

// The live blocks of one tile in increasing block index, eight entries each: block position = offs[workgroup] + live blocks of the
// workgroup before this one.  Pads (no member of the tile, or outside the grid) carry q = -1 and the block's first member's coordinate.
__global__ __launch_bounds__(kViewThreads) void view_select_blocks_kernel(ViewP p, ViewFrame f, float2 cellv, const int* __restrict__ offs,
                                                                          long n_blocks, int* __restrict__ q_index, float* __restrict__ coord,
                                                                          float* __restrict__ cell) {
    __shared__ int s_cnt[kViewWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    double y[kViewBlockQ], x[kViewBlockQ];
    int q[kViewBlockQ];
    const unsigned valid = view_block_points(p, (long)blockIdx.x * kViewThreads + tid, y, x, q);
    unsigned mem = 0;
    float2 c[kViewBlockQ];
#pragma unroll
    for (int e = 0; e < kViewBlockQ; ++e) {
        if (((valid >> e) & 1u) && view_member(y[e], x[e], f)) mem |= 1u << e;
        c[e] = view_coord(y[e], x[e], f);
    }
    float2 first = c[kViewBlockQ - 1];
#pragma unroll
    for (int e = kViewBlockQ - 2; e >= 0; --e)
        if ((mem >> e) & 1u) first = c[e];
    const unsigned long long mask = __ballot(mem != 0);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    long pos = offs[blockIdx.x];
#pragma unroll
    for (int w = 0; w < kViewWaves; ++w)
        if (w < wave) pos += s_cnt[w];
    const long o = pos + rank;
    if (mem == 0 || o < 0 || o >= n_blocks) return;        // o in range whenever offs / n_blocks come from the count of the same view and tile
#pragma unroll
    for (int e = 0; e < kViewBlockQ; ++e) {
        const bool m = (mem >> e) & 1u;
        const long s = o * kViewBlockQ + e;
        q_index[s] = m ? q[e] : -1;
        reinterpret_cast<float2*>(coord)[s] = m ? c[e] : first;
        reinterpret_cast<float2*>(cell)[s] = cellv;
    }
}

__global__ void view_coord_cell_kernel(ViewP p, ViewFrame f, float2 cellv, float* __restrict__ coord, float* __restrict__ cell) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < p.Q; q += (long)gridDim.x * blockDim.x) {
        double y, x;
        view_point(p, q, y, x);
        reinterpret_cast<float2*>(coord)[q] = view_coord(y, x, f);
        reinterpret_cast<float2*>(cell)[q] = cellv;
    }
}

__global__ void view_blend_kernel(float* __restrict__ E, float* __restrict__ Wt, long Q, const int* __restrict__ q_index,
                                  const float* __restrict__ rgb, long n) {
    for (long s = blockIdx.x * (long)blockDim.x + threadIdx.x; s < n; s += (long)gridDim.x * blockDim.x) {
        const long q = q_index ? (long)q_index[s] : s;
        if (q < 0 || q >= Q) continue;
        E[q] += rgb[s * 3];
        E[Q + q] += rgb[s * 3 + 1];
        E[2 * Q + q] += rgb[s * 3 + 2];
        Wt[q] += 1.f;
    }
}

__global__ void view_finalize_kernel(const float* __restrict__ E, const float* __restrict__ Wt, float* __restrict__ out, long Q, Fill3 fill) {
    const long n = 3 * Q;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i / Q);
        const long q = i - (long)c * Q;
        const float w = Wt[q];
        out[q * 3 + c] = w > 0.f ? E[i] / w : fill.v[c];
    }
}

static inline bool view_ok(const double* m, int Hv, int Wv) {
    if (!m || Hv <= 0 || Wv <= 0 || (long)Hv * Wv > (long)INT_MAX) return false;
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}
static inline ViewP view_p(const double* m, int Hv, int Wv) { return ViewP{m[0], m[1], m[2], m[3], m[4], m[5], Hv, Wv, (long)Hv * Wv}; }
// the view's cell in a th x tw frame: the norm of a matrix row is the output pixel's extent along that LR axis
static inline float2 view_cell(const double* m, const int* f) {
    return make_float2((float)(std::hypot(m[0], m[1]) * 2.0 / (double)f[2]), (float)(std::hypot(m[3], m[4]) * 2.0 / (double)f[3]));
}
// workgroups of the block kernels: one thread per 4 x 2 block of the output grid
static inline int view_block_wgs(int Hv, int Wv) {
    const long nb = (((long)Wv + 3) >> 2) * (((long)Hv + 1) >> 1);
    return (int)((nb + kViewThreads - 1) / kViewThreads);
}

}  // namespace ciaosr

using namespace ciaosr;

extern "C" int ciaosr_view_block_queries(void) { return kViewChunk; }

extern "C" size_t ciaosr_view_workspace_bytes(int Hv, int Wv, int n_tiles) {
    if (Hv <= 0 || Wv <= 0 || n_tiles <= 0 || (long)Hv * Wv > (long)INT_MAX) return 0;
    return (size_t)n_tiles * (size_t)view_blocks((long)Hv * Wv) * sizeof(int);
}

extern "C" int ciaosr_view_coord_cell_f32(float* coord, float* cell, const double* m, int Hv, int Wv, const int* frame, void* stream) {
    CIAOSR_CHECK_ARG(coord && cell && view_ok(m, Hv, Wv) && frame_ok(frame));
    ProfScope prof("view_coord_cell", (hipStream_t)stream);
    const ViewP p = view_p(m, Hv, Wv);
    hipLaunchKernelGGL(view_coord_cell_kernel, dim3(view_grid(p.Q)), dim3(256), 0, (hipStream_t)stream, p, frame_of(frame), view_cell(m, frame),
                       coord, cell);
    return launch_status("view_coord_cell");
}

extern "C" int ciaosr_view_count_i32(const double* m, int Hv, int Wv, const int* tiles, int n_tiles, int* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(view_ok(m, Hv, Wv) && tiles && n_tiles > 0 && counts && workspace && aligned16(tiles));
    if (workspace_bytes < ciaosr_view_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("view_count", (hipStream_t)stream);
    const ViewP p = view_p(m, Hv, Wv);
    const int n_blocks = view_blocks(p.Q);
    hipLaunchKernelGGL(view_count_kernel, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, tiles, n_tiles, n_blocks,
                       (int*)workspace);
    hipLaunchKernelGGL(view_scan_kernel, dim3(n_tiles), dim3(kWave), 0, (hipStream_t)stream, (int*)workspace, n_blocks, counts);
    return launch_status("view_count");
}

extern "C" int ciaosr_view_count_many_max_views(void) { return kViewMany; }

static inline size_t view_many_align(size_t n) { return (n + 255) & ~(size_t)255; }

// bytes in front of view `upto` (upto = n_views: the whole workspace); 0 for a list the count refuses.  `one_bytes`: the single-view size
static size_t view_many_offset(const int* sizes, int n_views, int n_tiles, int upto, size_t (*one_bytes)(int, int, int)) {
    if (!sizes || n_views <= 0 || n_tiles <= 0 || upto < 0 || upto > n_views) return 0;
    size_t off = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t one = one_bytes(sizes[2 * v], sizes[2 * v + 1], n_tiles);
        if (!one) return 0;
        if (v == upto) break;
        off += view_many_align(one);
    }
    return off;
}

extern "C" size_t ciaosr_view_many_workspace_bytes(const int* sizes, int n_views, int n_tiles) {
    return view_many_offset(sizes, n_views, n_tiles, n_views, ciaosr_view_workspace_bytes);
}

extern "C" size_t ciaosr_view_many_workspace_offset(const int* sizes, int n_views, int n_tiles, int view) {
    if (view < 0 || view >= n_views) return 0;
    return view_many_offset(sizes, n_views, n_tiles, view, ciaosr_view_workspace_bytes);
}

extern "C" int ciaosr_view_count_many_i32(const double* m, const int* sizes, int n_views, const int* tiles, int n_tiles, int* counts,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(m && sizes && n_views > 0 && tiles && n_tiles > 0 && counts && workspace && aligned16(tiles));
    CIAOSR_CHECK_ARG(((size_t)workspace & 3) == 0 && (long)n_views * n_tiles <= (long)INT_MAX);
    for (int v = 0; v < n_views; ++v) CIAOSR_CHECK_ARG(view_ok(m + 6 * v, sizes[2 * v], sizes[2 * v + 1]));
    const size_t need = ciaosr_view_many_workspace_bytes(sizes, n_views, n_tiles);
    if (!need || workspace_bytes < need) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("view_count_many", (hipStream_t)stream);
    size_t off = 0;                              // bytes, of the whole list: a later group continues where the one before ended
    for (int v0 = 0; v0 < n_views; v0 += kViewMany) {
        ViewManyP a = {};
        a.n_views = n_views - v0 < kViewMany ? n_views - v0 : kViewMany;
        for (int k = 0; k < a.n_views; ++k) {
            const int v = v0 + k;
            a.p[k] = view_p(m + 6 * v, sizes[2 * v], sizes[2 * v + 1]);
            a.first[k + 1] = a.first[k] + view_blocks(a.p[k].Q);
            a.part[k] = off / sizeof(int);
            off += view_many_align(ciaosr_view_workspace_bytes(sizes[2 * v], sizes[2 * v + 1], n_tiles));
        }
        for (int k = a.n_views; k < kViewMany; ++k) a.first[k + 1] = a.first[a.n_views];
        hipLaunchKernelGGL(view_count_many_kernel, dim3(a.first[a.n_views]), dim3(kViewThreads), 0, (hipStream_t)stream, a, tiles, n_tiles,
                           (int*)workspace);
        hipLaunchKernelGGL(view_scan_many_kernel, dim3(a.n_views * n_tiles), dim3(kWave), 0, (hipStream_t)stream, a, n_tiles,
                           (int*)workspace, counts + (size_t)v0 * n_tiles);
    }
    return launch_status("view_count_many");
}

extern "C" int ciaosr_view_select_f32(const double* m, int Hv, int Wv, const int* tile, int tile_index, int n_tiles, const void* workspace,
                                      size_t workspace_bytes, int n, int* q_index, float* coord, float* cell, void* stream) {
    CIAOSR_CHECK_ARG(view_ok(m, Hv, Wv) && frame_ok(tile) && n_tiles > 0 && tile_index >= 0 && tile_index < n_tiles && workspace);
    CIAOSR_CHECK_ARG(n > 0 && (long)n <= (long)Hv * Wv && q_index && coord && cell);
    if (workspace_bytes < ciaosr_view_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("view_select", (hipStream_t)stream);
    const ViewP p = view_p(m, Hv, Wv);
    const int n_blocks = view_blocks(p.Q);
    hipLaunchKernelGGL(view_select_kernel, dim3(n_blocks), dim3(kViewThreads), 0, (hipStream_t)stream, p, frame_of(tile), view_cell(m, tile),
                       (const int*)workspace + (size_t)tile_index * n_blocks, (long)n, q_index, coord, cell);
    return launch_status("view_select");
}

// ---- members in blocks ------------------------------------------------------------------------------------------------------------------
extern "C" int ciaosr_view_block_blocks(void) { return kViewThreads; }

extern "C" size_t ciaosr_view_blocks_workspace_bytes(int Hv, int Wv, int n_tiles) {
    if (Hv <= 0 || Wv <= 0 || n_tiles <= 0 || (long)Hv * Wv > (long)INT_MAX) return 0;
    return 2 * (size_t)n_tiles * (size_t)view_block_wgs(Hv, Wv) * sizeof(int);
}

extern "C" int ciaosr_view_count_blocks_i32(const double* m, int Hv, int Wv, const int* tiles, int n_tiles, int* counts, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(view_ok(m, Hv, Wv) && tiles && n_tiles > 0 && n_tiles <= INT_MAX / 2 && counts && workspace && aligned16(tiles));
    CIAOSR_CHECK_ARG(((size_t)workspace & 3) == 0);
    if (workspace_bytes < ciaosr_view_blocks_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("view_count_blocks", (hipStream_t)stream);
    const int n_wg = view_block_wgs(Hv, Wv);
    hipLaunchKernelGGL(view_count_blocks_kernel, dim3(n_wg), dim3(kViewThreads), 0, (hipStream_t)stream, view_p(m, Hv, Wv), tiles, n_tiles, n_wg,
                       (int*)workspace);
    // the rows (2 t, 2 t + 1) are scanned like 2 n_tiles tiles' rows: counts[2 t] members, counts[2 t + 1] live blocks
    hipLaunchKernelGGL(view_scan_kernel, dim3(2 * n_tiles), dim3(kWave), 0, (hipStream_t)stream, (int*)workspace, n_wg, counts);
    return launch_status("view_count_blocks");
}

extern "C" size_t ciaosr_view_blocks_many_workspace_bytes(const int* sizes, int n_views, int n_tiles) {
    return view_many_offset(sizes, n_views, n_tiles, n_views, ciaosr_view_blocks_workspace_bytes);
}

extern "C" size_t ciaosr_view_blocks_many_workspace_offset(const int* sizes, int n_views, int n_tiles, int view) {
    if (view < 0 || view >= n_views) return 0;
    return view_many_offset(sizes, n_views, n_tiles, view, ciaosr_view_blocks_workspace_bytes);
}

extern "C" int ciaosr_view_count_blocks_many_i32(const double* m, const int* sizes, int n_views, const int* tiles, int n_tiles, int* counts,
                                                 void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(m && sizes && n_views > 0 && tiles && n_tiles > 0 && counts && workspace && aligned16(tiles));
    CIAOSR_CHECK_ARG(((size_t)workspace & 3) == 0 && 2L * n_views * n_tiles <= (long)INT_MAX);
    for (int v = 0; v < n_views; ++v) CIAOSR_CHECK_ARG(view_ok(m + 6 * v, sizes[2 * v], sizes[2 * v + 1]));
    const size_t need = ciaosr_view_blocks_many_workspace_bytes(sizes, n_views, n_tiles);
    if (!need || workspace_bytes < need) return CIAOSR_ERR_WORKSPACE;
    ProfScope prof("view_count_blocks_many", (hipStream_t)stream);
    size_t off = 0;
    for (int v0 = 0; v0 < n_views; v0 += kViewMany) {
        ViewManyP a = {};
        a.n_views = n_views - v0 < kViewMany ? n_views - v0 : kViewMany;
        for (int k = 0; k < a.n_views; ++k) {
            const int v = v0 + k;
            a.p[k] = view_p(m + 6 * v, sizes[2 * v], sizes[2 * v + 1]);
            a.first[k + 1] = a.first[k] + view_block_wgs(sizes[2 * v], sizes[2 * v + 1]);
            a.part[k] = off / sizeof(int);
            off += view_many_align(ciaosr_view_blocks_workspace_bytes(sizes[2 * v], sizes[2 * v + 1], n_tiles));
        }
        for (int k = a.n_views; k < kViewMany; ++k) a.first[k + 1] = a.first[a.n_views];
        hipLaunchKernelGGL(view_count_blocks_many_kernel, dim3(a.first[a.n_views]), dim3(kViewThreads), 0, (hipStream_t)stream, a, tiles, n_tiles,
                           (int*)workspace);
        // a wave per (view, row): 2 n_tiles rows per view
        hipLaunchKernelGGL(view_scan_many_kernel, dim3(a.n_views * 2 * n_tiles), dim3(kWave), 0, (hipStream_t)stream, a, 2 * n_tiles,
                           (int*)workspace, counts + (size_t)v0 * 2 * n_tiles);
    }
    return launch_status("view_count_blocks_many");
}

extern "C" int ciaosr_view_select_blocks_f32(const double* m, int Hv, int Wv, const int* tile, int tile_index, int n_tiles, const void* workspace,
                                             size_t workspace_bytes, int n_blocks, int* q_index, float* coord, float* cell, void* stream) {
    CIAOSR_CHECK_ARG(view_ok(m, Hv, Wv) && frame_ok(tile) && n_tiles > 0 && tile_index >= 0 && tile_index < n_tiles && workspace);
    CIAOSR_CHECK_ARG(n_blocks > 0 && n_blocks <= INT_MAX / kViewBlockQ && q_index && coord && cell);
    if (workspace_bytes < ciaosr_view_blocks_workspace_bytes(Hv, Wv, n_tiles)) return CIAOSR_ERR_WORKSPACE;
    const int n_wg = view_block_wgs(Hv, Wv);
    CIAOSR_CHECK_ARG((long)n_blocks <= (long)n_wg * kViewThreads);
    ProfScope prof("view_select_blocks", (hipStream_t)stream);
    hipLaunchKernelGGL(view_select_blocks_kernel, dim3(n_wg), dim3(kViewThreads), 0, (hipStream_t)stream, view_p(m, Hv, Wv), frame_of(tile),
                       view_cell(m, tile), (const int*)workspace + ((size_t)tile_index * 2 + 1) * n_wg, (long)n_blocks, q_index, coord, cell);
    return launch_status("view_select_blocks");
}

extern "C" int ciaosr_view_blend_f32(float* E, float* Wt, int Q, const int* q_index, const float* rgb, int n, void* stream) {
    CIAOSR_CHECK_ARG(E && Wt && rgb && Q > 0 && n > 0 && (q_index || n <= Q));       // a block list with its pads can be longer than Q
    ProfScope prof("view_blend", (hipStream_t)stream);
    hipLaunchKernelGGL(view_blend_kernel, dim3(view_grid(n)), dim3(256), 0, (hipStream_t)stream, E, Wt, (long)Q, q_index, rgb, (long)n);
    return launch_status("view_blend");
}

extern "C" int ciaosr_view_finalize_f32(const float* E, const float* Wt, float* out_q3, int Q, const float* fill3, const float* mean3,
                                        const float* std3, void* stream) {
    CIAOSR_CHECK_ARG(E && Wt && out_q3 && Q > 0 && fill3 && mean3 && std3);
    Fill3 fill;
    for (int c = 0; c < 3; ++c) {
        CIAOSR_CHECK_ARG(fill3[c] >= 0.f && fill3[c] <= 1.f && std::isfinite(mean3[c]) && std::isfinite(std3[c]) && std3[c] != 0.f);
        fill.v[c] = fill_preimage(fill3[c], mean3[c], std3[c]);
    }
    ProfScope prof("view_finalize", (hipStream_t)stream);
    hipLaunchKernelGGL(view_finalize_kernel, dim3(view_grid(3L * Q)), dim3(256), 0, (hipStream_t)stream, E, Wt, out_q3, (long)Q, fill);
    return launch_status("view_finalize");
}
