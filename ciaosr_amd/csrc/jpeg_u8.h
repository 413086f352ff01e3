// What the JPEG translation units share (jpeg_u8.hip: baseline and optimised files; jpeg_prog_u8.hip: progressive files): the table
// that the host uploads, the kernels' parameter block, the host's parts of a call (request and argument check, crop geometry, the
// plan's common half, the stream workspace, work_bytes, launch, the driver's prologue and the launchers of the kernels of jpeg_u8.hip
// that the progressive path runs unchanged), the workgroup sums and scans, and libjpeg's table construction for one wave.
#pragma once
#include <climits>
#include <cstdint>
#include <vector>

#include "ops.h"

namespace ciaosr {
namespace jpeg {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kHuff = 272;                         // per table class: 256 AC entries by (run << 4 | size), then 12 DC entries by size
constexpr int kDhtRecord = CIAOSR_JPEG_DHT_RECORD_BYTES;   // 16 counts, 256 symbols (padded with zeros)
constexpr int kMaxDepth = 64;                      // code sizes before limiting: a depth d needs Fibonacci(d + 2) symbols, so < 44 below the limit
constexpr u64 kFreqLimit = 1000000000ull;          // a crop is refused when 64 x its blocks reaches this

struct Consts {
    int qdiv[2][64];                               // 8 x quantisation table, natural order; [0] luma, [1] chroma
    u32 huff[2][kHuff];                            // length << 16 | code
    int zig_of_nat[64];                            // position in zigzag order of the natural index row * 8 + column
};
struct TileT {
    int y0, x0, h, w;
    int mx, nmcu;                                  // MCUs per row, MCUs
    u32 first_chunk, block0;                       // its first chunk, its first block in scan order
};
struct ChunkT {
    int tile, mcu0, mcu1, pad_;
};

struct Params {
    const unsigned char* src;     // [H][pitch], 3 bytes per pixel (grey: 1)
    size_t pitch;
    int bgr, sub420, nt, nc;
    const Consts* consts;
    const TileT* tiles;
    const ChunkT* chunks;
    short* coef;                  // [blocks][64], zigzag order, blocks in scan order
    u32* block_bits;              // [blocks]
    u64* chunk_bits;              // [nc]
    u64* chunk_sum;               // [nc + 1]: prefix sum of chunk_bits
    u64* chunk_bitoff;            // [nc]: the chunk's first bit in the unstuffed buffer
    u64* chunk_b0;                // [nc]: the unstuffed bytes [b0, b1) that the chunk owns
    u64* chunk_b1;
    u32* chunk_pad;               // [nc]: 1-bits to OR into byte b1 - 1 (a tile's last byte), else 0
    u64* chunk_out;               // [nc]: bytes + 0xFF count of the chunk, then (in place) its final offset; [nc] = the total
    u64* tile_ubase;              // [nt]: the tile's first byte in the unstuffed buffer (4-byte aligned)
    u64* utotal;                  // [1]: bytes of the unstuffed buffer in use (a multiple of 4)
    u32* ubuf;                    // the unstuffed streams
    unsigned char* out;
    u64* tile_offs;               // [nt + 1]
    u64* total;                   // optional: tile_offs[nt] once more
    // optimised coding only (null otherwise)
    u32* tile_hist;               // [nt][4][256]: symbol counts per table, in the file's order of tables (kTables)
    u32* tile_huff;               // [nt][2][kHuff]: the tile's code tables in the layout of Consts::huff
    unsigned char* dht;          // [nt][4][kDhtRecord]: the tables as DHT segments hold them
    int grey;                     // one component (CIAOSR_JPEG_GREY): src holds one byte per pixel, one block per MCU, table class 0
};

// jpeg_u8.hip: the constants of a quality, and its kernels that every kind of file runs.  To jpeg_scan, jpeg_zero, jpeg_ffcount,
// jpeg_scan2 and jpeg_stuff a "tile" is one padded stream of the output and a chunk a run of blocks whose bits chunk_bits holds.
void make_consts(int quality, Consts* c);
int launch_coef(const Params& p, hipStream_t s);                           // jpeg_coef, one workgroup per chunk of p
int launch_scan_zero(const Params& p, size_t ubytes, hipStream_t s);       // jpeg_scan, jpeg_zero: the counted bits -> the places, a zeroed buffer
int launch_stuff(const Params& p, hipStream_t s);                          // jpeg_ffcount, jpeg_scan2, jpeg_stuff: the packed streams -> the output

static inline bool image_ok(int H, int W) { return H > 0 && W > 0 && H <= 65535 && W <= 65535; }
// the scan's layout as the plans name it
enum { kMode444 = 0, kMode420 = 1, kModeGrey = 2 };
static inline int default_mcus(int mode) { return mode == kModeGrey ? 768 : (mode ? 128 : 256); }     // 768 blocks per chunk
static inline int chunk_mcus(int mcus_arg, int mode) { return mcus_arg > 0 ? mcus_arg : default_mcus(mode); }
// the ABI's subsampling code -> kMode444, kMode420, kModeGrey, -1 (unknown)
static inline int sub_of(int subsampling) {
    return subsampling == CIAOSR_JPEG_444 ? kMode444 : (subsampling == CIAOSR_JPEG_420 ? kMode420 : (subsampling == CIAOSR_JPEG_GREY ? kModeGrey : -1));
}
static inline int blocks_per_mcu(int mode) { return mode == kModeGrey ? 1 : (mode ? 6 : 3); }
// bytes per pixel of the source that the ABI's subsampling code names
static inline size_t source_bytes(int subsampling) { return subsampling == CIAOSR_JPEG_GREY ? 1 : 3; }

// ---- the host's parts: what a call asks for, the crops' geometry, the workspace of the streams, the driver's prologue ---------------
struct Request {
    const unsigned char* src;
    size_t pitch;
    int H, W, bgr;                // H, W <= 0: the rects are not held against an image
    const int* rects;             // [n][4]: y0, x0, h, w
    int n, quality, mode, mcus;   // mode: kMode*, or -1; mcus: MCUs per chunk, 0 = default_mcus
};
// the H x W image as a rect list of one: the H x W forms of the entries forward to the rect forms
struct Whole {
    int rect[4];
    Whole(int H, int W) : rect{0, 0, H, W} {}
};
// what a size export plans: the geometry alone
static inline Request size_request(const int* rects, int n_tiles, int subsampling, int mcus_per_chunk) {
    return Request{nullptr, 0, 0, 0, 0, rects, n_tiles, 50, sub_of(subsampling), mcus_per_chunk};
}
// The argument check of every *_encode_tiles_u8 entry (`result`: where the offsets go), then the request.
static inline int checked_request(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles, int quality,
                                  int subsampling, int mcus_per_chunk, const void* out, const void* result, const void* workspace, Request* r) {
    CIAOSR_CHECK_ARG(src && rects && out && result && workspace && n_tiles > 0 && image_ok(H, W) && pitch >= source_bytes(subsampling) * (size_t)W);
    CIAOSR_CHECK_ARG((bgr == 0 || bgr == 1) && mcus_per_chunk >= 0 && quality >= 1 && quality <= 100);
    CIAOSR_CHECK_ARG(sub_of(subsampling) >= 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(result) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    *r = Request{src, pitch, H, W, bgr, rects, n_tiles, quality, sub_of(subsampling), mcus_per_chunk};
    return CIAOSR_OK;
}

// One rect in a mode.  CIAOSR_ERR_BAD_ARG: it is empty, too large or leaves the image; CIAOSR_ERR_UNSUPPORTED (`limited` only): its scan
// reaches the frequency limit.
struct Crop {
    int side, mx, nmcu;           // the MCU's side, MCUs per row, MCUs
    u64 blocks;
};
static inline int crop_of(const int* rect, int mode, int H, int W, bool limited, Crop* c) {
    const int y0 = rect[0], x0 = rect[1], h = rect[2], w = rect[3];
    if (!image_ok(h, w) || y0 < 0 || x0 < 0) return CIAOSR_ERR_BAD_ARG;
    if (H > 0 && ((long)y0 + h > H || (long)x0 + w > W)) return CIAOSR_ERR_BAD_ARG;
    c->side = mode == kMode420 ? 16 : 8;
    c->mx = ceil_div(w, c->side);
    c->nmcu = c->mx * ceil_div(h, c->side);
    c->blocks = (u64)c->nmcu * (u64)blocks_per_mcu(mode);
    return limited && 64ull * c->blocks >= kFreqLimit ? CIAOSR_ERR_UNSUPPORTED : CIAOSR_OK;
}

// What every plan holds.  The table as the device reads it begins [Consts][crops TileT nt][jpeg_coef's chunks ChunkT ncc]; a stream is
// one padded run of the output (baseline and optimised: a crop's scan, so ns = nt and nc = ncc; progressive: one of its ten scans).
struct CropPlan {
    int rc;                       // CIAOSR_OK, or why the rects cannot be coded
    int mode, per;                // kMode*; MCUs per chunk of jpeg_coef
    int nt, ncc, ns, nc;          // crops, jpeg_coef's chunks, streams, chunks of the streams
    u64 blocks;
    size_t capacity, ubytes;      // the stuffed worst case; the unstuffed one, every stream rounded up to 4 bytes
    size_t o_crops, o_cchunks, table_bytes;
};
// Validates the request and every rect, sums the crops; each(crop, h, w) adds what the caller sums besides.  A bad argument wins over a
// refusal.  Leaves table_bytes at the end of jpeg_coef's chunks.
template <typename F>
static inline void plan_crops(const Request& r, bool limited, CropPlan* t, F each) {
    t->rc = CIAOSR_ERR_BAD_ARG;
    if (!r.rects || r.n < 1 || r.mcus < 0 || r.quality < 1 || r.quality > 100 || r.mode < kMode444 || r.mode > kModeGrey) return;
    t->mode = r.mode;
    t->per = chunk_mcus(r.mcus, r.mode);
    u64 ncc = 0;
    int rc = CIAOSR_OK;
    for (int k = 0; k < r.n; ++k) {
        Crop c;
        const int one = crop_of(r.rects + 4 * k, r.mode, r.H, r.W, limited, &c);
        if (one == CIAOSR_ERR_BAD_ARG) return;
        if (one != CIAOSR_OK) rc = one;
        ncc += ((u64)c.nmcu + t->per - 1) / t->per;
        t->blocks += c.blocks;
        each(c, r.rects[4 * k + 2], r.rects[4 * k + 3]);
    }
    if (ncc > (u64)INT_MAX / 2 || t->blocks > (u64)INT_MAX) rc = CIAOSR_ERR_UNSUPPORTED;
    t->rc = rc;
    t->nt = r.n;
    t->ncc = (int)ncc;
    t->o_crops = sizeof(Consts);
    t->o_cchunks = t->o_crops + sizeof(TileT) * (size_t)r.n;
    t->table_bytes = t->o_cchunks + sizeof(ChunkT) * (size_t)ncc;
}
// the streams of an accepted plan: `bytes` = the most that all of them hold before stuffing
static inline void plan_streams(CropPlan* t, u64 ns, u64 nc, u64 bytes) {
    t->ns = (int)ns;
    t->nc = (int)nc;
    t->capacity = (size_t)(2 * bytes);
    t->ubytes = (size_t)bytes + 4 * (size_t)ns;
}
// the head of the table: the constants of the quality, the crops, jpeg_coef's chunks of `per` MCUs of ONE crop each
static inline void fill_crops(const Request& r, const CropPlan& t, unsigned char* table) {
    make_consts(r.quality, reinterpret_cast<Consts*>(table));
    TileT* tiles = reinterpret_cast<TileT*>(table + t.o_crops);
    ChunkT* chunks = reinterpret_cast<ChunkT*>(table + t.o_cchunks);
    u32 c = 0, blk = 0;
    for (int k = 0; k < r.n; ++k) {
        const int* rect = r.rects + 4 * k;
        Crop g;
        crop_of(rect, t.mode, 0, 0, false, &g);
        tiles[k] = TileT{rect[0], rect[1], rect[2], rect[3], g.mx, g.nmcu, c, blk};
        for (int m = 0; m < g.nmcu; m += t.per, ++c) chunks[c] = ChunkT{k, m, m + t.per < g.nmcu ? m + t.per : g.nmcu, 0};
        blk += (u32)g.blocks;
    }
}

// The arrays that both coders carve: the table, the coefficients, and what jpeg_scan .. jpeg_stuff keep per chunk and stream.  ubuf is
// the last take (Arena::take aligns before a take and does not round the last one: what follows it decides the exported size).
struct StreamWork {
    unsigned char* table;
    short* coef;
    u32 *chunk_pad, *ubuf;
    u64 *chunk_bits, *chunk_sum, *chunk_bitoff, *chunk_b0, *chunk_b1, *chunk_out, *tile_ubase, *utotal;
    void carve_head(Arena& a, const CropPlan& t) {
        table = a.take<unsigned char>(t.table_bytes);
        coef = a.take<short>(64 * (size_t)t.blocks);
    }
    void carve_streams(Arena& a, const CropPlan& t) {
        const size_t nc = (size_t)t.nc;
        chunk_pad = a.take<u32>(nc);
        chunk_bits = a.take<u64>(nc);
        chunk_sum = a.take<u64>(nc + 1);
        chunk_bitoff = a.take<u64>(nc);
        chunk_b0 = a.take<u64>(nc);
        chunk_b1 = a.take<u64>(nc);
        chunk_out = a.take<u64>(nc + 1);
        tile_ubase = a.take<u64>((size_t)t.ns);
        utotal = a.take<u64>(1);
        ubuf = a.take<u32>((t.ubytes + 3) / 4);
    }
    // jpeg_coef's parameters: the crops and their chunks of MCUs
    Params coef_params(const Request& r, const CropPlan& t) const {
        Params p{};
        p.src = r.src;
        p.pitch = r.pitch;
        p.bgr = r.bgr;
        p.sub420 = t.mode == kMode420;
        p.grey = t.mode == kModeGrey;
        p.nt = t.nt;
        p.nc = t.ncc;
        p.consts = reinterpret_cast<const Consts*>(table);
        p.tiles = reinterpret_cast<const TileT*>(table + t.o_crops);
        p.chunks = reinterpret_cast<const ChunkT*>(table + t.o_cchunks);
        p.coef = coef;
        return p;
    }
    void bind_streams(Params* p) const {
        p->chunk_bits = chunk_bits;
        p->chunk_sum = chunk_sum;
        p->chunk_bitoff = chunk_bitoff;
        p->chunk_b0 = chunk_b0;
        p->chunk_b1 = chunk_b1;
        p->chunk_pad = chunk_pad;
        p->chunk_out = chunk_out;
        p->tile_ubase = tile_ubase;
        p->utotal = utotal;
        p->ubuf = ubuf;
    }
};

// W: a coder's workspace, with carve(Arena&, const P&) over its plan P.  Offsets only: nothing is dereferenced.
template <typename W, typename P>
static inline size_t work_bytes(const P& t) {
    if (t.rc != CIAOSR_OK) return 0;
    static char origin[1];
    Arena a(origin, ~(size_t)0);
    W w;
    w.carve(a, t);
    return a.off;
}

template <typename K, typename P>
static inline int launch(const char* tag, K kernel, int grid, const P& p, hipStream_t s) {
    ProfScope prof(tag, s);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, s, p);
    return launch_status(tag);
}

// The driver's prologue, every check that the host can make before the first launch: a bad argument, another refusal of the plan, the
// output's capacity, the workspace's size; then the carve and the table's upload.
template <typename W, typename P>
static inline int prepare(const P& t, const std::vector<unsigned char>& table, size_t out_capacity, void* workspace, size_t workspace_bytes,
                          hipStream_t s, W* w) {
    CIAOSR_CHECK_ARG(t.rc != CIAOSR_ERR_BAD_ARG);             // a rect is empty or leaves the image; quality; subsampling
    if (t.rc != CIAOSR_OK) return t.rc;
    if (out_capacity < t.capacity) return CIAOSR_ERR_WORKSPACE;
    Arena a(workspace, workspace_bytes);
    w->carve(a, t);
    if (!a.ok) return CIAOSR_ERR_WORKSPACE;
    // from pageable memory: the copy has left `table` when the call returns
    return hipMemcpyAsync(w->s.table, table.data(), t.table_bytes, hipMemcpyHostToDevice, s) == hipSuccess ? CIAOSR_OK : CIAOSR_ERR_LAUNCH;
}

// ---- device helpers --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// sum of v over the workgroup, in every lane
__device__ __forceinline__ u64 wg_sum_u64(u64 v, u64* red /* LDS [kWaves] */) {
    const int tid = threadIdx.x;
    v = wave_sum_u64(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    u64 s = 0ull;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w];
    return s;
}

// exclusive prefix sum of v over the workgroup's lanes; *total = the sum
__device__ __forceinline__ u32 wg_scan_u32(u32 v, u32* wsum /* LDS [kWaves] */, u32* total) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    u32 inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const u32 t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
    __syncthreads();
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    u32 before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    *total = all;
    return before + inc - v;
}

// One workgroup: out[i] = sum of in[0 .. i) for i in [0, n], lane t owning a run of ceil(n / kThreads) elements.
__device__ __forceinline__ void wg_prefix_u64(const u64* in, u64* out, int n, u64* tot /* LDS [kThreads] */) {
    const int tid = threadIdx.x;
    const int per = (n + kThreads - 1) / kThreads;
    const int i0 = min(n, tid * per), i1 = min(n, i0 + per);
    u64 sum = 0ull;
    for (int i = i0; i < i1; ++i) sum += in[i];
    __syncthreads();
    tot[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0ull;
        for (int t = 0; t < kThreads; ++t) {
            const u64 v = tot[t];
            tot[t] = run;
            run += v;
        }
        out[n] = run;
    }
    __syncthreads();
    u64 off = tot[tid];
    for (int i = i0; i < i1; ++i) {
        const u64 v = in[i];
        out[i] = off;
        off += v;
    }
    __syncthreads();
}

__device__ __forceinline__ int bpm_of(const Params& p) { return p.grey ? 1 : (p.sub420 ? 6 : 3); }      // blocks per MCU

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }       // a >= 0; 0 -> 0

// the quantised DC that block j of the chunk's tile predicts from: the previous block of its component in scan order, 0 at the start
__device__ __forceinline__ int dc_pred(const Params& p, const TileT& t, u64 blk) {
    const int bpm = bpm_of(p);
    const u64 rel = blk - t.block0;
    const int k = (int)(rel % bpm);
    const u64 mcu = rel / bpm;
    u64 prev;
    if (p.sub420 && k > 0 && k < 4) {
        prev = blk - 1;
    } else {
        if (mcu == 0) return 0;
        prev = (p.sub420 && k == 0) ? blk - 3 : blk - bpm;
    }
    return (int)p.coef[prev * 64ull];
}

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, kWave);
        v = o < v ? o : v;
    }
    return v;
}

// One wave makes one Huffman table from the histogram hist[256] by libjpeg's rule; every wave of the workgroup calls
// it together (it synchronises the workgroup).  Lane l holds the symbols 4 l .. 4 l + 3, lane 0 also the pseudo-symbol 256 of frequency
// 1 that reserves the all-ones code.  A group of merged symbols is named by the one index that carries its frequency; the smaller of
// two groups is found as the wave's minimum of frequency << 9 | (256 - index): by frequency, ties to the larger index.  Integer only.
// It leaves size_of[symbol] = length << 16 | code (0: the symbol has no code), nbits[len] = the codes of length len = 1..16, and
// vals[] = the symbols in code order.
__device__ __forceinline__ void build_table(const u32* hist, u32* size_of /* LDS [256] */, u32* nbits /* LDS [kMaxDepth] */,
                                            unsigned char* vals /* LDS [256] */, int lane) {
    constexpr u64 kNone = ~0ull;
    u32 freq[5], size[5];
    int index[5], group[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        index[s] = s < 4 ? 4 * lane + s : 256 + lane;      // slot 4 is a symbol in lane 0 only
        freq[s] = s < 4 ? hist[index[s]] : (lane == 0 ? 1u : 0u);
        size[s] = 0u;
        group[s] = index[s];
    }
    for (;;) {
        u64 key[5], k1 = kNone, k2 = kNone;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            key[s] = freq[s] ? ((u64)freq[s] << 9) | (u64)(u32)(256 - index[s]) : kNone;
            k1 = key[s] < k1 ? key[s] : k1;
        }
        const u64 m1 = wave_min_u64(k1);
#pragma unroll
        for (int s = 0; s < 5; ++s)
            if (key[s] != m1 && key[s] < k2) k2 = key[s];
        const u64 m2 = wave_min_u64(k2);
        if (m2 == kNone) break;                             // one group is left
        const int c1 = 256 - (int)(m1 & 511ull), c2 = 256 - (int)(m2 & 511ull);
        const u32 sum = (u32)(m1 >> 9) + (u32)(m2 >> 9);
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            if (index[s] == c1) freq[s] = sum;
            if (index[s] == c2) freq[s] = 0u;
            if (group[s] == c1 || group[s] == c2) {
                ++size[s];
                group[s] = c1;
            }
        }
    }
    if (lane < kMaxDepth) nbits[lane] = 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) size_of[index[s]] = size[s];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 5; ++s)
        if (size[s]) atomicAdd(&nbits[min(size[s], (u32)(kMaxDepth - 1))], 1u);
    __syncthreads();
    if (lane == 0) {                                        // limiting to 16 bits, then the reserved code leaves
        u32* b = nbits;
        for (int i = kMaxDepth - 1; i > 16; --i)
            while (b[i] >= 2u) {
                int j = i - 2;
                while (j > 0 && b[j] == 0u) --j;
                if (j == 0) break;
                b[i] -= 2u;
                b[i - 1] += 1u;
                b[j + 1] += 2u;
                b[j] -= 1u;
            }
        int i = 16;
        while (i > 0 && b[i] == 0u) --i;
        if (i > 0) b[i] -= 1u;
    }
    // the code order: by size BEFORE limiting, then by symbol; the place of a symbol is the number of symbols before it
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const u32 c = size[s];
        if (c == 0u) continue;
        int before = 0;
        for (int j = 0; j < 256; ++j) {
            const u32 cj = size_of[j];
            before += (cj != 0u && (cj < c || (cj == c && j < index[s]))) ? 1 : 0;
        }
        vals[before] = (unsigned char)index[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) size_of[index[s]] = 0u;
    __syncthreads();
    if (lane == 0) {                                        // canonical codes from the counts and that order
        u32 code = 0u;
        int at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (u32 i = 0; i < nbits[len] && at < 256; ++i, ++at, ++code) size_of[vals[at]] = ((u32)len << 16) | code;
            code <<= 1;
        }
    }
    __syncthreads();
}

// the DHT record of a table that build_table left: 16 counts, then the symbols in code order, zeros behind the last
__device__ __forceinline__ void write_dht_record(unsigned char* rec /* [kDhtRecord] */, const u32* nbits, const unsigned char* vals, int lane) {
    int count = 0;
    for (int len = 1; len <= 16; ++len) count += (int)nbits[len];
    if (lane < 16) rec[lane] = (unsigned char)nbits[lane + 1];
    u32 word = 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (4 * lane + s < count) word |= (u32)vals[4 * lane + s] << (8 * s);
    reinterpret_cast<u32*>(rec + 16)[lane] = word;
}

}  // namespace jpeg
}  // namespace ciaosr
