// What the JPEG translation units share (jpeg_u8.hip: baseline and optimised files; jpeg_prog_u8.hip: progressive files): the table
// that the host uploads, the kernels' parameter block, the workgroup sums and scans, libjpeg's table construction for one wave, and
// the launchers of the kernels of jpeg_u8.hip that the progressive path runs unchanged.
#pragma once
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
enum Shared { kCoefKernel, kScanKernel, kZeroKernel, kFfcountKernel, kScan2Kernel, kStuffKernel };
int launch_shared(Shared which, int grid, const Params& p, hipStream_t s);
constexpr int kZeroGroups = 1024;

static inline bool image_ok(int H, int W) { return H > 0 && W > 0 && H <= 65535 && W <= 65535; }
// the scan's layout as the plans name it (`sub420` where only the first two can occur)
enum { kMode444 = 0, kMode420 = 1, kModeGrey = 2 };
static inline int default_mcus(int mode) { return mode == kModeGrey ? 768 : (mode ? 128 : 256); }     // 768 blocks per chunk
// the ABI's subsampling code -> kMode444, kMode420, kModeGrey, -1 (unknown)
static inline int sub_of(int subsampling) {
    return subsampling == CIAOSR_JPEG_444 ? kMode444 : (subsampling == CIAOSR_JPEG_420 ? kMode420 : (subsampling == CIAOSR_JPEG_GREY ? kModeGrey : -1));
}
static inline int blocks_per_mcu(int mode) { return mode == kModeGrey ? 1 : (mode ? 6 : 3); }

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
