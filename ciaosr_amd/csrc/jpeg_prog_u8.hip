// Progressive JPEG files of an 8-bit image coded on the device (ciaosr_amd/jpeg_hip.py `progressive=True`): libjpeg's progressive
// entropy coder (jcphuff.c) under the ten-scan script that Pillow's `progressive=True` selects, every scan with a Huffman table made
// from its own symbols, so that the files are byte for byte `PIL.Image.save(format='JPEG', quality=q, subsampling=0 | 2,
// progressive=True)`'s.  DESIGN 4.1i-e holds the contract.  The coefficients are jpeg_coef's (jpeg_u8.hip), unchanged.
//
// A crop's ten scans are ten padded streams of the output; an ITEM is one block of one scan (a DC scan walks the interleaved MCU order,
// dummy blocks included; an AC scan one component's real blocks in raster order) and a chunk is a run of items of ONE scan of one
// crop.  To jpeg_scan, jpeg_zero, jpeg_ffcount, jpeg_scan2 and jpeg_stuff of jpeg_u8.hip, which run unchanged, the 10 n streams are
// 10 n "tiles".  Thirteen launches and one memset, whatever the number of crops:
//   jpeg_coef     (jpeg_u8.hip)
//   prog_summary  one lane per AC item: does the block emit a symbol of its own, does it end in the EOB run, and how many correction
//                 bits its tail leaves buffered (one byte per item); per chunk, whether it holds nothing but empty EOB blocks.
//   prog_runs     an EOB run is state carried from block to block, but every block that emits a symbol resets it: one lane per
//                 SEGMENT HEAD (such a block, or the scan's first) walks the summaries up to the next head and follows libjpeg's
//                 greedy rule -- flush at 0x7FFF blocks or above 937 buffered bits -- marking the block that owns each flush (after
//                 itself: `post`; before its first symbol: `pre`) with the run's length and bits, and every member that has bits
//                 with the run's first block and the place of its bits in the run.  A chunk of nothing but empty EOB blocks is passed
//                 in one step.  The only single-lane walk, in a kernel of its own.
//   prog_hist     one lane per item: the chunk's symbols, the flushes its blocks own included, counted in LDS, then added to the crop's
//                 ten histograms with integer atomicAdd (zeroed by the memset).
//   prog_tables   one wave per table: build_table (jpeg_u8.h) -> the code tables and the DHT records.
//   prog_count    one lane per item: its bits with those codes; an owned flush counts with all the correction bits of its run.
//   jpeg_scan, jpeg_zero   (jpeg_u8.hip)
//   prog_pack     one lane per item, placed by a workgroup scan: its own symbols and flushes through atomicOr; behind a flush's EOBn
//                 symbol it leaves the gap of the run's correction bits and records where the gap begins.
//   prog_corr     one lane per member of a run: its tail's correction bits into the gap, at the place prog_runs gave it.
//   jpeg_ffcount, jpeg_scan2, jpeg_stuff   (jpeg_u8.hip)
// No floating point; the bytes do not depend on mcus_per_chunk, on the stream, on the list, or on what the workspace held.
#include <climits>
#include <cstring>
#include <vector>

#include "jpeg_u8.h"

namespace ciaosr {
namespace jpeg {

constexpr int kScans = 10;                         // streams per crop, and tables per crop (two for scan 1, none for scan 7)
constexpr u32 kMaxRun = 0x7fffu;                   // libjpeg flushes an EOB run that reaches this many blocks
constexpr u32 kMaxCorr = 937u;                     // ... or that buffers more correction bits than MAX_CORR_BITS - DCTSIZE2 + 1

struct ScanDef {
    int comp;                                      // -1: the three components interleaved (DC), else 0 Y, 1 Cb, 2 Cr
    int ss, se, ah, al;
    int table;                                     // the scan's first table among the crop's ten; -1: none
};
#define CIAOSR_PROG_SCRIPT                                                                                                          \
    {{-1, 0, 0, 0, 1, 0}, {0, 1, 5, 0, 2, 2}, {2, 1, 63, 0, 1, 3}, {1, 1, 63, 0, 1, 4}, {0, 6, 63, 0, 2, 5}, {0, 1, 63, 2, 1, 6}, \
     {-1, 0, 0, 1, 0, -1}, {2, 1, 63, 1, 0, 7}, {1, 1, 63, 1, 0, 8}, {0, 1, 63, 1, 0, 9}}
static const ScanDef kScript[kScans] = CIAOSR_PROG_SCRIPT;
__constant__ ScanDef dScript[kScans] = CIAOSR_PROG_SCRIPT;

// the most bits an item of the scan takes with arbitrary codes of up to 16 bits, correction bits charged to the block
// that holds their coefficient
static inline u64 item_bits(const ScanDef& sd) {
    if (sd.comp < 0) return sd.ah ? 1ull : 16ull + 11ull;
    return sd.ah ? 17ull * 63ull + 60ull : 26ull * (u64)(sd.se - sd.ss + 1) + 60ull;
}

struct PParams {
    Params b;                     // streams as tiles {first_chunk, block0 = first item, nmcu = items}, chunks {stream, item0, item1}
    const TileT* crops;           // the crops as jpeg_coef sees them
    unsigned char* summary;       // per item: bit 0 emits a symbol, bit 1 ends in the EOB run, bits 2..7 correction bits of its tail
    u32* chunk_empty;             // per chunk of an AC scan: 1 when every item's summary is 2 (in the run, no symbol, no correction bits)
    u32 per_items;                // items per chunk (a stream's last chunk may have fewer)
    u32* pre;                     // per item: the flush before its first symbol, run length | correction bits << 16; 0: none
    u32* post;                    // per item: the flush behind it
    u32* rstart;                  // per member with correction bits: the first block of its run (item of the scan) ...
    u32* cboff;                   // ... and the correction bits of the run before its own
    u64* corr_pos;                // per run, at its first block: the bit at which its correction bits begin in the unstuffed buffer
    u32* hist;                    // [crops][10][256]
    u32* codes;                   // [crops][10][256]: length << 16 | code by symbol
    unsigned char* dht;           // [crops][10][kDhtRecord]
    int ntables;
};

// ---- one block of one scan --------------------------------------------------------------------------------------------------------
// Walks the band of an AC scan: s.symbol(0, index, extra, n), s.raw(bits, n) for correction bits emitted inside the block.  Returns the
// item's summary; *tail = the correction bits that stay buffered behind its last symbol, first bit highest.
template <typename S>
__device__ __forceinline__ u32 walk_ac(const short* cf, const ScanDef& sd, S& s, u64* tail) {
    const uint4* v4 = reinterpret_cast<const uint4*>(cf);
    int eob = 0;                                            // refinement: the last coefficient that becomes non-zero in this scan
    if (sd.ah) {
#pragma unroll 1
        for (int g = 0; g < 8; ++g) {
            const uint4 q = v4[g];
            const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = 8 * g + i, v = (int)(short)(w[i >> 1] >> (16 * (i & 1)));
                if (k >= sd.ss && k <= sd.se && (abs(v) >> sd.al) == 1) eob = k;
            }
        }
    }
    int r = 0, nbr = 0;
    u64 br = 0ull;
    bool sym = false;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 q = v4[g];
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 8 * g + i, v = (int)(short)(w[i >> 1] >> (16 * (i & 1)));
            if (k < sd.ss || k > sd.se) continue;
            const int a = abs(v) >> sd.al;
            if (a == 0) {
                ++r;
                continue;
            }
            if (!sd.ah) {
                while (r > 15) {
                    s.symbol(0, 0xf0, 0u, 0);
                    r -= 16;
                }
                const int n = bit_length(a);
                s.symbol(0, (r << 4) | n, (u32)(v > 0 ? a : ~a) & ((1u << n) - 1u), n);
                r = 0;
                sym = true;
                continue;
            }
            while (r > 15 && k <= eob) {
                s.symbol(0, 0xf0, 0u, 0);
                r -= 16;
                s.raw(br, nbr);
                br = 0ull;
                nbr = 0;
            }
            if (a > 1) {
                br = (br << 1) | (u64)(a & 1);
                ++nbr;
                continue;
            }
            s.symbol(0, (r << 4) | 1, v < 0 ? 0u : 1u, 1);
            s.raw(br, nbr);
            br = 0ull;
            nbr = 0;
            r = 0;
            sym = true;
        }
    }
    *tail = br;
    return (sym ? 1u : 0u) | ((r > 0 || nbr > 0) ? 2u : 0u) | ((u32)nbr << 2);
}

// the EOBn symbol of a flush and the gap of its run's correction bits; `start`: the run's first block
template <typename S>
__device__ __forceinline__ void walk_flush(u32 rec, u32 start, S& s) {
    const u32 e = rec & kMaxRun;
    const int n = 31 - __clz(e);
    s.symbol(0, n << 4, e & ((1u << n) - 1u), n);
    s.gap(start, rec >> 16);
}

// the coefficients of item i of a component's AC scan: its blocks in raster order, from the interleaved order that jpeg_coef wrote
__device__ __forceinline__ const short* ac_block(const PParams& p, const TileT& crop, int comp, u32 i) {
    u64 blk;
    if (!p.b.sub420) {
        blk = (u64)crop.block0 + 3ull * i + (u64)comp;
    } else if (comp) {
        blk = (u64)crop.block0 + 6ull * i + 3ull + (u64)comp;
    } else {
        const u32 nbx = (u32)(crop.w + 7) >> 3, by = i / nbx, bx = i % nbx;
        blk = (u64)crop.block0 + 6ull * ((u64)(by >> 1) * (u64)crop.mx + (bx >> 1)) + 2u * (by & 1u) + (bx & 1u);
    }
    return p.b.coef + blk * 64ull;
}

// everything item i of the stream emits, in order
template <typename S>
__device__ __forceinline__ void walk_item(const PParams& p, const TileT& crop, const ScanDef& sd, u32 g0, u32 i, S& s) {
    if (sd.comp < 0) {
        const u64 blk = (u64)crop.block0 + i;
        const int v = (int)p.b.coef[blk * 64ull];
        if (sd.ah) {
            s.raw((u64)((v >> sd.al) & 1), 1);
            return;
        }
        const int d = (v >> sd.al) - (dc_pred(p.b, crop, blk) >> sd.al);
        const int n = bit_length(abs(d));
        const int k = (int)(i % (p.b.sub420 ? 6u : 3u));
        const int cls = p.b.sub420 ? (k < 4 ? 0 : 1) : (k == 0 ? 0 : 1);
        s.symbol(cls, n, (u32)(d < 0 ? d + (1 << n) - 1 : d) & ((1u << n) - 1u), n);
        return;
    }
    const u32 pre = p.pre[g0 + i];
    if (pre) walk_flush(pre, i - (pre & kMaxRun), s);
    u64 tail;
    walk_ac(ac_block(p, crop, sd.comp, i), sd, s, &tail);
    const u32 post = p.post[g0 + i];
    if (post) walk_flush(post, i + 1u - (post & kMaxRun), s);
}

struct Null {
    __device__ __forceinline__ void symbol(int, int, u32, int) {}
    __device__ __forceinline__ void raw(u64, int) {}
    __device__ __forceinline__ void gap(u32, u32) {}
};
struct Tally {
    u32* hist;                     // LDS [2][256]
    __device__ __forceinline__ void symbol(int t, int index, u32, int) { atomicAdd(&hist[t * 256 + index], 1u); }
    __device__ __forceinline__ void raw(u64, int) {}
    __device__ __forceinline__ void gap(u32, u32) {}
};
struct Counter {
    const u32* tab;                // LDS [2][256]
    u32 bits;
    __device__ __forceinline__ void symbol(int t, int index, u32, int n) { bits += (tab[t * 256 + index] >> 16) + (u32)n; }
    __device__ __forceinline__ void raw(u64, int n) { bits += (u32)n; }
    __device__ __forceinline__ void gap(u32, u32 be) { bits += be; }
};
// MSB-first into 32-bit words of the zeroed buffer.  Every word goes through atomicOr: the gap behind a flush is filled by other lanes
// (prog_corr), and integer OR does not depend on arrival order.  A byte stream: word w holds bytes 4 w .. 4 w + 3.
struct BitPacker {
    u32* buf;
    u64 w;
    u64 acc;
    int nacc;
    __device__ __forceinline__ void put(u32 val, int len) {            // len <= 32, nacc < 32
        if (len == 0) return;
        acc |= (u64)val << (64 - nacc - len);
        nacc += len;
        if (nacc >= 32) {
            atomicOr(&buf[w], __builtin_bswap32((u32)(acc >> 32)));
            ++w;
            acc <<= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void skip(u32 n) {
        const u64 tot = (u64)nacc + n;
        if (tot >= 32ull) {
            if (acc) atomicOr(&buf[w], __builtin_bswap32((u32)(acc >> 32)));
            w += tot >> 5;
            acc = 0ull;
        }
        nacc = (int)(tot & 31ull);
    }
    __device__ __forceinline__ u64 pos() const { return w * 32ull + (u64)nacc; }
    __device__ __forceinline__ void finish() {
        if (nacc > 0 && acc) atomicOr(&buf[w], __builtin_bswap32((u32)(acc >> 32)));
    }
};
struct Writer {
    const u32* tab;                // LDS [2][256]
    u64* corr_pos;                 // the stream's
    BitPacker pk;
    __device__ __forceinline__ void symbol(int t, int index, u32 extra, int n) {
        const u32 ent = tab[t * 256 + index];
        pk.put(((ent & 0xffffu) << n) | extra, (int)(ent >> 16) + n);
    }
    __device__ __forceinline__ void raw(u64 bits, int n) {
        while (n > 0) {
            const int m = n < 16 ? n : 16;
            pk.put((u32)(bits >> (n - m)) & ((1u << m) - 1u), m);
            n -= m;
        }
    }
    __device__ __forceinline__ void gap(u32 start, u32 be) {
        corr_pos[start] = pk.pos();
        pk.skip(be);
    }
};

// ---- kernels: one workgroup per chunk ------------------------------------------------------------------------------------------------
struct Where {
    ScanDef sd;
    TileT crop;
    int crop_index;
    u32 g0, n, i0, i1;            // the stream's first item and its items; the chunk's items [i0, i1)
    u32 first_chunk;              // the stream's first chunk
};
__device__ __forceinline__ Where where(const PParams& p) {
    const ChunkT ch = p.b.chunks[blockIdx.x];
    const TileT st = p.b.tiles[ch.tile];
    Where w;
    w.sd = dScript[ch.tile % kScans];
    w.crop_index = ch.tile / kScans;
    w.crop = p.crops[w.crop_index];
    w.g0 = st.block0;
    w.n = (u32)st.nmcu;
    w.i0 = (u32)ch.mcu0;
    w.i1 = (u32)ch.mcu1;
    w.first_chunk = st.first_chunk;
    return w;
}

__global__ __launch_bounds__(kThreads) void prog_summary_kernel(PParams p) {
    const Where w = where(p);
    if (w.sd.comp < 0) return;
    int other = 0;
    for (u32 i = w.i0 + threadIdx.x; i < w.i1; i += kThreads) {
        Null s;
        u64 tail;
        const u32 sum = walk_ac(ac_block(p, w.crop, w.sd.comp, i), w.sd, s, &tail);
        p.summary[w.g0 + i] = (unsigned char)sum;
        other |= sum != 2u;
    }
    other = __syncthreads_or(other);
    if (threadIdx.x == 0) p.chunk_empty[blockIdx.x] = other ? 0u : 1u;
}

// A head's walk: its own tail opens the run, every block up to the next head joins it.  pre and post start from zero (the memset).
__global__ __launch_bounds__(kThreads) void prog_runs_kernel(PParams p) {
    const Where w = where(p);
    if (w.sd.comp < 0) return;
    const unsigned char* sum = p.summary + w.g0;
    for (u32 i = w.i0 + threadIdx.x; i < w.i1; i += kThreads) {
        const u32 s = sum[i];
        if (!(s & 1u) && i != 0u) continue;
        u32 run = 0u, bits = 0u, start = i;
        if (s & 2u) {
            run = 1u;
            bits = s >> 2;
            if (bits) {
                p.rstart[w.g0 + i] = i;
                p.cboff[w.g0 + i] = 0u;
            }
        }
        u32 j = i + 1u;
        while (j < w.n) {
            if (j % p.per_items == 0u && p.chunk_empty[w.first_chunk + j / p.per_items]) {
                u32 left = min(p.per_items, w.n - j);            // a whole chunk of empty EOB blocks: only the 0x7FFF rule can cut
                while (left) {
                    if (run == 0u) start = j;
                    const u32 room = kMaxRun - run;
                    if (left < room) {
                        run += left;
                        j += left;
                        left = 0u;
                    } else {
                        j += room;
                        left -= room;
                        p.post[w.g0 + j - 1u] = kMaxRun | (bits << 16);
                        run = 0u;
                        bits = 0u;
                    }
                }
                continue;
            }
            const u32 sj = sum[j];
            if (sj & 1u) break;
            if (run == 0u) start = j;
            const u32 br = sj >> 2;
            if (br) {
                p.rstart[w.g0 + j] = start;
                p.cboff[w.g0 + j] = bits;
            }
            ++run;
            bits += br;
            if (run == kMaxRun || bits > kMaxCorr) {
                p.post[w.g0 + j] = run | (bits << 16);
                run = 0u;
                bits = 0u;
            }
            ++j;
        }
        if (run) {
            if (j < w.n) p.pre[w.g0 + j] = run | (bits << 16);
            else p.post[w.g0 + w.n - 1u] = run | (bits << 16);
        }
    }
}

__global__ __launch_bounds__(kThreads) void prog_hist_kernel(PParams p) {
    __shared__ u32 hist[2 * 256];
    const Where w = where(p);
    if (w.sd.table < 0) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * 256; i += kThreads) hist[i] = 0u;
    __syncthreads();
    for (u32 i = w.i0 + tid; i < w.i1; i += kThreads) {
        Tally ta{hist};
        walk_item(p, w.crop, w.sd, w.g0, i, ta);
    }
    __syncthreads();
    u32* dst = p.hist + ((size_t)w.crop_index * kScans + w.sd.table) * 256;     // scan 1: its two tables lie side by side
    for (int i = tid; i < (w.sd.comp < 0 ? 2 : 1) * 256; i += kThreads) {
        const u32 v = hist[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

// wave k of workgroup g makes table 4 g + k of the call's 10 n
__global__ __launch_bounds__(kThreads) void prog_tables_kernel(PParams p) {
    __shared__ u32 size_of[kWaves][256];
    __shared__ u32 nbits[kWaves][kMaxDepth];
    __shared__ unsigned char vals[kWaves][256];
    const int tid = threadIdx.x, k = tid >> 6, lane = tid & 63;
    const int table = blockIdx.x * kWaves + k;
    const int t = table < p.ntables ? table : p.ntables - 1;                    // a wave without a table repeats the last, and writes nothing
    build_table(p.hist + (size_t)t * 256, size_of[k], nbits[k], vals[k], lane);
    if (table >= p.ntables) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) p.codes[(size_t)t * 256 + 4 * lane + s] = size_of[k][4 * lane + s];
    write_dht_record(p.dht + (size_t)t * kDhtRecord, nbits[k], vals[k], lane);
}

__device__ __forceinline__ void load_codes(const PParams& p, const Where& w, u32* tab /* LDS [2][256] */) {
    if (w.sd.table >= 0) {
        const u32* src = p.codes + ((size_t)w.crop_index * kScans + w.sd.table) * 256;
        for (int i = threadIdx.x; i < (w.sd.comp < 0 ? 2 : 1) * 256; i += kThreads) tab[i] = src[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void prog_count_kernel(PParams p) {
    __shared__ u32 tab[2 * 256];
    __shared__ u64 red[kWaves];
    const Where w = where(p);
    load_codes(p, w, tab);
    u64 sum = 0ull;
    for (u32 i = w.i0 + threadIdx.x; i < w.i1; i += kThreads) {
        Counter c{tab, 0u};
        walk_item(p, w.crop, w.sd, w.g0, i, c);
        p.b.block_bits[w.g0 + i] = c.bits;
        sum += c.bits;
    }
    sum = wg_sum_u64(sum, red);
    if (threadIdx.x == 0) p.b.chunk_bits[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void prog_pack_kernel(PParams p) {
    __shared__ u32 tab[2 * 256];
    __shared__ u32 wsum[kWaves];
    const Where w = where(p);
    load_codes(p, w, tab);
    u64 pos = p.b.chunk_bitoff[blockIdx.x];
    for (u32 i0 = w.i0; i0 < w.i1; i0 += kThreads) {
        const u32 i = i0 + threadIdx.x;
        const u32 bits = i < w.i1 ? p.b.block_bits[w.g0 + i] : 0u;
        u32 step_bits;
        const u32 before = wg_scan_u32(bits, wsum, &step_bits);
        if (i < w.i1) {
            const u64 at = pos + before;
            Writer wr{tab, p.corr_pos + w.g0, BitPacker{p.b.ubuf, at >> 5, 0ull, (int)(at & 31ull)}};
            walk_item(p, w.crop, w.sd, w.g0, i, wr);
            wr.pk.finish();
        }
        pos += step_bits;
    }
}

__global__ __launch_bounds__(kThreads) void prog_corr_kernel(PParams p) {
    const Where w = where(p);
    if (w.sd.comp < 0 || !w.sd.ah) return;
    for (u32 i = w.i0 + threadIdx.x; i < w.i1; i += kThreads) {
        const int nb = (int)(p.summary[w.g0 + i] >> 2);
        if (nb == 0) continue;
        const u64 at = p.corr_pos[w.g0 + p.rstart[w.g0 + i]] + (u64)p.cboff[w.g0 + i];
        Null s;
        u64 tail;
        walk_ac(ac_block(p, w.crop, w.sd.comp, i), w.sd, s, &tail);
        Writer wr{nullptr, nullptr, BitPacker{p.b.ubuf, at >> 5, 0ull, (int)(at & 31ull)}};
        wr.raw(tail, nb);
        wr.pk.finish();
    }
}

// ---- the host's plan -------------------------------------------------------------------------------------------------------------
// items of a scan of an h x w crop
static inline u64 scan_items(const ScanDef& sd, const Crop& c, int h, int w) {
    if (sd.comp < 0) return c.blocks;
    if (sd.comp == 0) return (u64)ceil_div(h, 8) * (u64)ceil_div(w, 8);
    return (u64)c.nmcu;                                      // chroma: ceil(ceil(w / 2) / 8) = ceil(w / 16)
}

// The table as the device reads it: jpeg_u8.h's head [Consts][crops TileT n][jpeg_coef's chunks], then [streams TileT 10 n][chunks of
// the streams]: a stream is a tile {first_chunk, block0 = first item, nmcu = items}, its chunks are {stream, item0, item1}.
struct ProgPlan : CropPlan {
    u64 items, per_items;         // of all streams; items per chunk (a stream's last chunk may have fewer)
    size_t o_streams, o_chunks;
};
static ProgPlan plan(const Request& r, std::vector<unsigned char>* table) {
    ProgPlan t{};
    if (r.mode == kModeGrey) {                              // no one-component progressive files
        t.rc = CIAOSR_ERR_UNSUPPORTED;
        return t;
    }
    u64 nc = 0, bytes = 0;
    t.per_items = (u64)chunk_mcus(r.mcus, r.mode) * (u64)blocks_per_mcu(r.mode);
    plan_crops(r, true, &t, [&](const Crop& c, int h, int w) {
        for (int s = 0; s < kScans; ++s) {
            const u64 n = scan_items(kScript[s], c, h, w);
            t.items += n;
            nc += (n + t.per_items - 1) / t.per_items;
            bytes += (item_bits(kScript[s]) * n + 7ull) / 8ull;
        }
    });
    if (t.rc == CIAOSR_ERR_BAD_ARG) return t;
    if ((u64)t.ncc + nc > (u64)INT_MAX / 2 || t.items > (u64)INT_MAX || (u64)r.n * kScans > (u64)INT_MAX / 2) t.rc = CIAOSR_ERR_UNSUPPORTED;
    if (t.rc != CIAOSR_OK) return t;
    plan_streams(&t, (u64)r.n * kScans, nc, bytes);
    t.o_streams = t.table_bytes;
    t.o_chunks = t.o_streams + sizeof(TileT) * (size_t)t.ns;
    t.table_bytes = t.o_chunks + sizeof(ChunkT) * (size_t)nc;
    if (!table) return t;
    table->resize(t.table_bytes);
    fill_crops(r, t, table->data());
    TileT* streams = reinterpret_cast<TileT*>(table->data() + t.o_streams);
    ChunkT* chunks = reinterpret_cast<ChunkT*>(table->data() + t.o_chunks);
    u32 c = 0, item = 0;
    for (int k = 0; k < r.n; ++k) {
        const int* rect = r.rects + 4 * k;
        Crop g;
        crop_of(rect, t.mode, 0, 0, false, &g);
        for (int s = 0; s < kScans; ++s) {
            const u64 n = scan_items(kScript[s], g, rect[2], rect[3]);
            streams[k * kScans + s] = TileT{0, 0, 0, 0, 0, (int)n, c, item};
            for (u64 i = 0; i < n; i += t.per_items, ++c)
                chunks[c] = ChunkT{k * kScans + s, (int)i, (int)(i + t.per_items < n ? i + t.per_items : n), 0};
            item += (u32)n;
        }
    }
    return t;
}

struct ProgWork {
    StreamWork s;
    unsigned char* summary;
    u32 *block_bits, *zeroed, *rstart, *cboff, *codes, *chunk_empty;
    u64* corr_pos;
    size_t zeroed_words;          // the histograms, pre and post: one memset
    void carve(Arena& a, const ProgPlan& t) {
        const size_t items = (size_t)t.items;
        s.carve_head(a, t);
        block_bits = a.take<u32>(items);
        summary = a.take<unsigned char>(items);
        zeroed_words = (size_t)t.ns * 256 + 2 * items;
        zeroed = a.take<u32>(zeroed_words);
        rstart = a.take<u32>(items);
        cboff = a.take<u32>(items);
        corr_pos = a.take<u64>(items);
        codes = a.take<u32>((size_t)t.ns * 256);
        chunk_empty = a.take<u32>((size_t)t.nc);
        s.carve_streams(a, t);
    }
};

static int encode(const Request& r, unsigned char* out, size_t out_capacity, u64* offs /* [10 n + 1] */, unsigned char* dht /* [n][10][kDhtRecord] */,
                  void* workspace, size_t workspace_bytes, hipStream_t s) {
    std::vector<unsigned char> table;
    const ProgPlan t = plan(r, &table);
    ProgWork w;
    int rc;
    if ((rc = prepare(t, table, out_capacity, workspace, workspace_bytes, s, &w))) return rc;
    const Params c = w.s.coef_params(r, t);                  // jpeg_coef: the crops and their chunks of MCUs
    PParams p{};
    p.b = c;                                                 // everything behind it: the streams and their chunks of items
    p.b.nt = t.ns;
    p.b.nc = t.nc;
    p.b.tiles = reinterpret_cast<const TileT*>(w.s.table + t.o_streams);
    p.b.chunks = reinterpret_cast<const ChunkT*>(w.s.table + t.o_chunks);
    w.s.bind_streams(&p.b);
    p.b.block_bits = w.block_bits;
    p.b.out = out;
    p.b.tile_offs = offs;
    p.crops = c.tiles;
    p.summary = w.summary;
    p.chunk_empty = w.chunk_empty;
    p.per_items = (u32)t.per_items;
    p.hist = w.zeroed;
    p.pre = w.zeroed + (size_t)t.ns * 256;
    p.post = p.pre + (size_t)t.items;
    p.rstart = w.rstart;
    p.cboff = w.cboff;
    p.corr_pos = w.corr_pos;
    p.codes = w.codes;
    p.dht = dht;
    p.ntables = t.ns;
    // the workspace holds what the last call left: the histograms and the flush marks start from zero in every call
    if (hipMemsetAsync(w.zeroed, 0, sizeof(u32) * w.zeroed_words, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if ((rc = launch_coef(c, s))) return rc;
    if ((rc = launch("prog_summary", prog_summary_kernel, t.nc, p, s))) return rc;
    if ((rc = launch("prog_runs", prog_runs_kernel, t.nc, p, s))) return rc;
    if ((rc = launch("prog_hist", prog_hist_kernel, t.nc, p, s))) return rc;
    if ((rc = launch("prog_tables", prog_tables_kernel, (t.ns + kWaves - 1) / kWaves, p, s))) return rc;
    if ((rc = launch("prog_count", prog_count_kernel, t.nc, p, s))) return rc;
    if ((rc = launch_scan_zero(p.b, t.ubytes, s))) return rc;
    if ((rc = launch("prog_pack", prog_pack_kernel, t.nc, p, s))) return rc;
    if ((rc = launch("prog_corr", prog_corr_kernel, t.nc, p, s))) return rc;
    return launch_stuff(p.b, s);
}

}  // namespace jpeg
}  // namespace ciaosr

using namespace ciaosr;
using namespace ciaosr::jpeg;

extern "C" size_t ciaosr_jpeg_prog_result_bytes(int n_tiles) {
    return n_tiles < 1 ? 0 : 8 * ((size_t)kScans * n_tiles + 1) + (size_t)kScans * kDhtRecord * (size_t)n_tiles;
}
extern "C" size_t ciaosr_jpeg_prog_tiles_workspace_bytes(const int* rects, int n_tiles, int subsampling, int mcus_per_chunk) {
    return work_bytes<ProgWork>(plan(size_request(rects, n_tiles, subsampling, mcus_per_chunk), nullptr));
}
extern "C" size_t ciaosr_jpeg_prog_tiles_capacity_bytes(const int* rects, int n_tiles, int subsampling) {
    return plan(size_request(rects, n_tiles, subsampling, 0), nullptr).capacity;
}
extern "C" size_t ciaosr_jpeg_prog_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk) {
    return ciaosr_jpeg_prog_tiles_workspace_bytes(Whole(H, W).rect, 1, subsampling, mcus_per_chunk);
}
extern "C" size_t ciaosr_jpeg_prog_capacity_bytes(int H, int W, int subsampling) {
    return ciaosr_jpeg_prog_tiles_capacity_bytes(Whole(H, W).rect, 1, subsampling);
}

extern "C" int ciaosr_jpeg_prog_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                                int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                                void* result, void* workspace, size_t workspace_bytes, void* stream) {
    if (subsampling == CIAOSR_JPEG_GREY) return CIAOSR_ERR_UNSUPPORTED;      // refused before the arguments are looked at, as the plan would
    Request r;
    if (const int rc = checked_request(src, pitch, H, W, bgr, rects, n_tiles, quality, subsampling, mcus_per_chunk, out, result, workspace, &r))
        return rc;
    u64* offs = static_cast<u64*>(result);
    return encode(r, out, out_capacity, offs, reinterpret_cast<unsigned char*>(offs + (size_t)kScans * n_tiles + 1), workspace, workspace_bytes,
                  (hipStream_t)stream);
}

extern "C" int ciaosr_jpeg_prog_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                                          int mcus_per_chunk, unsigned char* out, size_t out_capacity, void* result, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return ciaosr_jpeg_prog_encode_tiles_u8(src, pitch, H, W, bgr, Whole(H, W).rect, 1, quality, subsampling, mcus_per_chunk, out, out_capacity, result,
                                            workspace, workspace_bytes, stream);
}
