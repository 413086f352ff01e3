// PNG encoding of an 8-bit image on the device, opt-in through `test_cfg.gpu_png` (ciaosr_amd/png_hip.py): the scanline filter and a
// literal-only dynamic-Huffman deflate coder; the *_lz_* entry points add LZ77 matches from a fixed set of distances (further down:
// "LZ77 matches"), and without them nothing here runs differently.  The container (signature, IHDR, IDAT, IEND and the chunk CRCs) is put together by the host.
//
// Stage 1, png_filter_kernel: one workgroup owns a band of `rows_per_band` image rows.  Per row it evaluates the five PNG filters
// (None, Sub, Up, Average, Paeth; 3 bytes per pixel, predecessors are the RAW pixels, the row above row 0 is zeros), picks the one whose
// filtered bytes have the smallest sum of min(b, 256 - b) -- ties to the lowest number -- and writes the filter byte plus 3 W filtered
// bytes in RGB order.  The same pass counts the band's 257-bin symbol histogram (256 literals + one end-of-block) in LDS and the band's
// Adler-32 partial sums.  filter_band is a template over the bytes per pixel: 3 (colour type 2) and 4 (colour type 6, the ciaosr_png_rgba_*
// entry points: rows of 1 + 4 W bytes in R G B A order, the left predecessor four bytes back, a pixel read as ONE aligned 32-bit word)
// and 1 (colour type 0, the ciaosr_png_grey_* entry points: rows of 1 + W bytes, the left predecessor one byte back, any alignment).
// Bit depth 16 (the ciaosr_png16_* and ciaosr_png16_grey_* entry points) is the same template at 6 and 2 stream bytes per pixel: the
// source is native uint16 samples (2-byte aligned, no more), the stream holds each sample high byte first, and the five filters work
// on those BYTES -- the left predecessor of a byte is the byte 6 or 2 back, and nothing is borrowed between the halves of a sample.
//
// Stage 2, four launches over a byte buffer split into bands:
//   deflate_hist_kernel   the 257-bin histogram of every band (skipped when stage 1 made it);
//   deflate_plan_kernel   one wave per band: code lengths <= 15 (an optimal Huffman code by the in-place minimum-redundancy construction
//                         on the sorted counts, then the Kraft-sum repair when a length exceeds the limit), canonical codes, the block
//                         header (code-length code <= 7 bits, with the run-length symbols 16 / 17 / 18) and the EXACT size of the band's
//                         segment: histogram x lengths + header; Huffman form or, when that is not smaller, stored blocks;
//   deflate_scan_kernel   one workgroup: prefix sum of the segment sizes -> 64-bit byte offsets and the total; for a zlib stream also
//                         the 2-byte header and the Adler-32 combined from the band partials;
//   deflate_pack_kernel   one workgroup per band writes its segment straight to its final offset.  Bits are gathered in an LDS window
//                         with integer OR (independent of arrival order), a lane then owns whole 32-bit output words; a segment begins
//                         and ends on a byte boundary, so the words it shares with its neighbours are written as single bytes and no
//                         two workgroups ever write the same byte: the output is bitwise repeatable and needs no zeroed buffer.
// A Huffman segment is one dynamic block (literals and end-of-block only, HDIST = 0 with its one distance code of length 0) followed by
// an empty stored block, which byte-aligns it; only the last band's last block carries BFINAL.
//
// Many crops of one image (ciaosr_png_encode_tiles_u8: the tiles of a pyramid level) run through the same stages in one set of launches.
// The host builds a band table from the rects (per band: its tile, its rows, its 64-bit offset in the filtered streams; per tile: its
// first band) and uploads it; png_filter_tiles_kernel filters each band as part of ITS crop (zeros left of the crop's first column and
// above its first row), the plan and pack kernels run unchanged on the table's offsets (a tile's last band carries BFINAL), and
// png_tiles_scan_kernel is the scan's segmented sibling: per tile 2 + segments + 4 bytes, a prefix sum over tiles, every band's offset,
// every tile's header and its Adler-32 from its own bands' partials.  Each tile's stream is byte for byte the single call's on the crop.
//
// What the literal coder and the match coder share on the device: wave_code_lengths and canonical_codes (both codes of both planners),
// BitSink<kWords>, code_length_runs and put_block_header (a dynamic block's header), and the packers' Segment, or_header, advance_window,
// block_exclusive, finish_segment and flush_words; each packer keeps its own symbol loop.
//
// The host side ("the host side", below the kernels): a call names what it keeps in its workspace as a Layout, carve() is the one list of
// those pieces and work_bytes() the same function over a fake origin, so the exported sizes are what the drivers carve.  Parameter
// structs are filled by named assignment (deflate_params, lz_params; an LzP carries the DeflateP it extends), launch() is ProfScope +
// launch + launch_status, and run_deflate() is the one launch sequence -- plan, scan, pack, and around them the match coder's memset,
// parse, plan and packer when an LzP is given -- for encode_entry, encode_tiles_entry and deflate_entry.  The extern "C" exports are
// one-line forwards to these bodies, in one block at the end.
//
// tiff_tiles.h, included at the very end, is the second front end of the same coder: the horizontal predictor over the fixed-size,
// edge-padded tiles of a TIFF level (Compression 8, Predictor 2), with entries and exports of its own (ciaosr_tiff_*).
#include <climits>
#include <cstring>
#include <vector>

#include "ops.h"

namespace ciaosr {
namespace png {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kSyms = 257;                         // 256 literals + end-of-block
constexpr int kStride = CIAOSR_PNG_HIST_STRIDE;    // u32 per band in histograms and code tables
constexpr int kHdrWords = 64;                      // u32 per band for the packed block header
constexpr int kMaxHdrBits = 32 * kHdrWords - 8;
constexpr int kLitLimit = 15, kClLimit = 7;
constexpr u32 kAdler = 65521u;
constexpr u32 kStoredMax = 65535u;
constexpr u64 kMaxBand = 1ull << 31;               // bytes per band: counts and their sums stay in 32 bits
constexpr int kPerLane = 16;                       // symbols per lane and step of the packer
constexpr int kChunk = kThreads * kPerLane;
constexpr int kWin = 2048;                         // words of the packer's LDS window: 24 + 2040 header bits + 4096 x 15 < 65536

static_assert(kStride > kSyms, "histogram stride; the planner keeps the one distance code's length behind the 257 others");

// bands of a byte buffer: explicit offsets [nb + 1], or uniform bands of band_bytes (the last one shorter)
struct Bands {
    const u64* offs;
    u64 band_bytes, total;
    int nb;
};
__device__ __forceinline__ u64 band_begin(const Bands& b, int i) {
    if (b.offs) return b.offs[i];
    const u64 v = (u64)i * b.band_bytes;
    return v < b.total ? v : b.total;
}

__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct TileBand {
    int tile, r0, r1, last;       // a band of the tile-batched form: rows [r0, r1) of tile `tile`; last: the tile's final band
};

struct FilterP {
    const unsigned char* src;     // [H][pitch], 1, 3 or 4 bytes per pixel, or 1 or 3 uint16 samples (the kernel's template argument)
    size_t pitch;
    int H, W, bgr, R;
    unsigned char* dst;           // [H][1 + bytes per pixel * W]
    u32* hist;                    // [nb][kStride]
    u32* adler;                   // [nb][2]: the band's Adler-32 sums a, b taken from a = b = 0, mod 65521
};

__device__ __forceinline__ u32 cost8(u32 b) { return b < 128u ? b : 256u - b; }

__device__ __forceinline__ void filters5(int v, int a, int b, int c, u32 f[5]) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = (u32)v;
    f[1] = (u32)(v - a) & 255u;
    f[2] = (u32)(v - b) & 255u;
    f[3] = (u32)(v - ((a + b) >> 1)) & 255u;
    f[4] = (u32)(v - pr) & 255u;
}

// The pixel at column x of row `cur` in stream order (R G B, then A): v its bytes, a those of the pixel to the left, b of the pixel above
// (`up`, null for the image's first row), c of the pixel above left; zeros where the image ends.  Four bytes per pixel are ONE aligned
// 32-bit load per pixel (the host checks src and pitch); three are single bytes.  BPP 2 and 6 are the 16-bit kinds: one or three native
// uint16 samples per pixel (16-bit loads: src and pitch are even, the host checks), each split into its high byte, then its low byte.
template <int BPP>
__device__ __forceinline__ void load_pixel(const unsigned char* cur, const unsigned char* up, int x, int bgr, int v[BPP], int a[BPP],
                                           int b[BPP], int c[BPP]) {
    const int s0 = bgr ? 2 : 0, s2 = bgr ? 0 : 2;
    if constexpr (BPP == 1) {                                 // grey: no channel order, no alignment rule
        v[0] = cur[x];
        a[0] = x > 0 ? cur[x - 1] : 0;
        b[0] = up ? up[x] : 0;
        c[0] = (up && x > 0) ? up[x - 1] : 0;
    } else if constexpr (BPP == 4) {
        const u32* q = reinterpret_cast<const u32*>(cur) + x;
        const u32* qu = reinterpret_cast<const u32*>(up) + x;
        const u32 pv = q[0], pa = x > 0 ? q[-1] : 0u;
        const u32 pb = up ? qu[0] : 0u, pc = (up && x > 0) ? qu[-1] : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sh = 8 * (k == 0 ? s0 : (k == 2 ? s2 : k));
            v[k] = (int)(pv >> sh & 255u);
            a[k] = (int)(pa >> sh & 255u);
            b[k] = (int)(pb >> sh & 255u);
            c[k] = (int)(pc >> sh & 255u);
        }
    } else if constexpr (BPP == 2 || BPP == 6) {
        constexpr int C = BPP / 2;
        const unsigned short* q = reinterpret_cast<const unsigned short*>(cur) + C * (size_t)x;
        const unsigned short* qu = reinterpret_cast<const unsigned short*>(up) + C * (size_t)x;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int sc = C == 1 ? 0 : (k == 0 ? s0 : (k == 1 ? 1 : s2));
            const u32 pv = q[sc], pa = x > 0 ? q[sc - C] : 0u;
            const u32 pb = up ? qu[sc] : 0u, pc = (up && x > 0) ? qu[sc - C] : 0u;
            v[2 * k] = (int)(pv >> 8), v[2 * k + 1] = (int)(pv & 255u);
            a[2 * k] = (int)(pa >> 8), a[2 * k + 1] = (int)(pa & 255u);
            b[2 * k] = (int)(pb >> 8), b[2 * k + 1] = (int)(pb & 255u);
            c[2 * k] = (int)(pc >> 8), c[2 * k + 1] = (int)(pc & 255u);
        }
    } else {
        static_assert(BPP == 3, "bytes per pixel");
        const unsigned char* q = cur + 3 * (size_t)x;
        const unsigned char* qu = up + 3 * (size_t)x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int sc = k == 0 ? s0 : (k == 1 ? 1 : s2);
            v[k] = q[sc];
            a[k] = x > 0 ? q[sc - 3] : 0;
            b[k] = up ? qu[sc] : 0;
            c[k] = (up && x > 0) ? qu[sc - 3] : 0;
        }
    }
}

// One workgroup, one band: rows [r0, r1) of the W pixels wide image at p.src, BPP bytes per pixel (row 0 and column 0 have zeros for
// predecessors), written from `dst` on; the band's histogram and Adler partials go to slot `band`.
template <int BPP>
__device__ __forceinline__ void filter_band(const FilterP& p, int band, int r0, int r1, unsigned char* dst) {
    __shared__ u32 h[kWaves][kStride];
    __shared__ u32 red[kWaves][5];
    __shared__ u64 red64[kWaves][2];
    __shared__ int s_best;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kWaves * kStride; i += kThreads) (&h[0][0])[i] = 0u;
    __syncthreads();
    const u64 L = (u64)BPP * (u64)p.W + 1ull;
    u32 A = 0u, B = 0u;                                   // thread 0: the band's Adler sums so far
    for (int row = r0; row < r1; ++row) {
        const unsigned char* cur = p.src + (size_t)row * p.pitch;
        const unsigned char* up = row > 0 ? cur - p.pitch : nullptr;
        u32 s[5] = {0u, 0u, 0u, 0u, 0u};
        for (int x = tid; x < p.W; x += kThreads) {
            int v[BPP], a[BPP], b[BPP], cc[BPP];
            load_pixel<BPP>(cur, up, x, p.bgr, v, a, b, cc);
#pragma unroll
            for (int c = 0; c < BPP; ++c) {
                u32 f[5];
                filters5(v[c], a[c], b[c], cc[c], f);
#pragma unroll
                for (int k = 0; k < 5; ++k) s[k] += cost8(f[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const u32 t = wave_sum_u32(s[k]);
            if (lane == 0) red[wave][k] = t;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            u32 bs = 0xffffffffu;
            for (int k = 0; k < 5; ++k) {
                u32 t = 0u;
                for (int w = 0; w < kWaves; ++w) t += red[w][k];
                if (t < bs) {                             // strict: ties go to the lowest filter number
                    bs = t;
                    best = k;
                }
            }
            s_best = best;
        }
        __syncthreads();
        const int best = s_best;
        unsigned char* out = dst + (u64)(row - r0) * L;
        u64 a1 = 0ull, a2 = 0ull;
        if (tid == 0) {
            out[0] = (unsigned char)best;
            atomicAdd(&h[0][best], 1u);
            a1 = (u64)best;
            a2 = L * (u64)best;
        }
        for (int x = tid; x < p.W; x += kThreads) {
            int v[BPP], a[BPP], b[BPP], cc[BPP];
            load_pixel<BPP>(cur, up, x, p.bgr, v, a, b, cc);
#pragma unroll
            for (int c = 0; c < BPP; ++c) {
                u32 f[5];
                filters5(v[c], a[c], b[c], cc[c], f);
                const u32 fb = best == 0 ? f[0] : best == 1 ? f[1] : best == 2 ? f[2] : best == 3 ? f[3] : f[4];
                const u64 j = 1ull + (u64)BPP * (u64)x + (u64)c;
                out[j] = (unsigned char)fb;
                atomicAdd(&h[wave][fb], 1u);
                a1 += fb;
                a2 += (L - j) * (u64)fb;              // L <= 6 * 65535 + 1 < 2^19: < 2^19 * 2^8 per byte, < 2^45 per row
            }
        }
        a1 = wave_sum_u64(a1);
        a2 = wave_sum_u64(a2);
        if (lane == 0) {
            red64[wave][0] = a1;
            red64[wave][1] = a2;
        }
        __syncthreads();
        if (tid == 0) {
            u64 t1 = 0ull, t2 = 0ull;
            for (int w = 0; w < kWaves; ++w) {
                t1 += red64[w][0];
                t2 += red64[w][1];
            }
            B = (u32)(((u64)B + (L % kAdler) * (u64)A + t2 % kAdler) % kAdler);
            A = (u32)(((u64)A + t1 % kAdler) % kAdler);
        }
        __syncthreads();                                   // red / red64 / s_best are rewritten by the next row
    }
    for (int i = tid; i < kSyms; i += kThreads) {
        u32 t = i == 256 ? 1u : 0u;                        // one end-of-block per band
        for (int w = 0; w < kWaves; ++w) t += h[w][i];
        p.hist[(size_t)band * kStride + i] = t;
    }
    if (tid == 0) {
        p.adler[2 * (size_t)band] = A;
        p.adler[2 * (size_t)band + 1] = B;
    }
}

template <int BPP>
__global__ __launch_bounds__(kThreads) void png_filter_kernel(FilterP p) {
    const int band = blockIdx.x;
    const int r0 = band * p.R, r1 = min(p.H, r0 + p.R);
    filter_band<BPP>(p, band, r0, r1, p.dst + (u64)r0 * ((u64)BPP * (u64)p.W + 1ull));
}

// The tile-batched form: band `blockIdx.x` of the table is rows [r0, r1) of tile `tile`, a crop y0, x0, h, w of the image.  The crop is
// filtered as an image of its own -- the pixels left of its first column and above its first row are zeros, whatever the image holds
// there -- into the stream at the band's offset.
struct TileFilterP {
    const unsigned char* src;     // [H][pitch]
    size_t pitch;
    int bgr;
    const int* rects;             // [n_tiles][4]: y0, x0, h, w
    const TileBand* bands;        // [nb]
    const u64* offs;              // [nb + 1]: the bands in the filtered stream
    unsigned char* dst;
    u32 *hist, *adler;
};
template <int BPP>
__global__ __launch_bounds__(kThreads) void png_filter_tiles_kernel(TileFilterP t) {
    const int band = blockIdx.x;
    const TileBand b = t.bands[band];
    const int* r = t.rects + 4 * (size_t)b.tile;
    FilterP p{t.src + (size_t)r[0] * t.pitch + BPP * (size_t)r[1], t.pitch, r[2], r[3], t.bgr, 0, nullptr, t.hist, t.adler};
    filter_band<BPP>(p, band, b.r0, b.r1, t.dst + t.offs[band]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct DeflateP {
    const unsigned char* data;
    Bands b;
    u32* hist;                    // [nb][kStride]
    u32* table;                   // [nb][kStride]: length << 16 | bit-reversed code
    u32* hdr;                     // [nb][kHdrWords]: the dynamic block's header, bit 0 of word 0 first
    u32* hdr_bits;                // [nb]
    u32* mode;                    // [nb]: 1 Huffman, 0 stored
    u64* seg_bytes;               // [nb]
    u64* out_offs;                // [nb + 1]
    u64 base;                     // offset of the first segment in out (2 behind a zlib header)
    unsigned char* out;
    const u32* adler;             // [nb][2] or null: zlib framing wanted
    u64* total;                   // device: bytes written to out
    const TileBand* tiles;        // [nb] or null: the bands of many streams (tiles); a tile's last band carries BFINAL
};

__global__ __launch_bounds__(kThreads) void deflate_hist_kernel(DeflateP p) {
    __shared__ u32 h[kWaves][kStride];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int band = blockIdx.x;
    for (int i = tid; i < kWaves * kStride; i += kThreads) (&h[0][0])[i] = 0u;
    __syncthreads();
    const u64 d0 = band_begin(p.b, band), d1 = band_begin(p.b, band + 1);
    for (u64 i = d0 + tid; i < d1; i += kThreads) atomicAdd(&h[wave][p.data[i]], 1u);
    __syncthreads();
    for (int i = tid; i < kSyms; i += kThreads) {
        u32 t = i == 256 ? 1u : 0u;
        for (int w = 0; w < kWaves; ++w) t += h[w][i];
        p.hist[(size_t)band * kStride + i] = t;
    }
}

// In-place minimum-redundancy code lengths of n >= 2 ascending weights (Moffat & Katajainen): key[i] becomes the depth of leaf i.
__device__ void min_redundancy(u32* key, int n) {
    key[0] += key[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || key[root] < key[leaf]) {
            key[next] = key[root];
            key[root++] = (u32)next;
        } else {
            key[next] = key[leaf++];
        }
        if (leaf >= n || (root < next && key[root] < key[leaf])) {
            key[next] += key[root];
            key[root++] = (u32)next;
        } else {
            key[next] += key[leaf++];
        }
    }
    key[n - 2] = 0u;
    for (int next = n - 3; next >= 0; --next) key[next] = key[key[next]] + 1u;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    int next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)key[root] == dpth) {
            ++used;
            --root;
        }
        while (avbl > used) {
            key[next--] = (u32)dpth;
            --avbl;
        }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
}

// One wave: f[nsym] counts -> len[nsym] (0 for unused symbols), a complete prefix code with lengths <= limit.  key / ord: nsym entries
// of LDS scratch, num: limit + 1 ints.  A single used symbol gets a one-bit code and an unused partner the other one (inflate refuses
// an incomplete code-length code).
__device__ void wave_code_lengths(const u32* f, int nsym, int limit, u32* key, unsigned short* ord, int* num, unsigned char* len) {
    const int lane = threadIdx.x;
    for (int i = lane; i < nsym; i += kWave) len[i] = 0;
    for (int i = lane; i < nsym; i += kWave) {
        const u32 fi = f[i];
        if (!fi) continue;
        int r = 0;                                          // rank by (count, symbol), ascending
        for (int j = 0; j < nsym; ++j) {
            const u32 fj = f[j];
            r += (fj != 0u) && (fj < fi || (fj == fi && j < i));
        }
        key[r] = fi;
        ord[r] = (unsigned short)i;
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0;
        for (int j = 0; j < nsym; ++j) n += f[j] != 0u;
        if (n == 1) {
            len[ord[0]] = 1;
            len[ord[0] == 0 ? 1 : 0] = 1;
        } else if (n >= 2) {
            min_redundancy(key, n);
            for (int l = 0; l <= limit; ++l) num[l] = 0;
            for (int i = 0; i < n; ++i) num[min((int)key[i], limit)]++;
            u32 total = 0u;
            for (int l = limit; l > 0; --l) total += (u32)num[l] << (limit - l);
            while (total != (1u << limit)) {                // over-subscribed by the clamp: lengthen the deepest shorter code
                num[limit]--;
                for (int l = limit - 1; l > 0; --l)
                    if (num[l]) {
                        num[l]--;
                        num[l + 1] += 2;
                        break;
                    }
                --total;
            }
            int j = n;                                      // the shortest codes to the most frequent symbols
            for (int l = 1; l <= limit; ++l)
                for (int k = num[l]; k > 0; --k) len[ord[--j]] = (unsigned char)l;
        }
    }
    __syncthreads();
}

// lane 0: canonical codes of len[nsym], bit-reversed for LSB-first emission, as length << 16 | code
__device__ void canonical_codes(const unsigned char* len, int nsym, int limit, int* num, u32* next, u32* out) {
    for (int l = 0; l <= limit; ++l) num[l] = 0;
    for (int i = 0; i < nsym; ++i) num[len[i]]++;
    num[0] = 0;
    u32 code = 0u;
    for (int l = 1; l <= limit; ++l) {
        code = (code + (u32)num[l - 1]) << 1;
        next[l] = code;
    }
    for (int i = 0; i < nsym; ++i) {
        const u32 l = len[i];
        out[i] = l ? (l << 16 | (__brev(next[l]++) >> (32 - l))) : 0u;
    }
}

// A block header of at most kWords words, bit 0 of word 0 first; `bits` counts on past the end, so that the planner sees an overflow.
template <int kWords>
struct BitSink {
    u32* words;
    u64 acc;
    int nacc, w, bits;
    __device__ void put(u32 v, int n) {
        acc |= (u64)v << nacc;
        nacc += n;
        bits += n;
        if (nacc >= 32) {
            if (w < kWords) words[w] = (u32)acc;
            ++w;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ void finish() {
        for (; w < kWords; ++w) {
            words[w] = (u32)acc;
            acc = 0ull;
        }
    }
};

// lane 0: the ncl code lengths seq[] of a dynamic block in the run-length symbols of RFC 1951, 3.2.7 -> the number of entries;
// ent[] (ncl entries at most) takes symbol | extra << 5, clf[19] the counts of the symbols (16: repeat the last length 3..6 times,
// 17 / 18: 3..10 / 11..138 zeros).
__device__ int code_length_runs(const unsigned char* seq, int ncl, unsigned short* ent, u32* clf) {
    for (int i = 0; i < 19; ++i) clf[i] = 0u;
    int ne = 0, i = 0;
    while (i < ncl) {
        const int v = seq[i];
        int run = 1;
        while (i + run < ncl && seq[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run > 0) {
                if (run >= 11) {
                    const int t = min(run, 138);
                    ent[ne++] = (unsigned short)(18 | (t - 11) << 5);
                    clf[18]++;
                    run -= t;
                } else if (run >= 3) {
                    ent[ne++] = (unsigned short)(17 | (run - 3) << 5);
                    clf[17]++;
                    run = 0;
                } else {
                    ent[ne++] = 0;
                    clf[0]++;
                    --run;
                }
            }
        } else {
            ent[ne++] = (unsigned short)v;
            clf[v]++;
            --run;
            while (run > 0) {
                if (run >= 3) {
                    const int t = min(run, 6);
                    ent[ne++] = (unsigned short)(16 | (t - 3) << 5);
                    clf[16]++;
                    run -= t;
                } else {
                    ent[ne++] = (unsigned short)v;
                    clf[v]++;
                    --run;
                }
            }
        }
    }
    return ne;
}

// lane 0: a dynamic block's header: BFINAL 0, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code (lengths cll[19], codes clc[19]) and
// the ne entries of code_length_runs; the rest of the sink's words are zeroed.
template <int kWords>
__device__ void put_block_header(BitSink<kWords>& s, int hlit, int hdist, const unsigned char* cll, const u32* clc,
                                 const unsigned short* ent, int ne) {
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 4;
    for (int k = 0; k < 19; ++k)
        if (cll[order[k]]) hclen = max(hclen, k + 1);
    s.put(4u, 3);                                          // BFINAL 0, BTYPE 10 (dynamic)
    s.put((u32)(hlit - 257), 5);
    s.put((u32)(hdist - 1), 5);
    s.put((u32)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) s.put(cll[order[k]], 3);
    for (int k = 0; k < ne; ++k) {
        const int sym = ent[k] & 31, extra = ent[k] >> 5;
        s.put(clc[sym] & 0xffffu, (int)(clc[sym] >> 16));
        if (sym == 16) s.put((u32)extra, 2);
        if (sym == 17) s.put((u32)extra, 3);
        if (sym == 18) s.put((u32)extra, 7);
    }
    s.finish();
}

__global__ __launch_bounds__(kWave) void deflate_plan_kernel(DeflateP p) {
    __shared__ u32 f[kStride];
    __shared__ u32 key[kStride];
    __shared__ unsigned short ord[kStride];
    __shared__ unsigned char len[kStride];
    __shared__ u32 code[kStride];
    __shared__ int num[kLitLimit + 1];
    __shared__ u32 next[kLitLimit + 1];
    __shared__ unsigned short ent[kSyms + 1];              // code-length symbols: symbol | extra << 5
    __shared__ u32 clf[19];
    __shared__ unsigned char cll[19];
    __shared__ u32 clc[19];
    __shared__ int s_nent;
    const int lane = threadIdx.x, band = blockIdx.x;
    for (int i = lane; i < kSyms; i += kWave) f[i] = p.hist[(size_t)band * kStride + i];
    __syncthreads();
    wave_code_lengths(f, kSyms, kLitLimit, key, ord, num, len);
    if (lane == 0) {
        canonical_codes(len, kSyms, kLitLimit, num, next, code);
        len[kSyms] = 0;                                    // the 258 code lengths: 257 literal / length codes + the one distance code of length 0
        s_nent = code_length_runs(len, kSyms + 1, ent, clf);
    }
    __syncthreads();
    wave_code_lengths(clf, 19, kClLimit, key, ord, num, cll);
    if (lane == 0) {
        canonical_codes(cll, 19, kClLimit, num, next, clc);
        BitSink<kHdrWords> s{p.hdr + (size_t)band * kHdrWords, 0ull, 0, 0, 0};
        put_block_header(s, kSyms, 1, cll, clc, ent, s_nent);
        u64 payload = 0ull;
        for (int i = 0; i < kSyms; ++i) payload += (u64)f[i] * len[i];
        const u64 n = band_begin(p.b, band + 1) - band_begin(p.b, band);
        const u64 huff = ((u64)s.bits + payload + 3ull + 7ull) / 8ull + 4ull;     // + the empty stored block: 3 bits, pad, LEN, NLEN
        const u64 stored = n + 5ull * ((n + kStoredMax - 1) / kStoredMax);
        const bool use = huff < stored && s.bits <= kMaxHdrBits;
        p.hdr_bits[band] = (u32)s.bits;
        p.mode[band] = use ? 1u : 0u;
        p.seg_bytes[band] = use ? huff : stored;
    }
    __syncthreads();
    for (int i = lane; i < kSyms; i += kWave) p.table[(size_t)band * kStride + i] = code[i];
}

// one workgroup: lane t owns the bands [t * per, (t + 1) * per)
__global__ __launch_bounds__(kThreads) void deflate_scan_kernel(DeflateP p) {
    __shared__ u64 tot[kThreads];
    __shared__ u32 ad[kThreads][3];
    const int tid = threadIdx.x, nb = p.b.nb;
    const int per = (nb + kThreads - 1) / kThreads;
    const int i0 = min(nb, tid * per), i1 = min(nb, i0 + per);
    u64 sum = 0ull;
    u32 a = 0u, b = 0u, n = 0u;                            // Adler sums and length (mod 65521) of this lane's run of bands
    for (int i = i0; i < i1; ++i) {
        sum += p.seg_bytes[i];
        if (p.adler) {
            const u32 ni = (u32)((band_begin(p.b, i + 1) - band_begin(p.b, i)) % kAdler);
            b = (u32)(((u64)b + (u64)p.adler[2 * (size_t)i + 1] + (u64)ni * a) % kAdler);
            a = (a + p.adler[2 * (size_t)i]) % kAdler;
            n = (n + ni) % kAdler;
        }
    }
    tot[tid] = sum;
    ad[tid][0] = a;
    ad[tid][1] = b;
    ad[tid][2] = n;
    __syncthreads();
    if (tid == 0) {
        u64 run = p.base;
        u32 ca = 0u, cb = 0u, cn = 0u;
        for (int t = 0; t < kThreads; ++t) {
            const u64 v = tot[t];
            tot[t] = run;
            run += v;
            cb = (u32)(((u64)cb + ad[t][1] + (u64)ad[t][2] * ca) % kAdler);
            ca = (ca + ad[t][0]) % kAdler;
            cn = (cn + ad[t][2]) % kAdler;
        }
        p.out_offs[nb] = run;
        if (p.adler) {                                      // zlib: CMF / FLG in front, Adler-32 (from a = 1, b = 0) behind, big-endian
            const u32 fa = (1u + ca) % kAdler, fb = (cn + cb) % kAdler;
            p.out[0] = 0x78;
            p.out[1] = 0x01;
            p.out[run + 0] = (unsigned char)(fb >> 8);
            p.out[run + 1] = (unsigned char)fb;
            p.out[run + 2] = (unsigned char)(fa >> 8);
            p.out[run + 3] = (unsigned char)fa;
            run += 4;
        }
        *p.total = run;
    }
    __syncthreads();
    u64 off = tot[tid];
    for (int i = i0; i < i1; ++i) {
        p.out_offs[i] = off;
        off += p.seg_bytes[i];
    }
}

// The scan of many streams: tile t owns the bands [first[t], first[t + 1]) and its stream is 2 header bytes, their segments, 4 bytes of
// Adler-32.  One workgroup; lane k owns the tiles [k * per, (k + 1) * per) and walks their bands, so any number of tiles and any number
// of bands per tile is covered.  Writes every tile's offset, header and Adler-32 (from its own bands' partials) and every band's offset.
struct TileScanP {
    const u64* offs;              // [nb + 1]: the bands in the filtered stream
    const u32* first;             // [nt + 1]
    const u64* seg_bytes;         // [nb]
    const u32* adler;             // [nb][2]
    u64* out_offs;                // [nb]
    u64* tile_offs;               // [nt + 1]
    unsigned char* out;
    int nt;
};
__global__ __launch_bounds__(kThreads) void png_tiles_scan_kernel(TileScanP p) {
    __shared__ u64 tot[kThreads];
    const int tid = threadIdx.x, nt = p.nt;
    const int per = (nt + kThreads - 1) / kThreads;
    const int t0 = min(nt, tid * per), t1 = min(nt, t0 + per);
    u64 sum = 0ull;
    for (int t = t0; t < t1; ++t) {
        sum += 6ull;
        for (u32 i = p.first[t]; i < p.first[t + 1]; ++i) sum += p.seg_bytes[i];
    }
    tot[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0ull;
        for (int k = 0; k < kThreads; ++k) {
            const u64 v = tot[k];
            tot[k] = run;
            run += v;
        }
        p.tile_offs[nt] = run;
    }
    __syncthreads();
    u64 off = tot[tid];
    for (int t = t0; t < t1; ++t) {
        p.tile_offs[t] = off;
        p.out[off] = 0x78;
        p.out[off + 1] = 0x01;
        u64 run = off + 2ull;
        u32 a = 0u, b = 0u, n = 0u;
        for (u32 i = p.first[t]; i < p.first[t + 1]; ++i) {
            p.out_offs[i] = run;
            run += p.seg_bytes[i];
            const u32 ni = (u32)((p.offs[i + 1] - p.offs[i]) % kAdler);
            b = (u32)(((u64)b + (u64)p.adler[2 * (size_t)i + 1] + (u64)ni * a) % kAdler);
            a = (a + p.adler[2 * (size_t)i]) % kAdler;
            n = (n + ni) % kAdler;
        }
        const u32 fa = (1u + a) % kAdler, fb = (n + b) % kAdler;        // from a = 1, b = 0, big-endian
        p.out[run + 0] = (unsigned char)(fb >> 8);
        p.out[run + 1] = (unsigned char)fb;
        p.out[run + 2] = (unsigned char)(fa >> 8);
        p.out[run + 3] = (unsigned char)fa;
        off = run + 4ull;
    }
}

__device__ __forceinline__ void or_bits(u32* win, u32 pos, u32 v) {
    const u64 x = (u64)v << (pos & 31u);
    atomicOr(&win[pos >> 5], (u32)x);
    if (x >> 32) atomicOr(&win[(pos >> 5) + 1], (u32)(x >> 32));
}

// words [0, nw) of the window, word w at byte abase + 4 (wdone + w) of out; only bytes in [lo, hi) are written
__device__ __forceinline__ void flush_words(const u32* win, int nw, unsigned char* out, u64 abase, u64 wdone, u64 lo, u64 hi) {
    for (int w = threadIdx.x; w < nw; w += kThreads) {
        const u64 g = abase + 4ull * (wdone + (u64)w);
        const u32 v = win[w];
        if (g >= lo && g + 4 <= hi) {
            *reinterpret_cast<u32*>(out + g) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (g + k >= lo && g + k < hi) out[g + k] = (unsigned char)(v >> (8 * k));
        }
    }
}

// ---- what the two packers share.  A packer's place in its segment: bytes [lo, hi) of out; window word 0 is the aligned output word at
// byte abase + 4 wdone, and its first `bitpos` (< 32, between two steps) bits are taken.
struct Segment {
    unsigned char* out;
    u64 lo, hi, abase, wdone;
    u32 bitpos;
};
__device__ __forceinline__ Segment segment_of(const DeflateP& p, int band) {
    Segment g;
    g.out = p.out;
    g.lo = p.out_offs[band];
    g.hi = g.lo + p.seg_bytes[band];                       // tiles: a trailer and a header lie before the next band
    g.abase = g.lo & ~3ull;
    g.wdone = 0ull;
    g.bitpos = (u32)(g.lo & 3ull) * 8u;
    return g;
}
__device__ __forceinline__ bool last_band(const DeflateP& p, int band) { return p.tiles ? p.tiles[band].last != 0 : band == p.b.nb - 1; }

// the hb bits of a band's header, ORed into the zeroed window behind the bits taken
__device__ __forceinline__ void or_header(u32* win, const Segment& g, const u32* hdr, u32 hb) {
    const int tid = threadIdx.x, nw = (int)((hb + 31u) >> 5);
    if (tid < nw) {
        const u64 x = (u64)hdr[tid] << g.bitpos;
        atomicOr(&win[tid], (u32)x);
        if (x >> 32) atomicOr(&win[tid + 1], (u32)(x >> 32));
    }
}

// All lanes, behind a barrier after the last OR: `nbits` more bits are in the window.  Its full words are flushed, the word in
// progress becomes word 0 and the rest is cleared for the next step.
__device__ __forceinline__ void advance_window(u32* win, Segment& g, u32 nbits) {
    const u32 newpos = g.bitpos + nbits;
    const int nfull = (int)(newpos >> 5);
    flush_words(win, nfull, g.out, g.abase, g.wdone, g.lo, g.hi);
    const u32 carry = win[nfull];
    __syncthreads();
    for (int i = threadIdx.x; i <= nfull; i += kThreads) win[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) win[0] = carry;
    __syncthreads();
    g.wdone += (u64)nfull;
    g.bitpos = newpos & 31u;
}

// All lanes: the sum of `bits` over the lanes before this one, and over the whole workgroup in *total.  wsum: kWaves words of LDS, free
// again after the caller's next barrier.
__device__ __forceinline__ u32 block_exclusive(u32 bits, u32* wsum, u32* total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u32 inc = bits;                                          // inclusive scan of the lanes' bit counts
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const u32 t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    u32 before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    *total = all;
    return before + inc - bits;
}

// The end of a Huffman segment: the end-of-block code `eob` (length << 16 | code) and the empty stored block that byte-aligns it, then
// the flush of what the window holds.
__device__ __forceinline__ void finish_segment(u32* win, const Segment& g, u32 eob, bool last, u32* wsum) {
    if (threadIdx.x == 0) {
        u32 pos = g.bitpos;
        or_bits(win, pos, eob & 0xffffu);
        pos += eob >> 16;
        or_bits(win, pos, last ? 1u : 0u);               // the empty stored block: BFINAL, BTYPE 00, pad, LEN 0, NLEN 0xffff
        pos = (pos + 3u + 7u) & ~7u;
        or_bits(win, pos + 16u, 0xffffu);
        wsum[0] = pos + 32u;
    }
    __syncthreads();
    flush_words(win, (int)((wsum[0] + 31u) >> 5), g.out, g.abase, g.wdone, g.lo, g.hi);
}

__global__ __launch_bounds__(kThreads) void deflate_pack_kernel(DeflateP p) {
    __shared__ u32 win[kWin];
    __shared__ u32 tab[kStride];
    __shared__ u32 wsum[kWaves];
    const int tid = threadIdx.x;
    const int band = blockIdx.x;
    const bool last = last_band(p, band);
    const u64 d0 = band_begin(p.b, band), n = band_begin(p.b, band + 1) - d0;
    Segment g = segment_of(p, band);
    if (p.mode[band] == 2u) return;                         // a band in match mode (the lz entry points only) is deflate_lz_pack_kernel's
    if (p.mode[band] == 0u) {                              // stored blocks of at most 65535 bytes: 5 framing bytes each
        const u64 nblk = (n + kStoredMax - 1) / kStoredMax;
        const u64 lo = g.lo, hi = g.hi;
        for (u64 j = tid; j < hi - lo; j += kThreads) {
            const u64 blk = j / (kStoredMax + 5ull);
            const u32 r = (u32)(j % (kStoredMax + 5ull));
            const u64 left = n - blk * kStoredMax;
            const u32 ln = left < kStoredMax ? (u32)left : kStoredMax;
            unsigned char v;
            if (r == 0) v = (last && blk == nblk - 1) ? 1 : 0;
            else if (r == 1) v = (unsigned char)ln;
            else if (r == 2) v = (unsigned char)(ln >> 8);
            else if (r == 3) v = (unsigned char)~ln;
            else if (r == 4) v = (unsigned char)(~ln >> 8);
            else v = p.data[d0 + blk * kStoredMax + (r - 5)];
            p.out[lo + j] = v;
        }
        return;
    }
    for (int i = tid; i < kSyms; i += kThreads) tab[i] = p.table[(size_t)band * kStride + i];
    for (int i = tid; i < kWin; i += kThreads) win[i] = 0u;
    __syncthreads();
    const u32 hb = p.hdr_bits[band];                        // the header stays in the window: the first chunk's bits follow it
    or_header(win, g, p.hdr + (size_t)band * kHdrWords, hb);
    g.bitpos += hb;
    __syncthreads();
    for (u64 c0 = 0; c0 < n; c0 += kChunk) {
        const u64 m0 = c0 + (u64)tid * kPerLane;
        const int cnt = m0 >= n ? 0 : (n - m0 < (u64)kPerLane ? (int)(n - m0) : kPerLane);
        u32 e[kPerLane];
        u32 bits = 0u;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            e[k] = k < cnt ? tab[p.data[d0 + m0 + k]] : 0u;
            bits += e[k] >> 16;
        }
        u32 chunk_bits;
        const u32 pos = g.bitpos + block_exclusive(bits, wsum, &chunk_bits);
        int w = (int)(pos >> 5);
        int nacc = (int)(pos & 31u);
        u64 acc = 0ull;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            acc |= (u64)(e[k] & 0xffffu) << nacc;
            nacc += (int)(e[k] >> 16);
            if (nacc >= 32) {
                atomicOr(&win[w], (u32)acc);
                ++w;
                acc >>= 32;
                nacc -= 32;
            }
        }
        if (nacc > 0 && acc) atomicOr(&win[w], (u32)acc);
        __syncthreads();
        advance_window(win, g, chunk_bits);
    }
    finish_segment(win, g, tab[256], last, wsum);
}

// ---- LZ77 matches (opt-in: the *_lz_* entry points) ------------------------------------------------------------------------------
// The contract, which tests/png_match_ref.py restates: a band is parsed in chunks of 4096 bytes counted from its start.  At position i
// the candidate distances are D = (1, 2, 3, 4, 6, 8, 12, 16, line - bpp, line, line + bpp), line the scanline length (line = 0: the first
// eight only); a candidate above 32768 or above i's offset in the band is skipped, so nothing is read from before the band.  The length
// for d is the run of data[i + j] == data[i + j - d], capped at 258 and at the end of the chunk (and so of the band); the longest
// candidate wins, ties go to the earliest in D, and it is a match iff its length is >= 8.  The parse is greedy from every chunk's start.
//
//   deflate_lz_match_kernel  one workgroup per chunk.  The chunk and its 16 predecessors are staged in LDS (the three line distances
//                            read global memory).  Per candidate a 4096-bit equality mask is built with one ballot per wave and pass;
//                            the run at i is a count of trailing ones over at most six words.  next[i] = i + (match ? length : 1);
//                            what the greedy walk visits is what is reachable from position 0, marked by pointer doubling (at most
//                            12 rounds, ended as soon as next^(2^k)[0] is the chunk's end).  The visited positions' tokens -- 16 bits:
//                            a literal is its byte, a match 0x8000 | index into D << 9 | length - 3 -- are compacted with a prefix sum
//                            to the chunk's slot (2 bytes per filtered byte at most) and counted in LDS, then added to the band's
//                            286 + 30 histogram with integer atomics (order-independent; the table is zeroed by a memset).
//   deflate_lz_plan_kernel   one wave per band, after deflate_plan_kernel: both codes by the same construction, HLIT / HDIST trimmed,
//                            one run-length coded sequence of code lengths, a single used distance symbol alone with length 1, the
//                            exact size; the band goes to match mode (mode 2) iff that is SMALLER than what deflate_plan_kernel chose.
//   deflate_lz_pack_kernel   one workgroup per band in match mode: as deflate_pack_kernel, over tokens.  A token is at most 48 bits,
//                            put in two parts of at most 20 and 28; a chunk's tokens cover at most 4096 bytes at no more than 15 bits
//                            per byte (a match: 48 bits for 8 bytes or more), so with the header flushed on its own the window bound
//                            is the literal coder's: 31 + 4096 x 15 < 65536 bits.
constexpr int kLzChunk = 4096;                     // bytes per parse chunk
constexpr int kLzPer = kLzChunk / kThreads;        // positions per lane
constexpr int kLzCand = 11, kLzNear = 8;
constexpr int kLzMin = 8, kLzMax = 258;
constexpr int kLzLit = 286, kLzDist = 30;
constexpr int kLzStride = 320;                     // u32 per band: 286 literal / length entries, then 30 distance entries
constexpr int kLzHdrWords = 144;                   // 14 + 19 x 3 + 316 x (7 + 7) bits at most
constexpr int kLzMaskWords = kLzChunk / 64;
static_assert(kLzPer == kPerLane && kLzChunk == kChunk, "the packer takes a chunk's tokens in one step");
static_assert(kLzStride >= kLzLit + kLzDist && 32 * kLzHdrWords >= 14 + 57 + (kLzLit + kLzDist) * 14, "lz tables");
static_assert(31 + kLzChunk * kLitLimit < 32 * (kWin - 1) && kLzHdrWords + 2 < kWin, "packer window");

struct LzP {
    DeflateP d;                   // the literal coder's call: data, bands and tiles; mode and seg_bytes hold deflate_plan_kernel's choice
                                  // (mode 2 where matches are smaller); out_offs and out as the scan left them
    const int* rects;             // the crops of the PNG tiles: the line of a band is its tile's, 1 + bpp w
    u64 line;                     // without rects (one image; TIFF tiles, tiff_tiles.h): every band's line, 0 = none
    int bpp;
    u64 base0;                    // the first band's offset in data: token slots are counted from there
    const u32* chunk_first;       // [nb + 1] first chunk of every band, or null: uniform bands of cpb chunks
    u32 cpb;
    u32 chunks;                   // parse chunks of all bands: the workgroups of deflate_lz_match_kernel
    unsigned short* tok;          // [total]: a chunk's tokens start at its first byte's offset
    u32* cnt;                     // [chunks]
    u32* hist;                    // [nb][kLzStride], zeroed before deflate_lz_match_kernel
    u32* table;                   // [nb][kLzStride]: length << 16 | bit-reversed code
    u32* hdr;                     // [nb][kLzHdrWords]
    u32* hdr_bits;                // [nb]
};

__device__ __forceinline__ u64 lz_line(const LzP& p, int band) {
    return p.rects ? 1ull + (u64)p.bpp * (u64)p.rects[4 * (size_t)p.d.tiles[band].tile + 3] : p.line;
}
// candidate c of a band with scanline length `line`: its distance, 0 when there is none
__device__ __forceinline__ u32 lz_distance(int c, u64 line, int bpp) {
    const u32 near[kLzNear] = {1u, 2u, 3u, 4u, 6u, 8u, 12u, 16u};
    if (c < kLzNear) return near[c];
    if (line == 0ull) return 0u;
    const u64 d = c == kLzNear ? line - (u64)bpp : (c == kLzNear + 1 ? line : line + (u64)bpp);
    return d > 32768ull ? 0u : (u32)d;
}
// RFC 1951, 3.2.5: length 3..258 -> symbol, extra bits and their value
__device__ __forceinline__ void lz_length_code(int length, int* sym, int* nx, u32* xv) {
    const u32 l = (u32)(length - 3);
    if (length == kLzMax) {
        *sym = 285, *nx = 0, *xv = 0u;
    } else if (l < 8u) {
        *sym = 257 + (int)l, *nx = 0, *xv = 0u;
    } else {
        const int e = 29 - __clz((int)l);                   // floor(log2 l) - 2
        *sym = 261 + 4 * e + (int)(l >> e & 3u), *nx = e, *xv = l & ((1u << e) - 1u);
    }
}
__device__ __forceinline__ void lz_distance_code(u32 d, int* sym, int* nx, u32* xv) {
    const u32 v = d - 1u;
    if (v < 4u) {
        *sym = (int)v, *nx = 0, *xv = 0u;
    } else {
        const int e = 30 - __clz((int)v);                   // floor(log2 v) - 1
        *sym = 2 * (e + 1) + (int)(v >> e & 1u), *nx = e, *xv = v & ((1u << e) - 1u);
    }
}
__device__ __forceinline__ int lz_length_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
__device__ __forceinline__ int lz_distance_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// the band and the chunk of workgroup `blk`; false: the block has no chunk (uniform bands: the last band is shorter)
__device__ __forceinline__ bool lz_locate(const LzP& p, u32 blk, int* band, u64* c0) {
    if (!p.chunk_first) {
        *band = (int)(blk / p.cpb);
        *c0 = (u64)(blk % p.cpb) * kLzChunk;
        return *c0 < band_begin(p.d.b, *band + 1) - band_begin(p.d.b, *band);
    }
    int lo = 0, hi = p.d.b.nb - 1;                            // the last band whose first chunk is <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.chunk_first[mid] <= blk) lo = mid;
        else hi = mid - 1;
    }
    *band = lo;
    *c0 = (u64)(blk - p.chunk_first[lo]) * kLzChunk;
    return true;
}

// trailing ones of the mask from bit i on, at most kLzMax
__device__ __forceinline__ int lz_run(const u64* m, int i) {
    int w = i >> 6;
    const int b = i & 63;
    const u64 x = ~(m[w] >> b);                             // the zeros shifted in end the run at the word's end
    int r = x ? __ffsll((long long)x) - 1 : 64;
    if (r < 64 - b) return r;
    r = 64 - b;
    while (r < kLzMax && ++w < kLzMaskWords) {
        const u64 y = ~m[w];
        if (y) {
            r += __ffsll((long long)y) - 1;
            break;
        }
        r += 64;
    }
    return min(r, kLzMax);
}

__global__ __launch_bounds__(kThreads) void deflate_lz_match_kernel(LzP p) {
    __shared__ unsigned char s[16 + kLzChunk];
    __shared__ u64 mask[kLzCand][kLzMaskWords];
    __shared__ unsigned short nxt[kLzChunk + 1];
    __shared__ unsigned short tokv[kLzChunk];
    __shared__ unsigned char reach[kLzChunk + 1];
    __shared__ u32 h[kLzStride];
    __shared__ u32 dist[kLzCand];
    __shared__ u32 wsum[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int band;
    u64 c0;
    if (!lz_locate(p, blockIdx.x, &band, &c0)) return;
    const u64 d0 = band_begin(p.d.b, band), n = band_begin(p.d.b, band + 1) - d0;
    const int m = (int)(n - c0 < (u64)kLzChunk ? n - c0 : (u64)kLzChunk);
    const unsigned char* src = p.d.data + d0 + c0;            // src[-k] is inside the band for k <= c0
    if (tid < kLzCand) dist[tid] = lz_distance(tid, lz_line(p, band), p.bpp);
    for (int i = tid; i < kLzStride; i += kThreads) h[i] = 0u;
    for (int i = tid; i < 16 + kLzChunk; i += kThreads) {
        const int k = i - 16;
        s[i] = (k < m && (k >= 0 || (u64)(-k) <= c0)) ? src[k] : 0;
    }
    __syncthreads();
    // equality masks: word 4 k + wave of candidate c holds positions 256 k + 64 wave + lane
    for (int k = 0; k < kLzPer; ++k) {
        const int i = k * kThreads + tid;
        const u32 v = s[16 + i];
        const u64 at = c0 + (u64)i;                          // i's offset from the band's start
#pragma unroll
        for (int c = 0; c < kLzCand; ++c) {
            const u32 d = dist[c];
            bool eq = false;
            if (i < m && d != 0u && (u64)d <= at) eq = v == (c < kLzNear ? (u32)s[16 + i - (int)d] : (u32)src[(long)i - (long)d]);
            const u64 bal = __ballot(eq);
            if (lane == 0) mask[c][k * kWaves + wave] = bal;
        }
    }
    __syncthreads();
    for (int k = 0; k < kLzPer; ++k) {
        const int i = k * kThreads + tid;
        int best = 0, bc = 0;
#pragma unroll
        for (int c = 0; c < kLzCand; ++c) {
            const int r = lz_run(mask[c], i);
            if (r > best) {                                  // strict: ties go to the earliest candidate
                best = r;
                bc = c;
            }
        }
        const bool match = best >= kLzMin;
        nxt[i] = (unsigned short)min(m, i + (match ? best : 1));
        tokv[i] = match ? (unsigned short)(0x8000 | bc << 9 | (best - 3)) : (unsigned short)s[16 + i];
        reach[i] = i == 0;
    }
    if (tid == 0) {
        nxt[kLzChunk] = (unsigned short)m;
        reach[kLzChunk] = 0;
    }
    __syncthreads();
    // what the greedy walk from 0 visits: after round r every position within 2^(r + 1) - 1 steps is marked and nxt is next^(2^(r + 1))
    for (int round = 0; round < 12; ++round) {
        for (int k = 0; k < kLzPer; ++k) {
            const int i = k * kThreads + tid;
            if (i < m && reach[i]) reach[nxt[i]] = 1;        // a mark seen early is a position the walk visits all the same
        }
        unsigned short j2[kLzPer];
#pragma unroll
        for (int k = 0; k < kLzPer; ++k) {
            const int i = k * kThreads + tid;
            j2[k] = i < m ? nxt[nxt[i]] : (unsigned short)m;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLzPer; ++k) {
            const int i = k * kThreads + tid;
            if (i < m) nxt[i] = j2[k];
        }
        __syncthreads();
        if (nxt[0] == m) break;                              // the walk ends within the steps already marked (uniform: one LDS word)
    }
    // compaction: lane t owns positions [16 t, 16 t + 16)
    u32 mine = 0u;
#pragma unroll
    for (int k = 0; k < kLzPer; ++k) {
        const int i = tid * kLzPer + k;
        mine |= (i < m && reach[i]) ? 1u << k : 0u;
    }
    const u32 cntl = (u32)__popc(mine);
    u32 inc = cntl;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const u32 t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    u32 before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    unsigned short* out = p.tok + (d0 - p.base0) + c0;       // total <= m tokens
    u32 at = before + inc - cntl;
#pragma unroll
    for (int k = 0; k < kLzPer; ++k) {
        if (!(mine >> k & 1u)) continue;
        const u32 t = tokv[tid * kLzPer + k];
        out[at++] = (unsigned short)t;
        if (t & 0x8000u) {
            int sym, nx;
            u32 xv;
            lz_length_code((int)(t & 0x1ffu) + 3, &sym, &nx, &xv);
            atomicAdd(&h[sym], 1u);
            lz_distance_code(dist[t >> 9 & 15u], &sym, &nx, &xv);
            atomicAdd(&h[kLzLit + sym], 1u);
        } else {
            atomicAdd(&h[t], 1u);
        }
    }
    if (tid == 0) p.cnt[blockIdx.x] = total;
    __syncthreads();
    for (int i = tid; i < kLzStride; i += kThreads)
        if (h[i]) atomicAdd(&p.hist[(size_t)band * kLzStride + i], h[i]);
}

__global__ __launch_bounds__(kWave) void deflate_lz_plan_kernel(LzP p) {
    __shared__ u32 f[kLzStride];
    __shared__ u32 key[kLzLit];
    __shared__ unsigned short ord[kLzLit];
    __shared__ unsigned char len[kLzStride];                // literal / length lengths, then distance lengths at kLzLit
    __shared__ u32 code[kLzStride];
    __shared__ int num[kLitLimit + 1];
    __shared__ u32 next[kLitLimit + 1];
    __shared__ unsigned char seq[kLzLit + kLzDist];
    __shared__ unsigned short ent[kLzLit + kLzDist];        // code-length symbols: symbol | extra << 5
    __shared__ u32 clf[19];
    __shared__ unsigned char cll[19];
    __shared__ u32 clc[19];
    __shared__ int s_nent, s_hlit, s_hdist;
    const int lane = threadIdx.x, band = blockIdx.x;
    for (int i = lane; i < kLzStride; i += kWave) {
        u32 v = i < kLzLit + kLzDist ? p.hist[(size_t)band * kLzStride + i] : 0u;
        if (i == 256) v += 1u;                              // one end-of-block per band
        f[i] = v;
    }
    __syncthreads();
    int nd = 0;
    for (int i = 0; i < kLzDist; ++i) nd += f[kLzLit + i] != 0u;
    if (nd == 0) return;                                    // no match in the band: the literal coder's block is never larger (uniform)
    wave_code_lengths(f, kLzLit, kLitLimit, key, ord, num, len);
    wave_code_lengths(f + kLzLit, kLzDist, kLitLimit, key, ord, num, len + kLzLit);
    if (lane == 0) {
        if (nd == 1) len[kLzLit + (ord[0] == 0 ? 1 : 0)] = 0;    // a single distance symbol stands alone: the one incomplete code allowed
        canonical_codes(len, kLzLit, kLitLimit, num, next, code);
        canonical_codes(len + kLzLit, kLzDist, kLitLimit, num, next, code + kLzLit);
        int hlit = 257, hdist = 1;
        for (int i = 257; i < kLzLit; ++i)
            if (len[i]) hlit = i + 1;
        for (int i = 1; i < kLzDist; ++i)
            if (len[kLzLit + i]) hdist = i + 1;
        for (int i = 0; i < hlit; ++i) seq[i] = len[i];
        for (int i = 0; i < hdist; ++i) seq[hlit + i] = len[kLzLit + i];
        s_nent = code_length_runs(seq, hlit + hdist, ent, clf);
        s_hlit = hlit;
        s_hdist = hdist;
    }
    __syncthreads();
    wave_code_lengths(clf, 19, kClLimit, key, ord, num, cll);
    if (lane == 0) {
        canonical_codes(cll, 19, kClLimit, num, next, clc);
        BitSink<kLzHdrWords> s{p.hdr + (size_t)band * kLzHdrWords, 0ull, 0, 0, 0};
        put_block_header(s, s_hlit, s_hdist, cll, clc, ent, s_nent);
        u64 payload = 0ull;
        for (int i = 0; i < kLzLit; ++i) payload += (u64)f[i] * (u64)(len[i] + lz_length_extra(i));
        for (int i = 0; i < kLzDist; ++i) payload += (u64)f[kLzLit + i] * (u64)(len[kLzLit + i] + lz_distance_extra(i));
        const u64 lz = ((u64)s.bits + payload + 3ull + 7ull) / 8ull + 4ull;       // + the empty stored block, as the literal coder's
        p.hdr_bits[band] = (u32)s.bits;
        if (lz < p.d.seg_bytes[band]) {                       // a tie stays with deflate_plan_kernel's choice
            p.d.mode[band] = 2u;
            p.d.seg_bytes[band] = lz;
        }
    }
    __syncthreads();
    for (int i = lane; i < kLzStride; i += kWave) p.table[(size_t)band * kLzStride + i] = code[i];
}

__global__ __launch_bounds__(kThreads) void deflate_lz_pack_kernel(LzP p) {
    __shared__ u32 win[kWin];
    __shared__ u32 tab[kLzStride];
    __shared__ u32 dcode[kLzCand], dbits[kLzCand];          // per candidate: distance code with its extra bits behind, and the bit count
    __shared__ u32 wsum[kWaves];
    const int tid = threadIdx.x;
    const int band = blockIdx.x;
    if (p.d.mode[band] != 2u) return;
    const bool last = last_band(p.d, band);
    const u64 d0 = band_begin(p.d.b, band), n = band_begin(p.d.b, band + 1) - d0;
    Segment g = segment_of(p.d, band);
    for (int i = tid; i < kLzStride; i += kThreads) tab[i] = p.table[(size_t)band * kLzStride + i];
    for (int i = tid; i < kWin; i += kThreads) win[i] = 0u;
    __syncthreads();
    if (tid < kLzCand) {
        const u32 d = lz_distance(tid, lz_line(p, band), p.bpp);
        u32 v = 0u, nb = 0u;
        if (d) {
            int sym, nx;
            u32 xv;
            lz_distance_code(d, &sym, &nx, &xv);
            const u32 e = tab[kLzLit + sym];
            v = (e & 0xffffu) | xv << (e >> 16);
            nb = (e >> 16) + (u32)nx;
        }
        dcode[tid] = v;
        dbits[tid] = nb;
    }
    const u32 hb = p.hdr_bits[band];                        // the header, flushed on its own: the window then holds one chunk's bits
    or_header(win, g, p.hdr + (size_t)band * kLzHdrWords, hb);
    __syncthreads();
    advance_window(win, g, hb);
    const u32 chunk0 = p.chunk_first ? p.chunk_first[band] : (u32)band * p.cpb;
    const unsigned short* toks = p.tok + (d0 - p.base0);
    u32 ch = 0u;
    for (u64 c0 = 0; c0 < n; c0 += kLzChunk, ++ch) {
        const int ntok = (int)p.cnt[chunk0 + ch];
        const int m0 = tid * kPerLane;
        const int cnt = m0 >= ntok ? 0 : min(ntok - m0, kPerLane);
        u32 t[kPerLane];
        u32 bits = 0u;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            t[k] = k < cnt ? (u32)toks[c0 + m0 + k] : 0xffffffffu;
            if (k < cnt) {
                if (t[k] & 0x8000u) {
                    int sym, nx;
                    u32 xv;
                    lz_length_code((int)(t[k] & 0x1ffu) + 3, &sym, &nx, &xv);
                    bits += (tab[sym] >> 16) + (u32)nx + dbits[t[k] >> 9 & 15u];
                } else {
                    bits += tab[t[k]] >> 16;
                }
            }
        }
        u32 chunk_bits;
        const u32 pos = g.bitpos + block_exclusive(bits, wsum, &chunk_bits);
        int w = (int)(pos >> 5);
        int nacc = (int)(pos & 31u);
        u64 acc = 0ull;
        auto put = [&](u32 v, u32 nb) {                      // nb <= 28 behind nacc < 32
            acc |= (u64)v << nacc;
            nacc += (int)nb;
            if (nacc >= 32) {
                atomicOr(&win[w], (u32)acc);
                ++w;
                acc >>= 32;
                nacc -= 32;
            }
        };
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            if (k >= cnt) continue;
            if (t[k] & 0x8000u) {
                int sym, nx;
                u32 xv;
                lz_length_code((int)(t[k] & 0x1ffu) + 3, &sym, &nx, &xv);
                const u32 e = tab[sym];
                put((e & 0xffffu) | xv << (e >> 16), (e >> 16) + (u32)nx);
                const u32 c = t[k] >> 9 & 15u;
                put(dcode[c], dbits[c]);
            } else {
                const u32 e = tab[t[k]];
                put(e & 0xffffu, e >> 16);
            }
        }
        if (nacc > 0 && acc) atomicOr(&win[w], (u32)acc);
        __syncthreads();
        advance_window(win, g, chunk_bits);
    }
    finish_segment(win, g, tab[256], last, wsum);
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
static inline int rows_per_band(int W, int rows, int bpp) {
    if (rows > 0) return rows;
    const long L = (long)bpp * W + 1;
    const long r = (128L * 1024L) / L;                       // bands of about 128 KiB of filtered bytes
    return (int)(r < 1 ? 1 : r);
}
static inline size_t capacity(size_t total, int nb, bool zlib) {
    return total + 5 * (total / kStoredMax + (size_t)nb) + (zlib ? 6 : 0) + 8;
}
static inline u64 lz_chunks_of(u64 bytes) { return (bytes + kLzChunk - 1) / kLzChunk; }

// What a call keeps in its workspace.  Callers allocate what work_bytes returns for a Layout and the drivers carve the same Layout up:
// one list of pieces, in one order, for every entry point.
struct Layout {
    int nb;                       // bands
    size_t filtered;              // bytes of filtered scanlines; 0: the caller's own bytes are coded
    size_t table;                 // bytes of the tiles' band table, or 0
    size_t chunks, tokens;        // the match coder's parse chunks and token slots, or 0 and 0: no match coder
};
struct Work {
    u64* offs_in;
    u32 *hist, *table, *hdr, *hdr_bits, *mode, *adler;
    u64 *seg_bytes, *out_offs;
    unsigned char* filtered;
    unsigned char* band_table;
    u32 *lz_hist, *lz_table, *lz_hdr, *lz_hdr_bits, *cnt, *chunk_first;
    unsigned short* tok;
};
// The literal coder's arrays, then the band table, then the match coder's: what a call adds lies behind what every call has, so the
// literal coder's layout is the same in all of them.
static void carve(Arena& a, const Layout& l, Work* w) {
    const size_t nb = (size_t)l.nb;
    *w = Work{};
    w->offs_in = a.take<u64>(nb + 1);
    w->hist = a.take<u32>(nb * kStride);
    w->table = a.take<u32>(nb * kStride);
    w->hdr = a.take<u32>(nb * kHdrWords);
    w->hdr_bits = a.take<u32>(nb);
    w->mode = a.take<u32>(nb);
    w->adler = a.take<u32>(2 * nb);
    w->seg_bytes = a.take<u64>(nb);
    w->out_offs = a.take<u64>(nb + 1);
    w->filtered = a.take<unsigned char>(l.filtered);
    if (l.table) w->band_table = a.take<unsigned char>(l.table);
    if (!l.chunks) return;
    w->lz_hist = a.take<u32>(nb * kLzStride);
    w->lz_table = a.take<u32>(nb * kLzStride);
    w->lz_hdr = a.take<u32>(nb * kLzHdrWords);
    w->lz_hdr_bits = a.take<u32>(nb);
    w->cnt = a.take<u32>(l.chunks);
    w->chunk_first = a.take<u32>(nb + 1);
    w->tok = a.take<unsigned short>(l.tokens);
}
static size_t work_bytes(const Layout& l) {
    static char origin[1];                                   // offsets only: nothing is dereferenced
    Arena a(origin, ~(size_t)0);
    Work w;
    carve(a, l, &w);
    return a.off;
}
// false: `bytes` is less than work_bytes(l)
static bool carve_workspace(void* ws, size_t bytes, const Layout& l, Work* w) {
    Arena a(ws, bytes);
    carve(a, l, w);
    return a.ok;
}

// one image (or the crops of one): nb bands over `total` filtered bytes; chunks: the match coder's parse chunks, 0 without it
static Layout image_layout(int nb, size_t total, size_t chunks) {
    Layout l{};
    l.nb = nb;
    l.filtered = total;
    l.chunks = chunks;
    l.tokens = chunks ? total : 0;
    return l;
}
// every band has at most ceil(bytes / 4096) <= bytes / 4096 + 1 chunks
static inline size_t lz_chunk_bound(size_t total_bytes, int n_bands) { return total_bytes / kLzChunk + (size_t)n_bands; }
// nb bands of the caller's own `total` bytes
static Layout bands_layout(int nb, size_t total, bool lz) {
    Layout l{};
    l.nb = nb;
    l.chunks = lz ? lz_chunk_bound(total, nb) : 0;
    l.tokens = lz ? total : 0;
    return l;
}

static Bands uniform_bands(u64 band_bytes, u64 total, int nb) {
    Bands b{};
    b.band_bytes = band_bytes;
    b.total = total;
    b.nb = nb;
    return b;
}
static Bands listed_bands(const u64* offs, int nb) {
    Bands b{};
    b.offs = offs;
    b.nb = nb;
    return b;
}
// A call's DeflateP over its workspace.  Where the result goes is the caller's to name: out, base, adler and total (a single stream),
// tiles, and out_offs where the caller keeps them itself.
static DeflateP deflate_params(const unsigned char* data, const Bands& b, const Work& w) {
    DeflateP p{};
    p.data = data;
    p.b = b;
    p.hist = w.hist;
    p.table = w.table;
    p.hdr = w.hdr;
    p.hdr_bits = w.hdr_bits;
    p.mode = w.mode;
    p.seg_bytes = w.seg_bytes;
    p.out_offs = w.out_offs;
    return p;
}
// The match coder's LzP beside a finished p.  The caller names the lines (line, or rects with p.tiles), bpp, base0 and the chunks
// (chunk_first or cpb, and their number).
static LzP lz_params(const DeflateP& p, const Work& w) {
    LzP q{};
    q.d = p;
    q.tok = w.tok;
    q.cnt = w.cnt;
    q.hist = w.lz_hist;
    q.table = w.lz_table;
    q.hdr = w.lz_hdr;
    q.hdr_bits = w.lz_hdr_bits;
    return q;
}

template <typename P>
static int launch(const char* name, void (*kernel)(P), size_t grid, int threads, hipStream_t s, const P& p) {
    ProfScope prof(name, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), 0, s, p);
    return launch_status(name);
}

// The coder's launches over the bands of p (histograms already in p.hist): plan, scan, pack.  With the match coder (q, null without
// it) the parse goes first and its plan and its packer follow the literal coder's.  `scan` runs between the plans and the packers:
// the single stream's scan or the tiles'.
template <typename Scan>
static int run_deflate(const DeflateP& p, const LzP* q, Scan scan, hipStream_t s) {
    const int nb = p.b.nb;
    int rc = CIAOSR_OK;
    if (q) {
        if (hipMemsetAsync(q->hist, 0, (size_t)nb * kLzStride * sizeof(u32), s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
        rc = launch("deflate_lz_match", deflate_lz_match_kernel, q->chunks, kThreads, s, *q);
    }
    if (!rc) rc = launch("deflate_plan", deflate_plan_kernel, nb, kWave, s, p);
    if (!rc && q) rc = launch("deflate_lz_plan", deflate_lz_plan_kernel, nb, kWave, s, *q);
    if (!rc) rc = scan();
    if (!rc) rc = launch("deflate_pack", deflate_pack_kernel, nb, kThreads, s, p);
    if (!rc && q) rc = launch("deflate_lz_pack", deflate_lz_pack_kernel, nb, kThreads, s, *q);
    return rc;
}

static int run_filter(int bpp, const unsigned char* src, size_t pitch, int H, int W, int bgr, int R, unsigned char* dst, u32* hist,
                      u32* adler, hipStream_t s) {
    FilterP f{};
    f.src = src;
    f.pitch = pitch;
    f.H = H;
    f.W = W;
    f.bgr = bgr;
    f.R = R;
    f.dst = dst;
    f.hist = hist;
    f.adler = adler;
    const int nb = ceil_div(H, R);
    if (bpp == 1) return launch("png_grey_filter_u8", png_filter_kernel<1>, nb, kThreads, s, f);
    if (bpp == 2) return launch("png16_grey_filter_u16", png_filter_kernel<2>, nb, kThreads, s, f);
    if (bpp == 6) return launch("png16_filter_u16", png_filter_kernel<6>, nb, kThreads, s, f);
    return bpp == 4 ? launch("png_rgba_filter_u8", png_filter_kernel<4>, nb, kThreads, s, f)
                    : launch("png_filter_u8", png_filter_kernel<3>, nb, kThreads, s, f);
}

static inline bool image_ok(int H, int W) { return H > 0 && W > 0 && H <= 65535 && W <= 65535; }

// what the filter asks of a source: rows of at least bpp W bytes; four bytes per pixel are read as aligned 32-bit words, 16-bit
// samples (bpp 2 and 6) as aligned 16-bit ones
static inline bool source_ok(int bpp, const unsigned char* src, size_t pitch, int W) {
    if (!src || pitch < (size_t)bpp * (size_t)W) return false;
    if (bpp == 2 || bpp == 6) return (reinterpret_cast<uintptr_t>(src) & 1u) == 0 && (pitch & 1u) == 0;
    return bpp != 4 || ((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (pitch & 3u) == 0);
}

// ---- many crops of one image -----------------------------------------------------------------------------------------------------
// The band table of a list of rects, as the device reads it: one block of memory, [offs u64 (nb + 1)][bands TileBand nb]
// [first u32 (nt + 1)][rects int 4 nt].
struct TilePlan {
    int rc;                       // CIAOSR_OK, or why the rects cannot be coded
    int nt, nb;
    u64 total;                    // bytes of all filtered streams
    size_t capacity;              // bytes the streams can take at most
    size_t o_bands, o_first, o_rects, table_bytes;
    u64 chunks;                   // parse chunks of all bands; with `lz` the table ends with [chunk_first u32 (nb + 1)] at o_chunks
    size_t o_chunks;
};
// `table` (optional) receives the table's bytes.  H, W <= 0: the rects are not held against an image.
static TilePlan plan_tiles(int bpp, const int* rects, int n_tiles, int rows_arg, int H, int W, std::vector<unsigned char>* table,
                           bool lz = false) {
    TilePlan t{};
    t.rc = CIAOSR_ERR_BAD_ARG;
    if (!rects || n_tiles < 1 || rows_arg < 0) return t;
    u64 nb = 0, total = 0, chunks = 0;
    size_t cap = 0;
    for (int k = 0; k < n_tiles; ++k) {
        const int y0 = rects[4 * k], x0 = rects[4 * k + 1], h = rects[4 * k + 2], w = rects[4 * k + 3];
        if (!image_ok(h, w) || y0 < 0 || x0 < 0) return t;
        if (H > 0 && ((long)y0 + h > H || (long)x0 + w > W)) return t;
        const u64 L = (u64)bpp * w + 1;
        const int R = rows_per_band(w, rows_arg, bpp);
        if ((u64)R * L > kMaxBand) {
            t.rc = CIAOSR_ERR_UNSUPPORTED;
            return t;
        }
        nb += (u64)ceil_div(h, R);
        chunks += (u64)(h / R) * lz_chunks_of((u64)R * L) + lz_chunks_of((u64)(h % R) * L);
        total += (u64)h * L;
        cap += capacity((size_t)h * L, ceil_div(h, R), true);
    }
    if (nb > (u64)INT_MAX / 2 || (lz && chunks > (u64)INT_MAX)) {
        t.rc = CIAOSR_ERR_UNSUPPORTED;
        return t;
    }
    t.rc = CIAOSR_OK;
    t.nt = n_tiles;
    t.nb = (int)nb;
    t.total = total;
    t.capacity = cap;
    t.o_bands = sizeof(u64) * ((size_t)nb + 1);
    t.o_first = t.o_bands + sizeof(TileBand) * (size_t)nb;
    t.o_rects = t.o_first + sizeof(u32) * ((size_t)n_tiles + 1);
    t.table_bytes = t.o_rects + 4 * sizeof(int) * (size_t)n_tiles;
    t.chunks = chunks;
    t.o_chunks = t.table_bytes;
    if (lz) t.table_bytes += sizeof(u32) * ((size_t)nb + 1);
    if (!table) return t;
    table->resize(t.table_bytes);
    u64* offs = reinterpret_cast<u64*>(table->data());
    TileBand* bands = reinterpret_cast<TileBand*>(table->data() + t.o_bands);
    u32* first = reinterpret_cast<u32*>(table->data() + t.o_first);
    memcpy(table->data() + t.o_rects, rects, 4 * sizeof(int) * (size_t)n_tiles);
    u64 off = 0;
    int i = 0;
    for (int k = 0; k < n_tiles; ++k) {
        const int h = rects[4 * k + 2], w = rects[4 * k + 3];
        const u64 L = (u64)bpp * w + 1;
        const int R = rows_per_band(w, rows_arg, bpp);
        first[k] = (u32)i;
        for (int r0 = 0; r0 < h; r0 += R, ++i) {
            const int r1 = r0 + R < h ? r0 + R : h;
            offs[i] = off;
            bands[i] = TileBand{k, r0, r1, r1 == h ? 1 : 0};
            off += (u64)(r1 - r0) * L;
        }
    }
    offs[i] = off;
    first[n_tiles] = (u32)i;
    if (lz) {
        u32* cf = reinterpret_cast<u32*>(table->data() + t.o_chunks);
        cf[0] = 0u;
        for (int j = 0; j < i; ++j) cf[j + 1] = cf[j] + (u32)lz_chunks_of(offs[j + 1] - offs[j]);
    }
    return t;
}
static Layout tile_layout(const TilePlan& t, bool lz) {
    Layout l = image_layout(t.nb, (size_t)t.total, lz ? (size_t)t.chunks : 0);
    l.table = t.table_bytes;
    return l;
}

}  // namespace png
}  // namespace ciaosr

using namespace ciaosr;
using namespace ciaosr::png;

// ---- the entry points' bodies, for 3 (R G B), 4 (R G B A) or 1 (grey) bytes per pixel, and 6 or 2 at bit depth 16; lz: the match
// coder's entry points -----------------------------------------------------------------------------------------------------------------
static int rows_per_band_entry(int bpp, int W, int rows_per_band_arg) {
    if (W <= 0 || W > 65535 || rows_per_band_arg < 0) return 0;
    return rows_per_band(W, rows_per_band_arg, bpp);
}

static int filter_entry(int bpp, const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg, unsigned char* dst,
                        unsigned int* hist, unsigned int* adler, void* stream) {
    CIAOSR_CHECK_ARG(dst && hist && adler && image_ok(H, W) && source_ok(bpp, src, pitch, W));
    CIAOSR_CHECK_ARG((bgr == 0 || bgr == 1) && rows_per_band_arg >= 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(hist) & 3u) == 0 && (reinterpret_cast<uintptr_t>(adler) & 3u) == 0);
    const int R = rows_per_band(W, rows_per_band_arg, bpp);
    if ((u64)R * ((u64)bpp * W + 1) > kMaxBand) return CIAOSR_ERR_UNSUPPORTED;
    return run_filter(bpp, src, pitch, H, W, bgr, R, dst, hist, adler, (hipStream_t)stream);
}

static size_t workspace_entry(int bpp, int H, int W, int rows_per_band_arg, bool lz) {
    if (!image_ok(H, W) || rows_per_band_arg < 0) return 0;
    const int R = rows_per_band(W, rows_per_band_arg, bpp);
    const size_t L = (size_t)bpp * (size_t)W + 1, total = (size_t)H * L;
    const int nb = ceil_div(H, R);
    if (!lz) return work_bytes(image_layout(nb, total, 0));
    if ((u64)R * L > kMaxBand) return 0;
    return work_bytes(image_layout(nb, total, (size_t)nb * (size_t)lz_chunks_of((u64)R * L)));
}

static size_t capacity_entry(int bpp, int H, int W, int rows_per_band_arg) {
    if (!image_ok(H, W) || rows_per_band_arg < 0) return 0;
    const int R = rows_per_band(W, rows_per_band_arg, bpp);
    return capacity((size_t)H * ((size_t)bpp * (size_t)W + 1), ceil_div(H, R), true);
}

static int encode_entry(int bpp, bool lz, const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                        unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes,
                        void* stream) {
    CIAOSR_CHECK_ARG(out && total_bytes && workspace && image_ok(H, W) && source_ok(bpp, src, pitch, W));
    CIAOSR_CHECK_ARG((bgr == 0 || bgr == 1) && rows_per_band_arg >= 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(total_bytes) & 7u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    const int R = rows_per_band(W, rows_per_band_arg, bpp);
    const u64 L = (u64)bpp * W + 1;
    if ((u64)R * L > kMaxBand) return CIAOSR_ERR_UNSUPPORTED;
    const int nb = ceil_div(H, R);
    const u64 total = (u64)H * L;
    if (out_capacity < capacity(total, nb, true)) return CIAOSR_ERR_WORKSPACE;
    const u64 cpb = lz_chunks_of((u64)R * L);
    const size_t chunks = (size_t)nb * (size_t)cpb;
    Work w;
    if (!carve_workspace(workspace, workspace_bytes, image_layout(nb, total, lz ? chunks : 0), &w)) return CIAOSR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int rc = run_filter(bpp, src, pitch, H, W, bgr, R, w.filtered, w.hist, w.adler, s);
    if (rc) return rc;
    DeflateP p = deflate_params(w.filtered, uniform_bands((u64)R * L, total, nb), w);
    p.base = 2ull;
    p.out = out;
    p.adler = w.adler;
    p.total = total_bytes;
    LzP q = lz_params(p, w);
    q.line = L;
    q.bpp = bpp;
    q.cpb = (u32)cpb;
    q.chunks = (u32)chunks;
    return run_deflate(p, lz ? &q : nullptr, [&] { return launch("deflate_scan", deflate_scan_kernel, 1, kThreads, s, p); }, s);
}

static size_t tiles_workspace_entry(int bpp, const int* rects, int n_tiles, int rows_per_band_arg, bool lz) {
    const TilePlan t = plan_tiles(bpp, rects, n_tiles, rows_per_band_arg, 0, 0, nullptr, lz);
    return t.rc == CIAOSR_OK ? work_bytes(tile_layout(t, lz)) : 0;
}
static size_t tiles_capacity_entry(int bpp, const int* rects, int n_tiles, int rows_per_band_arg) {
    const TilePlan t = plan_tiles(bpp, rects, n_tiles, rows_per_band_arg, 0, 0, nullptr);
    return t.rc == CIAOSR_OK ? t.capacity : 0;
}

static int encode_tiles_entry(int bpp, bool lz, const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects,
                              int n_tiles, int rows_per_band_arg, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                              void* workspace, size_t workspace_bytes, void* stream) {
    CIAOSR_CHECK_ARG(rects && out && tile_offs && workspace && n_tiles > 0 && image_ok(H, W) && source_ok(bpp, src, pitch, W));
    CIAOSR_CHECK_ARG((bgr == 0 || bgr == 1) && rows_per_band_arg >= 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(tile_offs) & 7u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    std::vector<unsigned char> table;
    const TilePlan t = plan_tiles(bpp, rects, n_tiles, rows_per_band_arg, H, W, &table, lz);
    CIAOSR_CHECK_ARG(t.rc != CIAOSR_ERR_BAD_ARG);             // a rect is empty or leaves the image
    if (t.rc != CIAOSR_OK) return t.rc;
    if (out_capacity < t.capacity) return CIAOSR_ERR_WORKSPACE;
    Work w;
    if (!carve_workspace(workspace, workspace_bytes, tile_layout(t, lz), &w)) return CIAOSR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // from pageable memory: the copy has left `table` when the call returns
    if (hipMemcpyAsync(w.band_table, table.data(), t.table_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    const u64* offs = reinterpret_cast<const u64*>(w.band_table);
    const TileBand* bands = reinterpret_cast<const TileBand*>(w.band_table + t.o_bands);
    const int* d_rects = reinterpret_cast<const int*>(w.band_table + t.o_rects);
    TileFilterP f{};
    f.src = src;
    f.pitch = pitch;
    f.bgr = bgr;
    f.rects = d_rects;
    f.bands = bands;
    f.offs = offs;
    f.dst = w.filtered;
    f.hist = w.hist;
    f.adler = w.adler;
    int rc = bpp == 1   ? launch("png_grey_filter_tiles_u8", png_filter_tiles_kernel<1>, t.nb, kThreads, s, f)
             : bpp == 2 ? launch("png16_grey_filter_tiles_u16", png_filter_tiles_kernel<2>, t.nb, kThreads, s, f)
             : bpp == 6 ? launch("png16_filter_tiles_u16", png_filter_tiles_kernel<6>, t.nb, kThreads, s, f)
             : bpp == 4 ? launch("png_rgba_filter_tiles_u8", png_filter_tiles_kernel<4>, t.nb, kThreads, s, f)
                        : launch("png_filter_tiles_u8", png_filter_tiles_kernel<3>, t.nb, kThreads, s, f);
    if (rc) return rc;
    DeflateP p = deflate_params(w.filtered, listed_bands(offs, t.nb), w);
    p.out = out;
    p.adler = w.adler;
    p.tiles = bands;
    LzP q = lz_params(p, w);
    q.rects = d_rects;
    q.bpp = bpp;
    q.chunk_first = reinterpret_cast<const u32*>(w.band_table + t.o_chunks);
    q.chunks = (u32)t.chunks;
    TileScanP sp{};
    sp.offs = offs;
    sp.first = reinterpret_cast<const u32*>(w.band_table + t.o_first);
    sp.seg_bytes = w.seg_bytes;
    sp.adler = w.adler;
    sp.out_offs = w.out_offs;
    sp.tile_offs = tile_offs;
    sp.out = out;
    sp.nt = t.nt;
    return run_deflate(p, lz ? &q : nullptr, [&] { return launch("png_tiles_scan", png_tiles_scan_kernel, 1, kThreads, s, sp); }, s);
}

// ---- raw deflate of the caller's bytes in explicit bands -----------------------------------------------------------------------------
static size_t deflate_workspace_entry(size_t total_bytes, int n_bands, bool lz) {
    if (n_bands <= 0) return 0;
    if (lz && (total_bytes < (size_t)n_bands || lz_chunk_bound(total_bytes, n_bands) > (size_t)INT_MAX)) return 0;
    return work_bytes(bands_layout(n_bands, total_bytes, lz));
}
static size_t deflate_capacity_entry(size_t total_bytes, int n_bands) { return n_bands <= 0 ? 0 : capacity(total_bytes, n_bands, false); }

// line, bpp: the match coder's (lz) only
static int deflate_entry(bool lz, const unsigned char* data, const unsigned long long* band_offsets, int n_bands, int line, int bpp,
                         unsigned char* out, size_t out_capacity, unsigned long long* seg_offsets, void* workspace, size_t workspace_bytes,
                         void* stream) {
    CIAOSR_CHECK_ARG(data && band_offsets && out && seg_offsets && workspace && n_bands > 0);
    if (lz) CIAOSR_CHECK_ARG(line >= 0 && bpp >= 1 && (line == 0 || line > bpp));             // line - bpp is a distance: >= 1
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(seg_offsets) & 7u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    std::vector<u32> first((size_t)n_bands + 1, 0u);          // the first parse chunk of every band
    for (int i = 0; i < n_bands; ++i) {
        CIAOSR_CHECK_ARG(band_offsets[i + 1] > band_offsets[i]);            // an empty band has no histogram to code
        if (band_offsets[i + 1] - band_offsets[i] > kMaxBand) return CIAOSR_ERR_UNSUPPORTED;
        first[i + 1] = first[i] + (u32)lz_chunks_of(band_offsets[i + 1] - band_offsets[i]);
    }
    const u64 total = band_offsets[n_bands] - band_offsets[0];
    const Layout l = bands_layout(n_bands, total, lz);
    if (l.chunks > (size_t)INT_MAX) return CIAOSR_ERR_UNSUPPORTED;
    if (out_capacity < capacity(total, n_bands, false)) return CIAOSR_ERR_WORKSPACE;
    Work w;
    if (!carve_workspace(workspace, workspace_bytes, l, &w)) return CIAOSR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // from pageable memory: both copies have left the host arrays when the calls return
    if (hipMemcpyAsync(w.offs_in, band_offsets, ((size_t)n_bands + 1) * sizeof(u64), hipMemcpyHostToDevice, s) != hipSuccess)
        return CIAOSR_ERR_LAUNCH;
    if (lz && hipMemcpyAsync(w.chunk_first, first.data(), first.size() * sizeof(u32), hipMemcpyHostToDevice, s) != hipSuccess)
        return CIAOSR_ERR_LAUNCH;
    DeflateP p = deflate_params(data, listed_bands(w.offs_in, n_bands), w);
    p.out_offs = seg_offsets;
    p.out = out;
    p.total = seg_offsets + n_bands;
    int rc = launch("deflate_hist", deflate_hist_kernel, n_bands, kThreads, s, p);
    if (rc) return rc;
    LzP q = lz_params(p, w);
    q.line = (u64)line;
    q.bpp = bpp;
    q.base0 = band_offsets[0];
    q.chunk_first = w.chunk_first;
    q.chunks = first[n_bands];
    return run_deflate(p, lz ? &q : nullptr, [&] { return launch("deflate_scan", deflate_scan_kernel, 1, kThreads, s, p); }, s);
}

// ---- the exports: the scanline filter alone, raw deflate alone, then the encoders as RGB / RGBA x literals / matches (lz) ----------
extern "C" int ciaosr_png_rows_per_band(int W, int rows_per_band_arg) { return rows_per_band_entry(3, W, rows_per_band_arg); }
extern "C" int ciaosr_png_rgba_rows_per_band(int W, int rows_per_band_arg) { return rows_per_band_entry(4, W, rows_per_band_arg); }

extern "C" int ciaosr_png_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                    unsigned char* dst, unsigned int* hist, unsigned int* adler, void* stream) {
    return filter_entry(3, src, pitch, H, W, bgr, rows_per_band_arg, dst, hist, adler, stream);
}
extern "C" int ciaosr_png_rgba_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                         unsigned char* dst, unsigned int* hist, unsigned int* adler, void* stream) {
    return filter_entry(4, src, pitch, H, W, bgr, rows_per_band_arg, dst, hist, adler, stream);
}

extern "C" size_t ciaosr_deflate_huff_workspace_bytes(int n_bands) { return deflate_workspace_entry(0, n_bands, false); }
extern "C" size_t ciaosr_deflate_lz_workspace_bytes(size_t total_bytes, int n_bands) { return deflate_workspace_entry(total_bytes, n_bands, true); }
extern "C" size_t ciaosr_deflate_huff_capacity_bytes(size_t total_bytes, int n_bands) { return deflate_capacity_entry(total_bytes, n_bands); }
extern "C" int ciaosr_deflate_huff_u8(const unsigned char* data, const unsigned long long* band_offsets, int n_bands,
                                      unsigned char* out, size_t out_capacity, unsigned long long* seg_offsets, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return deflate_entry(false, data, band_offsets, n_bands, 0, 1, out, out_capacity, seg_offsets, workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_deflate_lz_u8(const unsigned char* data, const unsigned long long* band_offsets, int n_bands, int line, int bpp,
                                    unsigned char* out, size_t out_capacity, unsigned long long* seg_offsets, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return deflate_entry(true, data, band_offsets, n_bands, line, bpp, out, out_capacity, seg_offsets, workspace, workspace_bytes, stream);
}

extern "C" size_t ciaosr_png_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(3, H, W, rows_per_band_arg, false); }
extern "C" size_t ciaosr_png_rgba_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(4, H, W, rows_per_band_arg, false); }
extern "C" size_t ciaosr_png_lz_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(3, H, W, rows_per_band_arg, true); }
extern "C" size_t ciaosr_png_rgba_lz_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(4, H, W, rows_per_band_arg, true); }
extern "C" size_t ciaosr_png_capacity_bytes(int H, int W, int rows_per_band_arg) { return capacity_entry(3, H, W, rows_per_band_arg); }
extern "C" size_t ciaosr_png_rgba_capacity_bytes(int H, int W, int rows_per_band_arg) { return capacity_entry(4, H, W, rows_per_band_arg); }

extern "C" int ciaosr_png_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                    unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return encode_entry(3, false, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_png_rgba_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                         unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return encode_entry(4, false, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_png_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                       unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return encode_entry(3, true, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_png_rgba_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                            unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return encode_entry(4, true, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}

extern "C" size_t ciaosr_png_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(3, rects, n_tiles, rows_per_band_arg, false);
}
extern "C" size_t ciaosr_png_rgba_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(4, rects, n_tiles, rows_per_band_arg, false);
}
extern "C" size_t ciaosr_png_lz_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(3, rects, n_tiles, rows_per_band_arg, true);
}
extern "C" size_t ciaosr_png_rgba_lz_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(4, rects, n_tiles, rows_per_band_arg, true);
}
extern "C" size_t ciaosr_png_tiles_capacity_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_capacity_entry(3, rects, n_tiles, rows_per_band_arg);
}
extern "C" size_t ciaosr_png_rgba_tiles_capacity_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_capacity_entry(4, rects, n_tiles, rows_per_band_arg);
}

extern "C" int ciaosr_png_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                          int rows_per_band_arg, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(3, false, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}
extern "C" int ciaosr_png_rgba_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                               int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                               unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(4, false, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}
extern "C" int ciaosr_png_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                             int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                             unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(3, true, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}
extern "C" int ciaosr_png_rgba_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects,
                                                  int n_tiles, int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                                  unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(4, true, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}

// one byte per pixel (colour type 0): the same entries on rows of 1 + W bytes; bgr is not read
extern "C" int ciaosr_png_grey_rows_per_band(int W, int rows_per_band_arg) { return rows_per_band_entry(1, W, rows_per_band_arg); }

extern "C" int ciaosr_png_grey_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                         unsigned char* dst, unsigned int* hist, unsigned int* adler, void* stream) {
    return filter_entry(1, src, pitch, H, W, bgr, rows_per_band_arg, dst, hist, adler, stream);
}
extern "C" size_t ciaosr_png_grey_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(1, H, W, rows_per_band_arg, false); }
extern "C" size_t ciaosr_png_grey_lz_workspace_bytes(int H, int W, int rows_per_band_arg) { return workspace_entry(1, H, W, rows_per_band_arg, true); }
extern "C" size_t ciaosr_png_grey_capacity_bytes(int H, int W, int rows_per_band_arg) { return capacity_entry(1, H, W, rows_per_band_arg); }

extern "C" int ciaosr_png_grey_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                         unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return encode_entry(1, false, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_png_grey_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,
                                            unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return encode_entry(1, true, src, pitch, H, W, bgr, rows_per_band_arg, out, out_capacity, total_bytes, workspace, workspace_bytes, stream);
}
extern "C" size_t ciaosr_png_grey_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(1, rects, n_tiles, rows_per_band_arg, false);
}
extern "C" size_t ciaosr_png_grey_lz_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_workspace_entry(1, rects, n_tiles, rows_per_band_arg, true);
}
extern "C" size_t ciaosr_png_grey_tiles_capacity_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {
    return tiles_capacity_entry(1, rects, n_tiles, rows_per_band_arg);
}
extern "C" int ciaosr_png_grey_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                               int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                               unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(1, false, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}
extern "C" int ciaosr_png_grey_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects,
                                                  int n_tiles, int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                                  unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_tiles_entry(1, true, src, pitch, H, W, bgr, rects, n_tiles, rows_per_band_arg, out, out_capacity, tile_offs, workspace,
                              workspace_bytes, stream);
}

// Bit depth 16: native uint16 samples, three (colour type 2, bpp 6: ciaosr_png16_*) or one (colour type 0, bpp 2: ciaosr_png16_grey_*)
// per pixel; the same entries on rows of 1 + 6 W or 1 + 2 W bytes.  src and pitch are even (source_ok).
#define CIAOSR_PNG16_EXPORTS(P, BPP)                                                                                                      \
    extern "C" int P##rows_per_band(int W, int rows_per_band_arg) { return rows_per_band_entry(BPP, W, rows_per_band_arg); }              \
    extern "C" int P##filter_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,                   \
                                 unsigned char* dst, unsigned int* hist, unsigned int* adler, void* stream) {                             \
        return filter_entry(BPP, reinterpret_cast<const unsigned char*>(src), pitch, H, W, bgr, rows_per_band_arg, dst, hist, adler,      \
                            stream);                                                                                                      \
    }                                                                                                                                     \
    extern "C" size_t P##workspace_bytes(int H, int W, int rows_per_band_arg) {                                                           \
        return workspace_entry(BPP, H, W, rows_per_band_arg, false);                                                                      \
    }                                                                                                                                     \
    extern "C" size_t P##lz_workspace_bytes(int H, int W, int rows_per_band_arg) {                                                        \
        return workspace_entry(BPP, H, W, rows_per_band_arg, true);                                                                       \
    }                                                                                                                                     \
    extern "C" size_t P##capacity_bytes(int H, int W, int rows_per_band_arg) { return capacity_entry(BPP, H, W, rows_per_band_arg); }     \
    extern "C" int P##encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,                   \
                                 unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,               \
                                 size_t workspace_bytes, void* stream) {                                                                  \
        return encode_entry(BPP, false, reinterpret_cast<const unsigned char*>(src), pitch, H, W, bgr, rows_per_band_arg, out,            \
                            out_capacity, total_bytes, workspace, workspace_bytes, stream);                                               \
    }                                                                                                                                     \
    extern "C" int P##lz_encode_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, int rows_per_band_arg,                \
                                    unsigned char* out, size_t out_capacity, unsigned long long* total_bytes, void* workspace,            \
                                    size_t workspace_bytes, void* stream) {                                                               \
        return encode_entry(BPP, true, reinterpret_cast<const unsigned char*>(src), pitch, H, W, bgr, rows_per_band_arg, out,             \
                            out_capacity, total_bytes, workspace, workspace_bytes, stream);                                               \
    }                                                                                                                                     \
    extern "C" size_t P##tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {                                    \
        return tiles_workspace_entry(BPP, rects, n_tiles, rows_per_band_arg, false);                                                      \
    }                                                                                                                                     \
    extern "C" size_t P##lz_tiles_workspace_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {                                 \
        return tiles_workspace_entry(BPP, rects, n_tiles, rows_per_band_arg, true);                                                       \
    }                                                                                                                                     \
    extern "C" size_t P##tiles_capacity_bytes(const int* rects, int n_tiles, int rows_per_band_arg) {                                     \
        return tiles_capacity_entry(BPP, rects, n_tiles, rows_per_band_arg);                                                              \
    }                                                                                                                                     \
    extern "C" int P##encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,     \
                                       int rows_per_band_arg, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,     \
                                       void* workspace, size_t workspace_bytes, void* stream) {                                           \
        return encode_tiles_entry(BPP, false, reinterpret_cast<const unsigned char*>(src), pitch, H, W, bgr, rects, n_tiles,              \
                                  rows_per_band_arg, out, out_capacity, tile_offs, workspace, workspace_bytes, stream);                   \
    }                                                                                                                                     \
    extern "C" int P##lz_encode_tiles_u16(const unsigned short* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,  \
                                          int rows_per_band_arg, unsigned char* out, size_t out_capacity,                                 \
                                          unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {         \
        return encode_tiles_entry(BPP, true, reinterpret_cast<const unsigned char*>(src), pitch, H, W, bgr, rects, n_tiles,               \
                                  rows_per_band_arg, out, out_capacity, tile_offs, workspace, workspace_bytes, stream);                   \
    }
CIAOSR_PNG16_EXPORTS(ciaosr_png16_, 6)
CIAOSR_PNG16_EXPORTS(ciaosr_png16_grey_, 2)
#undef CIAOSR_PNG16_EXPORTS

#include "tiff_tiles.h"
