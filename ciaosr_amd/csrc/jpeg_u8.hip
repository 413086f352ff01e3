// Baseline JPEG encoding of an 8-bit image on the device (ciaosr_amd/jpeg_hip.py): libjpeg's integer pipeline as Pillow drives it, so
// that the files are byte for byte `PIL.Image.save(format='JPEG', quality=q, subsampling=0 | 2)`'s (DESIGN 4.1i-d holds the contract).
// The device makes the entropy-coded scan, stuffed and padded; the host wraps it in the header (which depends on h, w, quality and
// subsampling only) and EOI.
//
// One image and many crops of one image run through the same eight launches; the host uploads one table (constants of the quality,
// the tiles, the chunks: `mcus_per_chunk` MCUs of ONE tile each) and every kernel but the two scans has one workgroup per chunk:
//   jpeg_coef    8 lanes per block: lane r converts the 8 samples of row r (colour conversion, 4:2:0 box filter, edge replication as
//                clamped coordinates of the crop), runs the row pass of jfdctint, the block is transposed through LDS, lane c runs the
//                column pass, quantises and writes int16 coefficients in zigzag order, blocks in scan order.  A dummy luma block of
//                4:2:0 is computed from the block whose DC it repeats, its AC zeroed.
//   jpeg_count   one lane per block: the block's code length in bits; its DC difference reads the previous block's quantised DC of the
//                same component, so nothing is carried from block to block.  The lengths are summed per chunk.
//   jpeg_scan    one workgroup: prefix sum of the chunks' bits, per tile its unstuffed bytes and a 4-byte aligned place in the
//                unstuffed buffer, per chunk its bit offset, the byte range it owns there and the pad mask of a tile's last byte.
//   jpeg_zero    zeroes the unstuffed buffer up to the total that the scan found.
//   jpeg_pack    one lane per block: a workgroup scan of the lengths gives the block's bit offset; the lane shifts its codes into a
//                64-bit accumulator, MSB first, and writes whole 32-bit words.  Blocks do not begin on byte boundaries: the first and
//                the last word of a block go through atomicOr on the zeroed buffer, the words between them belong to the block alone.
//                Integer OR does not depend on arrival order.
//   jpeg_ffcount per chunk the 0xFF bytes of its byte range (the byte that holds a chunk's first bit belongs to the chunk before).
//   jpeg_scan2   one workgroup: prefix sum of bytes + 0xFF counts -> every chunk's final offset, the tiles' offsets, the total.
//   jpeg_stuff   copies the bytes to their final place with a 0x00 after every 0xFF; a tile's last byte is padded with 1-bits.
// With optimised Huffman tables (the ciaosr_jpeg_opt_* entry points: Pillow's optimize=True files) two launches follow jpeg_coef, and
// jpeg_count / jpeg_pack read the tile's own code tables where they otherwise read the Annex K constants:
//   jpeg_hist    one lane per block, the same block walk: the chunk's symbols counted per table in LDS (4 x 256), the bins that are
//                not zero added to the tile's histograms with integer atomicAdd (zeroed by a memset on the stream in every call).
//   jpeg_tables  one workgroup per tile, one wave per table: libjpeg's rule -- merge the two smallest frequencies (ties to the larger
//                index) with a pseudo-symbol that reserves the all-ones code, limit the lengths to 16, order the symbols by the
//                size they had BEFORE limiting -- gives the DHT record for the host and the length << 16 | code table for the scan.
// No floating point anywhere; the bytes do not depend on mcus_per_chunk, on the stream or on what else is in the list.
// The host's parts of a call (request and argument check, crop geometry, stream workspace, prologue, launch) are jpeg_u8.h's, shared with
// jpeg_prog_u8.hip; this unit adds its Plan and Work, and defines the launchers of the kernels that every kind of file runs.
#include <climits>
#include <cstring>
#include <vector>

#include "jpeg_u8.h"

namespace ciaosr {
namespace jpeg {

constexpr int kBlocksPerStep = kThreads / 8;       // coefficient kernel: 8 lanes per block
constexpr u64 kBlockBytes = 208;                   // 64 coefficients x (16-bit code + 10 extra bits): the most a block can take
constexpr int kStuffPerLane = 16;                  // bytes per lane and step of the stuffing kernels
// optimised coding: the four tables of a file in the order of its DHT segments -- DC luma, AC luma, DC chroma, AC chroma
constexpr int kTables = 4;
constexpr u64 kOptBlockBits = 16 + 11 + 63 * (16 + 10);   // 1665: what a block can take with arbitrary codes of up to 16 bits

static const unsigned char kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                            69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                            81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K "typical" Huffman tables: code counts per length 1..16, then the symbols in code order
static const unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

static void canonical(const unsigned char* bits, const unsigned char* vals, u32* by_symbol) {
    u32 code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) by_symbol[vals[k]] = ((u32)len << 16) | code;
        code <<= 1;
    }
}

void make_consts(int quality, Consts* c) {
    memset(c, 0, sizeof(*c));
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int base[2] = {kBaseLuma[i], kBaseChroma[i]};
        for (int t = 0; t < 2; ++t) {
            int q = (base[t] * s + 50) / 100;
            q = q < 1 ? 1 : (q > 255 ? 255 : q);
            c->qdiv[t][i] = 8 * q;
        }
    }
    static const unsigned char dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int t = 0; t < 2; ++t) {
        canonical(kAcBits[t], kAcVals[t], c->huff[t]);
        canonical(kDcBits[t], dc_vals, c->huff[t] + 256);
    }
    int k = 0;                                              // the zigzag walk over the anti-diagonals
    for (int d = 0; d < 15; ++d)
        for (int i = 0; i < 8; ++i) {
            const int r = (d & 1) ? i : 7 - i, col = d - r;  // odd diagonals run down, even ones up
            if (col < 0 || col > 7) continue;
            c->zig_of_nat[r * 8 + col] = k++;
        }
}

// ---- coefficients ----------------------------------------------------------------------------------------------------------------

constexpr int kF0_298 = 2446, kF0_390 = 3196, kF0_541 = 4433, kF0_765 = 6270, kF0_899 = 7373, kF1_175 = 9633, kF1_501 = 12299,
              kF1_847 = 15137, kF1_961 = 16069, kF2_053 = 16819, kF2_562 = 20995, kF3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's 8-point pass; FIRST: the row pass (outputs scaled up by 2^2), else the column pass
template <bool FIRST>
__device__ __forceinline__ void dct8(int d[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15;
    d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * kF0_541;
    d[2] = descale(z1 + t13 * kF0_765, n);
    d[6] = descale(z1 - t12 * kF1_847, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * kF1_175;
    const int a4 = t4 * kF0_298, a5 = t5 * kF2_053, a6 = t6 * kF3_072, a7 = t7 * kF1_501;
    z1 *= -kF0_899;
    z2 *= -kF2_562;
    z3 = z3 * -kF1_961 + z5;
    z4 = z4 * -kF0_390 + z5;
    d[7] = descale(a4 + z1 + z3, n);
    d[5] = descale(a5 + z2 + z4, n);
    d[3] = descale(a6 + z2 + z3, n);
    d[1] = descale(a7 + z1 + z4, n);
}

// component `comp` of the pixel at q (3 bytes)
__device__ __forceinline__ int ycc(const unsigned char* q, int bgr, int comp) {
    const int r = q[bgr ? 2 : 0], g = q[1], b = q[bgr ? 0 : 2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(kThreads) void jpeg_coef_kernel(Params p) {
    __shared__ int xpose[kBlocksPerStep][8][9];
    __shared__ int qdiv[2][64];
    __shared__ int zig[64];
    const int tid = threadIdx.x, slot = tid >> 3, l8 = tid & 7;
    if (tid < 128) qdiv[tid >> 6][tid & 63] = p.consts->qdiv[tid >> 6][tid & 63];
    if (tid < 64) zig[tid] = p.consts->zig_of_nat[tid];
    const ChunkT ch = p.chunks[blockIdx.x];
    const TileT t = p.tiles[ch.tile];
    const int bpm = bpm_of(p);
    const int nblk = (ch.mcu1 - ch.mcu0) * bpm;
    const u64 base = (u64)t.block0 + (u64)ch.mcu0 * bpm;
    const unsigned char* org = p.src + (size_t)t.y0 * p.pitch + (p.grey ? 1 : 3) * (size_t)t.x0;
    const int nby = (t.h + 7) >> 3, nbx = (t.w + 7) >> 3;
    __syncthreads();
    for (int j0 = 0; j0 < nblk; j0 += kBlocksPerStep) {
        const int j = j0 + slot;
        const bool active = j < nblk;
        int comp = 0;
        bool dummy = false;
        int d[8];
        if (active) {
            const int mcu = ch.mcu0 + j / bpm, k = j % bpm;
            const int my = mcu / t.mx, mxi = mcu % t.mx;
            if (p.grey) {                                   // one component: the samples are the bytes
                const unsigned char* row = org + (size_t)min(my * 8 + l8, t.h - 1) * p.pitch;
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i] = (int)row[min(mxi * 8 + i, t.w - 1)] - 128;
            } else if (!p.sub420 || k < 4) {                // a full-resolution block
                int by = my, bx = mxi;
                comp = k;
                if (p.sub420) {
                    comp = 0;
                    int kk = k;                             // a dummy block repeats the nearest real block before it in the MCU
                    while (kk > 0 && (2 * my + (kk >> 1) >= nby || 2 * mxi + (kk & 1) >= nbx)) --kk;
                    dummy = kk != k;
                    by = 2 * my + (kk >> 1);
                    bx = 2 * mxi + (kk & 1);
                }
                const unsigned char* row = org + (size_t)min(by * 8 + l8, t.h - 1) * p.pitch;
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i] = ycc(row + 3 * (size_t)min(bx * 8 + i, t.w - 1), p.bgr, comp) - 128;
            } else {                                        // 4:2:0 chroma: rows to even, columns to 16 k, halve, rows to 8 k
                comp = k - 3;
                const int h2 = (t.h + 1) >> 1;
                const int i2 = min(my * 8 + l8, h2 - 1);
                const unsigned char* ra = org + (size_t)min(2 * i2, t.h - 1) * p.pitch;
                const unsigned char* rb = org + (size_t)min(2 * i2 + 1, t.h - 1) * p.pitch;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int jx = mxi * 8 + i;
                    const size_t xa = 3 * (size_t)min(2 * jx, t.w - 1), xb = 3 * (size_t)min(2 * jx + 1, t.w - 1);
                    const int sum = ycc(ra + xa, p.bgr, comp) + ycc(ra + xb, p.bgr, comp) + ycc(rb + xa, p.bgr, comp) + ycc(rb + xb, p.bgr, comp);
                    d[i] = ((sum + 1 + (i & 1)) >> 2) - 128;
                }
            }
            dct8<true>(d);
#pragma unroll
            for (int i = 0; i < 8; ++i) xpose[slot][l8][i] = d[i];
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = xpose[slot][i][l8];
            dct8<false>(d);
            short* dst = p.coef + (base + (u64)j) * 64ull;
            const int* qd = qdiv[comp ? 1 : 0];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int nat = i * 8 + l8;
                const int div = qd[nat];
                const int a = abs(d[i]);
                int q = (a + (div >> 1)) / div;
                if (d[i] < 0) q = -q;
                if (dummy && nat != 0) q = 0;
                dst[zig[nat]] = (short)q;
            }
        }
        __syncthreads();
    }
}

// ---- entropy coding --------------------------------------------------------------------------------------------------------------

// Walks one block: s.symbol(index, extra, n) for the DC difference (index 256 + n) and every AC symbol (index run << 4 | n; ZRL and
// EOB with n = 0), `extra` being the n bits that follow the symbol's code.
template <typename S>
__device__ __forceinline__ void walk_block(const short* cf, int pred, S& s) {
    const uint4* v4 = reinterpret_cast<const uint4*>(cf);
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 q = v4[g];
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v = (int)(short)(w[i >> 1] >> (16 * (i & 1)));
            const bool dc = g == 0 && i == 0;
            if (dc) v -= pred;
            if (v == 0 && !dc) {
                ++run;
                continue;
            }
            const int n = bit_length(abs(v));
            const u32 extra = (u32)(v < 0 ? v + (1 << n) - 1 : v) & ((1u << n) - 1u);
            if (dc) {
                s.symbol(256 + n, extra, n);
            } else {
                while (run > 15) {
                    s.symbol(0xf0, 0u, 0);
                    run -= 16;
                }
                s.symbol((run << 4) | n, extra, n);
                run = 0;
            }
        }
    }
    if (run > 0) s.symbol(0x00, 0u, 0);
}

// e.put(value, length) for every symbol of the block, its code from `tab` with the extra bits appended
template <typename E>
struct Coder {
    const u32* tab;                // [kHuff]
    E& e;
    __device__ __forceinline__ void symbol(int index, u32 extra, int n) {
        const u32 ent = tab[index];
        e.put(((ent & 0xffffu) << n) | extra, (int)(ent >> 16) + n);
    }
};
template <typename E>
__device__ __forceinline__ void code_block(const short* cf, int pred, const u32* tab /* [kHuff] */, E& e) {
    Coder<E> c{tab, e};
    walk_block(cf, pred, c);
}

struct Counter {
    u32 bits;
    __device__ __forceinline__ void put(u32, int len) { bits += (u32)len; }
};

// MSB-first packer into 32-bit words of the zeroed buffer: the first word it writes and its last, partial one are shared with the
// neighbouring blocks (atomicOr), the words between belong to this block alone.  A byte stream: word w holds bytes 4 w .. 4 w + 3.
struct Packer {
    u32* buf;
    u64 w;
    u64 acc;
    int nacc;
    bool first;
    __device__ __forceinline__ void put(u32 val, int len) {            // 1 <= len <= 27, nacc < 32
        acc |= (u64)val << (64 - nacc - len);
        nacc += len;
        if (nacc >= 32) {
            const u32 word = __builtin_bswap32((u32)(acc >> 32));
            if (first) {
                atomicOr(&buf[w], word);
                first = false;
            } else {
                buf[w] = word;
            }
            ++w;
            acc <<= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0) atomicOr(&buf[w], __builtin_bswap32((u32)(acc >> 32)));
    }
};

__device__ __forceinline__ int table_of(const Params& p, const TileT& t, u64 blk) {
    const int bpm = bpm_of(p);
    const int k = (int)((blk - t.block0) % bpm);
    return p.sub420 ? (k < 4 ? 0 : 1) : (k == 0 ? 0 : 1);
}

__global__ __launch_bounds__(kThreads) void jpeg_count_kernel(Params p) {
    __shared__ u32 tab[2][kHuff];
    __shared__ u64 red[kWaves];
    const int tid = threadIdx.x;
    const ChunkT ch = p.chunks[blockIdx.x];
    const u32* huff = p.tile_huff ? p.tile_huff + (size_t)ch.tile * (2 * kHuff) : &p.consts->huff[0][0];
    for (int i = tid; i < 2 * kHuff; i += kThreads) (&tab[0][0])[i] = huff[i];
    const TileT t = p.tiles[ch.tile];
    const int bpm = bpm_of(p);
    const int nblk = (ch.mcu1 - ch.mcu0) * bpm;
    const u64 base = (u64)t.block0 + (u64)ch.mcu0 * bpm;
    __syncthreads();
    u64 sum = 0ull;
    for (int j = tid; j < nblk; j += kThreads) {
        const u64 blk = base + (u64)j;
        Counter c{0u};
        code_block(p.coef + blk * 64ull, dc_pred(p, t, blk), tab[table_of(p, t, blk)], c);
        p.block_bits[blk] = c.bits;
        sum += c.bits;
    }
    sum = wg_sum_u64(sum, red);
    if (tid == 0) p.chunk_bits[blockIdx.x] = sum;
}

// ---- optimised coding: the tile's histograms and its tables -------------------------------------------------------------------------
struct Tally {
    u32* dc;                       // LDS [256] each: the DC and the AC histogram of the block's table class
    u32* ac;
    __device__ __forceinline__ void symbol(int index, u32, int) { atomicAdd(index >= 256 ? &dc[index - 256] : &ac[index], 1u); }
};

// One workgroup per chunk: the symbols of its blocks counted in LDS, the bins that are not zero added to the tile's histograms (zeroed
// on the stream before every call).  Integer addition: the sums do not depend on the order of arrival.
__global__ __launch_bounds__(kThreads) void jpeg_hist_kernel(Params p) {
    __shared__ u32 hist[kTables][256];
    const int tid = threadIdx.x;
    for (int i = tid; i < kTables * 256; i += kThreads) (&hist[0][0])[i] = 0u;
    const ChunkT ch = p.chunks[blockIdx.x];
    const TileT t = p.tiles[ch.tile];
    const int bpm = bpm_of(p);
    const int nblk = (ch.mcu1 - ch.mcu0) * bpm;
    const u64 base = (u64)t.block0 + (u64)ch.mcu0 * bpm;
    __syncthreads();
    for (int j = tid; j < nblk; j += kThreads) {
        const u64 blk = base + (u64)j;
        const int cls = table_of(p, t, blk);
        Tally ta{hist[2 * cls], hist[2 * cls + 1]};
        walk_block(p.coef + blk * 64ull, dc_pred(p, t, blk), ta);
    }
    __syncthreads();
    u32* dst = p.tile_hist + (size_t)ch.tile * (kTables * 256);
    for (int i = tid; i < kTables * 256; i += kThreads) {
        const u32 v = (&hist[0][0])[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

// One workgroup per tile, wave k makes table k (kTables) from its histogram by libjpeg's rule (build_table, jpeg_u8.h).
__global__ __launch_bounds__(kThreads) void jpeg_tables_kernel(Params p) {
    __shared__ u32 size_of[kTables][256];          // code size before limiting per symbol; later the symbol's length << 16 | code
    __shared__ u32 nbits[kTables][kMaxDepth];      // symbols per code size
    __shared__ unsigned char vals[kTables][256];   // the symbols in code order
    const int tid = threadIdx.x, k = tid >> 6, lane = tid & 63, tile = blockIdx.x;
    build_table(p.tile_hist + ((size_t)tile * kTables + k) * 256, size_of[k], nbits[k], vals[k], lane);
    // the tile's code tables as jpeg_count and jpeg_pack read them: per class 256 AC entries by symbol, then the DC entries by size
    u32* tab = p.tile_huff +((size_t)tile * 2 + (k >> 1)) * kHuff;
    if (k & 1) {
#pragma unroll
        for (int s = 0; s < 4; ++s) tab[4 * lane + s] = size_of[k][4 * lane + s];
    } else if (lane < kHuff - 256) {
        tab[256 + lane] = size_of[k][lane];
    }
    write_dht_record(p.dht + ((size_t)tile * kTables + k) * kDhtRecord, nbits[k], vals[k], lane);
}

__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(Params p) {
    __shared__ u64 tot[kThreads];
    const int tid = threadIdx.x, nt = p.nt, nc = p.nc;
    wg_prefix_u64(p.chunk_bits, p.chunk_sum, nc, tot);
    // tiles: bytes of each unstuffed stream, placed at multiples of 4
    {
        const int per = (nt + kThreads - 1) / kThreads;
        const int t0 = min(nt, tid * per), t1 = min(nt, t0 + per);
        u64 sum = 0ull;
        for (int t = t0; t < t1; ++t) {
            const u32 c0 = p.tiles[t].first_chunk, c1 = t + 1 < nt ? p.tiles[t + 1].first_chunk : (u32)nc;
            const u64 bits = p.chunk_sum[c1] - p.chunk_sum[c0];
            sum += (((bits + 7ull) >> 3) + 3ull) & ~3ull;
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
            *p.utotal = run;
        }
        __syncthreads();
        u64 off = tot[tid];
        for (int t = t0; t < t1; ++t) {
            const u32 c0 = p.tiles[t].first_chunk, c1 = t + 1 < nt ? p.tiles[t + 1].first_chunk : (u32)nc;
            const u64 bits = p.chunk_sum[c1] - p.chunk_sum[c0];
            p.tile_ubase[t] = off;
            off += (((bits + 7ull) >> 3) + 3ull) & ~3ull;
        }
        __syncthreads();
    }
    for (int c = tid; c < nc; c += kThreads) {
        const int t = p.chunks[c].tile;
        const u32 c0 = p.tiles[t].first_chunk, c1 = t + 1 < nt ? p.tiles[t + 1].first_chunk : (u32)nc;
        const u64 rel0 = p.chunk_sum[c] - p.chunk_sum[c0], rel1 = p.chunk_sum[c + 1] - p.chunk_sum[c0];
        const u64 ub = p.tile_ubase[t];
        p.chunk_bitoff[c] = ub * 8ull + rel0;
        p.chunk_b0[c] = ub + ((rel0 + 7ull) >> 3);
        p.chunk_b1[c] = ub + ((rel1 + 7ull) >> 3);
        // the pad goes to the chunk that owns the tile's last byte: the last chunk, unless its bits (a progressive scan's chunk may
        // have few or none) end in a byte that an earlier chunk began
        const u64 all = p.chunk_sum[c1] - p.chunk_sum[c0];
        const bool last_byte = ((rel1 + 7ull) >> 3) > ((rel0 + 7ull) >> 3) && ((rel1 + 7ull) >> 3) == ((all + 7ull) >> 3);
        p.chunk_pad[c] = (last_byte && (all & 7ull)) ? (0xffu >> (u32)(all & 7ull)) : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_zero_kernel(Params p) {
    const u64 words = *p.utotal >> 2;
    for (u64 i = (u64)blockIdx.x * kThreads + threadIdx.x; i < words; i += (u64)gridDim.x * kThreads) p.ubuf[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(Params p) {
    __shared__ u32 tab[2][kHuff];
    __shared__ u32 wsum[kWaves];
    const int tid = threadIdx.x;
    const ChunkT ch = p.chunks[blockIdx.x];
    const u32* huff = p.tile_huff ? p.tile_huff + (size_t)ch.tile * (2 * kHuff) : &p.consts->huff[0][0];
    for (int i = tid; i < 2 * kHuff; i += kThreads) (&tab[0][0])[i] = huff[i];
    const TileT t = p.tiles[ch.tile];
    const int bpm = bpm_of(p);
    const int nblk = (ch.mcu1 - ch.mcu0) * bpm;
    const u64 base = (u64)t.block0 + (u64)ch.mcu0 * bpm;
    u64 pos = p.chunk_bitoff[blockIdx.x];
    __syncthreads();
    for (int j0 = 0; j0 < nblk; j0 += kThreads) {
        const int j = j0 + tid;
        const u64 blk = base + (u64)j;
        const u32 bits = j < nblk ? p.block_bits[blk] : 0u;
        u32 step_bits;
        const u32 before = wg_scan_u32(bits, wsum, &step_bits);
        if (j < nblk) {
            const u64 at = pos + before;
            Packer pk{p.ubuf, at >> 5, 0ull, (int)(at & 31ull), true};
            code_block(p.coef + blk * 64ull, dc_pred(p, t, blk), tab[table_of(p, t, blk)], pk);
            pk.finish();
        }
        pos += step_bits;
    }
}

// byte i of the unstuffed buffer as the chunk that owns it sees it
__device__ __forceinline__ u32 ubyte(const unsigned char* u, u64 i, u64 b1, u32 pad) {
    u32 v = u[i];
    if (i + 1 == b1) v |= pad;
    return v;
}

__global__ __launch_bounds__(kThreads) void jpeg_ffcount_kernel(Params p) {
    __shared__ u64 red[kWaves];
    const int c = blockIdx.x;
    const u64 b0 = p.chunk_b0[c], b1 = p.chunk_b1[c];
    const u32 pad = p.chunk_pad[c];
    const unsigned char* u = reinterpret_cast<const unsigned char*>(p.ubuf);
    u64 n = 0ull;
    for (u64 i = b0 + threadIdx.x; i < b1; i += kThreads) n += ubyte(u, i, b1, pad) == 0xffu ? 1ull : 0ull;
    n = wg_sum_u64(n, red);
    if (threadIdx.x == 0) p.chunk_out[c] = (b1 - b0) + n;
}

__global__ __launch_bounds__(kThreads) void jpeg_scan2_kernel(Params p) {
    __shared__ u64 tot[kThreads];
    const int tid = threadIdx.x, nt = p.nt, nc = p.nc;
    wg_prefix_u64(p.chunk_out, p.chunk_out, nc, tot);
    for (int t = tid; t <= nt; t += kThreads) p.tile_offs[t] = p.chunk_out[t < nt ? p.tiles[t].first_chunk : (u32)nc];
    if (tid == 0 && p.total) *p.total = p.chunk_out[nc];
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_kernel(Params p) {
    __shared__ u32 wsum[kWaves];
    const int c = blockIdx.x, tid = threadIdx.x;
    const u64 b0 = p.chunk_b0[c], b1 = p.chunk_b1[c];
    const u32 pad = p.chunk_pad[c];
    const unsigned char* u = reinterpret_cast<const unsigned char*>(p.ubuf);
    u64 o = p.chunk_out[c];
    for (u64 s0 = b0; s0 < b1; s0 += (u64)kThreads * kStuffPerLane) {
        const u64 i0 = s0 + (u64)tid * kStuffPerLane;
        u32 v[kStuffPerLane];
        u32 n = 0u, ff = 0u;
#pragma unroll
        for (int k = 0; k < kStuffPerLane; ++k) {
            const bool in = i0 + k < b1;
            v[k] = in ? ubyte(u, i0 + k, b1, pad) : 0u;
            n += in ? 1u : 0u;
            ff += v[k] == 0xffu ? 1u : 0u;
        }
        u32 step_total;
        const u32 before = wg_scan_u32(n + ff, wsum, &step_total);
        unsigned char* dst = p.out + o + before;
#pragma unroll
        for (int k = 0; k < kStuffPerLane; ++k) {
            if ((u32)k < n) {
                *dst++ = (unsigned char)v[k];
                if (v[k] == 0xffu) *dst++ = 0;
            }
        }
        o += step_total;
    }
}

// ---- the kernels that every kind of file runs (declared in jpeg_u8.h) ----------------------------------------------------------------
constexpr int kZeroGroups = 1024;

int launch_coef(const Params& p, hipStream_t s) { return launch("jpeg_coef", jpeg_coef_kernel, p.nc, p, s); }

int launch_scan_zero(const Params& p, size_t ubytes, hipStream_t s) {
    if (const int rc = launch("jpeg_scan", jpeg_scan_kernel, 1, p, s)) return rc;
    const u64 zero_groups = (ubytes / 4 + kThreads - 1) / kThreads;
    return launch("jpeg_zero", jpeg_zero_kernel, (int)(zero_groups < (u64)kZeroGroups ? zero_groups : (u64)kZeroGroups), p, s);
}

int launch_stuff(const Params& p, hipStream_t s) {
    int rc;
    if ((rc = launch("jpeg_ffcount", jpeg_ffcount_kernel, p.nc, p, s))) return rc;
    if ((rc = launch("jpeg_scan2", jpeg_scan2_kernel, 1, p, s))) return rc;
    return launch("jpeg_stuff", jpeg_stuff_kernel, p.nc, p, s);
}

// ---- the host's plan -------------------------------------------------------------------------------------------------------------

// A crop is one stream; the table is jpeg_u8.h's head and nothing more.  The stuffed worst case: 2 x 208 bytes per block (optimised:
// 2 x ceil(1665 x blocks / 8) per crop).  `table` (optional) receives the table's bytes.
struct Plan : CropPlan {
    bool opt;                     // optimised Huffman tables: a crop at the frequency limit is refused
};
static Plan plan(const Request& r, bool opt, std::vector<unsigned char>* table) {
    Plan t{};
    t.opt = opt;
    u64 opt_bytes = 0;
    plan_crops(r, opt, &t, [&](const Crop& c, int, int) { opt_bytes += (kOptBlockBits * c.blocks + 7ull) / 8ull; });
    if (t.rc != CIAOSR_OK) return t;
    plan_streams(&t, (u64)t.nt, (u64)t.ncc, opt ? opt_bytes : kBlockBytes * t.blocks);
    if (!table) return t;
    table->resize(t.table_bytes);
    fill_crops(r, t, table->data());
    return t;
}

struct Work {
    StreamWork s;
    u32 *block_bits, *tile_hist, *tile_huff;
    u64* offs2;
    void carve(Arena& a, const Plan& t) {
        s.carve_head(a, t);
        block_bits = a.take<u32>((size_t)t.blocks);
        offs2 = a.take<u64>(2);
        s.carve_streams(a, t);
        tile_hist = tile_huff = nullptr;
        if (t.opt) {
            tile_hist = a.take<u32>((size_t)t.nt * kTables * 256);
            tile_huff = a.take<u32>((size_t)t.nt * 2 * kHuff);
        }
    }
};

// `dht`: optimised tables, [n][4][kDhtRecord]; null: the Annex K tables
static int encode(const Request& r, unsigned char* out, size_t out_capacity, u64* tile_offs, u64* total, unsigned char* dht, void* workspace,
                  size_t workspace_bytes, hipStream_t s) {
    std::vector<unsigned char> table;
    const Plan t = plan(r, dht != nullptr, &table);
    Work w;
    int rc;
    if ((rc = prepare(t, table, out_capacity, workspace, workspace_bytes, s, &w))) return rc;
    Params p = w.s.coef_params(r, t);
    w.s.bind_streams(&p);
    p.block_bits = w.block_bits;
    p.out = out;
    p.tile_offs = tile_offs ? tile_offs : w.offs2;
    p.total = total;
    p.tile_hist = w.tile_hist;
    p.tile_huff = w.tile_huff;
    p.dht = dht;
    // the workspace holds what the last call left: the histograms start from zero in every call
    if (t.opt && hipMemsetAsync(w.tile_hist, 0, sizeof(u32) * (size_t)t.nt * kTables * 256, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    if ((rc = launch_coef(p, s))) return rc;
    if (t.opt) {
        if ((rc = launch("jpeg_hist", jpeg_hist_kernel, t.nc, p, s))) return rc;
        if ((rc = launch("jpeg_tables", jpeg_tables_kernel, t.nt, p, s))) return rc;
    }
    if ((rc = launch("jpeg_count", jpeg_count_kernel, t.nc, p, s))) return rc;
    if ((rc = launch_scan_zero(p, t.ubytes, s))) return rc;
    if ((rc = launch("jpeg_pack", jpeg_pack_kernel, t.nc, p, s))) return rc;
    return launch_stuff(p, s);
}

}  // namespace jpeg
}  // namespace ciaosr

using namespace ciaosr;
using namespace ciaosr::jpeg;

extern "C" size_t ciaosr_jpeg_tiles_workspace_bytes(const int* rects, int n_tiles, int subsampling, int mcus_per_chunk) {
    return work_bytes<Work>(plan(size_request(rects, n_tiles, subsampling, mcus_per_chunk), false, nullptr));
}
extern "C" size_t ciaosr_jpeg_tiles_capacity_bytes(const int* rects, int n_tiles, int subsampling) {
    return plan(size_request(rects, n_tiles, subsampling, 0), false, nullptr).capacity;
}
extern "C" size_t ciaosr_jpeg_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk) {
    return ciaosr_jpeg_tiles_workspace_bytes(Whole(H, W).rect, 1, subsampling, mcus_per_chunk);
}
extern "C" size_t ciaosr_jpeg_capacity_bytes(int H, int W, int subsampling) {
    return ciaosr_jpeg_tiles_capacity_bytes(Whole(H, W).rect, 1, subsampling);
}

extern "C" int ciaosr_jpeg_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                           int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                           unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    Request r;
    if (const int rc = checked_request(src, pitch, H, W, bgr, rects, n_tiles, quality, subsampling, mcus_per_chunk, out, tile_offs, workspace, &r))
        return rc;
    return encode(r, out, out_capacity, tile_offs, nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ciaosr_jpeg_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                                     int mcus_per_chunk, unsigned char* out, size_t out_capacity, unsigned long long* total_bytes,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    const Whole whole(H, W);
    Request r;
    if (const int rc = checked_request(src, pitch, H, W, bgr, whole.rect, 1, quality, subsampling, mcus_per_chunk, out, total_bytes, workspace, &r))
        return rc;
    return encode(r, out, out_capacity, nullptr, total_bytes, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- optimised Huffman tables ---------------------------------------------------------------------------------------------------------
extern "C" size_t ciaosr_jpeg_opt_result_bytes(int n_tiles) {
    return n_tiles < 1 ? 0 : 8 * ((size_t)n_tiles + 1) + (size_t)kTables * kDhtRecord * (size_t)n_tiles;
}
extern "C" size_t ciaosr_jpeg_opt_tiles_workspace_bytes(const int* rects, int n_tiles, int subsampling, int mcus_per_chunk) {
    return work_bytes<Work>(plan(size_request(rects, n_tiles, subsampling, mcus_per_chunk), true, nullptr));
}
extern "C" size_t ciaosr_jpeg_opt_tiles_capacity_bytes(const int* rects, int n_tiles, int subsampling) {
    return plan(size_request(rects, n_tiles, subsampling, 0), true, nullptr).capacity;
}
extern "C" size_t ciaosr_jpeg_opt_workspace_bytes(int H, int W, int subsampling, int mcus_per_chunk) {
    return ciaosr_jpeg_opt_tiles_workspace_bytes(Whole(H, W).rect, 1, subsampling, mcus_per_chunk);
}
extern "C" size_t ciaosr_jpeg_opt_capacity_bytes(int H, int W, int subsampling) {
    return ciaosr_jpeg_opt_tiles_capacity_bytes(Whole(H, W).rect, 1, subsampling);
}

extern "C" int ciaosr_jpeg_opt_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects, int n_tiles,
                                               int quality, int subsampling, int mcus_per_chunk, unsigned char* out, size_t out_capacity,
                                               void* result, void* workspace, size_t workspace_bytes, void* stream) {
    Request r;
    if (const int rc = checked_request(src, pitch, H, W, bgr, rects, n_tiles, quality, subsampling, mcus_per_chunk, out, result, workspace, &r))
        return rc;
    u64* offs = static_cast<u64*>(result);
    return encode(r, out, out_capacity, offs, nullptr, reinterpret_cast<unsigned char*>(offs + n_tiles + 1), workspace, workspace_bytes,
                  (hipStream_t)stream);
}

extern "C" int ciaosr_jpeg_opt_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int quality, int subsampling,
                                         int mcus_per_chunk, unsigned char* out, size_t out_capacity, void* result, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return ciaosr_jpeg_opt_encode_tiles_u8(src, pitch, H, W, bgr, Whole(H, W).rect, 1, quality, subsampling, mcus_per_chunk, out, out_capacity, result,
                                           workspace, workspace_bytes, stream);
}
