// The TIFF front end of the deflate coder (ciaosr_amd/tiff_hip.py): part of png_u8.hip's translation unit, included at
// its end, so that the coder -- band table, Layout, run_deflate, the tiles scan, the match coder -- is the PNG path's own code.
//
// A level of a pyramidal TIFF is cut into T x T tiles, row-major, ceil(W / T) x ceil(H / T) of them; a tile that reaches past the image
// repeats the image's last column and row (P[r][c] = I[min(ty T + r, H - 1)][min(tx T + c, W - 1)]).  A tile's data under
// Compression = 8, Predictor = 2 is ONE zlib stream of its T * T * C * S / 8 predicted bytes: per SAMPLE (8 or 16 bits, not per byte)
// D[r][c][k] = P[r][c][k] - P[r][c - 1][k] mod 2^S, D[r][0][k] = P[r][0][k]; the stream holds r, then c, then k, a 16-bit sample low
// byte first.  There is no filter byte and no filter choice: a line of the band table is BPP * T bytes.
//
// tiff_predict_tiles_kernel<BPP>: one workgroup per band of rows of one tile (the band table of plan_tiff: the PNG tiles' table without
// rects -- a tile's place follows from its index).  It reads the source once (every index clamped to H - 1, W - 1: nothing is read
// past the image nor past a pitched crop's last row), writes the predicted bytes at the band's offset and hands the coder what
// filter_band hands it: the band's 257-bin histogram (counted in LDS) and its Adler-32 partials.  From there on: run_deflate with
// png_tiles_scan_kernel.  The match coder gets the line explicitly (LzP.line = BPP * T, no rects): its far candidates are L - BPP, L
// and L + BPP, and a padding row is an exact repeat at distance L.
//
// halve_box_u16_kernel: the 16-bit levels below the LR size, out = (a[2i][2j] + a[2i][j1] + a[i1][2j] + a[i1][j1] + 2) >> 2 with
// i1 = min(2i + 1, h - 1), j1 = min(2j + 1, w - 1), per sample, in unsigned 32-bit arithmetic.
#pragma once

namespace ciaosr {
namespace png {

struct TiffP {
    const unsigned char* src;     // [H][pitch]: BPP 1, 3, 4 bytes per pixel, or BPP / 2 native uint16 samples
    size_t pitch;
    int H, W, bgr;
    int T, ntx;                   // the tile's side; tiles per row of tiles
    const TileBand* bands;        // [nb]
    const u64* offs;              // [nb + 1]: the bands in the predicted stream
    unsigned char* dst;
    u32 *hist, *adler;            // [nb][kStride], [nb][2] as FilterP's
};

// The samples of pixel x of the row at `cur` in stream order (R G B, then A; one grey sample): BPP 1, 3, 4 are 8-bit samples (four
// bytes per pixel: ONE aligned 32-bit load), BPP 2 and 6 one or three 16-bit samples (aligned 16-bit loads).
template <int BPP>
__device__ __forceinline__ void load_samples(const unsigned char* cur, int x, int bgr, u32* v) {
    const int s0 = bgr ? 2 : 0, s2 = bgr ? 0 : 2;
    if constexpr (BPP == 1) {
        v[0] = cur[x];
    } else if constexpr (BPP == 2) {
        v[0] = reinterpret_cast<const unsigned short*>(cur)[x];
    } else if constexpr (BPP == 4) {
        const u32 pv = reinterpret_cast<const u32*>(cur)[x];
        v[0] = pv >> (8 * s0) & 255u;
        v[1] = pv >> 8 & 255u;
        v[2] = pv >> (8 * s2) & 255u;
        v[3] = pv >> 24;
    } else if constexpr (BPP == 6) {
        const unsigned short* q = reinterpret_cast<const unsigned short*>(cur) + 3 * (size_t)x;
        v[0] = q[s0], v[1] = q[1], v[2] = q[s2];
    } else {
        static_assert(BPP == 3, "bytes per pixel");
        const unsigned char* q = cur + 3 * (size_t)x;
        v[0] = q[s0], v[1] = q[1], v[2] = q[s2];
    }
}

template <int BPP>
__global__ __launch_bounds__(kThreads) void tiff_predict_tiles_kernel(TiffP t) {
    constexpr bool k16 = BPP == 2 || BPP == 6;
    constexpr int C = k16 ? BPP / 2 : BPP;                   // samples per pixel
    constexpr u32 kMask = k16 ? 0xffffu : 0xffu;
    __shared__ u32 h[kWaves][kStride];
    __shared__ u64 red64[kWaves][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int band = blockIdx.x;
    const TileBand b = t.bands[band];
    const int y0 = (b.tile / t.ntx) * t.T, x0 = (b.tile % t.ntx) * t.T;
    for (int i = tid; i < kWaves * kStride; i += kThreads) (&h[0][0])[i] = 0u;
    __syncthreads();
    const u64 L = (u64)BPP * (u64)t.T;
    unsigned char* dst = t.dst + t.offs[band];
    u32 A = 0u, B = 0u;                                      // thread 0: the band's Adler sums so far
    for (int row = b.r0; row < b.r1; ++row) {
        const unsigned char* cur = t.src + (size_t)min(y0 + row, t.H - 1) * t.pitch;
        unsigned char* out = dst + (u64)(row - b.r0) * L;
        u64 a1 = 0ull, a2 = 0ull;
        for (int c = tid; c < t.T; c += kThreads) {
            u32 v[C], a[C];
            load_samples<BPP>(cur, min(x0 + c, t.W - 1), t.bgr, v);
            if (c > 0) {
                load_samples<BPP>(cur, min(x0 + c - 1, t.W - 1), t.bgr, a);
            } else {
#pragma unroll
                for (int k = 0; k < C; ++k) a[k] = 0u;
            }
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const u32 d = (v[k] - a[k]) & kMask;
#pragma unroll
                for (int e = 0; e < (k16 ? 2 : 1); ++e) {    // a 16-bit sample: low byte first
                    const u32 fb = e == 0 ? d & 255u : d >> 8;
                    const u64 j = (u64)BPP * (u64)c + (u64)((k16 ? 2 : 1) * k + e);
                    out[j] = (unsigned char)fb;
                    atomicAdd(&h[wave][fb], 1u);
                    a1 += fb;
                    a2 += (L - j) * (u64)fb;                 // L <= 6 * 4096 < 2^15: < 2^23 per byte, < 2^38 per row
                }
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
        __syncthreads();                                     // red64 is rewritten by the next row
    }
    for (int i = tid; i < kSyms; i += kThreads) {
        u32 s = i == 256 ? 1u : 0u;                          // one end-of-block per band
        for (int w = 0; w < kWaves; ++w) s += h[w][i];
        t.hist[(size_t)band * kStride + i] = s;
    }
    if (tid == 0) {
        t.adler[2 * (size_t)band] = A;
        t.adler[2 * (size_t)band + 1] = B;
    }
}

struct HalveP {
    const unsigned char* src;     // uint16 [h][w][C], rows pitch BYTES apart
    size_t pitch;
    int h, w, C;
    unsigned char* dst;           // uint16 [ceil(h / 2)][ceil(w / 2)][C], rows dst_pitch BYTES apart
    size_t dst_pitch;
};
__global__ __launch_bounds__(kThreads) void halve_box_u16_kernel(HalveP p) {
    const int wo = (p.w + 1) >> 1;
    const int i = blockIdx.y, e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= wo * p.C) return;
    const int j = e / p.C, k = e - j * p.C;
    const int i1 = min(2 * i + 1, p.h - 1), j1 = min(2 * j + 1, p.w - 1);
    const unsigned short* r0 = reinterpret_cast<const unsigned short*>(p.src + (size_t)(2 * i) * p.pitch);
    const unsigned short* r1 = reinterpret_cast<const unsigned short*>(p.src + (size_t)i1 * p.pitch);
    const size_t c0 = (size_t)(2 * j) * p.C + k, c1 = (size_t)j1 * p.C + k;
    const u32 s = (u32)r0[c0] + (u32)r0[c1] + (u32)r1[c0] + (u32)r1[c1] + 2u;
    reinterpret_cast<unsigned short*>(p.dst + (size_t)i * p.dst_pitch)[e] = (unsigned short)(s >> 2);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
static inline bool tiff_bpp_ok(int bpp) { return bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6; }
static inline bool tiff_tile_ok(int T) { return T >= 16 && T <= 4096 && T % 16 == 0; }
// rows of a tile per band: the argument (at most T) if > 0, else about 128 KiB of predicted bytes
static inline int tiff_rows_per_band(int bpp, int T, int rows) {
    const long r = rows > 0 ? rows : (128L * 1024L) / ((long)bpp * T);
    return (int)(r < 1 ? 1 : (r > T ? T : r));
}

// The band table of a level: [offs u64 (nb + 1)][bands TileBand nb][first u32 (nt + 1)] and with `lz` [chunk_first u32 (nb + 1)].
// Every tile has the same ceil(T / R) bands of lines of BPP * T bytes.
struct TiffPlan {
    int rc;
    int nt, ntx, nb, R;
    u64 total;                    // bytes of all predicted tiles
    size_t capacity;
    size_t o_bands, o_first, o_chunks, table_bytes;
    u64 chunks;
};
static TiffPlan plan_tiff(int bpp, int H, int W, int T, int rows_arg, bool lz, std::vector<unsigned char>* table) {
    TiffPlan t{};
    t.rc = CIAOSR_ERR_BAD_ARG;
    if (!tiff_bpp_ok(bpp) || !image_ok(H, W) || !tiff_tile_ok(T) || rows_arg < 0) return t;
    const int R = tiff_rows_per_band(bpp, T, rows_arg);
    const u64 L = (u64)bpp * (u64)T;
    const int ntx = ceil_div(W, T), nty = ceil_div(H, T), bpt = ceil_div(T, R);
    const u64 nt = (u64)ntx * (u64)nty, nb = nt * (u64)bpt;
    const u64 cpt = (u64)(T / R) * lz_chunks_of((u64)R * L) + lz_chunks_of((u64)(T % R) * L);       // parse chunks per tile
    t.rc = CIAOSR_ERR_UNSUPPORTED;
    if (nb > (u64)INT_MAX / 2 || (lz && nt * cpt > (u64)INT_MAX)) return t;
    t.rc = CIAOSR_OK;
    t.nt = (int)nt;
    t.ntx = ntx;
    t.nb = (int)nb;
    t.R = R;
    t.total = nt * (u64)T * L;
    t.capacity = (size_t)nt * capacity((size_t)T * (size_t)L, bpt, true);
    t.chunks = nt * cpt;
    t.o_bands = sizeof(u64) * ((size_t)nb + 1);
    t.o_first = t.o_bands + sizeof(TileBand) * (size_t)nb;
    t.o_chunks = t.o_first + sizeof(u32) * ((size_t)nt + 1);
    t.table_bytes = t.o_chunks + (lz ? sizeof(u32) * ((size_t)nb + 1) : 0);
    if (!table) return t;
    table->resize(t.table_bytes);
    u64* offs = reinterpret_cast<u64*>(table->data());
    TileBand* bands = reinterpret_cast<TileBand*>(table->data() + t.o_bands);
    u32* first = reinterpret_cast<u32*>(table->data() + t.o_first);
    u64 off = 0;
    int i = 0;
    for (int k = 0; k < t.nt; ++k) {
        first[k] = (u32)i;
        for (int r0 = 0; r0 < T; r0 += R, ++i) {
            const int r1 = r0 + R < T ? r0 + R : T;
            offs[i] = off;
            bands[i] = TileBand{k, r0, r1, r1 == T ? 1 : 0};
            off += (u64)(r1 - r0) * L;
        }
    }
    offs[i] = off;
    first[t.nt] = (u32)i;
    if (lz) {
        u32* cf = reinterpret_cast<u32*>(table->data() + t.o_chunks);
        cf[0] = 0u;
        for (int j = 0; j < i; ++j) cf[j + 1] = cf[j] + (u32)lz_chunks_of(offs[j + 1] - offs[j]);
    }
    return t;
}
static Layout tiff_layout(const TiffPlan& t, bool lz) {
    Layout l = image_layout(t.nb, (size_t)t.total, lz ? (size_t)t.chunks : 0);
    l.table = t.table_bytes;
    return l;
}

}  // namespace png
}  // namespace ciaosr

static size_t tiff_workspace_entry(int bpp, int H, int W, int T, int rows, bool lz) {
    const ciaosr::png::TiffPlan t = ciaosr::png::plan_tiff(bpp, H, W, T, rows, lz, nullptr);
    return t.rc == CIAOSR_OK ? ciaosr::png::work_bytes(ciaosr::png::tiff_layout(t, lz)) : 0;
}

static int tiff_encode_entry(bool lz, int bpp, const void* image, size_t pitch, int H, int W, int bgr, int T, int rows,
                             unsigned char* out, size_t out_capacity, unsigned long long* tile_offs, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace ciaosr;
    using namespace ciaosr::png;
    const unsigned char* src = static_cast<const unsigned char*>(image);
    CIAOSR_CHECK_ARG(tiff_bpp_ok(bpp) && tiff_tile_ok(T) && rows >= 0 && (bgr == 0 || bgr == 1));
    CIAOSR_CHECK_ARG(out && tile_offs && workspace && image_ok(H, W) && source_ok(bpp, src, pitch, W));
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(tile_offs) & 7u) == 0);
    CIAOSR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    std::vector<unsigned char> table;
    const TiffPlan t = plan_tiff(bpp, H, W, T, rows, lz, &table);
    if (t.rc != CIAOSR_OK) return t.rc;
    if (out_capacity < t.capacity) return CIAOSR_ERR_WORKSPACE;
    Work w;
    if (!carve_workspace(workspace, workspace_bytes, tiff_layout(t, lz), &w)) return CIAOSR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // from pageable memory: the copy has left `table` when the call returns
    if (hipMemcpyAsync(w.band_table, table.data(), t.table_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return CIAOSR_ERR_LAUNCH;
    const u64* offs = reinterpret_cast<const u64*>(w.band_table);
    const TileBand* bands = reinterpret_cast<const TileBand*>(w.band_table + t.o_bands);
    TiffP f{};
    f.src = src;
    f.pitch = pitch;
    f.H = H;
    f.W = W;
    f.bgr = bgr;
    f.T = T;
    f.ntx = t.ntx;
    f.bands = bands;
    f.offs = offs;
    f.dst = w.filtered;
    f.hist = w.hist;
    f.adler = w.adler;
    int rc = bpp == 1   ? launch("tiff_predict_tiles", tiff_predict_tiles_kernel<1>, t.nb, kThreads, s, f)
             : bpp == 2 ? launch("tiff_predict_tiles", tiff_predict_tiles_kernel<2>, t.nb, kThreads, s, f)
             : bpp == 3 ? launch("tiff_predict_tiles", tiff_predict_tiles_kernel<3>, t.nb, kThreads, s, f)
             : bpp == 4 ? launch("tiff_predict_tiles", tiff_predict_tiles_kernel<4>, t.nb, kThreads, s, f)
                        : launch("tiff_predict_tiles", tiff_predict_tiles_kernel<6>, t.nb, kThreads, s, f);
    if (rc) return rc;
    DeflateP p = deflate_params(w.filtered, listed_bands(offs, t.nb), w);
    p.out = out;
    p.adler = w.adler;
    p.tiles = bands;
    LzP q = lz_params(p, w);
    q.line = (u64)bpp * (u64)T;                               // no rects: every tile's line is the same
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

extern "C" int ciaosr_tiff_rows_per_band(int bytes_per_pixel, int T, int rows_per_band_arg) {
    if (!ciaosr::png::tiff_bpp_ok(bytes_per_pixel) || !ciaosr::png::tiff_tile_ok(T) || rows_per_band_arg < 0) return 0;
    return ciaosr::png::tiff_rows_per_band(bytes_per_pixel, T, rows_per_band_arg);
}
extern "C" size_t ciaosr_tiff_tiles_workspace_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band_arg) {
    return tiff_workspace_entry(bytes_per_pixel, H, W, T, rows_per_band_arg, false);
}
extern "C" size_t ciaosr_tiff_lz_tiles_workspace_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band_arg) {
    return tiff_workspace_entry(bytes_per_pixel, H, W, T, rows_per_band_arg, true);
}
extern "C" size_t ciaosr_tiff_tiles_capacity_bytes(int bytes_per_pixel, int H, int W, int T, int rows_per_band_arg) {
    const ciaosr::png::TiffPlan t = ciaosr::png::plan_tiff(bytes_per_pixel, H, W, T, rows_per_band_arg, false, nullptr);
    return t.rc == CIAOSR_OK ? t.capacity : 0;
}
extern "C" int ciaosr_tiff_encode_tiles(int bytes_per_pixel, const void* image, size_t pitch, int H, int W, int bgr, int T,
                                        int rows_per_band_arg, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return tiff_encode_entry(false, bytes_per_pixel, image, pitch, H, W, bgr, T, rows_per_band_arg, out, out_capacity, tile_offs,
                             workspace, workspace_bytes, stream);
}
extern "C" int ciaosr_tiff_lz_encode_tiles(int bytes_per_pixel, const void* image, size_t pitch, int H, int W, int bgr, int T,
                                           int rows_per_band_arg, unsigned char* out, size_t out_capacity,
                                           unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream) {
    return tiff_encode_entry(true, bytes_per_pixel, image, pitch, H, W, bgr, T, rows_per_band_arg, out, out_capacity, tile_offs,
                             workspace, workspace_bytes, stream);
}

extern "C" int ciaosr_halve_box_u16(const unsigned short* src, size_t pitch, int h, int w, int channels, unsigned short* dst,
                                    size_t dst_pitch, void* stream) {
    using namespace ciaosr;
    using namespace ciaosr::png;
    CIAOSR_CHECK_ARG(src && dst && h > 0 && w > 0 && (channels == 1 || channels == 3));
    CIAOSR_CHECK_ARG(pitch >= 2 * (size_t)channels * (size_t)w && dst_pitch >= 2 * (size_t)channels * (size_t)((w + 1) / 2));
    CIAOSR_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | pitch | dst_pitch) & 1u) == 0);
    if (h > 2 * 65535 || w > (1 << 24)) return CIAOSR_ERR_UNSUPPORTED;           // one grid row per output row
    HalveP p{reinterpret_cast<const unsigned char*>(src), pitch, h, w, channels, reinterpret_cast<unsigned char*>(dst), dst_pitch};
    const int ho = (h + 1) / 2, wo = (w + 1) / 2;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("halve_box_u16", s);
    hipLaunchKernelGGL(halve_box_u16_kernel, dim3((unsigned)ceil_div(wo * channels, kThreads), (unsigned)ho), dim3(kThreads), 0, s, p);
    return launch_status("halve_box_u16");
}
