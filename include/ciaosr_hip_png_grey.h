/* The grey PNG entry points of libciaosr_hip.so (version 340): part of the C ABI of ciaosr_hip.h, which includes this
 * file -- include that one.  They stand in a file of their own because the PNG size exports declared in ciaosr_hip.h are exactly the
 * ones whose values tests/golden/png_sizes.json records (tests/test_png_sizes_host.py), a record made before this family existed;
 * tests/test_grey_host.py holds these declarations to the ctypes table (_lib.GREY_PNG_SIGNATURES) and their sizes to the formulae. */
#ifndef CIAOSR_HIP_PNG_GREY_H
#define CIAOSR_HIP_PNG_GREY_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The one-byte-per-pixel siblings of the PNG calls of ciaosr_hip.h (the ciaosr_png_rgba_* and ciaosr_png_rgba_lz_* entries), with the same
 * arguments and contracts; where those say 4 W these say W.  rows of one band: rows_per_band if > 0, else max(1, 131072 / (W + 1)).
 * src[y * pitch + x], pitch >= W, no alignment rule: a crop may start at any byte.  bgr must be 0 or 1 and is not read: there is no
 * channel order.  A row of dst is 1 + W bytes; the left predecessor of a byte is the byte before it, the upper one the byte above;
 * zeros stand left of column 0 and above row 0, of a crop too.  Everything after the filter is the same code on the shorter rows.
 * The match candidates of the *_lz_* entries are 1, 2, 3, 4, 6, 8, 12, 16, L - 1, L, L + 1 with L = W + 1; for narrow images the last
 * three coincide with near distances, and "ties go to the earliest" decides.  The host wraps a stream with IHDR colour type 0. */
int ciaosr_png_grey_rows_per_band(int W, int rows_per_band);
int ciaosr_png_grey_filter_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* dst,
                              unsigned int* hist, unsigned int* adler, void* stream);
size_t ciaosr_png_grey_workspace_bytes(int H, int W, int rows_per_band);
size_t ciaosr_png_grey_capacity_bytes(int H, int W, int rows_per_band);
int ciaosr_png_grey_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                              size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_png_grey_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
size_t ciaosr_png_grey_tiles_capacity_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_grey_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/, int n_tiles,
                                    int rows_per_band, unsigned char* out, size_t out_capacity, unsigned long long* tile_offs,
                                    void* workspace, size_t workspace_bytes, void* stream);
size_t ciaosr_png_grey_lz_workspace_bytes(int H, int W, int rows_per_band);
int ciaosr_png_grey_lz_encode_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, int rows_per_band, unsigned char* out,
                                 size_t out_capacity, unsigned long long* total_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t ciaosr_png_grey_lz_tiles_workspace_bytes(const int* rects /*host*/, int n_tiles, int rows_per_band);
int ciaosr_png_grey_lz_encode_tiles_u8(const unsigned char* src, size_t pitch, int H, int W, int bgr, const int* rects /*host*/,
                                       int n_tiles, int rows_per_band, unsigned char* out, size_t out_capacity,
                                       unsigned long long* tile_offs, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIAOSR_HIP_PNG_GREY_H */
