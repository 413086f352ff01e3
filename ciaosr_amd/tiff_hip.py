"""Pyramidal tiled TIFF files written from device images on the MI355X (csrc/tiff_tiles.h, the second front end of png_u8.hip's coder).

The file (DESIGN 4.1i-b7 holds the contract): classic little-endian TIFF (`II`, 42; no BigTIFF), one image file directory (IFD) per
level chained through the next-IFD offsets, the full-resolution level first, every later IFD with NewSubfileType = 1 -- the layout of
generic pyramidal-TIFF readers and of GDAL's overviews; no SubIFDs.  Per IFD exactly the tags 254, 256, 257, 258, 259 (= 8, Adobe
deflate), 262 (1 grey, 2 RGB / RGBA), 277, 284 (= 1), 317 (= 2, the horizontal predictor), 322, 323, 324, 325, for RGBA 338 (= 2,
unassociated alpha: the colour as stored), and 339 (= 1).  Tiles are T x T (T a multiple of 16 in 16..4096, default 256), row-major;
a tile that reaches past the level repeats the level's last column and row, so padding costs zeros after the predictor and repeats
of the row above.  The predictor works per sample -- at 16 bits on the samples, not on their bytes -- and a 16-bit sample is stored low
byte first.  A tile's data is ONE zlib stream of its T * T * C * S / 8 predicted bytes, made by the coder that follows the PNG filter:
bands of dynamic Huffman blocks of literals, and with `matches=True` LZ77 matches at the distances 1, 2, 3, 4, 6, 8, 12, 16 and
L - B, L, L + B (L = B * T the tile's line, B the bytes per pixel) where that makes a band smaller -- a padding row is one repeat at
distance L.  Every tile's data and every IFD starts at an even offset; a level's tile data comes first, then its out-of-line tag
values, then its IFD.

The device makes the tile streams of one level in one set of launches (predict, plan, tiles scan, pack; the match coder: a memset and
three more) and the host reads them in two synchronising copies per level: the offsets, then the streams.  The host only lays out
the container (`plan_file`: pure integer code).  Images: uint8 [H, W] (grey), [H, W, 3] (`order` 'bgr' as `tensor2img_u8` makes it,
or 'rgb'), [H, W, 4] ('bgra' / 'rgba'; 'bgr' / 'rgb' name the same), and torch.uint16 [H, W], [H, W, 3], with `png_hip`'s image
rules (pitched rows are fine).  There is no CPU fallback: a host array raises.  Limits: files below 4 GiB, no 16-bit alpha, no
strips, no JPEG tiles, no metadata beyond the tags above.
"""
import ctypes as C
import os
import struct

import torch

from . import _lib, hip_ops, png_hip
from ._lib import CiaoSRHipError

TILE_DEFAULT = 256
TILE_MIN, TILE_MAX, TILE_STEP = 16, 4096, 16
MAX_OFFSET = (1 << 32) - 1
SHORT, LONG = 3, 4
TAGS = (254, 256, 257, 258, 259, 262, 277, 284, 317, 322, 323, 324, 325, 338, 339)


def check_tile(tile):
    """The tile side as an int; ValueError unless it is a multiple of 16 in 16..4096."""
    if isinstance(tile, bool) or not isinstance(tile, int) or not (TILE_MIN <= tile <= TILE_MAX) or tile % TILE_STEP:
        raise ValueError(f'tile={tile!r}: a multiple of {TILE_STEP} in {TILE_MIN}..{TILE_MAX}')
    return tile


def tiff_level_sizes(height, width, tile=TILE_DEFAULT):
    """[(H_l, W_l)] of a pyramid's levels, the top first: each next level is (ceil(h / 2), ceil(w / 2)) (`pyramid.level_sizes`'s
    sizes), and the first level with max(h, w) <= tile is the last.  An image that fits one tile has one level."""
    tile = check_tile(tile)
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f'empty image {height} x {width}')
    sizes = [(h, w)]
    while max(h, w) > tile:
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((h, w))
    return sizes


def _check_meta(meta):
    h, w, samples, bits, tile = (meta[k] for k in ('height', 'width', 'samples', 'bits', 'tile'))
    check_tile(tile)
    if int(h) < 1 or int(w) < 1:
        raise ValueError(f'empty level {h} x {w}')
    if samples not in (1, 3, 4) or bits not in (8, 16):
        raise ValueError(f'samples={samples!r}, bits={bits!r}: 1, 3 or 4 samples of 8 or 16 bits')
    if samples == 4 and bits == 16:
        raise ValueError('four samples of 16 bits: no 16-bit alpha')
    return int(h), int(w), samples, bits, tile


def _even(n):
    return n + (n & 1)


def plan_file(levels_meta, tile_lengths):
    """The container of a file from numbers alone.  levels_meta: per level, the top first, dict(height, width, samples 1 / 3 / 4,
    bits 8 / 16, tile); tile_lengths: per level the byte counts of its tiles' streams, row-major.  -> dict(header: the 8 bytes,
    levels: per level dict(tile_offsets, extra_offset, extra: the out-of-line tag values, ifd_offset, ifd: the IFD's bytes),
    total: the file's size).  Layout: header; per level its tile data (every tile at an even offset), its out-of-line values, its
    IFD (even).  ValueError for a wrong count of tiles and -- before anything is written anywhere -- for a file whose offsets would
    pass 2^32 - 1."""
    levels_meta, tile_lengths = list(levels_meta), [list(t) for t in tile_lengths]
    if not levels_meta or len(levels_meta) != len(tile_lengths):
        raise ValueError(f'{len(levels_meta)} levels but {len(tile_lengths)} lists of tile lengths')
    pos = 8
    places = []
    for meta, lengths in zip(levels_meta, tile_lengths):
        h, w, samples, bits, tile = _check_meta(meta)
        nt = -(-h // tile) * -(-w // tile)
        if len(lengths) != nt or any(int(n) < 1 for n in lengths):
            raise ValueError(f'a {h} x {w} level has {nt} tiles of {tile}, got {len(lengths)} lengths (every one at least 1)')
        offsets = []
        for n in lengths:
            offsets.append(pos)
            pos = _even(pos + int(n))
        extra_offset = pos
        wide = 2 * samples if samples > 2 else 0              # BitsPerSample and SampleFormat: SHORT x samples, inline up to two
        many = 4 * nt if nt > 1 else 0                        # TileOffsets and TileByteCounts: LONG x tiles, inline for one
        o_bits, o_offs, o_counts, o_format = (extra_offset, extra_offset + wide, extra_offset + wide + many,
                                              extra_offset + wide + 2 * many)
        ifd_offset = o_format + wide
        n_tags = 15 if samples == 4 else 14
        pos = ifd_offset + 2 + 12 * n_tags + 4
        places.append(dict(h=h, w=w, samples=samples, bits=bits, tile=tile, nt=nt, lengths=[int(n) for n in lengths], offsets=offsets,
                           extra_offset=extra_offset, o=(o_bits, o_offs, o_counts, o_format), ifd_offset=ifd_offset))
        if pos > MAX_OFFSET:
            raise ValueError(f'the file would pass 2^32 - 1 bytes ({pos} after {len(places)} levels): no BigTIFF here')
    out = []
    for k, p in enumerate(places):
        samples, nt = p['samples'], p['nt']
        o_bits, o_offs, o_counts, o_format = p['o']
        extra = b''
        if samples > 2:
            extra += struct.pack(f'<{samples}H', *([p['bits']] * samples))
        if nt > 1:
            extra += struct.pack(f'<{nt}I', *p['offsets']) + struct.pack(f'<{nt}I', *p['lengths'])
        if samples > 2:
            extra += struct.pack(f'<{samples}H', *([1] * samples))

        def short(tag, v):
            return struct.pack('<HHIHH', tag, SHORT, 1, v, 0)

        def long(tag, v):
            return struct.pack('<HHII', tag, LONG, 1, v)

        def shorts(tag, v, where):
            if samples == 1:
                return short(tag, v)
            return struct.pack('<HHII', tag, SHORT, samples, where)

        def longs(tag, values, where):
            return long(tag, values[0]) if nt == 1 else struct.pack('<HHII', tag, LONG, nt, where)

        entries = [long(254, 1 if k else 0), long(256, p['w']), long(257, p['h']), shorts(258, p['bits'], o_bits), short(259, 8),
                   short(262, 1 if samples == 1 else 2), short(277, samples), short(284, 1), short(317, 2), long(322, p['tile']),
                   long(323, p['tile']), longs(324, p['offsets'], o_offs), longs(325, p['lengths'], o_counts)]
        if samples == 4:
            entries.append(short(338, 2))
        entries.append(shorts(339, 1, o_format))
        nxt = places[k + 1]['ifd_offset'] if k + 1 < len(places) else 0
        ifd = struct.pack('<H', len(entries)) + b''.join(entries) + struct.pack('<I', nxt)
        out.append(dict(tile_offsets=p['offsets'], extra_offset=p['extra_offset'], extra=extra, ifd_offset=p['ifd_offset'], ifd=ifd))
    return dict(header=b'II' + struct.pack('<HI', 42, places[0]['ifd_offset']), levels=out, total=pos)


def _order_of(img, order):
    """`order` for png_hip's image check: a four-channel image takes 'bgr' / 'rgb' as 'bgra' / 'rgba'."""
    if isinstance(img, torch.Tensor) and img.dim() == 3 and img.shape[2] == 4:
        return {'bgr': 'bgra', 'rgb': 'rgba'}.get(order, order)
    return order


def _kind(img):
    """(samples per pixel, bits per sample) of an image tensor"""
    return (1 if img.dim() == 2 else img.shape[2]), 8 * img.element_size()


def encode_tiff_tiles_device(img, tile=TILE_DEFAULT, order='bgr', rows_per_band=0, matches=False):
    """ciaosr_tiff_encode_tiles on the current stream, no synchronisation -> (streams uint8 [capacity], offsets int64 [n + 1]) on the
    device: tile k's zlib stream (row-major, n = ceil(H / tile) * ceil(W / tile)) is streams[offsets[k]:offsets[k + 1]], offsets[0] =
    0, no gaps.  `rows_per_band`: tile rows per independently coded band, 0 = about 128 KiB of predicted bytes."""
    lz = png_hip._check_matches(matches)
    tile = check_tile(tile)
    h, w, rows, bpp, bgr = png_hip._checked(img, _order_of(img, order), rows_per_band, 'encode_tiff_tiles')
    n = -(-h // tile) * -(-w // tile)
    dev = img.device
    lib = _lib.load()
    cap = lib.ciaosr_tiff_tiles_capacity_bytes(bpp, h, w, tile, rows)
    nbytes = getattr(lib, f'ciaosr_tiff_{lz}tiles_workspace_bytes')(bpp, h, w, tile, rows)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_tiff_tiles: unsupported geometry {h}x{w}, tile={tile}, rows_per_band={rows}')
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.call(f'ciaosr_tiff_{lz}encode_tiles', bpp, hip_ops.ptr(img), C.c_size_t(png_hip._pitch(img)), h, w, bgr, tile, rows,
              hip_ops.ptr(out), C.c_size_t(cap), hip_ops.ptr(offs), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return out, offs


def _tiles_host(img, tile, order, rows_per_band, matches):
    """-> (the streams as one host buffer, the offsets as a list): the two synchronising copies of a level"""
    out, offs = encode_tiff_tiles_device(img, tile, order, rows_per_band, matches)
    o = offs.cpu().tolist()                                 # copy 1: the offsets
    return memoryview(out[:o[-1]].cpu().numpy()), o         # copy 2: the streams


def encode_tiff_tiles(img, tile=TILE_DEFAULT, order='bgr', rows_per_band=0, matches=False):
    """The tiles' zlib streams (list of bytes, row-major) of one device image, from ONE set of launches and two synchronising copies
    whatever the number of tiles."""
    raw, o = _tiles_host(img, tile, order, rows_per_band, matches)
    return [bytes(raw[o[k]:o[k + 1]]) for k in range(len(o) - 1)]


def _check_levels(levels):
    """A single image is a one-level list; the levels are of one kind and each is the halving of the one above.  ValueErrors only:
    the image rules themselves are the encoder's."""
    if isinstance(levels, torch.Tensor):
        levels = [levels]
    levels = list(levels)
    if not levels:
        raise ValueError('no levels')
    for im in levels:
        if not isinstance(im, torch.Tensor):
            raise CiaoSRHipError(f'expected device image tensors, got {type(im).__name__}')
    kinds = {(im.dim(), tuple(im.shape[2:]), im.dtype) for im in levels}
    if len(kinds) != 1:
        raise ValueError(f'the levels of one file are of one kind, got {sorted(str(k) for k in kinds)}')
    for a, b in zip(levels, levels[1:]):
        if (b.shape[0], b.shape[1]) != ((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2):
            raise ValueError(f'level {tuple(b.shape[:2])} is not the halving of {tuple(a.shape[:2])}: the top level goes first')
    return levels


def _encode_file(levels, tile, order, rows_per_band, matches):
    """-> (plan, [(host buffer, offsets)]) of the file of `levels`"""
    png_hip._check_matches(matches)
    tile = check_tile(tile)
    levels = _check_levels(levels)
    coded = [_tiles_host(im, tile, order, rows_per_band, matches) for im in levels]
    metas = []
    for im in levels:
        samples, bits = _kind(im)
        metas.append(dict(height=im.shape[0], width=im.shape[1], samples=samples, bits=bits, tile=tile))
    plan = plan_file(metas, [[o[k + 1] - o[k] for k in range(len(o) - 1)] for _, o in coded])
    return plan, coded


def _pieces(plan, coded):
    """The file's bytes in order, piece by piece"""
    yield plan['header']
    for lv, (raw, o) in zip(plan['levels'], coded):
        for k in range(len(o) - 1):
            yield raw[o[k]:o[k + 1]]
            if (o[k + 1] - o[k]) & 1:
                yield b'\0'
        yield lv['extra']
        yield lv['ifd']


def encode_tiff(levels, tile=TILE_DEFAULT, order='bgr', rows_per_band=0, matches=False):
    """The pyramidal TIFF file (bytes) of the device images `levels`, the top level first, each next one its halving (as
    `tiff_level_sizes` lists them; a single image: a one-level file)."""
    return b''.join(bytes(p) for p in _pieces(*_encode_file(levels, tile, order, rows_per_band, matches)))


def imwrite_gpu_tiff(levels_or_image, path, tile=TILE_DEFAULT, order='bgr', rows_per_band=0, matches=False):
    """`encode_tiff` into the file `path`: the tiles are coded on the device, the container is planned from their sizes (a file past
    4 GiB raises before a byte is written) and the streams are written in order, piece by piece.  -> dict(levels, tiles, bytes)."""
    plan, coded = _encode_file(levels_or_image, tile, order, rows_per_band, matches)
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        for piece in _pieces(plan, coded):
            f.write(piece)
    return dict(levels=len(coded), tiles=sum(len(o) - 1 for _, o in coded), bytes=plan['total'])


def halve_box_u16(img):
    """The next 16-bit level down: uint16 [h, w] or [h, w, 3] device image (rows may be pitched) -> [ceil(h / 2), ceil(w / 2)(, 3)],
    out[i, j, k] = (a[2i, 2j] + a[2i, j1] + a[i1, 2j] + a[i1, j1] + 2) >> 2 with i1 = min(2i + 1, h - 1), j1 = min(2j + 1, w - 1), in
    unsigned 32-bit arithmetic: GDAL's "average" overview."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint16 or img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
        what = f'{img.dtype} {tuple(img.shape)}' if isinstance(img, torch.Tensor) else type(img).__name__
        raise ValueError(f'halve_box_u16 expects a uint16 [H, W] or [H, W, 3] image, got {what}')
    png_hip._check_image(img, 'bgr')
    h, w = img.shape[0], img.shape[1]
    ch = 1 if img.dim() == 2 else 3
    ho, wo = (h + 1) // 2, (w + 1) // 2
    out = torch.empty((ho, wo) if ch == 1 else (ho, wo, 3), dtype=torch.uint16, device=img.device)
    _lib.call('ciaosr_halve_box_u16', hip_ops.ptr(img), C.c_size_t(png_hip._pitch(img)), h, w, ch, hip_ops.ptr(out),
              C.c_size_t(2 * ch * wo), hip_ops.stream_ptr(img.device))
    return out
