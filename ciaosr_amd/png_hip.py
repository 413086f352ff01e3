"""PNG files written from uint8 images on the MI355X (csrc/png_u8.hip), opt-in through `test_cfg.gpu_png`.

The device filters the scanlines (the usual minimum-sum-of-absolute-values rule, per row) and codes them band by band with dynamic
Huffman blocks of literals -- by default no LZ77 matches: on photographic content they gain nothing over filter + Huffman -- into one
zlib stream.  The host only wraps that stream: signature, IHDR, IDAT chunks, IEND, with `zlib.crc32` for the chunk CRCs.  The files
hold other bytes than Pillow's but decode to exactly the same pixels.  Two copies synchronise per image: the stream's size, then the
stream.  There is no CPU fallback: a host array raises.  `encode_png_tiles` codes many crops of one image (the tiles of a pyramid
level, pyramid.py) in one set of launches and two synchronising copies per call; each file is byte for byte the single call's on that
crop.

`matches=True` (every entry point; off by default, and then every byte is as before) lets a band use LZ77 matches from a fixed set of
distances -- 1, 2, 3, 4, 6, 8, 12, 16 and the scanline length L = 1 + C W with L - C and L + C, lengths of 8 to 258 inside chunks of
4096 bytes, greedy -- where that makes the band smaller: flat regions (a fill, a transparent surround) then cost a few bits per 258
bytes and not one bit per byte, and no file gets larger.

A uint8 [H, W, 4] image (`order` 'bgra', as `metrics_hip.tensor2img_bgra_u8` makes it, or 'rgba') goes through the four-byte-per-pixel
siblings of the same calls and becomes a colour type 6 file; every entry point here takes either kind.

A 2-D uint8 [H, W] image is a GREY image (`order` left at its default, or 'grey'; as `metrics_hip.tensor2img_grey_u8` makes it): the
one-byte-per-pixel siblings, rows of 1 + W bytes with the left predecessor one byte back, a colour type 0 file that Pillow opens as
mode L.  No alignment rule: a crop may start at any byte.

A `torch.uint16` image -- 2-D [H, W] (grey, as `metrics_hip.tensor2img_grey_u16` makes it) or [H, W, 3] (`order` 'bgr', as
`metrics_hip.tensor2img_u16` makes it, or 'rgb') -- becomes a file of BIT DEPTH 16, colour type 0 or 2, through the ciaosr_png16_*
siblings of the same calls: every sample big-endian in the stream, rows of 1 + 2 C W bytes, the five filters per byte with the left
predecessor 2 C bytes back, and from there on the same coder (bands, literals, `matches=True` with L - 2 C and L + 2 C, tiles).  The
files decode to the exact uint16 samples.  A crop may start at any pixel.  A uint16 [H, W, 4] image is refused: there is no 16-bit
alpha.  "Bytes per pixel" below means stream bytes: 1, 3, 4, or 2 and 6 at depth 16.
"""
import ctypes as C
import os
import struct
import zlib

import torch

from . import _lib, hip_ops
from ._lib import CiaoSRHipError

SIGNATURE = b'\x89PNG\r\n\x1a\n'
IDAT_MAX = (1 << 31) - 1                   # a chunk's length field is below 2^31
HIST_STRIDE = 260                          # CIAOSR_PNG_HIST_STRIDE
ADLER = 65521
MAX_SIDE = 65535
ORDERS = {'bgr': 1, 'rgb': 0}
ORDERS_RGBA = {'bgra': 1, 'rgba': 0}
COLOUR_TYPES = {3: 2, 4: 6}                # bytes per pixel -> IHDR colour type (`container(channels=)`; grey is its own keyword)
COLOUR_TYPE_GREY = 0
_ABI = {1: 'ciaosr_png_grey_', 3: 'ciaosr_png_', 4: 'ciaosr_png_rgba_', 2: 'ciaosr_png16_grey_', 6: 'ciaosr_png16_'}
DEPTHS = (8, 16)


def _abi(ch, name):
    """The export `name` ('filter_u8', 'lz_encode_tiles_u8', 'capacity_bytes', ...) for `ch` stream bytes per pixel; the calls that
    take an image end in the sample type."""
    if ch in (2, 6) and name.endswith('_u8'):
        name = name[:-3] + '_u16'
    return _ABI[ch] + name


def _check_matches(matches):
    if not isinstance(matches, bool):
        raise ValueError(f'matches must be True or False, got {matches!r}')
    return 'lz_' if matches else ''


def _pitch(img):
    """Bytes from one row to the next; a one-row image has no next row, and torch may report any stride for it."""
    return img.stride(0) * img.element_size() if img.shape[0] > 1 else img.shape[1] * channels_of(img)


def channels_of(img):
    """Bytes per pixel of an image tensor: its samples per pixel (1 for a 2-D, grey, one) times the bytes of a sample."""
    return (1 if img.dim() == 2 else img.shape[2]) * img.element_size()


def _check_image(img, order):
    """The image rules of this module: a uint8 [H, W, 3] or [H, W, 4] device tensor with packed pixels (rows may be pitched) and an
    `order` of its channel count -> (channels, the ABI's bgr flag).  A wrong order is a ValueError before the device is looked at."""
    if not isinstance(img, torch.Tensor):
        raise CiaoSRHipError(f'expected a uint8 HxWx3 or HxWx4 cuda tensor, got {type(img).__name__}')
    if img.dtype == torch.uint16:
        return _check_u16(img, order)
    if img.dtype == torch.uint8 and img.dim() == 2:
        return _check_grey(img, order)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] not in (3, 4):
        raise CiaoSRHipError(f'expected a uint8 HxWx3 or HxWx4 image, got {img.dtype} {tuple(img.shape)}')
    ch = img.shape[2]
    orders = ORDERS if ch == 3 else ORDERS_RGBA
    if order not in orders:
        raise ValueError(f"order of a {ch}-channel image must be {' or '.join(repr(o) for o in orders)}, got {order!r}")
    if not img.is_cuda:
        hip_ops.require_gpu(img)              # raises: no CPU fallback
    h, w = img.shape[0], img.shape[1]                  # (the stride of a dimension of size 1 means nothing: torch keeps any)
    if img.stride(2) != 1 or (w > 1 and img.stride(1) != ch) or (h > 1 and img.stride(0) < ch * w):
        raise CiaoSRHipError(f'expected HWC rows of {ch}*W contiguous bytes (a crop of a larger image is fine)')
    if ch == 4 and (_pitch(img) % 4 or img.data_ptr() % 4):
        raise CiaoSRHipError('a 4-channel image is read in 32-bit words: its first byte and its row pitch must be multiples of 4')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')
    return ch, orders[order]


def _check_grey(img, order):
    """`_check_image` for a 2-D image: `order` is the default or 'grey'; rows of W contiguous bytes, any pitch >= W, any alignment."""
    if order not in ('bgr', 'grey'):
        raise ValueError(f"order of a grey [H, W] image stays at its default or is 'grey', got {order!r}")
    if not img.is_cuda:
        hip_ops.require_gpu(img)              # raises: no CPU fallback
    h, w = img.shape
    if (w > 1 and img.stride(1) != 1) or (h > 1 and img.stride(0) < w):
        raise CiaoSRHipError('expected rows of W contiguous bytes (a crop of a larger image is fine)')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')
    return 1, 0


def _check_u16(img, order):
    """`_check_image` for a torch.uint16 image, [H, W] or [H, W, 3] -> (stream bytes per pixel 2 or 6, bgr flag).  Rows of C W
    contiguous samples, any pitch; a crop may start at any pixel (the device reads single 16-bit samples)."""
    if img.dim() == 3 and img.shape[2] == 4:
        raise CiaoSRHipError('a uint16 [H, W, 4] image cannot be coded: no 16-bit alpha (colour types 4 and 6 at depth 16 are not built)')
    if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
        raise CiaoSRHipError(f'expected a uint16 HxW or HxWx3 image, got {tuple(img.shape)}')
    ch = 1 if img.dim() == 2 else 3
    if ch == 1 and order not in ('bgr', 'grey'):
        raise ValueError(f"order of a grey [H, W] image stays at its default or is 'grey', got {order!r}")
    if ch == 3 and order not in ORDERS:
        raise ValueError(f"order of a 3-channel image must be {' or '.join(repr(o) for o in ORDERS)}, got {order!r}")
    if not img.is_cuda:
        hip_ops.require_gpu(img)              # raises: no CPU fallback
    h, w = img.shape[0], img.shape[1]
    if (ch == 3 and img.stride(2) != 1) or (w > 1 and img.stride(1) != ch) or (h > 1 and img.stride(0) < ch * w):
        raise CiaoSRHipError(f'expected rows of {ch}*W contiguous samples (a crop of a larger image is fine)')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')
    return 2 * ch, ORDERS[order] if ch == 3 else 0


def chunk(tag, data):
    """One PNG chunk: length, type, data, CRC-32 of type + data."""
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(data, zlib.crc32(tag)) & 0xffffffff)


def container(h, w, zstream, idat_max=IDAT_MAX, channels=3, grey=False, depth=8):
    """The PNG file of an h x w 8-bit RGB (`channels=4`: RGBA, colour type 6; `grey=True`: one byte per pixel, colour type 0, whatever
    `channels` is) image whose IDAT data is `zstream` (a zlib stream of the filtered scanlines), split into IDAT chunks of at most
    `idat_max` bytes.  `depth=16`: IHDR says bit depth 16 (RGB or grey; with `channels=4` a ValueError: no 16-bit alpha)."""
    if not (0 < idat_max <= IDAT_MAX):
        raise ValueError(f'idat_max={idat_max}')
    if not isinstance(grey, bool):
        raise ValueError(f'grey is True or False, got {grey!r}')
    if channels not in COLOUR_TYPES:
        raise ValueError(f'channels={channels!r}: 3 (RGB) or 4 (RGBA)')
    if isinstance(depth, bool) or depth not in DEPTHS:
        raise ValueError(f'depth={depth!r}: 8 or 16')
    if depth == 16 and channels == 4 and not grey:
        raise ValueError('depth=16 with channels=4: no 16-bit alpha (colour type 6 at depth 16 is not built)')
    colour_type = COLOUR_TYPE_GREY if grey else COLOUR_TYPES[channels]
    parts = [SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour_type, 0, 0, 0))]
    view = memoryview(zstream)
    for i in range(0, max(len(view), 1), idat_max):
        parts.append(chunk(b'IDAT', bytes(view[i:i + idat_max])))
    parts.append(chunk(b'IEND', b''))
    return b''.join(parts)


def adler32_combine(partials):
    """Adler-32 of a stream from its bands' (sum of bytes, weighted sum, length): what the device does with the filter's partials
    (`ciaosr_png_filter_u8`: both sums mod 65521, taken from a = b = 0)."""
    a, b, n = 0, 0, 0
    for s1, s2, length in partials:
        b = (b + s2 + length * a) % ADLER
        a = (a + s1) % ADLER
        n += length
    return (((n + b) % ADLER) << 16) | ((1 + a) % ADLER)


def zlib_stream(segments, partials):
    """The zlib stream of the composition, assembled on the host from the two stages' outputs: header, the bands' deflate segments
    (the last one carries BFINAL), Adler-32 combined from the bands' partial sums."""
    return b'\x78\x01' + b''.join(segments) + struct.pack('>I', adler32_combine(partials))


def _checked(img, order, rows_per_band, what='encode_png'):
    """The checks of every encoder -> (h, w, rows_per_band as an int, 0 = the default, channels, bgr flag)"""
    ch, bgr = _check_image(img, order)
    h, w = img.shape[0], img.shape[1]
    rows = int(rows_per_band)
    if rows < 0:
        raise ValueError(f'rows_per_band={rows_per_band}')
    if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise CiaoSRHipError(f'{what}: {h}x{w} is outside 1..{MAX_SIDE} per side')
    return h, w, rows, ch, bgr


def _geometry(img, order, rows_per_band):
    """-> (h, w, rows per band, bands, channels, bgr flag)"""
    h, w, rows, ch, bgr = _checked(img, order, rows_per_band)
    rows = getattr(_lib.load(), _abi(ch, 'rows_per_band'))(w, rows)
    return h, w, rows, -(-h // rows), ch, bgr


def filter_u8(img, order='bgr', rows_per_band=0):
    """Stage 1 alone: (scanline stream uint8 [H * (1 + C W)], histograms int32 [bands, 260], Adler partials int32 [bands, 2]) on the
    device, C = 3 or 4 channels, 1 for a 2-D (grey) image; no synchronisation.  A uint16 image gives the depth-16 stream (C = 6 or 2
    bytes per pixel, samples big-endian): the name says what the stream is made of, bytes."""
    h, w, rows, nb, ch, bgr = _geometry(img, order, rows_per_band)
    dev = img.device
    stream = torch.empty(h * (ch * w + 1), dtype=torch.uint8, device=dev)
    hist = torch.empty((nb, HIST_STRIDE), dtype=torch.int32, device=dev)
    adler = torch.empty((nb, 2), dtype=torch.int32, device=dev)
    _lib.call(_abi(ch, 'filter_u8'), hip_ops.ptr(img), C.c_size_t(_pitch(img)), h, w, bgr, rows, hip_ops.ptr(stream),
              hip_ops.ptr(hist), hip_ops.ptr(adler), hip_ops.stream_ptr(dev))
    return stream, hist, adler


def deflate_huff(data, band_offsets, matches=False, line=0, bpp=1):
    """Stage 2 alone: raw deflate of the device byte tensor `data`, one segment per band [band_offsets[i], band_offsets[i + 1]) ->
    list of `bytes`, whose concatenation is one deflate stream.  An empty band raises before anything is launched.  `matches=True`:
    the match coder, with the candidate distances `line - bpp`, `line`, `line + bpp` beside the near ones (`line=0`: without)."""
    _check_matches(matches)
    line, bpp = int(line), int(bpp)
    if matches and (line < 0 or bpp < 1 or 0 < line <= bpp):
        raise ValueError(f'line={line}, bpp={bpp}: line is 0 or above bpp >= 1')
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        raise CiaoSRHipError('deflate_huff expects a uint8 cuda tensor (no CPU fallback)')
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise CiaoSRHipError(f'deflate_huff expects a contiguous 1-d uint8 tensor, got {data.dtype} {tuple(data.shape)}')
    if data.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'data on cuda:{data.device.index} but the current device is cuda:{torch.cuda.current_device()}')
    offs = [int(v) for v in band_offsets]
    nb = len(offs) - 1
    if nb < 1 or offs[0] < 0 or offs[-1] > data.numel():
        raise ValueError(f'band offsets {offs[:4]}... do not lie inside the {data.numel()} bytes')
    dev = data.device
    lib = _lib.load()
    total = C.c_size_t(max(offs[-1] - offs[0], 0))
    cap = lib.ciaosr_deflate_huff_capacity_bytes(total, nb)
    nbytes = lib.ciaosr_deflate_lz_workspace_bytes(total, nb) if matches else lib.ciaosr_deflate_huff_workspace_bytes(nb)
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    seg = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    host_offs = (C.c_ulonglong * (nb + 1))(*offs)
    args = [hip_ops.ptr(data), host_offs, nb, hip_ops.ptr(out), C.c_size_t(cap), hip_ops.ptr(seg), hip_ops.ptr(ws), C.c_size_t(nbytes),
            hip_ops.stream_ptr(dev)]
    if matches:                                             # the same call with the scanline behind the bands
        args[3:3] = [line, bpp]
    _lib.call('ciaosr_deflate_lz_u8' if matches else 'ciaosr_deflate_huff_u8', *args)
    so = seg.cpu().tolist()
    raw = out[:so[-1]].cpu().numpy().tobytes()
    return [raw[so[i]:so[i + 1]] for i in range(nb)]


def encode_zlib(img, order='bgr', rows_per_band=0, matches=False):
    """The zlib stream of the image's filtered scanlines, made on the device -> bytes.  Synchronises twice: size, then stream."""
    lz = _check_matches(matches)
    h, w, rows, nb, ch, bgr = _geometry(img, order, rows_per_band)
    dev = img.device
    lib = _lib.load()
    cap = getattr(lib, _abi(ch, 'capacity_bytes'))(h, w, rows)
    nbytes = getattr(lib, _abi(ch, lz + 'workspace_bytes'))(h, w, rows)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_png: unsupported geometry {h}x{w}, rows_per_band={rows}')
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call(_abi(ch, lz + 'encode_u8'), hip_ops.ptr(img), C.c_size_t(_pitch(img)), h, w, bgr, rows, hip_ops.ptr(out),
              C.c_size_t(cap), hip_ops.ptr(total), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    n = int(total.item())                                   # copy 1: the size
    return out[:n].cpu().numpy().tobytes()                  # copy 2: the stream


def _wrap(img, h, w, z):
    """`container` for an h x w image (or crop) of `img`'s kind"""
    depth = 8 * img.element_size()
    return container(h, w, z, grey=True, depth=depth) if img.dim() == 2 else container(h, w, z, channels=img.shape[2], depth=depth)


def encode_png(img_u8_hwc, order='bgr', rows_per_band=0, matches=False):
    """PNG file (bytes) of a uint8 [H, W, 3] device image; `order`: 'bgr' as `tensor2img_u8` makes it, or 'rgb'.  Rows may be pitched
    (a crop view of a larger image).  `rows_per_band`: image rows per independently coded band, 0 = about 128 KiB of scanline bytes.
    A [H, W, 4] image with `order` 'bgra' (as `tensor2img_bgra_u8` makes it) or 'rgba' gives an RGBA file, a 2-D [H, W] image (as
    `tensor2img_grey_u8` makes it) a grey one that Pillow opens as mode L.  A torch.uint16 image, [H, W] or [H, W, 3], gives a file of
    bit depth 16 (the module's text).
    `matches=True`: bands may use LZ77 matches (see the module's text); the file is never larger and decodes to the same pixels."""
    z = encode_zlib(img_u8_hwc, order, rows_per_band, matches)
    return _wrap(img_u8_hwc, img_u8_hwc.shape[0], img_u8_hwc.shape[1], z)


def check_rects(rects, h, w):
    """[(y0, x0, h, w), ...] as ints; ValueError for an empty list, an empty rect or one that leaves the h x w image."""
    out = []
    for r in rects:
        r = tuple(r)
        if len(r) != 4 or any(int(v) != v for v in r):
            raise ValueError(f'a rect is (y0, x0, h, w) in whole pixels, got {r!r}')
        y0, x0, hh, ww = (int(v) for v in r)
        if hh < 1 or ww < 1 or y0 < 0 or x0 < 0 or y0 + hh > h or x0 + ww > w:
            raise ValueError(f'rect (y0, x0, h, w) = {(y0, x0, hh, ww)} is empty or outside the {h} x {w} image')
        out.append((y0, x0, hh, ww))
    if not out:
        raise ValueError('no rects')
    return out


def encode_tiles_device(img, rects, order='bgr', rows_per_band=0, matches=False):
    """ciaosr_png_encode_tiles_u8 on the current stream, no synchronisation -> (streams uint8 [capacity], offsets int64 [n + 1]) on the
    device: crop k's zlib stream is streams[offsets[k]:offsets[k + 1]], offsets[0] = 0, no gaps."""
    lz = _check_matches(matches)
    h, w, rows, ch, bgr = _checked(img, order, rows_per_band, 'encode_png_tiles')
    rects = check_rects(rects, h, w)
    n = len(rects)
    dev = img.device
    lib = _lib.load()
    host_rects = (C.c_int * (4 * n))(*[v for r in rects for v in r])
    cap = getattr(lib, _abi(ch, 'tiles_capacity_bytes'))(host_rects, n, rows)
    nbytes = getattr(lib, _abi(ch, lz + 'tiles_workspace_bytes'))(host_rects, n, rows)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_png_tiles: unsupported geometry ({n} rects, rows_per_band={rows})')
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.call(_abi(ch, lz + 'encode_tiles_u8'), hip_ops.ptr(img), C.c_size_t(_pitch(img)), h, w, bgr, host_rects, n, rows,
              hip_ops.ptr(out), C.c_size_t(cap), hip_ops.ptr(offs), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return out, offs


def encode_zlib_tiles(img, rects, order='bgr', rows_per_band=0, matches=False):
    """The zlib streams of many crops (y0, x0, h, w) of one device image, from ONE set of launches -> list of bytes; stream k is byte
    for byte `encode_zlib(img[y0:y0 + h, x0:x0 + w], ...)`.  Synchronises twice per call, whatever the number of crops: the offsets
    table, then the streams."""
    out, offs = encode_tiles_device(img, rects, order, rows_per_band, matches)
    o = offs.cpu().tolist()                                 # copy 1: the offsets
    raw = memoryview(out[:o[-1]].cpu().numpy())             # copy 2: the streams
    return [bytes(raw[o[k]:o[k + 1]]) for k in range(len(o) - 1)]


def encode_png_tiles(img_u8_hwc, rects, order='bgr', rows_per_band=0, matches=False):
    """PNG files (list of bytes) of the crops `rects` = [(y0, x0, h, w), ...] of a uint8 [H, W, 3] (or [H, W, 4]) device image, coded
    together: file k is byte for byte `encode_png(img[y0:y0 + h, x0:x0 + w], order, rows_per_band, matches)`.  The rects may overlap.  A bad rect is a
    ValueError before any device work; two synchronising copies per call."""
    _check_matches(matches)
    rects = list(rects)
    zs = encode_zlib_tiles(img_u8_hwc, rects, order, rows_per_band, matches)
    return [_wrap(img_u8_hwc, int(r[2]), int(r[3]), z) for r, z in zip(rects, zs)]


def imwrite_gpu(img_u8_hwc, path, order='bgr', matches=False):
    """`imageio.imwrite` for an image that is already on the device: encode there, write the file here.  uint8 or uint16 (depth 16)."""
    data = encode_png(img_u8_hwc, order, matches=matches)
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
