"""PNG files written from uint8 images on the MI355X (csrc/png_u8.hip), opt-in through `test_cfg.gpu_png`.

The device filters the scanlines (the usual minimum-sum-of-absolute-values rule, per row) and codes them band by band with dynamic
Huffman blocks of literals -- no LZ77 matches: on this content they gain nothing over filter + Huffman -- into one zlib stream.  The
host only wraps that stream: signature, IHDR, IDAT chunks, IEND, with `zlib.crc32` for the chunk CRCs.  The files hold other bytes
than Pillow's but decode to exactly the same pixels.  Two copies synchronise per image: the stream's size, then the stream.  There is
no CPU fallback: a host array raises.
"""
import ctypes as C
import os
import struct
import zlib

import torch

from . import _lib, hip_ops
from ._lib import CiaoSRHipError
from .metrics_hip import _check_image

SIGNATURE = b'\x89PNG\r\n\x1a\n'
IDAT_MAX = (1 << 31) - 1                   # a chunk's length field is below 2^31
HIST_STRIDE = 260                          # CIAOSR_PNG_HIST_STRIDE
ADLER = 65521
MAX_SIDE = 65535
ORDERS = {'bgr': 1, 'rgb': 0}


def chunk(tag, data):
    """One PNG chunk: length, type, data, CRC-32 of type + data."""
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(data, zlib.crc32(tag)) & 0xffffffff)


def container(h, w, zstream, idat_max=IDAT_MAX):
    """The PNG file of an h x w 8-bit RGB image whose IDAT data is `zstream` (a zlib stream of the filtered scanlines), split into
    IDAT chunks of at most `idat_max` bytes."""
    if not (0 < idat_max <= IDAT_MAX):
        raise ValueError(f'idat_max={idat_max}')
    parts = [SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))]
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


def _geometry(img, order, rows_per_band):
    _check_image(img)
    if order not in ORDERS:
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    h, w = img.shape[0], img.shape[1]
    rows = int(rows_per_band)
    if rows < 0:
        raise ValueError(f'rows_per_band={rows_per_band}')
    if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise CiaoSRHipError(f'encode_png: {h}x{w} is outside 1..{MAX_SIDE} per side')
    rows = _lib.load().ciaosr_png_rows_per_band(w, rows)
    return h, w, rows, -(-h // rows)


def filter_u8(img, order='bgr', rows_per_band=0):
    """Stage 1 alone: (scanline stream uint8 [H * (1 + 3 W)], histograms int32 [bands, 260], Adler partials int32 [bands, 2]) on the
    device; no synchronisation."""
    h, w, rows, nb = _geometry(img, order, rows_per_band)
    dev = img.device
    stream = torch.empty(h * (3 * w + 1), dtype=torch.uint8, device=dev)
    hist = torch.empty((nb, HIST_STRIDE), dtype=torch.int32, device=dev)
    adler = torch.empty((nb, 2), dtype=torch.int32, device=dev)
    _lib.call('ciaosr_png_filter_u8', hip_ops.ptr(img), C.c_size_t(img.stride(0)), h, w, ORDERS[order], rows, hip_ops.ptr(stream),
              hip_ops.ptr(hist), hip_ops.ptr(adler), hip_ops.stream_ptr(dev))
    return stream, hist, adler


def deflate_huff(data, band_offsets):
    """Stage 2 alone: raw deflate of the device byte tensor `data`, one segment per band [band_offsets[i], band_offsets[i + 1]) ->
    list of `bytes`, whose concatenation is one deflate stream.  An empty band raises before anything is launched."""
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
    cap = lib.ciaosr_deflate_huff_capacity_bytes(C.c_size_t(max(offs[-1] - offs[0], 0)), nb)
    nbytes = lib.ciaosr_deflate_huff_workspace_bytes(nb)
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    seg = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    host_offs = (C.c_ulonglong * (nb + 1))(*offs)
    _lib.call('ciaosr_deflate_huff_u8', hip_ops.ptr(data), host_offs, nb, hip_ops.ptr(out), C.c_size_t(cap), hip_ops.ptr(seg),
              hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    so = seg.cpu().tolist()
    raw = out[:so[-1]].cpu().numpy().tobytes()
    return [raw[so[i]:so[i + 1]] for i in range(nb)]


def encode_zlib(img, order='bgr', rows_per_band=0):
    """The zlib stream of the image's filtered scanlines, made on the device -> bytes.  Synchronises twice: size, then stream."""
    h, w, rows, nb = _geometry(img, order, rows_per_band)
    dev = img.device
    lib = _lib.load()
    cap = lib.ciaosr_png_capacity_bytes(h, w, rows)
    nbytes = lib.ciaosr_png_workspace_bytes(h, w, rows)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_png: unsupported geometry {h}x{w}, rows_per_band={rows}')
    ws = hip_ops.workspace(nbytes, dev, slot='png')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call('ciaosr_png_encode_u8', hip_ops.ptr(img), C.c_size_t(img.stride(0)), h, w, ORDERS[order], rows, hip_ops.ptr(out),
              C.c_size_t(cap), hip_ops.ptr(total), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    n = int(total.item())                                   # copy 1: the size
    return out[:n].cpu().numpy().tobytes()                  # copy 2: the stream


def encode_png(img_u8_hwc, order='bgr', rows_per_band=0):
    """PNG file (bytes) of a uint8 [H, W, 3] device image; `order`: 'bgr' as `tensor2img_u8` makes it, or 'rgb'.  Rows may be pitched
    (a crop view of a larger image).  `rows_per_band`: image rows per independently coded band, 0 = about 128 KiB of scanline bytes."""
    z = encode_zlib(img_u8_hwc, order, rows_per_band)
    return container(img_u8_hwc.shape[0], img_u8_hwc.shape[1], z)


def imwrite_gpu(img_u8_hwc, path, order='bgr'):
    """`imageio.imwrite` for an image that is already on the device: encode there, write the file here."""
    data = encode_png(img_u8_hwc, order)
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
