"""Baseline JPEG files written from uint8 images on the MI355X (csrc/jpeg_u8.hip), byte for byte Pillow's.

The device runs libjpeg's integer pipeline as `PIL.Image.save(format='JPEG', quality=q, subsampling=0 | 2)` drives it -- colour
conversion, 4:2:0 box filter, "islow" DCT, quantisation, the Annex K Huffman codes, 0xFF stuffing, padding -- and returns the
entropy-coded scan.  The host only wraps it: `header(h, w, quality, subsampling)` in front (SOI, APP0, two DQT, SOF0, four DHT, the
SOS header; it depends on nothing else), EOI behind.  DESIGN 4.1i-d holds the contract.  Two copies synchronise per call: the sizes,
then the bytes.  There is no CPU fallback: a host array raises.  `encode_jpeg_tiles` codes many crops of one image (the tiles of a
pyramid level, pyramid.py) in one set of launches; each file is byte for byte the single call's on that crop.

`optimize=True` writes Pillow's `optimize=True` files instead (libjpeg's optimize_coding): the same coefficients and symbols, coded with
four Huffman tables derived per file from the histograms of its own symbols.  The device counts the symbols, makes the tables by
libjpeg's rule and codes with them; the tables come back as DHT records in the buffer that holds the sizes, so a call still
synchronises twice, and `header(..., tables=)` writes them into the file's four DHT segments.

`progressive=True` writes Pillow's `progressive=True` files (csrc/jpeg_prog_u8.hip): the same coefficients in the ten
scans of libjpeg's progressive script, every scan with a table made from its own symbols -- Pillow writes the same bytes with and
without `optimize=True`, so `optimize` does not matter then.  The device returns the ten scans of every crop and their ten tables in
the same two copies; `assemble_progressive` writes the SOF2 header and the DHT and SOS headers between them.

A 2-D uint8 [H, W] image is a GREY image: the file is byte for byte `Image.fromarray(grey, 'L').save(format='JPEG', quality=q[,
optimize=True])` -- one component, one DQT, two DHT (`header(..., grey=True)`); the device codes one block per MCU with the luma tables
(CIAOSR_JPEG_GREY).  `subsampling` stays '444' (Pillow's '420' file of a grey image has other bytes) and there is no progressive form.

The three kinds share one path: `kind_of` checks the two flags once per entry point and names the kind (the ABI's prefix, the streams
and the DHT records per crop in a result); `_scans_device`, `_scans` and `_scan` do the device work for any kind, `_split` parses any
result, `_dht` writes and validates every DHT segment and `_file` assembles the file.  Only the return shapes differ by flag.
"""
import collections
import ctypes as C
import os
import struct

import torch

from . import _lib, hip_ops
from ._lib import CiaoSRHipError
from .metrics_hip import _check_image
from .png_hip import MAX_SIDE, ORDERS, _check_grey, _pitch, check_rects

SUBSAMPLINGS = {'444': 0, '420': 2}        # CIAOSR_JPEG_444 / CIAOSR_JPEG_420: Pillow's `subsampling=` numbers
GREY = 4                                    # CIAOSR_JPEG_GREY: one component, what a 2-D image is coded as
EOI = b'\xff\xd9'

# Annex K base quantisation tables, natural (row-major) order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
             103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36
# natural index of the k-th coefficient in zigzag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K "typical" Huffman tables as a DHT segment holds them, in the file's order: (class << 4 | id, code counts per length 1..16,
# symbols in code order)
HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
      0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
      0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
      0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
      0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
      0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
      0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
      0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
      0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
      0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
      0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
      0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
      0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
      0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
)


def check_params(quality, subsampling):
    """(quality as int, the ABI's subsampling code); ValueError otherwise."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f'quality is a whole number in 1..100, got {quality!r}')
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be '444' or '420', got {subsampling!r}")
    return int(quality), SUBSAMPLINGS[subsampling]


FREQUENCY_LIMIT = 1_000_000_000            # optimised coding: a crop is refused when 64 x (blocks of its scan) reaches this
DHT_RECORD_BYTES = 272                     # CIAOSR_JPEG_DHT_RECORD_BYTES: 16 counts, 256 symbols padded with zeros
TABLE_IDS = tuple(t[0] for t in HUFFMAN)   # class << 4 | id of the four DHT segments, in the file's order


def check_optimize(optimize):
    """`optimize` is a bool; ValueError otherwise (before any device work)."""
    if not isinstance(optimize, bool):
        raise ValueError(f'optimize is True or False, got {optimize!r}')
    return optimize


# progressive files: the ten scans (component: None = Y, Cb, Cr interleaved, else 0 Y / 1 Cb / 2 Cr; Ss, Se, Ah, Al), Cr before Cb ...
SCAN_SCRIPT = ((None, 0, 0, 0, 1), (0, 1, 5, 0, 2), (2, 1, 63, 0, 1), (1, 1, 63, 0, 1), (0, 6, 63, 0, 2), (0, 1, 63, 2, 1),
               (None, 0, 0, 1, 0), (2, 1, 63, 1, 0), (1, 1, 63, 1, 0), (0, 1, 63, 1, 0))
# ... and class << 4 | id of the ten DHT segments in the file's order: two in front of scan 1, one in front of every AC scan
PROGRESSIVE_TABLE_IDS = (0x00, 0x01, 0x10, 0x11, 0x11, 0x10, 0x10, 0x11, 0x11, 0x10)


def check_progressive(progressive):
    """`progressive` is a bool; ValueError otherwise (before any device work)."""
    if not isinstance(progressive, bool):
        raise ValueError(f'progressive is True or False, got {progressive!r}')
    return progressive


def scan_block_count(h, w, subsampling, grey=False):
    """Blocks of the scan of an h x w image: all components, the dummy blocks of 4:2:0 included; `grey`: the one component's."""
    if grey:
        return -(-h // 8) * -(-w // 8)
    if subsampling == '420':
        return 6 * -(-h // 16) * -(-w // 16)
    return 3 * -(-h // 8) * -(-w // 8)


def check_frequency_limit(h, w, subsampling, grey=False):
    """Optimised coding counts symbols in 32 bits and follows libjpeg only below its sentinel frequency: a crop whose scan could hold
    FREQUENCY_LIMIT symbols (64 per block) is a ValueError."""
    blocks = scan_block_count(h, w, subsampling, grey)
    if 64 * blocks >= FREQUENCY_LIMIT:
        raise ValueError(f'optimize=True: {h} x {w} in {"grey" if grey else subsampling} has {blocks} blocks; 64 x blocks must stay below {FREQUENCY_LIMIT}')
    return blocks


def quant_tables(quality):
    """(luma, chroma): 64 values each, natural order -- libjpeg's quality scaling of the Annex K tables."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (BASE_LUMA, BASE_CHROMA))


def _frame(h, w, quality, subsampling, sof, grey=False):
    """SOI, APP0, the two DQT segments and the frame header under the marker `sof`; `grey`: the luma DQT and the one-component frame."""
    parts = [b'\xff\xd8', b'\xff\xe0', struct.pack('>H5sBBBHHBB', 16, b'JFIF\0', 1, 1, 0, 1, 1, 0, 0)]
    for k, q in enumerate(quant_tables(quality)[:1 if grey else 2]):
        parts += [b'\xff\xdb', struct.pack('>HB', 67, k), bytes(q[i] for i in ZIGZAG)]
    if grey:
        return b''.join(parts + [sof, struct.pack('>HBHHB', 11, 8, h, w, 1), bytes((1, 0x11, 0))])
    parts += [sof, struct.pack('>HBHHB', 17, 8, h, w, 3), bytes((1, 0x22 if subsampling == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1))]
    return b''.join(parts)


def progressive_header(h, w, quality, subsampling):
    """A progressive file up to its first scan's DHT segments: SOI, APP0, two DQT, SOF2 (SOF0's payload)."""
    quality, _ = check_params(quality, subsampling)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f'{h} x {w} is outside 1..{MAX_SIDE} per side')
    return _frame(h, w, quality, subsampling, b'\xff\xc2')


def _dht(tc_th, table):
    """The DHT segment of one (counts, symbols) pair under class << 4 | id; ValueError unless it is 16 counts and sum(counts) symbols."""
    counts, vals = table
    if len(counts) != 16 or len(vals) != sum(counts) or not 1 <= len(vals) <= 256:
        raise ValueError('tables: (16 counts, sum(counts) symbols) pairs')
    return b'\xff\xc4' + struct.pack('>HB', 19 + len(vals), tc_th) + bytes(counts) + bytes(vals)


ANNEX_K_DHT = tuple(_dht(t[0], t[1:]) for t in HUFFMAN)     # the four DHT segments of a file without tables of its own

def scan_header(s, tables):
    """What a progressive file holds in front of the entropy-coded data of scan s = 0..9: the DHT segments of the tables the scan is
    coded with (`tables`: the file's ten (counts, symbols) pairs in the order of PROGRESSIVE_TABLE_IDS), then the SOS header."""
    comp, ss, se, ah, al = SCAN_SCRIPT[s]
    if comp is None:
        slots = (0, 1) if ah == 0 else ()
        selectors = (1, 0x00, 2, 0x10, 3, 0x10) if ah == 0 else (1, 0x00, 2, 0x00, 3, 0x00)
    else:
        slots = (s + 1 if s < 6 else s,)                    # scan 7 (s = 6) has no table
        selectors = (comp + 1, 0 if comp == 0 else 1)
    parts = [_dht(PROGRESSIVE_TABLE_IDS[k], tables[k]) for k in slots]
    n = len(selectors) // 2
    parts += [b'\xff\xda', struct.pack('>HB', 6 + 2 * n, n), bytes(selectors), bytes((ss, se, (ah << 4) | al))]
    return b''.join(parts)


def assemble_progressive(h, w, quality, subsampling, scans, tables):
    """The progressive file of an h x w image from its ten entropy-coded scans and its ten tables."""
    if len(scans) != len(SCAN_SCRIPT) or len(tables) != len(PROGRESSIVE_TABLE_IDS):
        raise ValueError('a progressive file has ten scans and ten tables')
    parts = [progressive_header(h, w, quality, subsampling)]
    for s, data in enumerate(scans):
        parts += [scan_header(s, tables), data]
    return b''.join(parts) + EOI


def header(h, w, quality, subsampling='444', tables=None, grey=False):
    """The file from SOI up to and including the SOS header, as Pillow writes it for an h x w RGB image.  `tables`: four (counts,
    symbols) pairs in the file's order (DC luma, AC luma, DC chroma, AC chroma) for the DHT segments of an optimised file -- 16 counts
    per code length 1..16 and exactly sum(counts) symbols each; None: the Annex K tables.
    `grey=True`: as Pillow writes it for a mode-L image -- one DQT, SOF0 with the component (1, 0x11, 0), the two luma DHT segments
    (of `tables`, an optimised call's four pairs or the first two, only the first two are read) and the one-component SOS."""
    quality, _ = check_params(quality, subsampling)
    if not isinstance(grey, bool):
        raise ValueError(f'grey is True or False, got {grey!r}')
    if grey and subsampling != '444':
        raise ValueError(f"a grey file has no subsampling: leave it at '444', got {subsampling!r}")
    dht = ANNEX_K_DHT[:2 if grey else 4]
    if tables is not None:
        tables = [(tuple(int(c) for c in counts), tuple(int(v) for v in symbols)) for counts, symbols in tables]
        if len(tables) not in ((2, 4) if grey else (4,)):
            raise ValueError(f'tables: {"two or " if grey else ""}four (16 counts, sum(counts) symbols) pairs')
        dht = [_dht(tc_th, t) for tc_th, t in zip(TABLE_IDS[:len(dht)], tables)]
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f'{h} x {w} is outside 1..{MAX_SIDE} per side')
    parts = [_frame(h, w, quality, subsampling, b'\xff\xc0', grey), *dht]
    if grey:
        parts += [b'\xff\xda', struct.pack('>HB', 8, 1), bytes((1, 0x00, 0, 0x3f, 0))]
    else:
        parts += [b'\xff\xda', struct.pack('>HB', 12, 3), bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3f, 0))]
    return b''.join(parts)


def is_grey(img):
    """A 2-D uint8 tensor: a grey image, coded as a one-component file."""
    return isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.dim() == 2


# A kind of file: the ABI's prefix of its entry points, the streams per crop in a call's result and the DHT records per crop behind them
Kind = collections.namedtuple('Kind', 'prefix streams tables')
BASELINE, OPTIMISED, PROGRESSIVE = Kind('', 1, 0), Kind('opt_', 1, len(TABLE_IDS)), Kind('prog_', len(SCAN_SCRIPT), len(PROGRESSIVE_TABLE_IDS))


def kind_of(img, optimize, progressive):
    """The Kind that the two flags select for `img`; ValueError (before any device work) unless both are bools, and for a grey image
    with progressive=True: there is no one-component progressive file.  `progressive` wins over `optimize`."""
    check_optimize(optimize)
    if check_progressive(progressive) and is_grey(img):
        raise ValueError('progressive=True: a grey [H, W] image has no progressive form here')
    return PROGRESSIVE if progressive else (OPTIMISED if optimize else BASELINE)


def _check(img, quality, subsampling, order, mcus_per_chunk, what):
    """The argument checks of every entry point, before any device work -> (h, w, quality, subsampling code, mcus_per_chunk)."""
    quality, sub = check_params(quality, subsampling)
    grey = is_grey(img)
    if grey:
        if subsampling != '444':
            raise ValueError(f"a grey [H, W] image has no subsampling (Pillow's {subsampling!r} file of it holds other bytes): leave it at '444'")
        if order not in ('bgr', 'grey'):
            raise ValueError(f"order of a grey [H, W] image stays at its default or is 'grey', got {order!r}")
        sub = GREY
    elif order not in ORDERS:
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    if int(mcus_per_chunk) != mcus_per_chunk or mcus_per_chunk < 0:
        raise ValueError(f'mcus_per_chunk={mcus_per_chunk!r}')
    if grey:
        _check_grey(img, order)
    else:
        _check_image(img)
    h, w = img.shape[0], img.shape[1]
    if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise CiaoSRHipError(f'{what}: {h}x{w} is outside 1..{MAX_SIDE} per side')
    return h, w, quality, sub, int(mcus_per_chunk)


def _split(result, n, streams, tables):
    """The host copy (a tensor or a sequence of int64) of a call's result on n crops -> (offsets [streams n + 1], tables): tables[k] holds
    crop k's `tables` (counts, symbols) pairs, read from the DHT records behind the offsets (None where the kind has no tables)."""
    raw = bytes(memoryview(result.numpy()).cast('B')) if isinstance(result, torch.Tensor) else bytes(result)
    at = 8 * (streams * n + 1)
    offsets = list(struct.unpack(f'<{streams * n + 1}q', raw[:at]))
    if not tables:
        return offsets, [None] * n
    records = [raw[at + DHT_RECORD_BYTES * k:at + DHT_RECORD_BYTES * (k + 1)] for k in range(tables * n)]
    pairs = [(tuple(rec[:16]), tuple(rec[16:16 + sum(rec[:16])])) for rec in records]
    return offsets, [pairs[tables * k:tables * (k + 1)] for k in range(n)]


def split_result(result, n):
    """The host copy (a sequence of int64) of an optimised call's result -> (offsets [n + 1], tables): tables[k] holds crop k's four
    (counts, symbols) pairs as `header(..., tables=)` takes them."""
    return _split(result, n, OPTIMISED.streams, OPTIMISED.tables)


def split_progressive_result(result, n):
    """The host copy of a progressive call's result -> (offsets [10 n + 1], tables): scan s of crop k lies at offsets[10 k + s] ..
    offsets[10 k + s + 1], tables[k] holds crop k's ten (counts, symbols) pairs in the order of PROGRESSIVE_TABLE_IDS."""
    return _split(result, n, PROGRESSIVE.streams, PROGRESSIVE.tables)


def _scans_device(kind, img, rects, quality, subsampling, order, mcus_per_chunk, out=None, capacity=None):
    """`encode_scans_device` of a kind: every check, then ciaosr_jpeg_<prefix>encode_tiles_u8 on the current stream."""
    h, w, quality, sub, mcus = _check(img, quality, subsampling, order, mcus_per_chunk, 'encode_jpeg_tiles')
    rects = check_rects(rects, h, w)
    n = len(rects)
    if kind.tables:
        for r in rects:
            check_frequency_limit(r[2], r[3], subsampling, sub == GREY)
    dev = img.device
    lib = _lib.load()
    host_rects = (C.c_int * (4 * n))(*[v for r in rects for v in r])
    cap = getattr(lib, f'ciaosr_jpeg_{kind.prefix}tiles_capacity_bytes')(host_rects, n, sub)
    nbytes = getattr(lib, f'ciaosr_jpeg_{kind.prefix}tiles_workspace_bytes')(host_rects, n, sub, mcus)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_jpeg_tiles: unsupported geometry ({n} rects, mcus_per_chunk={mcus})')
    ws = hip_ops.workspace(nbytes, dev, slot='jpeg')
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
    words = getattr(lib, f'ciaosr_jpeg_{kind.prefix}result_bytes')(n) // 8 if kind.tables else n + 1
    offs = torch.empty(words, dtype=torch.int64, device=dev)
    _lib.call(f'ciaosr_jpeg_{kind.prefix}encode_tiles_u8', hip_ops.ptr(img), C.c_size_t(_pitch(img)), h, w, ORDERS.get(order, 0), host_rects, n,
              quality, sub, mcus, hip_ops.ptr(out), C.c_size_t(cap if capacity is None else capacity), hip_ops.ptr(offs), hip_ops.ptr(ws),
              C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return out, offs


def encode_scans_device(img, rects, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, out=None, capacity=None, optimize=False,
                        progressive=False):
    """ciaosr_jpeg_encode_tiles_u8 on the current stream, no synchronisation -> (scans uint8 [capacity], offsets int64 [n + 1]) on the
    device: crop k's entropy-coded scan is scans[offsets[k]:offsets[k + 1]], offsets[0] = 0, no gaps.  `out`, `capacity`: a buffer of
    the caller's and the size to declare for it (default: `ciaosr_jpeg_tiles_capacity_bytes`, the worst case).
    `optimize=True`: ciaosr_jpeg_opt_encode_tiles_u8 -> (scans, result int64 [n + 1 + 136 n]): the offsets, then the crops' DHT records
    (`split_result` takes the host copy apart); the default capacity is `ciaosr_jpeg_opt_tiles_capacity_bytes`.
    `progressive=True` (whatever `optimize` is): ciaosr_jpeg_prog_encode_tiles_u8 -> (scans, result int64 [10 n + 1 + 340 n]): the
    offsets of the crops' ten scans each, then their ten DHT records each (`split_progressive_result`)."""
    return _scans_device(kind_of(img, optimize, progressive), img, rects, quality, subsampling, order, mcus_per_chunk, out, capacity)


def _scans(kind, img, rects, quality, subsampling, order, mcus_per_chunk):
    """(scans, tables) of the crops, one entry per crop: its scan (progressive: the list of its ten), its tables (baseline: None).
    Synchronises twice: the offsets and the tables, then the bytes."""
    out, offs = _scans_device(kind, img, rects, quality, subsampling, order, mcus_per_chunk)
    o, tables = _split(offs.cpu(), len(rects), kind.streams, kind.tables)     # copy 1: the offsets and the tables
    raw = memoryview(out[:o[-1]].cpu().numpy())                               # copy 2: the scans
    scans = [bytes(raw[o[k]:o[k + 1]]) for k in range(len(o) - 1)]
    if kind.streams > 1:
        scans = [scans[kind.streams * k:kind.streams * (k + 1)] for k in range(len(rects))]
    return scans, tables


def encode_scans(img, rects, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, optimize=False, progressive=False):
    """The entropy-coded scans of many crops (y0, x0, h, w) of one device image, from ONE set of launches -> list of bytes; scan k is
    byte for byte `encode_scan(img[y0:y0 + h, x0:x0 + w], ...)`.  Synchronises twice per call: the offsets table, then the bytes.
    `optimize=True` -> (scans, tables): tables[k] holds the four (counts, symbols) pairs that scan k is coded with; the first copy
    brings the offsets and the tables.  `progressive=True` -> (scans, tables): scans[k] holds crop k's TEN scans, tables[k] its ten
    tables, as `assemble_progressive` takes them."""
    kind = kind_of(img, optimize, progressive)
    scans, tables = _scans(kind, img, list(rects), quality, subsampling, order, mcus_per_chunk)
    return (scans, tables) if kind.tables else scans


def _scan(kind, img, quality, subsampling, order, mcus_per_chunk):
    """(scan, tables) of the whole image, as `_scans` gives them for one crop.  The kinds with tables go through the tiles entry, whose
    result brings them; the baseline scan through ciaosr_jpeg_encode_u8: size, then bytes."""
    h, w, quality_, sub, mcus = _check(img, quality, subsampling, order, mcus_per_chunk, 'encode_jpeg')
    if kind.tables:
        scans, tables = _scans(kind, img, [(0, 0, h, w)], quality, subsampling, order, mcus_per_chunk)
        return scans[0], tables[0]
    dev = img.device
    lib = _lib.load()
    cap = lib.ciaosr_jpeg_capacity_bytes(h, w, sub)
    nbytes = lib.ciaosr_jpeg_workspace_bytes(h, w, sub, mcus)
    if cap == 0 or nbytes == 0:
        raise CiaoSRHipError(f'encode_jpeg: unsupported geometry {h}x{w}, mcus_per_chunk={mcus}')
    ws = hip_ops.workspace(nbytes, dev, slot='jpeg')
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call('ciaosr_jpeg_encode_u8', hip_ops.ptr(img), C.c_size_t(_pitch(img)), h, w, ORDERS.get(order, 0), quality_, sub, mcus,
              hip_ops.ptr(out), C.c_size_t(cap), hip_ops.ptr(total), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    n = int(total.item())                                   # copy 1: the size
    return out[:n].cpu().numpy().tobytes(), None            # copy 2: the scan


def encode_scan(img, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, optimize=False, progressive=False):
    """The entropy-coded scan of the image, stuffed and padded (the file between the SOS header and EOI), made on the device -> bytes.
    Synchronises twice: size, then bytes.  `optimize=True` -> (scan, its four (counts, symbols) tables); size and tables, then bytes.
    `progressive=True` -> (the file's ten scans, its ten tables)."""
    kind = kind_of(img, optimize, progressive)
    scan, tables = _scan(kind, img, quality, subsampling, order, mcus_per_chunk)
    return (scan, tables) if kind.tables else scan


def _file(kind, h, w, quality, subsampling, scan, tables, grey):
    """The file of an h x w image from what `_scan` or `_scans` returned for it."""
    if kind.streams > 1:
        return assemble_progressive(h, w, quality, subsampling, scan, tables)
    return header(h, w, quality, subsampling, tables, grey) + scan + EOI


def encode_jpeg(img_u8_hwc, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, optimize=False, progressive=False):
    """JPEG file (bytes) of a uint8 [H, W, 3] device image, byte for byte `PIL.Image.save(format='JPEG', quality=quality,
    subsampling=0 or 2)` of the same pixels (a 2-D [H, W] image: of the mode-L image, see the module's text); `order`: 'bgr' as
    `tensor2img_u8` makes it, or 'rgb'.  Rows may be pitched (a crop view of a larger image).  `mcus_per_chunk`: MCUs per workgroup,
    0 = the library's choice; the bytes do not depend on it.
    `optimize=True`: byte for byte `PIL.Image.save(..., optimize=True)`: Huffman tables made for this file on the device.
    `progressive=True`: byte for byte `PIL.Image.save(..., progressive=True)`, whatever `optimize` is."""
    kind = kind_of(img_u8_hwc, optimize, progressive)
    scan, tables = _scan(kind, img_u8_hwc, quality, subsampling, order, mcus_per_chunk)
    return _file(kind, img_u8_hwc.shape[0], img_u8_hwc.shape[1], quality, subsampling, scan, tables, is_grey(img_u8_hwc))


def encode_jpeg_tiles(img_u8_hwc, rects, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, optimize=False, progressive=False):
    """JPEG files (list of bytes) of the crops `rects` = [(y0, x0, h, w), ...] of a uint8 [H, W, 3] device image, coded together: file k
    is byte for byte `encode_jpeg(img[y0:y0 + h, x0:x0 + w], ...)`.  The rects may overlap.  A bad rect, quality or subsampling is a
    ValueError before any device work; two synchronising copies per call.  `optimize=True`: every file with its own Huffman tables,
    byte for byte Pillow's `optimize=True` file of the crop; still ten launches and two copies whatever the number of crops.
    `progressive=True`: every file Pillow's `progressive=True` file of the crop; thirteen launches and two copies."""
    rects = list(rects)
    kind = kind_of(img_u8_hwc, optimize, progressive)
    scans, tables = _scans(kind, img_u8_hwc, rects, quality, subsampling, order, mcus_per_chunk)
    grey = is_grey(img_u8_hwc)
    return [_file(kind, int(r[2]), int(r[3]), quality, subsampling, s, t, grey) for r, s, t in zip(rects, scans, tables)]


def imwrite_gpu_jpeg(img_u8_hwc, path, quality=90, subsampling='444', order='bgr', optimize=False, progressive=False):
    """`imageio.imwrite` as JPEG for an image that is already on the device: encode there, write the file here."""
    data = encode_jpeg(img_u8_hwc, quality, subsampling, order, optimize=optimize, progressive=progressive)
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
