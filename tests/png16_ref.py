"""PNG of bit depth 16 in plain numpy, written from the PNG specification (sections 7.2 "scanlines", 9 "filtering") and the contract of
DESIGN 4.1i-b6, not from the kernel: the judge of tests/test_depth16_host.py and tests/test_depth16_gpu.py.

A sample is two bytes in the stream, most significant first; a pixel is C = 1 (colour type 0) or 3 (colour type 2, R G B) samples, so a
scanline is 1 + 2 C W bytes.  The filters work on BYTES: the left predecessor of a byte is the byte bpp = 2 C before it, the upper one
the same byte of the row above; both are 0 outside the image.  Nothing is carried between the two bytes of a sample.  The row rule is
this project's: the filter with the smallest sum of min(b, 256 - b) over the row's filtered bytes, ties to the lowest number.
For the match coder the tests use tests/png_match_ref.py (`parse(band, line, bpp)`, `inflate_tokens`) with these rows."""
import struct
import zlib

import numpy as np

from tests.png_match_ref import inflate_tokens, parse        # noqa: F401  (re-exported: the match contract on these rows)

ADLER = 65521
SIGNATURE = b'\x89PNG\r\n\x1a\n'


# -- the quantiser and the grey value, restated ------------------------------------------------------------------------------------------
def q16(t):
    """rint(fp32(clamp(v, 0, 1) * 65535)) of a torch fp32 tensor, as int32 on the tensor's device: one fp32 multiply, round half even."""
    import torch
    return (t.float().clamp(0, 1) * 65535).round().to(torch.int32)


def image_of(t):
    """uint16 numpy [H, W, 3] in B G R order of a [3, H, W] / [1, 3, H, W] render, by `q16`."""
    t = t.reshape(3, t.shape[-2], t.shape[-1])
    return q16(t).cpu().numpy().astype(np.uint16)[::-1].transpose(1, 2, 0).copy()


def grey16(bgr16):
    """(19595 R + 38470 G + 7471 B + 32768) >> 16 of uint16 [..., 3] B G R, in Python-exact integers -> uint16 [...]."""
    c = np.asarray(bgr16).astype(np.int64)
    v = (19595 * c[..., 2] + 38470 * c[..., 1] + 7471 * c[..., 0] + 32768) >> 16
    assert v.max(initial=0) <= 65535
    return v.astype(np.uint16)


# -- rows, filters, the row rule -----------------------------------------------------------------------------------------------------------
def channels(img):
    return 1 if img.ndim == 2 else img.shape[2]


def byte_rows(img):
    """uint16 [H, W] or [H, W, 3] (stream order: R G B) -> uint8 [H, 2 C W]: every sample's high byte, then its low byte."""
    img = np.asarray(img)
    assert img.dtype == np.uint16 and (img.ndim == 2 or img.shape[2] == 3)
    h = img.shape[0]
    hi, lo = (img >> 8).astype(np.uint8), (img & 255).astype(np.uint8)
    return np.stack([hi, lo], axis=-1).reshape(h, -1)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def five_filters(row, above, bpp):
    """The five filtered forms (each uint8-valued int64 [n]) of the byte row `row` under `above` (zeros for the first row)."""
    v, b = row.astype(np.int64), above.astype(np.int64)
    a, c = np.zeros_like(v), np.zeros_like(v)
    a[bpp:], c[bpp:] = v[:-bpp], b[:-bpp]
    return [f & 255 for f in (v, v - a, v - b, v - ((a + b) >> 1), v - _paeth(a, b, c))]


def filter_rows(img, force=None):
    """-> (the scanline stream uint8 [H * (1 + 2 C W)], the filter of every row, the five costs of every row).  `force`: a filter number,
    or one per row, used instead of the rule."""
    rows = byte_rows(img)
    h, n = rows.shape
    bpp = 2 * channels(np.asarray(img))
    out = np.zeros((h, 1 + n), dtype=np.uint8)
    kinds, costs = [], []
    for y in range(h):
        cand = five_filters(rows[y], rows[y - 1] if y > 0 else np.zeros(n, dtype=np.uint8), bpp)
        cost = [int(np.minimum(f, 256 - f).sum()) for f in cand]
        k = cost.index(min(cost)) if force is None else (force if isinstance(force, int) else force[y])
        out[y, 0] = k
        out[y, 1:] = cand[k]
        kinds.append(k)
        costs.append(cost)
    return out.reshape(-1), kinds, costs


# -- bands -----------------------------------------------------------------------------------------------------------------------------
def rows_per_band(w, rows, bpp):
    return rows if rows > 0 else max(1, 131072 // (bpp * w + 1))


def band_offsets(h, line, rows):
    return [min(i * rows, h) * line for i in range(-(-h // rows))] + [h * line]


def band_tables(stream, h, line, rows):
    """(histograms int64 [bands, 257]: the count of every byte value and 1 end-of-block; Adler partials int64 [bands, 2]: (sum of the
    band's bytes, sum of byte * (bytes from it to the band's end)) mod 65521) of the stream cut into bands of `rows` image rows."""
    offs = band_offsets(h, line, rows)
    hist = np.zeros((len(offs) - 1, 257), dtype=np.int64)
    adler = np.zeros((len(offs) - 1, 2), dtype=np.int64)
    for i in range(len(offs) - 1):
        part = [int(v) for v in stream[offs[i]:offs[i + 1]]]
        n = len(part)
        hist[i, :256] = np.bincount(np.array(part, dtype=np.int64), minlength=256)
        hist[i, 256] = 1
        adler[i, 0] = sum(part) % ADLER
        adler[i, 1] = sum(v * (n - j) for j, v in enumerate(part)) % ADLER
    return hist, adler


# -- files -----------------------------------------------------------------------------------------------------------------------------
def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def chunks(png):
    """[(tag, data)] of a PNG file; every CRC is checked."""
    assert png[:8] == SIGNATURE
    out, pos = [], 8
    while pos < len(png):
        n, tag = struct.unpack('>I4s', png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff, tag
        out.append((tag, data))
        pos += 12 + n
    assert pos == len(png) and out[-1] == (b'IEND', b'')
    return out


def ihdr(png):
    """(w, h, depth, colour type, compression, filter method, interlace)"""
    tag, data = chunks(png)[0]
    assert tag == b'IHDR' and len(data) == 13
    return struct.unpack('>IIBBBBB', data)


def idat(png):
    return b''.join(d for tag, d in chunks(png) if tag == b'IDAT')


def unfilter(stream, h, line, bpp):
    """The inverse of the filters, byte by byte in Python integers -> uint8 [H, line - 1]."""
    n = line - 1
    out = np.zeros((h, n), dtype=np.uint8)
    prev = [0] * n
    for y in range(h):
        k = int(stream[y * line])
        f = [int(v) for v in stream[y * line + 1:(y + 1) * line]]
        cur = [0] * n
        for i in range(n):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if k == 0:
                pred = 0
            elif k == 1:
                pred = a
            elif k == 2:
                pred = b
            elif k == 3:
                pred = (a + b) // 2
            else:
                assert k == 4, k
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[i] = (f[i] + pred) % 256
        out[y] = cur
        prev = cur
    return out


def decode_png16(png):
    """uint16 [H, W] or [H, W, 3] (R G B) of a depth-16 file of colour type 0 or 2: chunks, zlib.decompress, `unfilter`."""
    w, h, depth, colour, comp, method, interlace = ihdr(png)
    assert depth == 16 and colour in (0, 2) and (comp, method, interlace) == (0, 0, 0)
    c = 1 if colour == 0 else 3
    line = 1 + 2 * c * w
    raw = zlib.decompress(idat(png))
    assert len(raw) == h * line
    rows = unfilter(np.frombuffer(raw, dtype=np.uint8), h, line, 2 * c).astype(np.uint16)
    samples = (rows[:, 0::2] << 8) | rows[:, 1::2]
    return samples if c == 1 else samples.reshape(h, w, 3)


def write_png16(img, force=None, idat_sizes=None, interlace=0, colour_type=None, level=6):
    """A depth-16 PNG file of uint16 [H, W] / [H, W, 3] (R G B) with filter `force` (a number, or one per row; None: the row rule) on
    every row, its zlib stream cut into IDAT chunks of `idat_sizes` bytes (None: one chunk).  `interlace` / `colour_type` only
    overwrite the IHDR fields: for the readers' refusals, such files are not valid images."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    stream = filter_rows(img, force)[0]
    z = zlib.compress(bytes(stream), level)
    ct = (0 if img.ndim == 2 else 2) if colour_type is None else colour_type
    parts = [SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16, ct, 0, 0, interlace))]
    step = idat_sizes or max(len(z), 1)
    for i in range(0, len(z), step):
        parts.append(chunk(b'IDAT', z[i:i + step]))
    parts.append(chunk(b'IEND', b''))
    return b''.join(parts)


# -- contents --------------------------------------------------------------------------------------------------------------------------
CONTENTS = ('noise', 'wrap_ramp', 'vertical', 'smooth', 'diagonal', 'flat', 'bytes')


def make16(h, w, c, content, seed=0):
    """uint16 [h, w] (c = 1) or [h, w, 3] test images.  Between them the row rule picks every filter 0..4, for both bpp
    (tests/test_depth16_host.py asserts that with this file alone).
      noise      uniform 16-bit noise: None wins most rows
      wrap_ramp  even rows: a horizontal ramp of step 37 per sample, whose LOW byte wraps while the high byte steps; odd rows: one
                 value.  Under a flat row (or none) Paeth predicts the left byte, so it ties with Sub and Sub, the lower number, wins
                 every ramp row -- with residuals 37 in the low bytes and 0 or 1 in the high ones, per byte
      vertical   every row the row above plus a constant that carries into the high byte now and then: Up
      smooth     a sum of two sinusoids scaled to 16 bits
      diagonal   an integer plane a x + b y with odd strides: Average / Paeth territory
      flat       one value
      bytes      every sample 0xHHLL with HH = 3 i + 1 and LL = 251 - 5 i mod 256 of its index: high and low bytes distinct and asymmetric,
                 so a swapped byte order cannot pass"""
    rng = np.random.RandomState(1000 * seed + 10 * h + w + c)
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing='ij')
    if content == 'noise':
        img = rng.randint(0, 65536, (h, w, c))
    elif content == 'wrap_ramp':
        img = np.where(y % 2 == 0, 37 * x + 4099 * (y // 2) + 1000 * k, 0x5A5A + 3 * y + 0 * x)
    elif content == 'vertical':
        col = rng.randint(0, 65536, (1, w, c))
        img = col + 181 * y
    elif content == 'smooth':
        img = 32768 + 20000 * np.sin(x / 5.0 + k) * np.cos(y / 3.0) + 9000 * np.sin((x + y) / 2.5)
    elif content == 'diagonal':
        img = 301 * x + 577 * y + 1111 * k + rng.randint(0, 3, (h, w, c))
    elif content == 'flat':
        img = np.full((h, w, c), 0xA53C)
    elif content == 'bytes':
        i = (y * w + x) * c + k
        img = (((3 * i + 1) % 256) << 8) | ((251 - 5 * i) % 256)
    else:
        raise KeyError(content)
    img = (np.asarray(img).astype(np.int64) % 65536).astype(np.uint16)
    return img[:, :, 0].copy() if c == 1 else img
