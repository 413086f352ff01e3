"""A plain numpy restatement of the RGBA definitions, independent of the package: the alpha of a quantised pixel, the
four-byte-per-pixel PNG scanline filter with its selection rule, the per-band histogram and Adler partials the device leaves beside
the stream, and a decoder of colour type 6 files (chunk CRCs checked, `zlib.decompress`, unfilter) that owes Pillow nothing."""
import struct
import zlib

import numpy as np

ADLER = 65521
HIST_STRIDE = 260
BPP = 4


def alpha_of_bgr(bgr_u8):
    """uint8 [..., 3] B G R bytes of the rendered alpha image -> uint8 [...]: (4899 R + 9617 G + 1868 B + 8192) >> 14 in integers."""
    v = np.asarray(bgr_u8).astype(np.int64)
    a = (4899 * v[..., 2] + 9617 * v[..., 1] + 1868 * v[..., 0] + 8192) >> 14
    assert a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


def pack_bgra(bgr_u8, grey_bgr_u8):
    """uint8 [H, W, 4] B G R A: the colour bytes and the alpha of the grey image's bytes."""
    return np.concatenate([np.asarray(bgr_u8), alpha_of_bgr(grey_bgr_u8)[..., None]], axis=-1).astype(np.uint8)


def rows_per_band(w, rows=0):
    return rows if rows > 0 else max(1, 131072 // (BPP * w + 1))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rgba):
    """uint8 [H, W, 4] R G B A -> (the scanline stream, uint8 [H * (1 + 4 W)]; the filter chosen per row; the five costs per row).
    The left predecessor of a byte is the same channel of the pixel before it, the upper one the same byte of the row above; zeros left
    of column 0 and above row 0.  Per row the filter with the smallest sum of min(b, 256 - b); ties to the lowest number."""
    img = np.asarray(rgba).astype(np.int64)
    h, w, ch = img.shape
    assert ch == BPP
    out = np.zeros((h, 1 + BPP * w), dtype=np.uint8)
    kinds, costs = [], []
    for y in range(h):
        v = img[y]
        a = np.zeros_like(v)
        a[1:] = v[:-1]
        b = img[y - 1] if y > 0 else np.zeros_like(v)
        c = np.zeros_like(v)
        if y > 0:
            c[1:] = img[y - 1, :-1]
        cand = [v, v - a, v - b, v - ((a + b) >> 1), v - _paeth(a, b, c)]
        cand = [(f & 255).reshape(-1) for f in cand]
        cost = [int(np.minimum(f, 256 - f).sum()) for f in cand]
        k = cost.index(min(cost))                                   # the first of equals: the lowest number
        out[y, 0] = k
        out[y, 1:] = cand[k]
        kinds.append(k)
        costs.append(cost)
    return out.reshape(-1), kinds, costs


def band_tables(stream, h, w, rows):
    """(histograms int64 [bands, 260], Adler partials int64 [bands, 2]) of the stream cut into bands of `rows` image rows: per band the
    count of every byte value and 1 at index 256; (sum of its bytes, sum of byte * (bytes from it to the band's end)) mod 65521."""
    line = 1 + BPP * w
    nb = -(-h // rows)
    hist = np.zeros((nb, HIST_STRIDE), dtype=np.int64)
    adler = np.zeros((nb, 2), dtype=np.int64)
    for i in range(nb):
        part = np.asarray(stream[i * rows * line:min(h, (i + 1) * rows) * line]).astype(np.int64)
        hist[i, :256] = np.bincount(part, minlength=256)
        hist[i, 256] = 1
        n = len(part)
        adler[i, 0] = int(part.sum()) % ADLER
        adler[i, 1] = int((part * (n - np.arange(n))).sum()) % ADLER
    return hist, adler


def unfilter(stream, h, w):
    """The inverse of `filter_rows`: bytes of H rows of 1 + 4 W -> uint8 [H, W, 4] R G B A."""
    line = 1 + BPP * w
    data = np.frombuffer(bytes(stream), dtype=np.uint8).reshape(h, line)
    img = np.zeros((h, w, BPP), dtype=np.int64)
    for y in range(h):
        k = int(data[y, 0])
        f = data[y, 1:].astype(np.int64).reshape(w, BPP)
        b = img[y - 1] if y > 0 else np.zeros((w, BPP), dtype=np.int64)
        if k == 0:
            img[y] = f
        elif k == 1:
            img[y] = np.cumsum(f, axis=0) & 255
        elif k == 2:
            img[y] = (f + b) & 255
        elif k in (3, 4):
            left = [0] * BPP
            for x in range(w):
                up = [int(t) for t in b[x]]
                ul = [int(t) for t in b[x - 1]] if x > 0 else [0] * BPP
                cur = []
                for ch in range(BPP):
                    if k == 3:
                        pred = (left[ch] + up[ch]) >> 1
                    else:
                        p = left[ch] + up[ch] - ul[ch]
                        pa, pb, pc = abs(p - left[ch]), abs(p - up[ch]), abs(p - ul[ch])
                        pred = left[ch] if (pa <= pb and pa <= pc) else (up[ch] if pb <= pc else ul[ch])
                    cur.append((int(f[x, ch]) + pred) & 255)
                img[y, x] = cur
                left = cur
        else:
            raise ValueError(f'row {y}: filter type {k}')
    return img.astype(np.uint8)


def chunks(png):
    """[(tag, data)] of a PNG file; the signature and every chunk's CRC are checked."""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    out, i = [], 8
    while i < len(png):
        n, = struct.unpack('>I', png[i:i + 4])
        tag, data = png[i + 4:i + 8], png[i + 8:i + 8 + n]
        crc, = struct.unpack('>I', png[i + 8 + n:i + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff, tag
        out.append((tag, data))
        i += 12 + n
    assert i == len(png) and out[0][0] == b'IHDR' and out[-1] == (b'IEND', b'')
    return out


def decode_rgba_png(png):
    """A colour type 6, 8-bit, non-interlaced PNG file -> uint8 [H, W, 4] R G B A."""
    parts = chunks(png)
    w, h, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', parts[0][1])
    assert (depth, colour, comp, flt, lace) == (8, 6, 0, 0, 0), (depth, colour, comp, flt, lace)
    raw = zlib.decompress(b''.join(d for t, d in parts if t == b'IDAT'))
    assert len(raw) == h * (1 + BPP * w)
    return unfilter(raw, h, w)
