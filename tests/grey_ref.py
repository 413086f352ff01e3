"""A plain numpy restatement of the grey definitions, independent of the package: the grey byte of a quantised pixel,
the one-byte-per-pixel PNG scanline filter with its selection rule, the per-band histogram and Adler partials the device leaves
beside the stream, and the quantised blocks of a one-component JPEG scan for tests/jpeg_opt_ref.py's table rule."""
import numpy as np

from tests import jpeg_opt_ref as opt
from tests import jpeg_ref

ADLER = 65521
HIST_STRIDE = 260


def grey_of_bgr(bgr_u8):
    """uint8 [..., 3] B G R bytes -> uint8 [...]: L = (19595 R + 38470 G + 7471 B + 32768) >> 16 in integers."""
    v = np.asarray(bgr_u8).astype(np.int64)
    g = (19595 * v[..., 2] + 38470 * v[..., 1] + 7471 * v[..., 0] + 32768) >> 16
    assert g.min() >= 0 and g.max() <= 255
    return g.astype(np.uint8)


def alpha_of_bgr(bgr_u8):
    """The alpha formula of the RGBA feature, which the grey byte is NOT: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    v = np.asarray(bgr_u8).astype(np.int64)
    return ((4899 * v[..., 2] + 9617 * v[..., 1] + 1868 * v[..., 0] + 8192) >> 14).astype(np.uint8)


def disagreement_set():
    """int64 [n, 3] B G R: every one of the 2^24 triples on which the grey byte and the alpha formula differ."""
    out = []
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing='ij')
    for r in range(256):
        grey = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
        alpha = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
        gi, bi = np.nonzero(grey != alpha)
        assert (np.abs(grey - alpha)[gi, bi] == 1).all()
        out.append(np.stack([b[gi, bi], g[gi, bi], np.full(len(gi), r, dtype=np.int64)], axis=-1))
    return np.concatenate(out)


def rows_per_band(w, rows=0):
    return rows if rows > 0 else max(1, 131072 // (w + 1))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(grey):
    """uint8 [H, W] -> (the scanline stream, uint8 [H * (1 + W)]; the filter chosen per row; the five costs per row).  The left
    predecessor of a byte is the byte before it, the upper one the byte above; zeros left of column 0 and above row 0.  Per row the
    filter with the smallest sum of min(b, 256 - b); ties to the lowest number."""
    img = np.asarray(grey).astype(np.int64)
    h, w = img.shape
    out = np.zeros((h, 1 + w), dtype=np.uint8)
    kinds, costs = [], []
    for y in range(h):
        v = img[y]
        a = np.zeros_like(v)
        a[1:] = v[:-1]
        b = img[y - 1] if y > 0 else np.zeros_like(v)
        c = np.zeros_like(v)
        if y > 0:
            c[1:] = img[y - 1, :-1]
        cand = [(f & 255) for f in (v, v - a, v - b, v - ((a + b) >> 1), v - _paeth(a, b, c))]
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
    line = 1 + w
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


def band_offsets(h, w, rows):
    """The byte offsets of the bands of `rows` image rows in the stream of an h x w grey image."""
    line = 1 + w
    return [min(i * rows, h) * line for i in range(-(-h // rows))] + [h * line]


def jpeg_blocks(grey, quality):
    """The blocks of the one-component scan in coding order, as tests/jpeg_opt_ref.py takes them: [(0, int coefficients [64] in zigzag
    order)] -- the samples with the last column and row repeated up to whole blocks, the luma table, row-major."""
    g = np.asarray(grey).astype(np.int64)
    h, w = g.shape
    plane = np.pad(g, ((0, -h % 8), (0, -w % 8)), mode='edge')
    blocks = jpeg_ref.blocks_of(plane, jpeg_ref.quant_tables(quality)[0])
    return [(0, blocks[i, j]) for i in range(blocks.shape[0]) for j in range(blocks.shape[1])]


def jpeg_table_depths(grey, quality):
    """The depths BEFORE limiting of the two Huffman trees (DC, AC) that libjpeg's rule makes for the one-component scan."""
    hist = opt.histograms(opt.symbols(jpeg_blocks(grey, quality)))
    return [opt.table_from_histogram(hist[k])[2] for k in (0, 1)]
