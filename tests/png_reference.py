"""A tiny numpy reference of the PNG pieces that csrc/png_u8.hip implements, written for the tests (not product code):

* `filter_stream`  the scanline stream under the fixed filter rule: per row the filter in {0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth} whose
  filtered bytes have the smallest sum of (b < 128 ? b : 256 - b), ties to the lowest number; 3 bytes per pixel, raw predecessors,
  the row above row 0 is zeros;
* `unfilter`       the PNG reconstruction of such a stream (PNG specification, section 9);
* `model_bytes`    the size of a literal-only coder with ONE optimal, unlimited-depth Huffman code per band and a plain header.

The judges of the encoder's output are Python's `zlib` and Pillow's decoder; this module only says which bytes the filter stage must
produce and how small an ideal Huffman coder would get them.
"""
import heapq
import struct
import zlib

import numpy as np


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_candidates(rgb):
    """int [5, H, 3 W]: the five filters of every row of a uint8 [H, W, 3] RGB image."""
    h, w, _ = rgb.shape
    x = rgb.reshape(h, 3 * w).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]) & 255


def filter_stream(rgb):
    """(stream bytes, filter number per row) of a uint8 [H, W, 3] RGB image under the rule above."""
    rgb = np.ascontiguousarray(rgb)
    h, w, _ = rgb.shape
    cand = filtered_candidates(rgb)
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)              # [5, H]
    best = np.argmin(cost, axis=0)                                          # first minimum = lowest number
    rows = np.empty((h, 3 * w + 1), dtype=np.uint8)
    rows[:, 0] = best
    rows[:, 1:] = cand[best, np.arange(h)]
    return rows.tobytes(), best


def unfilter(stream, h, w):
    """uint8 [h, w, 3] RGB from a scanline stream (any filter per row)."""
    line = 3 * w + 1
    assert len(stream) == h * line, (len(stream), h, w)
    out = np.zeros((h, 3 * w), dtype=np.int64)
    src = np.frombuffer(stream, dtype=np.uint8).reshape(h, line)
    for y in range(h):
        ft, f = int(src[y, 0]), src[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(3 * w, dtype=np.int64)
        if ft == 0:
            out[y] = f
        elif ft == 2:
            out[y] = (f + up) & 255
        elif ft in (1, 3, 4):
            row = out[y]
            for i in range(3 * w):
                a = row[i - 3] if i >= 3 else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + up[i]) >> 1
                else:
                    c = up[i - 3] if i >= 3 else 0
                    p = a + up[i] - c
                    pa, pb, pc = abs(p - a), abs(p - up[i]), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (up[i] if pb <= pc else c)
                row[i] = (f[i] + pred) & 255
        else:
            raise ValueError(f'row {y}: filter type {ft}')
    return out.astype(np.uint8).reshape(h, w, 3)


def huffman_lengths(counts):
    """{symbol: depth} of an optimal (unlimited-depth) Huffman code of the symbols with a non-zero count."""
    heap = [(int(c), i, (i,)) for i, c in enumerate(counts) if c]
    if len(heap) == 1:
        return {heap[0][1]: 1}
    depth = {s: 0 for _, s, _ in heap}
    heapq.heapify(heap)
    tick = len(counts)
    while len(heap) > 1:
        c1, _, s1 = heapq.heappop(heap)
        c2, _, s2 = heapq.heappop(heap)
        for s in s1 + s2:
            depth[s] += 1
        tick += 1
        heapq.heappush(heap, (c1 + c2, tick, s1 + s2))
    return depth


def band_histogram(band):
    """257 counts: the bytes of a band and one end-of-block."""
    h = np.bincount(np.frombuffer(band, dtype=np.uint8), minlength=256).tolist()
    return h + [1]


def band_model_bits(band):
    """Bits of one dynamic block for `band` under the model: optimal Huffman lengths for the 257 symbols; header = 3 + 14 bits, 19 x 3
    bits of code-length-code lengths, and the 258 code lengths sent one by one (no run-length symbols) under their own optimal code."""
    hist = band_histogram(band)
    depth = huffman_lengths(hist)
    payload = sum(hist[s] * d for s, d in depth.items())
    lens = [depth.get(s, 0) for s in range(257)] + [0]
    cl = {}
    for v in lens:
        cl[v] = cl.get(v, 0) + 1
    keys = sorted(cl)
    cl_depth = huffman_lengths([cl[k] for k in keys])
    header = 3 + 14 + 19 * 3 + sum(cl[keys[i]] * d for i, d in cl_depth.items())
    return header + payload, max(depth.values())


def band_split(n_rows, line, rows_per_band):
    """Byte offsets of the bands of rows_per_band rows in a stream of n_rows lines."""
    return [min(r, n_rows) * line for r in range(0, n_rows + rows_per_band, rows_per_band) if r - rows_per_band < n_rows]


def model_bytes(stream, offsets):
    """zlib-stream bytes under the model: per band its block, byte-aligned by an empty stored block (3 bits, pad, 4 bytes); 2 + 4 bytes
    of zlib framing."""
    total = 6
    for i in range(len(offsets) - 1):
        bits, _ = band_model_bits(stream[offsets[i]:offsets[i + 1]])
        total += (bits + 3 + 7) // 8 + 4
    return total


def png_overhead(n_idat=1):
    """Container bytes around the IDAT data: signature, IHDR, n_idat IDAT frames, IEND."""
    return 8 + 25 + 12 * n_idat + 12


def png_from_stream(stream, h, w, level=6):
    """A PNG file whose IDAT is zlib.compress(stream): the reference's own file, for Pillow to decode."""
    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(stream, level)) + chunk(b'IEND', b''))


def idat_payload(png):
    """(h, w, concatenated IDAT data) of a PNG file; checks every chunk's CRC."""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    pos, h, w, parts = 8, None, None, []
    while pos < len(png):
        n, tag = struct.unpack('>I4s', png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff, tag
        if tag == b'IHDR':
            w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', data)
            assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
        elif tag == b'IDAT':
            parts.append(data)
        pos += 12 + n
    assert tag == b'IEND'
    return h, w, b''.join(parts)
