"""The pyramidal tiled TIFF of DESIGN 4.1i-b7 in plain numpy + zlib, written from the TIFF 6.0 specification (sections 2 "TIFF
structure", 14 "differencing predictor", 15 "tiled images") and the contract, not from the kernel: the judge of
tests/test_tiff_host.py and tests/test_tiff_gpu.py.

Images here are numpy arrays in STREAM order: uint8 or uint16, [H, W] (grey) or [H, W, C] with R G B (A) samples.  A level is cut into
T x T tiles, row-major; a tile that reaches past the level repeats its last column and row.  The predictor differences SAMPLES (mod
2^8 or mod 2^16) against the sample of the pixel to the left, the first column stays; the bytes are row, then column, then sample, a
16-bit sample low byte first (an `II` file).  A tile's data is one zlib stream of those bytes.  `read_tiff` is a small reader of
exactly such files: the IFD chain, the tiles, inflate, the predictor undone, the padding cropped; tests/test_tiff_host.py holds it to
Pillow on the kinds Pillow reads, and it is the decoder of RGB 16, which Pillow returns as 8-bit."""
import struct
import zlib

import numpy as np

TAG_NAMES = {254: 'NewSubfileType', 256: 'ImageWidth', 257: 'ImageLength', 258: 'BitsPerSample', 259: 'Compression',
             262: 'PhotometricInterpretation', 277: 'SamplesPerPixel', 284: 'PlanarConfiguration', 317: 'Predictor', 322: 'TileWidth',
             323: 'TileLength', 324: 'TileOffsets', 325: 'TileByteCounts', 338: 'ExtraSamples', 339: 'SampleFormat'}
KINDS = ('rgb8', 'grey8', 'grey16', 'rgba8', 'rgb16')


def kind_shape(kind):
    """(samples per pixel, numpy dtype)"""
    return {'rgb8': (3, np.uint8), 'grey8': (1, np.uint8), 'grey16': (1, np.uint16), 'rgba8': (4, np.uint8), 'rgb16': (3, np.uint16)}[kind]


def make_image(h, w, kind, seed=0):
    """A test image of `kind`: smooth ramps plus noise, with samples 0 and the largest value side by side in places, so that the
    predictor wraps and (at 16 bits) borrows across the byte boundary."""
    c, dtype = kind_shape(kind)
    top = int(np.iinfo(dtype).max)
    rng = np.random.RandomState(7919 * seed + 131 * h + 17 * w + c + top % 255)
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing='ij')
    img = (top // 3) + (top // 97) * x + (top // 61) * y + (top // 7) * k + rng.randint(0, max(2, top // 50), (h, w, c))
    edge = rng.rand(h, w, c) < 0.15
    img = np.where(edge, np.where((x + y + k) % 2 == 0, 0, top), img % (top + 1))
    img = img.astype(dtype)
    return img[:, :, 0].copy() if c == 1 else img


def level_sizes(h, w, tile):
    sizes = [(h, w)]
    while max(h, w) > tile:
        h, w = -(-h // 2), -(-w // 2)
        sizes.append((h, w))
    return sizes


def halve_box(a):
    """(a[2i, 2j] + a[2i, j1] + a[i1, 2j] + a[i1, j1] + 2) >> 2 with i1 = min(2i + 1, h - 1), j1 = min(2j + 1, w - 1), per sample,
    in Python-exact integers."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    i0, j0 = 2 * np.arange(-(-h // 2)), 2 * np.arange(-(-w // 2))
    i1, j1 = np.minimum(i0 + 1, h - 1), np.minimum(j0 + 1, w - 1)
    b = a.astype(np.int64)
    s = b[i0][:, j0] + b[i0][:, j1] + b[i1][:, j0] + b[i1][:, j1] + 2
    return (s >> 2).astype(a.dtype)


def pyramid_of(img, tile):
    """The levels of `img` by the box halving, the top first, as `level_sizes` lists them."""
    levels = [np.asarray(img)]
    for _ in level_sizes(img.shape[0], img.shape[1], tile)[1:]:
        levels.append(halve_box(levels[-1]))
    return levels


def padded_tile(img, ty, tx, tile):
    """P[r, c, k] = I[min(ty T + r, H - 1), min(tx T + c, W - 1), k] -> [T, T, C]"""
    h, w = img.shape[:2]
    rows = np.minimum(ty * tile + np.arange(tile), h - 1)
    cols = np.minimum(tx * tile + np.arange(tile), w - 1)
    return img[rows][:, cols].reshape(tile, tile, -1)


def predicted_bytes(p):
    """The byte stream of a padded tile [T, T, C]: per sample D[r, 0] = P[r, 0], D[r, c] = P[r, c] - P[r, c - 1] mod 2^S; r, then c,
    then k, a 16-bit sample low byte first."""
    bits = 8 * p.dtype.itemsize
    v = p.astype(np.int64)
    d = v.copy()
    d[:, 1:] = (v[:, 1:] - v[:, :-1]) % (1 << bits)
    d = d.reshape(-1)
    if bits == 8:
        return d.astype(np.uint8).tobytes()
    return np.stack([d & 255, d >> 8], axis=-1).astype(np.uint8).tobytes()


def tile_grid(h, w, tile):
    return [(ty, tx) for ty in range(-(-h // tile)) for tx in range(-(-w // tile))]


def tiles_bytes(img, tile):
    """The predicted bytes of every tile of the level `img`, row-major."""
    img = np.asarray(img)
    return [predicted_bytes(padded_tile(img, ty, tx, tile)) for ty, tx in tile_grid(img.shape[0], img.shape[1], tile)]


def meta_of(img, tile):
    img = np.asarray(img)
    return dict(height=img.shape[0], width=img.shape[1], samples=1 if img.ndim == 2 else img.shape[2], bits=8 * img.dtype.itemsize,
                tile=tile)


# -- the reader ------------------------------------------------------------------------------------------------------------------------
def read_ifds(data):
    """[(offset of the IFD, {tag: (type, [values])})] of a classic little-endian TIFF, following the chain."""
    assert data[:4] == b'II*\0', data[:4]
    off = struct.unpack('<I', data[4:8])[0]
    out, seen = [], set()
    while off:
        assert off not in seen and off % 2 == 0 and off + 2 <= len(data), off
        seen.add(off)
        n = struct.unpack('<H', data[off:off + 2])[0]
        tags = {}
        last = 0
        for k in range(n):
            tag, typ, count, val = struct.unpack('<HHI4s', data[off + 2 + 12 * k:off + 14 + 12 * k])
            assert tag > last, 'tags ascend'
            last = tag
            size, code = {3: (2, 'H'), 4: (4, 'I')}[typ]
            if size * count <= 4:
                raw = val[:size * count]
            else:
                where = struct.unpack('<I', val)[0]
                assert where % 2 == 0, (tag, where)
                raw = data[where:where + size * count]
            tags[tag] = (typ, list(struct.unpack(f'<{count}{code}', raw)))
        out.append((off, tags))
        off = struct.unpack('<I', data[off + 2 + 12 * n:off + 6 + 12 * n])[0]
    return out


def unpredict(raw, tile, samples, bits):
    """The padded tile [T, T, C] of its predicted bytes."""
    b = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    assert b.size == tile * tile * samples * bits // 8, (b.size, tile, samples, bits)
    d = b if bits == 8 else b[0::2] | (b[1::2] << 8)
    d = d.reshape(tile, tile, samples)
    return (np.cumsum(d, axis=1) % (1 << bits)).astype(np.uint8 if bits == 8 else np.uint16)


def read_tiff(data):
    """The levels of a file of this contract, the top first: uint8 / uint16 [H, W] or [H, W, C] in stream order.  Asserts the
    structure as it goes: the tag values, the tile counts, each tile ONE zlib stream that ends where its byte count says."""
    levels = []
    for k, (_, tags) in enumerate(read_ifds(data)):
        v = {t: vals for t, (_, vals) in tags.items()}
        samples, bits = v[277][0], v[258][0]
        assert v[254] == [1 if k else 0] and v[259] == [8] and v[284] == [1] and v[317] == [2]
        assert v[258] == [bits] * samples and v[339] == [1] * samples and bits in (8, 16)
        assert v[262] == [1 if samples == 1 else 2] and (v.get(338) == [2]) == (samples == 4)
        w, h, tile = v[256][0], v[257][0], v[322][0]
        assert v[323] == [tile]
        grid = tile_grid(h, w, tile)
        assert len(v[324]) == len(v[325]) == len(grid)
        img = np.zeros((h, w, samples), dtype=np.uint8 if bits == 8 else np.uint16)
        for (ty, tx), off, n in zip(grid, v[324], v[325]):
            assert off % 2 == 0
            z = zlib.decompressobj()
            raw = z.decompress(data[off:off + n])
            assert z.eof and z.unused_data == b'', 'one zlib stream per tile, no more and no less'
            p = unpredict(raw, tile, samples, bits)
            y0, x0 = ty * tile, tx * tile
            hh, ww = min(tile, h - y0), min(tile, w - x0)
            img[y0:y0 + hh, x0:x0 + ww] = p[:hh, :ww]
            assert np.array_equal(p, padded_tile(img[:y0 + hh, :x0 + ww], ty, tx, tile)), 'padding repeats the last column and row'
        levels.append(img[:, :, 0].copy() if samples == 1 else img)
    return levels


def pillow_pages(data):
    """Every page of the file as Pillow decodes it (numpy arrays)."""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    pages = []
    for k in range(im.n_frames):
        im.seek(k)
        pages.append(np.array(im))
    return pages
