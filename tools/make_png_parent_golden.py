"""Builds tests/golden/png_rgb_parent.npz: the three-channel PNG files of two seeded images as the library of the commit BEFORE the
RGBA coder wrote them (`encode_png` of a 23x31 image, `encode_png_tiles` of a 64x200 image with three rects).  The RGBA change made the
scanline filter a template over bytes per pixel; tests/test_rgba_gpu.py holds its three-byte instantiation to these bytes.

    python tools/make_png_parent_golden.py [OUT.npz]        # on the MI355X, with the library to record

Run it once on the parent commit; rerunning it on a later commit only records that commit against itself.

A second, separate recording, tests/golden/png_parent_digests.json: the length and SHA-256 of every output of `digest_cases` as the
library of the commit BEFORE the coder's drivers, layouts and packer helpers were unified (library version 330) wrote it.  The cases
reach every launch path and every kind of band -- stored, literals only, with matches (`check_band_kinds`, a condition on the INPUTS
that the recording commit alone has to meet) -- and tests/test_png_refactor_gpu.py holds every later commit to these bytes.

    python tools/make_png_parent_golden.py --digests [OUT.json]     # on the MI355X, with the library to record
"""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from ciaosr_amd import png_hip  # noqa: E402
from tests import png_match_ref as mref  # noqa: E402

SMALL = (23, 31, 11)                                        # h, w, seed
WIDE = (64, 200, 12)
RECTS = [(0, 0, 64, 200), (5, 7, 33, 65), (63, 199, 1, 1)]  # (y0, x0, h, w)


def image(h, w, seed):
    """Seeded uint8 [h, w, 3]: a ramp plus noise, so that the filters differ from row to row."""
    g = np.random.default_rng(seed)
    ramp = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 5 + np.arange(3)[None, None, :] * 40)
    return ((ramp + g.integers(0, 24, (h, w, 3))) % 256).astype(np.uint8)


def main(out):
    dev = torch.device('cuda:0')
    small = torch.from_numpy(image(*SMALL)).to(dev)
    wide = torch.from_numpy(image(*WIDE)).to(dev)
    arrs = {'rects': np.asarray(RECTS, dtype=np.int32)}
    for order in ('bgr', 'rgb'):
        arrs[f'small_{order}'] = np.frombuffer(png_hip.encode_png(small, order), dtype=np.uint8)
        arrs[f'small_{order}_rows3'] = np.frombuffer(png_hip.encode_png(small, order, 3), dtype=np.uint8)
        for k, data in enumerate(png_hip.encode_png_tiles(wide, RECTS, order, 7)):
            arrs[f'wide_{order}_tile{k}'] = np.frombuffer(data, dtype=np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrs)
    print(f'{out}: {len(arrs)} arrays, {os.path.getsize(out)} bytes')


# ---- the second recording: digests of every path of the coder ------------------------------------------------------------------------
HALF = (64, 200, 14)                                        # h, w, seed: the lower half one flat colour
HALF_ROWS = 24                                              # bands of 24, 24 and 16 rows: four parse chunks each, three in the last
NOISE = (150, 150, 15)                                      # one band of 150 x 451 bytes > 65535: two stored blocks
ORDERS = {3: ('bgr', 'rgb'), 4: ('bgra', 'rgba')}
DEFLATE_OFFS = [100, 9130, 14130, 17130, 21330]             # explicit bands, not from 0
DEFLATE_LINE = (301, 3)                                     # line, bpp of the bands' first part


def image_c(h, w, seed, channels):
    """`image` with `channels` channels."""
    g = np.random.default_rng(seed)
    ramp = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 5 + np.arange(channels)[None, None, :] * 40)
    return ((ramp + g.integers(0, 24, (h, w, channels))) % 256).astype(np.uint8)


def half_flat(h, w, seed, channels):
    img = image_c(h, w, seed, channels)
    img[h // 2:] = np.array([17, 99, 200, 255][:channels], dtype=np.uint8)
    return img


def deflate_bytes():
    """Bytes for `deflate_huff`: 100 unused ones, a band of 30 copies of one 301-byte line of noise (matches at the line distance
    only), a band of noise (stored), a band of eight-level noise (literals), a band of zeros (matches at distance 1)."""
    g = np.random.default_rng(16)
    parts = [g.integers(0, 256, 100), np.tile(g.integers(0, 256, 301), 30), g.integers(0, 256, 5000), g.integers(0, 8, 3000),
             np.zeros(4200, dtype=np.int64)]
    data = np.concatenate(parts).astype(np.uint8)
    assert len(data) == DEFLATE_OFFS[-1]
    return data


def digest_cases(dev):
    """(name, [output bytes, ...], [raw deflate stream, ...]) of every case, in a fixed order."""
    for ch in (3, 4):
        small = torch.from_numpy(image_c(*SMALL, ch)).to(dev)
        half = torch.from_numpy(half_flat(*HALF, ch)).to(dev)
        for order in ORDERS[ch]:
            for m in (False, True):
                runs = [('small', png_hip.encode_png(small, order, 0, m)), ('small_rows3', png_hip.encode_png(small, order, 3, m)),
                        ('half', png_hip.encode_png(half, order, 0, m)),
                        (f'half_rows{HALF_ROWS}', png_hip.encode_png(half, order, HALF_ROWS, m))]
                runs += [(f'half_tile{k}', f) for k, f in enumerate(png_hip.encode_png_tiles(half, RECTS, order, 7, m))]
                if ch == 3:
                    noise = np.random.default_rng(NOISE[2]).integers(0, 256, (NOISE[0], NOISE[1], 3)).astype(np.uint8)
                    runs.append(('noise', png_hip.encode_png(torch.from_numpy(noise).to(dev), order, NOISE[0], m)))
                for name, f in runs:
                    yield f'{name}_{order}_{"lz" if m else "huff"}', [f], [idat(f)[2:-4]]
    data = torch.from_numpy(deflate_bytes()).to(dev)
    for m, line, bpp in ((False, 0, 1), (True, 0, 1), (True,) + DEFLATE_LINE):
        segs = png_hip.deflate_huff(data, DEFLATE_OFFS, m, line, bpp)
        yield f'deflate_{"lz" if m else "huff"}_line{line}', segs, [b''.join(segs)]


def idat(png):
    """The concatenated IDAT data of a PNG file."""
    pos, parts = 8, []
    while pos < len(png):
        n, tag = struct.unpack('>I4s', png[pos:pos + 8])
        if tag == b'IDAT':
            parts.append(png[pos + 8:pos + 8 + n])
        pos += 12 + n
    return b''.join(parts)


def band_kinds(deflate):
    """The kinds of the blocks of a raw deflate stream of this coder, in order: 'stored', 'literal' (a dynamic block without matches) or
    'match'.  The empty stored block behind every dynamic block is its band's trailer and is not counted."""
    blocks, _, _ = mref.inflate_tokens(deflate)
    kinds = []
    for b in blocks:
        if b['type'] == 2:
            kinds.append('match' if any(isinstance(t, tuple) for t in b['tokens']) else 'literal')
        elif b['tokens']:
            kinds.append('stored')
    return kinds


def check_band_kinds(streams):
    """What the cases have to reach: every kind of band somewhere, and one stream in which two neighbouring bands differ in kind."""
    kinds = [band_kinds(s) for s in streams]
    seen = {k for ks in kinds for k in ks}
    assert seen == {'stored', 'literal', 'match'}, seen
    assert any(a != b for ks in kinds for a, b in zip(ks, ks[1:])), 'no stream has two adjacent bands of different kinds'
    return kinds


def digest(parts):
    return [sum(len(p) for p in parts), hashlib.sha256(b''.join(parts)).hexdigest()]


def main_digests(out):
    cases = list(digest_cases(torch.device('cuda:0')))
    for (name, _, streams) in cases:
        print(name, [band_kinds(s) for s in streams], flush=True)
    check_band_kinds([s for _, _, streams in cases for s in streams])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump({name: digest(parts) for name, parts, _ in cases}, f, indent=0)
        f.write('\n')
    print(f'{out}: {len(cases)} cases, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
    if sys.argv[1:2] == ['--digests']:
        sys.exit(main_digests(sys.argv[2] if len(sys.argv) > 2 else os.path.join(golden, 'png_parent_digests.json')))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(golden, 'png_rgb_parent.npz'))
