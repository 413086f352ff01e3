"""Builds tests/golden/png_rgb_parent.npz: the three-channel PNG files of two seeded images as the library of the commit BEFORE the
RGBA coder wrote them (`encode_png` of a 23x31 image, `encode_png_tiles` of a 64x200 image with three rects).  The RGBA change made the
scanline filter a template over bytes per pixel; tests/test_rgba_gpu.py holds its three-byte instantiation to these bytes.

    python tools/make_png_parent_golden.py [OUT.npz]        # on the MI355X, with the library to record

Run it once on the parent commit; rerunning it on a later commit only records that commit against itself.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from ciaosr_amd import png_hip  # noqa: E402

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


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'png_rgb_parent.npz'))
