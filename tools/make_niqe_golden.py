#!/usr/bin/env python
"""Writes the NIQE fixtures of tests/test_niqe_host.py and tests/test_niqe_gpu.py from the REFERENCE's own code.

    python tools/make_niqe_golden.py --reference /path/to/reference [--out tests/golden]

Runs only where the reference checkout is; no test calls it.  It imports the reference's `mmedited/core/evaluation/metrics.py` from
its path and runs `niqe_core` as written.  The modules that file imports and this machine may lack are stubbed: `cv2`, `mmcv`
(`bgr2ycbcr(y_only=True)` = ciaosr_amd.metrics.bgr2y, the restatement the PSNR tests pin), `mmedit.*`, and
`scipy.ndimage.filters.convolve` = `scipy.ndimage.convolve`.

`MATLABLikeResize` is RESTATED here, not imported: mmedit is not installed where this was written, so the class below follows the
general rule of MATLAB's imresize (kernel width 4 / scale for a down-scale, ceil(width) + 2 taps per output, weights normalised to
sum 1, indices reflected symmetrically, the height axis first and then the width) and could NOT be checked against mmedit's
`matlab_like_resize.py` offline.  It does not use the eight-tap shortcut of the kernel; the taps of an output are added one after the
other from the lowest index up, in the dtype numpy gives float64 weights times the image.

Files:
  niqe_pris_params.npz   a copy of the reference's data file (mu_pris_param, cov_pris_param, gaussian_window)
  niqe_cases.npz         per case i: img_i uint8 BGR, crop_i, y_i (the rounded Y plane; integers, stored as uint8), feat32_i / niqe32_i
                         (niqe_core on the float32 plane: the reference as written), feat64_i / niqe64_i (the same code on the plane
                         as float64); g_feat / g_niqe: per case the largest relative gap between the two runs (non-alpha feature
                         columns; NIQE), the reference's own noise that the device tolerance is taken from; names.

The generator asserts that no alpha entry differs between the two runs of a case (a case that had one would be re-seeded), and that the
painted block of the 'flat' case gives the same NaN pattern in both.
"""
import argparse
import importlib.util
import math
import os
import shutil
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ALPHA_COLS = [0] + [2 + 4 * k for k in range(4)]
ALPHA_COLS = ALPHA_COLS + [18 + c for c in ALPHA_COLS]
FLAT_MARGIN = 12       # the painted rectangle exceeds its block by this much where a neighbour adjoins: 4 pixels of resample reach
                       # plus 3 half-size pixels of window reach, so the block's MSCN map is flat at both scales


class MATLABLikeResize:
    """MATLAB imresize (bicubic, antialiased) from its general rule -- restated, see the module docstring."""

    def __init__(self, keys=None, scale=None, output_shape=None, kernel='bicubic', kernel_width=4.0):
        assert kernel == 'bicubic' and scale is not None
        self.scale, self.kernel_width = float(scale), float(kernel_width)

    @staticmethod
    def _cubic(x):
        ax = np.abs(x)
        return ((1.5 * ax ** 3 - 2.5 * ax ** 2 + 1) * (ax <= 1)
                + (-0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2)))

    def _contributions(self, in_len, out_len):
        scale, width = self.scale, self.kernel_width
        if scale < 1:
            width = width / scale
        x = np.arange(1, out_len + 1).astype(np.float64)
        u = x / scale + 0.5 * (1 - 1 / scale)
        left = np.floor(u - width / 2)
        p = int(math.ceil(width)) + 2
        ind = left[:, None] + np.arange(p)[None, :]
        w = scale * self._cubic(scale * (u[:, None] - ind)) if scale < 1 else self._cubic(u[:, None] - ind)
        w = w / np.sum(w, axis=1, keepdims=True)
        aux = np.concatenate((np.arange(in_len), np.arange(in_len - 1, -1, -1)))
        return w, aux[np.mod(ind.astype(np.int64) - 1, aux.size)]

    def _resize(self, img):
        out = img
        for dim in (0, 1):
            n = out.shape[dim]
            w, idx = self._contributions(n, int(math.ceil(n * self.scale)))
            src = np.moveaxis(out, dim, 0)
            acc = 0
            for k in range(w.shape[1]):
                acc = acc + w[:, k].reshape((-1,) + (1,) * (src.ndim - 1)) * src[idx[:, k]]
            out = np.moveaxis(acc, 0, dim)
        return out


def import_reference_metrics(ref_root):
    import scipy.ndimage
    from ciaosr_amd import metrics as own

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod('cv2', COLOR_BGR2GRAY=6)
    mod('mmcv', bgr2ycbcr=lambda img, y_only=False: own.bgr2y(img))
    mod('mmedit')
    mod('mmedit.datasets')
    mod('mmedit.datasets.pipelines')
    mod('mmedit.datasets.pipelines.matlab_like_resize', MATLABLikeResize=MATLABLikeResize)
    mod('mmedit.core')
    mod('mmedit.core.evaluation')
    mod('mmedit.core.evaluation.metric_utils', gauss_gradient=None)
    mod('scipy.ndimage.filters', convolve=scipy.ndimage.convolve)
    path = os.path.join(ref_root, 'mmedited', 'core', 'evaluation', 'metrics.py')
    spec = importlib.util.spec_from_file_location('reference_metrics', path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def synthetic(h, w, seed):
    """Seeded structure plus noise, uint8 BGR: waves and a ramp posterised to a few levels (so the file compresses), softened edges,
    Gaussian noise of 2.5 grey levels per channel."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s = np.zeros((h, w))
    for _ in range(6):
        fy, fx = rng.uniform(0.01, 0.12, 2)
        s += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
    s += 1.5 * (xx / w - yy / h)
    s = (s - s.min()) / (s.max() - s.min())
    levels = np.floor(s * 6).clip(0, 5)
    soft = levels.copy()
    soft[1:-1, 1:-1] = (levels[1:-1, 1:-1] * 2 + levels[:-2, 1:-1] + levels[2:, 1:-1] + levels[1:-1, :-2] + levels[1:-1, 2:]) / 6
    img = np.empty((h, w, 3))
    for c, off in enumerate((0.0, 6.0, -5.0)):
        img[:, :, c] = 40 + 34 * soft + off + rng.normal(0, 2.5, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def run_case(ref, params, img, crop):
    """-> (y plane float32, feat32, niqe32, feat64, niqe64) of one image by the reference's niqe_core."""
    y = img.astype(np.float32)
    y = ref.mmcv.bgr2ycbcr(y / 255., y_only=True) * 255.
    y = np.squeeze(y)
    if crop != 0:
        y = y[crop:-crop, crop:-crop]
    y = y.round()
    assert y.dtype == np.float32
    runs = []
    for plane in (y, y.astype(np.float64)):
        rows = []
        orig = ref.compute_feature

        def record(block, _orig=orig, _rows=rows):
            f = _orig(block)
            _rows.append([float(v) for v in f])
            return f
        ref.compute_feature = record
        try:
            with np.errstate(all='ignore'):
                q = float(ref.niqe_core(plane, params['mu_pris_param'], params['cov_pris_param'], params['gaussian_window']))
        finally:
            ref.compute_feature = orig
        nb = len(rows) // 2
        runs.append((np.concatenate([np.array(rows[:nb]), np.array(rows[nb:])], axis=1), q))
    return y, runs[0][0], runs[0][1], runs[1][0], runs[1][1]


def gaps(f32, q32, f64, q64):
    other = [c for c in range(36) if c not in ALPHA_COLS]
    a, b = f32[:, other], f64[:, other]
    ok = ~np.isnan(b)
    assert (np.isnan(a) == np.isnan(b)).all(), 'the two runs of the reference disagree on which features are NaN'
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))), abs(q32 - q64) / abs(q64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    import warnings
    warnings.simplefilter('ignore')
    ref = import_reference_metrics(args.reference)
    src = os.path.join(args.reference, 'mmedited', 'core', 'evaluation', 'niqe_pris_params.npz')
    dst = os.path.join(args.out, 'niqe_pris_params.npz')
    shutil.copyfile(src, dst)
    os.chmod(dst, 0o644)
    with np.load(src) as f:
        params = {k: f[k] for k in f.files}

    base = synthetic(192, 288, 11)
    flat = base.copy()
    m = FLAT_MARGIN
    # Block (row 0, column 1) and its margin, one colour.  NIQE is ill-conditioned on flat areas: x - mu of a constant is 0 or a
    # rounding residue of one sign, by the bits of the constant, and a residue counts as a sample.  Grey 106 has Y = 107, one of the
    # three luma values (107, 179, 214) whose filtered value is the constant exactly at both scales in BOTH runs of the reference
    # (found by trying all of 16..235); the assertions below would catch another outcome.
    flat[0:96 + m, 96 - m:192 + m] = (106, 106, 106)
    cases = [('192x288', base, 0), ('288x384', synthetic(288, 384, 12), 0), ('96x192', synthetic(96, 192, 13), 0),
             ('200x301_crop3', synthetic(200, 301, 14), 3), ('192x288_flat', flat, 0)]
    out = {'names': np.array([c[0] for c in cases])}
    g_feat, g_niqe = [], []
    for i, (name, img, crop) in enumerate(cases):
        y, f32, q32, f64, q64 = run_case(ref, params, img, crop)
        a32, a64 = f32[:, ALPHA_COLS], f64[:, ALPHA_COLS]
        assert np.array_equal(a32, a64), f'{name}: an alpha differs between the float32 and the float64 run; re-seed the case'
        gf, gq = gaps(f32, q32, f64, q64)
        nan_rows = int(np.isnan(f64).any(axis=1).sum())
        assert nan_rows == (1 if name.endswith('flat') else 0), (name, nan_rows)
        assert np.isfinite(q32) and np.isfinite(q64)
        assert (y == np.rint(y)).all() and y.min() >= 0 and y.max() <= 255
        print(f'{name}: blocks {f64.shape[0]} NaN rows {nan_rows} NIQE {q64:.6f} (float32 run {q32:.6f}) G features {gf:.3e} G NIQE {gq:.3e}')
        g_feat.append(gf)
        g_niqe.append(gq)
        out.update({f'img_{i}': img, f'crop_{i}': np.int64(crop), f'y_{i}': y.astype(np.uint8), f'feat32_{i}': f32,
                    f'niqe32_{i}': np.float64(q32), f'feat64_{i}': f64, f'niqe64_{i}': np.float64(q64)})
    out['g_feat'], out['g_niqe'] = np.array(g_feat), np.array(g_niqe)
    path = os.path.join(args.out, 'niqe_cases.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f'{path}: {size} bytes; largest G: features {max(g_feat):.3e}, NIQE {max(g_niqe):.3e}')
    assert size < 1000000, size


if __name__ == '__main__':
    main()
