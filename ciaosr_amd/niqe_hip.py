"""NIQE of an 8-bit image on the MI355X (csrc/niqe_f32.hip): the blind quality score of renders that have no ground truth.

The definition is the reference's `niqe` / `niqe_core` (mmedited/core/evaluation/metrics.py:340-532): Y of the BGR image, cropped by
`crop_border` and rounded; cropped to whole 96x96 blocks; at scale 1 and, after MATLAB's antialiased bicubic halving, at scale 2 the
MSCN map with the pristine model's 7x7 window; per block 18 AGGD features from the block and four products with itself rolled inside
the block; the distance between the Gaussian fitted to the [blocks, 36] features and the pristine one.

The device does the image work and leaves six sums per scale, block and map (`moments_u8`, no synchronisation).  The host finishes
in float64 (`features`, `finish`): a few hundred kilobytes cross, once.  There is no CPU fallback for the image work: a host image
raises `CiaoSRHipError`.  Only `convert_to='y'` exists ('gray' goes through cv2 in the reference).

The pristine model (`mu_pris_param` [1, 36], `cov_pris_param` [36, 36], `gaussian_window` [7, 7], float64) is supplied by the user,
like a checkpoint: the reference's `niqe_pris_params.npz`.  It is not part of the package.

NaN rules, as the reference: a map without a negative or without a positive sample (a flat block) has NaN features; `alpha` of such a
map is the first grid value (argmin of an all-NaN array is 0).  A row with a NaN stays in the mean over blocks (`nanmean`, per column)
and is left out of the covariance.  Where the reference would return NaN or crash -- fewer than two blocks, fewer than two rows
without a NaN -- this raises `ValueError`.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, hip_ops
from ._lib import CiaoSRHipError

BLOCK = 96
MAPS, SUMS = 5, 6
PARAM_SHAPES = {'mu_pris_param': (1, 36), 'cov_pris_param': (36, 36), 'gaussian_window': (7, 7)}
# np.roll shifts of compute_feature (metrics.py:387); map 0 is the block itself
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
# MATLAB imresize by 0.5 on an even length: output o = sum_k HALF_TAPS[k] * input[reflect(2 o - 3 + k)]
HALF_TAPS = tuple(v / 256.0 for v in (-3, -9, 29, 111, 111, 29, -9, -3))


def half_index(o, k, n):
    """Input index of tap k (0..7) of output o on an axis of n samples: 2 o - 3 + k, reflected symmetrically (edge sample repeated)."""
    i = 2 * o - 3 + k
    return -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)


def load_params(src):
    """The pristine model from an .npz path or a mapping -> {name: float64 array}.  Anything but the three arrays with their shapes,
    float64 and finite, is a ValueError."""
    if isinstance(src, dict) and src.get('_niqe_params') is True:
        return src
    if isinstance(src, (str, bytes)) or hasattr(src, '__fspath__'):
        try:
            with np.load(src) as f:
                src = {k: f[k] for k in f.files}
        except (OSError, ValueError) as e:
            raise ValueError(f'cannot read NIQE parameters from {src!r}: {e}')
    if not hasattr(src, 'keys'):
        raise ValueError(f'NIQE parameters: expected an .npz path or a mapping, got {type(src).__name__}')
    out = {'_niqe_params': True, '_window_dev': {}}
    for name, shape in PARAM_SHAPES.items():
        if name not in src.keys():
            raise ValueError(f'NIQE parameters: {name} is missing')
        a = src[name]
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape:
            raise ValueError(f'NIQE parameters: {name} must be float64 {list(shape)}, got '
                             f'{getattr(a, "dtype", type(a).__name__)} {list(getattr(a, "shape", ()))}')
        if not np.isfinite(a).all():
            raise ValueError(f'NIQE parameters: {name} has non-finite entries')
        out[name] = np.ascontiguousarray(a)
    return out


def geometry(h, w, crop_border=0):
    """(rows of blocks, columns of blocks) of an h x w image; ValueError for fewer than two blocks."""
    crop = int(crop_border)
    if crop < 0:
        raise ValueError(f'crop_border={crop_border} is negative')
    nbh, nbw = max(h - 2 * crop, 0) // BLOCK, max(w - 2 * crop, 0) // BLOCK
    if nbh * nbw < 2:
        raise ValueError(f'NIQE needs at least two {BLOCK}x{BLOCK} blocks: a {h}x{w} image with crop_border={crop} has {nbh * nbw}')
    return nbh, nbw


def _check_convert(convert_to):
    if not (isinstance(convert_to, str) and convert_to.lower() == 'y'):
        raise ValueError(f'NIQE: only convert_to="y" is built (got {convert_to!r}); "gray" needs cv2')


def moments_u8(img, params, crop_border=0, return_luma=False):
    """The five launches of `ciaosr_niqe_moments_u8` on a uint8 [H, W, 3] BGR device image (rows may be pitched): the float64 device
    tensor [2, blocks, 5, 6] of block sums, blocks in the reference's order (column of blocks outer).  Does not synchronise (the first
    call with a model copies its window to the device).  `return_luma`: also the rounded Y plane, fp32 [H - 2 crop, W - 2 crop].
    A grey uint8 [H, W] image gives the moments of its (v, v, v) image, bit for bit (through a temporary of 3 H W bytes)."""
    import torch
    from .metrics_hip import _check_image
    params = load_params(params)
    crop = int(crop_border)
    if isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.dim() == 2:
        geometry(img.shape[0], img.shape[1], crop)
        img = img.unsqueeze(2).expand(-1, -1, 3).contiguous()
    if isinstance(img, torch.Tensor) and img.dim() == 3:
        geometry(img.shape[0], img.shape[1], crop)         # a ValueError of the arguments comes before anything about the device
    _check_image(img)
    h, w = img.shape[0], img.shape[1]
    nbh, nbw = geometry(h, w, crop)
    dev = img.device
    nbytes = _lib.load().ciaosr_niqe_workspace_bytes(h, w, crop)
    if nbytes == 0:
        raise CiaoSRHipError(f'niqe_moments_u8: a {h}x{w} image with crop_border={crop} is beyond the kernel\'s index range')
    window = params['_window_dev'].get(dev)
    if window is None:
        window = params['_window_dev'][dev] = torch.from_numpy(params['gaussian_window'].reshape(-1).copy()).to(dev)
    ws = hip_ops.workspace(nbytes, dev, slot='metrics')
    out = torch.empty((2, nbh * nbw, MAPS, SUMS), dtype=torch.float64, device=dev)
    luma = torch.empty((h - 2 * crop, w - 2 * crop), dtype=torch.float32, device=dev) if return_luma else None
    _lib.call('ciaosr_niqe_moments_u8', hip_ops.ptr(img), C.c_size_t(img.stride(0)), h, w, crop, hip_ops.ptr(window), hip_ops.ptr(out),
              hip_ops.ptr(luma), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return (out, luma) if return_luma else out


# ---- host finishing: plain float64 --------------------------------------------------------------------------------------------------
_tables = None


def gamma_tables():
    """(gam, r_gam, sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a)) on the grid of estimate_aggd_param, built once per process."""
    global _tables
    if _tables is None:
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        g = lambda v: np.array([math.gamma(x) for x in v])
        r_gam = np.square(g(rec * 2)) / (g(rec) * g(rec * 3))
        assert gam.shape == (9801,) and (np.diff(r_gam) > 0).all()
        g1 = g(1 / gam)
        _tables = (gam, r_gam, np.sqrt(g1 / g(3 / gam)), g(2 / gam) / g1)
    return _tables


def aggd_index(target):
    """`np.argmin((r_gam - t) ** 2)` for every t of an array, without the 9801-entry pass per value: r_gam increases, so the minimum
    is next to the insertion point; the lowest index wins a tie, and an all-NaN / all-inf row of differences gives 0, as argmin."""
    r_gam = gamma_tables()[1]
    t = np.asarray(target, dtype=np.float64)
    at = np.searchsorted(r_gam, t.reshape(-1))
    cand = np.clip(at[:, None] + np.arange(-2, 2)[None, :], 0, r_gam.size - 1)
    with np.errstate(all='ignore'):
        d = (r_gam[cand] - t.reshape(-1, 1)) ** 2
        pick = np.argmin(d, axis=1)
        idx = cand[np.arange(cand.shape[0]), pick]
        idx = np.where(np.isfinite(d.min(axis=1)), idx, 0)
    return idx.reshape(t.shape)


def features(moments):
    """[2, blocks, 5, 6] block sums (device tensor or array) -> the float64 [blocks, 36] feature matrix of niqe_core (`distparam`)."""
    m = moments.cpu().numpy() if hasattr(moments, 'cpu') else np.asarray(moments)
    m = m.astype(np.float64, copy=False)
    if m.ndim != 4 or m.shape[0] != 2 or m.shape[2:] != (MAPS, SUMS):
        raise ValueError(f'expected moments [2, blocks, {MAPS}, {SUMS}], got {list(m.shape)}')
    gam, _, beta_tab, mean_tab = gamma_tables()
    out = np.empty((m.shape[1], 36))
    with np.errstate(all='ignore'):
        for s in range(2):
            n = float((BLOCK >> s) ** 2)
            left = np.sqrt(m[s, :, :, 1] / m[s, :, :, 0])          # 0 / 0: no sample on that side -> NaN
            right = np.sqrt(m[s, :, :, 3] / m[s, :, :, 2])
            gammahat = left / right
            rhat = (m[s, :, :, 4] / n) ** 2 / (m[s, :, :, 5] / n)
            rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
            idx = aggd_index(rhatnorm)
            alpha = gam[idx]
            beta_l, beta_r = left * beta_tab[idx], right * beta_tab[idx]
            f = out[:, 18 * s:18 * s + 18]
            f[:, 0] = alpha[:, 0]
            f[:, 1] = (beta_l[:, 0] + beta_r[:, 0]) / 2
            for k in range(1, MAPS):
                f[:, 4 * k - 2] = alpha[:, k]
                f[:, 4 * k - 1] = (beta_r[:, k] - beta_l[:, k]) * mean_tab[idx[:, k]]
                f[:, 4 * k] = beta_l[:, k]
                f[:, 4 * k + 1] = beta_r[:, k]
    return out


def finish(feats, params):
    """NIQE from the [blocks, 36] features and the pristine model (metrics.py:467-478)."""
    params = load_params(params)
    feats = np.asarray(feats, dtype=np.float64)
    if feats.ndim != 2 or feats.shape[1] != 36:
        raise ValueError(f'expected features [blocks, 36], got {list(feats.shape)}')
    if feats.shape[0] < 2:
        raise ValueError(f'NIQE needs at least two blocks, got {feats.shape[0]}')
    clean = feats[~np.isnan(feats).any(axis=1)]
    if clean.shape[0] < 2:
        raise ValueError(f'NIQE needs at least two blocks without a NaN feature, got {clean.shape[0]} of {feats.shape[0]}')
    mu_d = np.nanmean(feats, axis=0)
    cov_d = np.cov(clean, rowvar=False)
    inv = np.linalg.pinv((params['cov_pris_param'] + cov_d) / 2)
    diff = params['mu_pris_param'] - mu_d
    return float(np.squeeze(np.sqrt(np.matmul(np.matmul(diff, inv), np.transpose(diff)))))


def niqe_u8(img, params, crop_border=0, convert_to='y'):
    """The reference's `niqe(img, crop_border, convert_to='y')` of a uint8 [H, W, 3] BGR device image -> float.  The copy of the block
    sums to the host is the only synchronisation.  A grey [H, W] image scores as its (v, v, v) image."""
    _check_convert(convert_to)
    params = load_params(params)
    return finish(features(moments_u8(img, params, crop_border)), params)
