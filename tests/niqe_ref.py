"""NIQE restated in plain float64 numpy: the contract of the reference's `niqe_core` (mmedited/core/evaluation/metrics.py:340-478)
for a rounded Y plane, independent of ciaosr_amd/niqe_hip.py and of scipy.  Checker only.

- the 7x7 window is applied as scipy's `convolve(mode='nearest')`: the flipped window walked in raster order over an edge-padded
  image, the 49 products added one after the other (the order scipy's loop has);
- the halving between the scales is MATLAB's `imresize` from its GENERAL rule (`matlab_resize_weights`): kernel width 4 / scale,
  ceil(width) + 2 taps, weights normalised, symmetric indices; along the height first, then along the width, taps added from the
  lowest index up;
- a straightforward loop over blocks (column of blocks outer), `np.roll` of each block, `argmin` on the 9801-entry gamma table.
"""
import math

import numpy as np

BLOCK = 96
SHIFTS = ([0, 1], [1, 0], [1, 1], [1, -1])

_GAM = np.arange(0.2, 10.001, 0.001)
_R_GAM = None


def _gamma(v):
    return np.array([math.gamma(x) for x in np.ravel(v)]).reshape(np.shape(v))


def r_gam():
    global _R_GAM
    if _R_GAM is None:
        rec = np.reciprocal(_GAM)
        _R_GAM = np.square(_gamma(rec * 2)) / (_gamma(rec) * _gamma(rec * 3))
    return _R_GAM


def cubic(x):
    """MATLAB's bicubic kernel (a = -0.5)."""
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2))


def matlab_resize_weights(in_len, scale):
    """(weights [out_len, P], 0-based indices [out_len, P]) of MATLAB imresize along one axis, antialiased for scale < 1 (the
    `contributions` function of imresize.m), all-zero tap columns kept."""
    out_len = int(math.ceil(in_len * scale))
    width = 4.0 / scale if scale < 1 else 4.0
    x = np.arange(1, out_len + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - width / 2)
    p = int(math.ceil(width)) + 2
    ind = left[:, None] + np.arange(p)[None, :]                    # 1-based
    arg = u[:, None] - ind
    w = scale * cubic(scale * arg) if scale < 1 else cubic(arg)
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(in_len), np.arange(in_len - 1, -1, -1)])
    idx = aux[np.mod(ind.astype(np.int64) - 1, 2 * in_len)]
    return w, idx


def resize_along(img, w, idx, axis):
    """sum_k w[:, k] * img[idx[:, k]] along `axis`, taps added in order."""
    img = np.moveaxis(img, axis, 0)
    out = np.zeros((w.shape[0],) + img.shape[1:], dtype=np.float64)
    for k in range(w.shape[1]):
        out = out + w[:, k].reshape((-1,) + (1,) * (img.ndim - 1)) * img[idx[:, k]]
    return np.moveaxis(out, 0, axis)


def matlab_half(img):
    """MATLABLikeResize(scale=0.5): along the height first, then along the width."""
    for axis in (0, 1):
        w, idx = matlab_resize_weights(img.shape[axis], 0.5)
        img = resize_along(img, w, idx, axis)
    return img


def convolve_nearest(img, window):
    """scipy.ndimage.convolve(img, window, mode='nearest') for an odd square window."""
    k = window.shape[0]
    r = k // 2
    pad = np.pad(img, r, mode='edge')
    wf = window[::-1, ::-1]
    h, w = img.shape
    out = np.zeros_like(img)
    for a in range(k):
        for b in range(k):
            out = out + pad[a:a + h, b:b + w] * wf[a, b]
    return out


def mscn(img, window):
    mu = convolve_nearest(img, window)
    sigma = np.sqrt(np.abs(convolve_nearest(np.square(img), window) - np.square(mu)))
    return (img - mu) / (sigma + 1)


def aggd(block):
    """estimate_aggd_param (metrics.py:340-367)."""
    block = block.flatten()
    with np.errstate(all='ignore'):
        neg, pos = block[block < 0], block[block > 0]
        left_std = np.sqrt(np.mean(neg ** 2)) if neg.size else np.nan
        right_std = np.sqrt(np.mean(pos ** 2)) if pos.size else np.nan
        gammahat = left_std / right_std
        rhat = (np.mean(np.abs(block))) ** 2 / np.mean(block ** 2)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        alpha = _GAM[np.argmin((r_gam() - rhatnorm) ** 2)]
        c = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return alpha, left_std * c, right_std * c


def block_features(block):
    """compute_feature (metrics.py:370-393)."""
    alpha, bl, br = aggd(block)
    feat = [alpha, (bl + br) / 2]
    for shift in SHIFTS:
        alpha, bl, br = aggd(block * np.roll(block, shift, axis=(0, 1)))
        feat.extend([alpha, (br - bl) * (math.gamma(2 / alpha) / math.gamma(1 / alpha)), bl, br])
    return feat


def niqe_features(y, window):
    """[blocks, 36] features of a rounded Y plane (any float dtype; computed in float64)."""
    img = np.asarray(y, dtype=np.float64)
    nbh, nbw = img.shape[0] // BLOCK, img.shape[1] // BLOCK
    img = img[:nbh * BLOCK, :nbw * BLOCK]
    parts = []
    for scale in (1, 2):
        m = mscn(img, window)
        bs = BLOCK // scale
        parts.append(np.array([block_features(m[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]) for j in range(nbw) for i in range(nbh)]))
        if scale == 1:
            img = matlab_half(img / 255.) * 255.
    return np.concatenate(parts, axis=1)


def niqe_finish(feats, mu_p, cov_p):
    mu_d = np.nanmean(feats, axis=0)
    clean = feats[~np.isnan(feats).any(axis=1)]
    cov_d = np.cov(clean, rowvar=False)
    inv = np.linalg.pinv((cov_p + cov_d) / 2)
    return float(np.squeeze(np.sqrt(np.matmul(np.matmul(mu_p - mu_d, inv), np.transpose(mu_p - mu_d)))))


def niqe(y, params):
    """(features, NIQE) of a rounded Y plane under the pristine model `params` (the three arrays by name)."""
    feats = niqe_features(y, np.asarray(params['gaussian_window'], dtype=np.float64))
    return feats, niqe_finish(feats, params['mu_pris_param'], params['cov_pris_param'])


def moments(y, window):
    """The six sums per scale, block and map the device kernel leaves, [2, blocks, 5, 6], by numpy from a Y plane."""
    img = np.asarray(y, dtype=np.float64)
    nbh, nbw = img.shape[0] // BLOCK, img.shape[1] // BLOCK
    img = img[:nbh * BLOCK, :nbw * BLOCK]
    out = np.zeros((2, nbh * nbw, 5, 6))
    for s in range(2):
        m = mscn(img, window)
        bs = BLOCK >> s
        for j in range(nbw):
            for i in range(nbh):
                b = m[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]
                for k, v in enumerate([b] + [b * np.roll(b, sh, axis=(0, 1)) for sh in SHIFTS]):
                    out[s, j * nbh + i, k] = [(v < 0).sum(), (v[v < 0] ** 2).sum(), (v > 0).sum(), (v[v > 0] ** 2).sum(),
                                              np.abs(v).sum(), (v ** 2).sum()]
        if s == 0:
            img = matlab_half(img / 255.) * 255.
    return out
