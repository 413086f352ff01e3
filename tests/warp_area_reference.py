"""The definition of an area-sampled warp (include/ciaosr_hip.h, "area-sampled warps") restated in numpy float64, one rounded operation
per numpy call: what tests/test_warp_area_host.py and tests/test_warp_area_gpu.py hold scene.py's helpers and the kernels to.  Independent
of scene.py; the raw footprints are tests/warp_pp_reference.py's, membership and frame coordinates tests/warp_reference.py's."""
import numpy as np


def counts(g, hi, n_max):
    """Samples per axis, [n] int64: n = 1; while n < n_max and g > hi n: n = 2 n.  +inf: n_max; NaN: 0."""
    g = np.asarray(g, dtype=np.float64)
    hi = np.float64(hi)
    n = np.ones(g.shape, dtype=np.int64)
    k = 1
    while k < n_max:
        with np.errstate(invalid='ignore'):
            n = np.where((n == k) & (g > hi * np.float64(k)), 2 * k, n)
        k *= 2
    return np.where(np.isnan(g), 0, n)


def table(gy, gx, rng, n_max):
    """-> (first [Q + 1] int64, ny [Q], nx [Q], fy [Q], fx [Q]) of the raw footprints (gy, gx), each [Q] in row-major pixel order: a NaN
    component leaves the pixel without samples (n = 0, f = NaN); f = min(max(g / n, lo), hi)."""
    lo, hi = np.float64(rng[0]), np.float64(rng[1])
    ny, nx = counts(gy, hi, n_max), counts(gx, hi, n_max)
    has = (ny > 0) & (nx > 0)
    ny, nx = np.where(has, ny, 0), np.where(has, nx, 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        fy = np.where(has, np.minimum(np.maximum(np.asarray(gy, dtype=np.float64) / np.maximum(ny, 1), lo), hi), np.nan)
        fx = np.where(has, np.minimum(np.maximum(np.asarray(gx, dtype=np.float64) / np.maximum(nx, 1), lo), hi), np.nan)
    first = np.concatenate([[0], np.cumsum(ny * nx)]).astype(np.int64)
    return first, ny, nx, fy, fx


def samples(h, hv, wv, first, ny, nx, fy, fx):
    """Every sample in increasing sample id: -> (pixel [S] int64, y_lr [S], x_lr [S], f_y [S], f_x [S]).  Sample s = a n_x + b of pixel
    (i, j) sits at v = i + (2a + 1) / (2 n_y), u = j + (2b + 1) / (2 n_x); its LR position is the homography's formula there."""
    h = [np.float64(c) for c in h]
    cnt = ny * nx
    pix = np.repeat(np.arange(hv * wv, dtype=np.int64), cnt)
    s = np.arange(int(first[-1]), dtype=np.int64) - first[pix]
    a, b = s // nx[pix], s % nx[pix]
    i, j = pix // wv, pix % wv
    v = i.astype(np.float64) + (2 * a + 1).astype(np.float64) / (2 * ny[pix]).astype(np.float64)
    u = j.astype(np.float64) + (2 * b + 1).astype(np.float64) / (2 * nx[pix]).astype(np.float64)
    big_y = (h[0] * v + h[1] * u) + h[2]
    big_x = (h[3] * v + h[4] * u) + h[5]
    d = (h[6] * v + h[7] * u) + h[8]
    return pix, big_y / d, big_x / d, fy[pix], fx[pix]


def box_mean(fine, ny, nx):
    """The resolve's mean of a fine render [..., ny Hv, nx Wv] float32 torch tensor over ny x nx boxes: added sequentially in fp32 in the
    order s = a nx + b, then times 1 / (ny nx)."""
    import torch
    hv, wv = fine.shape[-2] // ny, fine.shape[-1] // nx
    acc = torch.zeros(*fine.shape[:-2], hv, wv, dtype=torch.float32, device=fine.device)
    for a in range(ny):
        for b in range(nx):
            acc = acc + fine[..., a::ny, b::nx]
    return acc * (1.0 / (ny * nx))
