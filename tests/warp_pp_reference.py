"""The definition of a per-pixel warp (include/ciaosr_hip.h, "per-pixel warps") restated in numpy float64, one rounded operation per numpy
call: what tests/test_warp_pp_host.py and tests/test_warp_pp_gpu.py hold scene.py's helpers and the per-pixel warp kernels to.  The
positions, membership and frame coordinates are tests/warp_reference.py's."""
import numpy as np

from tests import warp_reference as wr


def raw_jacobian(h, hv, wv):
    """(g_y, g_x), each [hv * wv] float64: the norms of the rows of the Jacobian of the homography at every pixel centre, sqrt of the
    rounded sum of the rounded squares."""
    y, x = wr.lr_points(h, hv, wv)
    d = wr.denominators(h, hv, wv)
    h = [np.float64(c) for c in h]
    out = []
    for c, p in ((0, y), (3, x)):
        a = (h[c] - p * h[6]) / d
        b = (h[c + 1] - p * h[7]) / d
        out.append(np.sqrt(a * a + b * b))
    return out[0], out[1]


def _derivative(p, axis):
    """d p / d (grid step) along `axis` of p [hv, wv]: central where both neighbours lie in the grid and are finite, else one-sided with the
    one neighbour that does, else missing.  -> (derivative [hv, wv], defined [hv, wv] bool)."""
    p = np.moveaxis(p, axis, 0)
    nan_row = np.full((1, p.shape[1]), np.nan)
    before = np.concatenate([nan_row, p[:-1]], 0)                    # p[-1]; NaN outside the grid
    after = np.concatenate([p[1:], nan_row], 0)                      # p[+1]
    fb, fa = np.isfinite(before), np.isfinite(after)
    with np.errstate(invalid='ignore'):
        central = (after - before) * 0.5
        forward = after - p
        backward = p - before
    d = np.where(fb & fa, central, np.where(fa, forward, backward))
    return np.moveaxis(d, 0, axis), np.moveaxis(fb | fa, 0, axis)


def raw_differences(mp):
    """(g_y, g_x, has), each [hv * wv]: the differences source on the map mp [hv, wv, 2]; `has` False where the pixel has no footprint
    (g is NaN there)."""
    g, has = [], np.ones(mp.shape[:2], dtype=bool)
    for c in range(2):
        dv, ok_v = _derivative(mp[..., c], 0)
        du, ok_u = _derivative(mp[..., c], 1)
        has &= ok_v & ok_u
        with np.errstate(invalid='ignore'):
            g.append(np.sqrt(dv * dv + du * du))
    g = [np.where(has, v, np.nan).ravel() for v in g]
    return g[0], g[1], has.ravel()


def clamp(gy, gx, rng):
    """(f_y, f_x, has): min(max(g, lo), hi) per axis; a NaN component leaves the pixel without a footprint (both NaN)."""
    lo, hi = np.float64(rng[0]), np.float64(rng[1])
    has = ~(np.isnan(gy) | np.isnan(gx))
    with np.errstate(invalid='ignore'):
        fy = np.where(has, np.minimum(np.maximum(gy, lo), hi), np.nan)
        fx = np.where(has, np.minimum(np.maximum(gx, lo), hi), np.nan)
    return fy, fx, has


def cells_in(fy, fx, frame):
    """[n, 2] float32: the members' cells in the frame (y0, x0, th, tw)."""
    _, _, th, tw = frame
    return np.ascontiguousarray(np.stack([(fy * 2.0 / th).astype(np.float32), (fx * 2.0 / tw).astype(np.float32)], 1))
