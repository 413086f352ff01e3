"""The definition of a warp (include/ciaosr_hip.h, "warps") restated in numpy float64, one rounded operation per numpy call: what
tests/test_warp_host.py and tests/test_warp_gpu.py hold scene.py's helpers and the warp kernels to.  After the LR position a warp follows
the view's rule: membership and the frame coordinate are tests/view_reference.py's `members` and `coord_in`."""
import numpy as np

from tests import view_reference as vr

members, coord_in, edge_distance = vr.members, vr.coord_in, vr.edge_distance


def _centres(hv, wv):
    v = (np.arange(hv, dtype=np.float64) + 0.5).repeat(wv)
    u = np.tile(np.arange(wv, dtype=np.float64) + 0.5, hv)
    return v, u


def denominators(h, hv, wv):
    """D = (h20 v + h21 u) + h22 at the centres of the output pixels, [hv * wv] float64."""
    h = [np.float64(c) for c in h]
    v, u = _centres(hv, wv)
    return (h[6] * v + h[7] * u) + h[8]


def lr_points(h, hv, wv):
    """(y_lr, x_lr), each [hv * wv] float64, of the centres of the output pixels under the homography h, q = i * wv + j."""
    h = [np.float64(c) for c in h]
    v, u = _centres(hv, wv)
    big_y = (h[0] * v + h[1] * u) + h[2]
    big_x = (h[3] * v + h[4] * u) + h[5]
    d = (h[6] * v + h[7] * u) + h[8]
    return big_y / d, big_x / d


def footprint(h, v, u):
    """(f_y, f_x): the norms of the rows of the Jacobian of the homography at the output position (v, u)."""
    h = [np.float64(c) for c in h]
    v, u = np.float64(v), np.float64(u)
    d = (h[6] * v + h[7] * u) + h[8]
    y = ((h[0] * v + h[1] * u) + h[2]) / d
    x = ((h[3] * v + h[4] * u) + h[5]) / d
    return (float(np.hypot((h[0] - y * h[6]) / d, (h[1] - y * h[7]) / d)), float(np.hypot((h[3] - x * h[6]) / d, (h[4] - x * h[7]) / d)))


def centre_footprint(h, hv, wv):
    """The default footprint of a homography on an hv x wv output: at (v, u) = (hv / 2, wv / 2)."""
    return footprint(h, hv / 2.0, wv / 2.0)


def cell_in(fp, frame):
    """[2] float32: the warp's cell in the frame (y0, x0, th, tw)."""
    _, _, th, tw = frame
    return np.array([np.float32(np.float64(fp[0]) * 2.0 / th), np.float32(np.float64(fp[1]) * 2.0 / tw)], dtype=np.float32)


def max_scale(fp):
    return max(1.0 / fp[0], 1.0 / fp[1])


def radial_map(y, x, centre, k, hv, wv, nan_patch=None):
    """[hv, wv, 2] float64: the points (y, x) displaced radially about `centre` by the factor 1 + k r^2; `nan_patch` = (i0, j0, rows,
    columns) of output pixels set to NaN."""
    dy, dx = y - np.float64(centre[0]), x - np.float64(centre[1])
    f = 1.0 + np.float64(k) * (dy * dy + dx * dx)
    out = np.stack([np.float64(centre[0]) + dy * f, np.float64(centre[1]) + dx * f], 1).reshape(hv, wv, 2)
    if nan_patch is not None:
        i0, j0, n_i, n_j = nan_patch
        out[i0:i0 + n_i, j0:j0 + n_j] = np.nan
    return np.ascontiguousarray(out)
