"""The definition of an affine view (include/ciaosr_hip.h, "views") restated in numpy float64, one rounded operation per numpy call: what
tests/test_view_host.py and tests/test_view_gpu.py hold scene.py's helpers and the view kernels to."""
import numpy as np


def lr_points(m, hv, wv):
    """(y_lr, x_lr), each [hv * wv] float64, of the centres of the output pixels, q = i * wv + j."""
    m = [np.float64(v) for v in m]
    v = (np.arange(hv, dtype=np.float64) + 0.5).repeat(wv)
    u = np.tile(np.arange(wv, dtype=np.float64) + 0.5, hv)
    return (m[0] * v + m[1] * u) + m[2], (m[3] * v + m[4] * u) + m[5]


def members(y, x, frame):
    y0, x0, th, tw = frame
    return (y >= y0) & (y < y0 + th) & (x >= x0) & (x < x0 + tw)


def coord_in(y, x, frame):
    """[Q, 2] float32: the coordinate in the frame (y0, x0, th, tw), one rounding of the float64 value."""
    y0, x0, th, tw = (np.float64(v) for v in frame)
    return np.stack([(((y - y0) / th) * 2.0 - 1.0).astype(np.float32), (((x - x0) / tw) * 2.0 - 1.0).astype(np.float32)], 1)


def cell_in(m, frame):
    """[2] float32: the view's cell in the frame."""
    _, _, th, tw = frame
    return np.array([np.float32(np.hypot(np.float64(m[0]), np.float64(m[1])) * 2.0 / th),
                     np.float32(np.hypot(np.float64(m[3]), np.float64(m[4])) * 2.0 / tw)], dtype=np.float32)


def edge_distance(y, x, frames):
    """Smallest distance, in LR pixels, of any centre to any edge of any frame."""
    d = np.inf
    for y0, x0, th, tw in frames:
        for vals, edges in ((y, (y0, y0 + th)), (x, (x0, x0 + tw))):
            for e in edges:
                d = min(d, np.abs(vals - e).min())
    return d
