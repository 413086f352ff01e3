"""Encode once, render any scale or window: the host side of the persistent head scene (include/ciaosr_hip.h, "a persistent head scene").

Pure Python, no GPU: the window planner (which LR tiles a window of the HR grid touches, and which part of each), the least-recently-used
cache that bounds the bytes of tile scenes kept alive, the record `CiaoSR.encode` returns, and the affine views of
`CiaoSR.render_view` (their matrices, cells and tile lists, and `view_blocks_fit`: when a cut view may be queried in 4 x 2 blocks), the
warps of `CiaoSR.render_warp` (homographies and coordinate maps, their footprints and checks, the sample counts of `minify='area'`),
and for `CiaoSR.render_many` the target records `Grid` / `View` / `Warp` and the tile-major plan (`plan_union`, `group_missing`).  The
device work is in `PackedHead.prepare` / `query` (head_hip.py), `hip_ops.make_coord_cell_window` and the `hip_ops.view_*` / `warp_*` wrappers.
"""
import ctypes
import math
import numbers
from collections import OrderedDict

from . import tile_plan


def target_size(h, w, size=None, scale=None):
    """(Ht, Wt) of a render: `size` as given, else round(h * s), round(w * s) -- the reference's rule (ciaosr.py:166-169)."""
    if (size is None) == (scale is None):
        raise ValueError('give exactly one of size=(Ht, Wt) and scale')
    if size is not None:
        ht, wt = int(size[0]), int(size[1])
    else:
        ht, wt = round(h * scale), round(w * scale)
    if ht < 1 or wt < 1:
        raise ValueError(f'empty target grid {ht} x {wt}')
    return ht, wt


def check_window(ht, wt, window=None):
    """(i0, j0, h, w) in HR pixels, the whole grid by default; ValueError when it is empty or leaves the ht x wt grid."""
    if window is None:
        return 0, 0, ht, wt
    i0, j0, hh, ww = (int(v) for v in window)
    if hh < 1 or ww < 1 or i0 < 0 or j0 < 0 or i0 + hh > ht or j0 + ww > wt:
        raise ValueError(f'window (i0, j0, h, w) = {(i0, j0, hh, ww)} is empty or outside the {ht} x {wt} grid')
    return i0, j0, hh, ww


def plan_window(h, w, tile, overlap, ht, wt, window=None, scale=None, any_scale=False):
    """The LR tiles of an h x w image (the reference's tiling, ciaosr.py:227-234, row-major: its blend order) that a window of the ht x wt
    target touches.  Per touched tile a dict:
        index            position in the full row-major tile list
        y0, x0, th, tw   the LR tile
        a0, a1, b0, b1   rows [a0, a1) x columns [b0, b1) of the HR grid: the tile's HR rectangle intersected with the window
        grid             (Ht, Wt, i0, i1, j0, j1, frame): the arguments of hip_ops.make_coord_cell_window for that part
    any_scale = False: `clip_test`'s meaning -- (ht, wt) must be (h * scale, w * scale) for the integer `scale` (ValueError otherwise:
    `restore` cannot produce that image either); a tile's queries are the tile-local make_coord grid of (th * scale, tw * scale).
    any_scale = True: `tile_plan`'s -- HR pixels by centre membership, the global grid seen in the tile's frame."""
    wi0, wj0, wh, ww = check_window(ht, wt, window)
    wi1, wj1 = wi0 + wh, wj0 + ww
    tile = min(int(tile), h, w)
    overlap = int(overlap or 0)
    if any_scale:
        overlap = min(overlap, tile - 1)
    else:
        if scale is None or int(scale) != scale or (ht, wt) != (h * int(scale), w * int(scale)):
            raise ValueError(f'tiled rendering without test_cfg.tile_any_scale makes the ({h} * s) x ({w} * s) image of the integer '
                             f'test_cfg.scale only (asked: {ht} x {wt}, scale {scale})')
        scale = int(scale)
    ys, xs = tile_plan.tile_starts(h, tile, overlap), tile_plan.tile_starts(w, tile, overlap)

    def span(p0, n_lr, n_hr):
        return tile_plan.hr_span(p0, tile, n_lr, n_hr) if any_scale else (p0 * scale, (p0 + tile) * scale)

    out = []
    for ny, y0 in enumerate(ys):
        i0, i1 = span(y0, h, ht)
        a0, a1 = max(i0, wi0), min(i1, wi1)
        if a0 >= a1:
            continue
        for nx, x0 in enumerate(xs):
            j0, j1 = span(x0, w, wt)
            b0, b1 = max(j0, wj0), min(j1, wj1)
            if b0 >= b1:
                continue
            if any_scale:
                grid = (ht, wt, a0, a1, b0, b1, (h, y0, tile, w, x0, tile))
            else:
                grid = (tile * scale, tile * scale, a0 - i0, a1 - i0, b0 - j0, b1 - j0, None)
            out.append(dict(index=ny * len(xs) + nx, y0=y0, x0=x0, th=tile, tw=tile, a0=a0, a1=a1, b0=b0, b1=b1, grid=grid))
    return out


# ---- self-ensemble (include/ciaosr_hip.h, "self-ensemble") ---------------------------------------------------------------------------
# Member k in 0..7 is the model's answer for T_k(lq): k & 1 flips the columns, then k & 2 the rows, then k & 4 transposes the two axes;
# the answers are mapped back by U_k, the inverse, and averaged in member order (hip_ops.dihedral / dihedral_accum).
def dihedral_ids(value):
    """`self_ensemble` as a tuple of member ids: True -> (0, .., 7); a sequence of distinct ints in 0..7 -> itself, in its order;
    False / None -> None (off).  Anything else -- duplicates, an id outside 0..7, a string, a float, an empty sequence -- is a
    ValueError.  Pure host work: called before any device work."""
    if value is None or value is False:
        return None
    if value is True:
        return tuple(range(8))
    if isinstance(value, (str, bytes)) or not hasattr(value, '__iter__'):
        raise ValueError(f'self_ensemble is True (all eight members) or a sequence of distinct ids in 0..7, got {value!r}')
    ids = list(value)
    if not ids or any(isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 0 <= k <= 7 for k in ids) or len(set(ids)) != len(ids):
        raise ValueError(f'self_ensemble is True (all eight members) or a sequence of distinct ids in 0..7, got {value!r}')
    return tuple(int(k) for k in ids)


def dihedral_window(k, ht, wt, window=None):
    """The window (i0, j0, hh, ww) of an ht x wt grid as member k sees it: -> (ht_k, wt_k, window_k) with
    U_k(T_k(A)[window_k]) == A[window] for every A [ht, wt].  Column flip: j0' = wt - j0 - ww; row flip: i0' = ht - i0 - hh;
    transpose: both pairs swapped.  `window` None: the whole grid."""
    i0, j0, hh, ww = check_window(ht, wt, window)
    if k & 1:
        j0 = wt - j0 - ww
    if k & 2:
        i0 = ht - i0 - hh
    if k & 4:
        return wt, ht, (j0, i0, ww, hh)
    return ht, wt, (i0, j0, hh, ww)


# ---- affine views (include/ciaosr_hip.h, "views") ------------------------------------------------------------------------------------
# A view is an output grid Hv x Wv and m = (m_yy, m_yx, t_y, m_xy, m_xx, t_x), y first: output pixel (i, j), centre v = i + 0.5,
# u = j + 0.5, looks at y_lr = (m_yy v + m_yx u) + t_y, x_lr = (m_xy v + m_xx u) + t_x in LR pixel units (the image is [0, h) x [0, w),
# LR pixel k has its centre at k + 0.5), fp64, every operation rounded on its own.
_QUARTER_TURNS = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}


def view_matrix(center, zoom, angle_deg, size):
    """The matrix of the Hv x Wv view (`size`) whose centre (v, u) = (Hv / 2, Wv / 2) looks at `center` = (cy, cx), LR pixel units,
    with `zoom` output pixels per LR pixel, turned by `angle_deg`:
        y_lr - cy = (cos a (v - Hv / 2) - sin a (u - Wv / 2)) / zoom
        x_lr - cx = (sin a (v - Hv / 2) + cos a (u - Wv / 2)) / zoom
    -- the rotation matrix [[cos, -sin], [sin, cos]] on (v, u), y first.  Sign: a positive angle turns the picture clockwise on the
    screen (the camera counter-clockwise).  At 90 degrees the view's top-left corner shows the image's bottom-left, and walking right
    in the view walks up the image; -32 degrees straightens a picture that hangs 32 degrees clockwise.  Multiples of 90 degrees use exact
    0 / +-1 for cos / sin, so the entries are exactly 0 or +-1 / zoom."""
    cy, cx = (float(v) for v in center)
    hv, wv = int(size[0]), int(size[1])
    zoom = float(zoom)
    if not (zoom > 0 and math.isfinite(zoom)) or hv < 1 or wv < 1:
        raise ValueError(f'view_matrix needs zoom > 0 and a grid of at least 1 x 1 (zoom {zoom}, size {hv} x {wv})')
    turn = math.fmod(float(angle_deg), 360.0) % 360.0
    c, s = _QUARTER_TURNS.get(turn) or (math.cos(math.radians(turn)), math.sin(math.radians(turn)))
    inv = 1.0 / zoom
    myy, myx, mxy, mxx = c * inv + 0.0, -s * inv + 0.0, s * inv + 0.0, c * inv + 0.0
    return (myy, myx, cy - (myy * (hv / 2.0) + myx * (wv / 2.0)), mxy, mxx, cx - (mxy * (hv / 2.0) + mxx * (wv / 2.0)))


def view_of_window(h, w, ht, wt, window=None):
    """(matrix, (Hv, Wv)) of the axis-aligned view that looks at the window (i0, j0, hh, ww) of the ht x wt target grid of an h x w image
    (default: the whole grid): what `render(enc, size=(ht, wt), window=window)` shows.  Not bitwise that render: its coordinates round
    three times in fp32 (make_coord), a view's once from fp64; the two differ by at most 2^-22."""
    i0, j0, hh, ww = check_window(ht, wt, window)
    sy, sx = h / ht, w / wt
    return (sy, 0.0, i0 * sy, 0.0, sx, j0 * sx), (hh, ww)


def _f32(v):
    return ctypes.c_float(v).value


def view_cell(matrix, th, tw):
    """(cell_y, cell_x) of a view in a th x tw frame, the fp32 values the kernels write: hypot(row) * 2 / t -- the norm of a matrix row is
    the extent of an output pixel along that LR axis, so this is make_cell's 2 / Ht for an axis-aligned view and does not change under
    rotation.  ValueError for a singular (or non-finite) matrix and for a cell component >= 1: the reference divides by 1 - cell."""
    m = [float(v) for v in matrix]
    if len(m) != 6 or not all(math.isfinite(v) for v in m):
        raise ValueError(f'a view matrix is six finite numbers (m_yy, m_yx, t_y, m_xy, m_xx, t_x), got {matrix!r}')
    if m[0] * m[4] - m[1] * m[3] == 0.0:
        raise ValueError(f'singular view matrix {tuple(m)}: the view collapses onto a line or a point of the image')
    cell = (_f32(math.hypot(m[0], m[1]) * 2.0 / th), _f32(math.hypot(m[3], m[4]) * 2.0 / tw))
    if max(cell) >= 1.0:
        raise ValueError(f'view cell {cell} >= 1 in a {th} x {tw} frame: an output pixel may span less than half the frame '
                         f'(the reference divides by 1 - cell)')
    return cell


def view_max_scale(matrix):
    """Output pixels per LR pixel along the finer of the two LR axes: what `encode`'s max_scale is set to by a first view render."""
    return max(1.0 / math.hypot(matrix[0], matrix[1]), 1.0 / math.hypot(matrix[3], matrix[4]))


def view_blocks_fit(matrix):
    """Whether every 4 wide x 2 high block of output pixels of the view is a row tile the chained 16-bit head kernel answers on its own:
    3 |m_yx| + |m_yy| <= 2 and 3 |m_xx| + |m_xy| <= 2.  The eight pixel centres of a block span 3 steps of u and 1 of v, so at most
    that many LR pixels along each LR axis; the key samples sit within the same +-0.5 LR pixel of their query, so keys that lie no more
    than 2 apart round into at most 4 distinct rows (columns): the kernel's 4 x 4 gather window.  True at any angle from
    zoom 1.6 up (the worst angle is atan(1 / 3): sqrt(10) / zoom <= 2).  What `test_cfg.view_blocks` asks before it selects in blocks."""
    m = [float(v) for v in matrix]
    return 3.0 * abs(m[1]) + abs(m[0]) <= 2.0 and 3.0 * abs(m[4]) + abs(m[3]) <= 2.0


def plan_view(h, w, tile=None, overlap=None, any_scale=False):
    """The frames (y0, x0, th, tw) a view of an h x w image is sorted into, row-major (the reference's blend order): the whole image
    without `tile`, else the reference's LR tiling (`plan_window`'s).  A query belongs to every frame its LR position lies in -- 1, 2 or
    4 with overlapping tiles.  Tiled views need `tile_any_scale`: `clip_test`'s integer-scale HR rectangles mean nothing under a
    rotation or a fractional pan."""
    if not tile:
        return [(0, 0, h, w)]
    if not any_scale:
        raise ValueError(f'tiled rendering without test_cfg.tile_any_scale makes the ({h} * s) x ({w} * s) image of the integer '
                         f'test_cfg.scale only (asked: an affine view)')
    tile = min(int(tile), h, w)
    overlap = min(int(overlap or 0), tile - 1)
    return [(y0, x0, tile, tile) for y0 in tile_plan.tile_starts(h, tile, overlap) for x0 in tile_plan.tile_starts(w, tile, overlap)]


def check_view(matrix, size, fill, h, w, tile=None, overlap=None, any_scale=False):
    """The arguments of a view render, checked in `CiaoSR.render_view`'s order: -> (m, (hv, wv), fill3, frames) with m six floats, fill3
    three floats in [0, 1] and frames = `plan_view`'s list.  ValueError for an empty grid, tiles without `tile_any_scale`, a singular
    matrix, a cell >= 1 and a fill outside [0, 1]."""
    hv, wv = int(size[0]), int(size[1])
    if hv < 1 or wv < 1:
        raise ValueError(f'empty view grid {hv} x {wv}')
    m = tuple(float(v) for v in matrix)
    frames = plan_view(h, w, tile, overlap, any_scale)
    view_cell(m, frames[0][2], frames[0][3])                      # ValueError: singular, or a cell >= 1
    fill = tuple(float(v) for v in fill) if hasattr(fill, '__len__') else (float(fill),) * 3
    if len(fill) != 3 or not all(0.0 <= v <= 1.0 for v in fill):
        raise ValueError(f'fill is one number or three in [0, 1], got {fill}')
    return m, (hv, wv), fill, frames


# ---- warps (include/ciaosr_hip.h, "warps") -------------------------------------------------------------------------------------------
# A warp is an output grid Hv x Wv, a point source that gives every output pixel (i, j) an LR position (y_lr, x_lr) in the views' LR pixel
# units, and ONE footprint (f_y, f_x): the LR extent of an output pixel along each LR axis.  Two point sources.  A homography
# h = (h00, h01, h02, h10, h11, h12, h20, h21, h22), y first: with v = i + 0.5, u = j + 0.5, in fp64, every operation rounded on its own,
#     Y = (h00 v + h01 u) + h02,  X = (h10 v + h11 u) + h12,  D = (h20 v + h21 u) + h22,  y_lr = Y / D,  x_lr = X / D
# -- a view's position, bit for bit, when the last row is (0, 0, 1).  Or a map: a device tensor [Hv, Wv, 2] of (y_lr, x_lr).  After the
# position everything is the view's rule: membership, frame coordinate, tile plan, blend order, fill.  The footprint is what reaches the
# model (the cell, and through it the shift radius): ONE per warp, so a warp whose local scale varies strongly over the output -- strong
# perspective -- should be cut into several warps by the caller, or rendered as a per-pixel warp (below).
def homography_of_view(matrix):
    """The nine numbers of an affine view: its two rows and (0, 0, 1).  The warp of it is `render_view` of the matrix, bit for bit."""
    m = [float(v) for v in matrix]
    if len(m) != 6:
        raise ValueError(f'a view matrix is six numbers (m_yy, m_yx, t_y, m_xy, m_xx, t_x), got {matrix!r}')
    return (*m, 0.0, 0.0, 1.0)


def homography_from_points(out_pts4, lr_pts4):
    """The homography (h22 = 1) that takes the four output-pixel positions `out_pts4` = [(v, u)] * 4 (pixel (i, j) has its centre at
    (i + 0.5, j + 0.5); the corners of an Hv x Wv output are (0, 0), (0, Wv), (Hv, Wv), (Hv, 0)) to the four LR positions `lr_pts4` =
    [(y, x)] * 4: one float64 solve of the 8 x 8 system.  ValueError when the points do not determine it (three on a line)."""
    import numpy as np
    src, dst = np.asarray(out_pts4, dtype=np.float64), np.asarray(lr_pts4, dtype=np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2) or not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError('homography_from_points takes four finite (v, u) output positions and four finite (y, x) LR positions')
    a, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((v, u), (y, x)) in enumerate(zip(src, dst)):
        a[2 * k] = (v, u, 1.0, 0.0, 0.0, 0.0, -y * v, -y * u)
        a[2 * k + 1] = (0.0, 0.0, 0.0, v, u, 1.0, -x * v, -x * u)
        b[2 * k], b[2 * k + 1] = y, x
    try:
        sol = np.linalg.solve(a, b)
    except np.linalg.LinAlgError:
        raise ValueError('homography_from_points: the four point pairs do not determine a homography (three points on a line?)') from None
    if not np.isfinite(sol).all():
        raise ValueError('homography_from_points: the four point pairs do not determine a homography (three points on a line?)')
    return (*(float(v) for v in sol), 1.0)


def _h9(homography):
    h = tuple(float(v) for v in homography)
    if len(h) != 9 or not all(math.isfinite(v) for v in h):
        raise ValueError(f'a homography is nine finite numbers (h00, h01, h02, h10, h11, h12, h20, h21, h22), got {homography!r}')
    return h


def warp_footprint(homography, size):
    """The default footprint (f_y, f_x) of a homography on an Hv x Wv (`size`) output: the norms of the rows of its Jacobian at the
    output centre (v, u) = (Hv / 2, Wv / 2), fp64:
        J_yv = (h00 - y h20) / D, J_yu = (h01 - y h21) / D, f_y = hypot(J_yv, J_yu); likewise x.
    With the last row (0, 0, 1) exactly hypot(m_yy, m_yx), hypot(m_xy, m_xx): the cell is then bitwise the view's."""
    h = _h9(homography)
    v, u = int(size[0]) / 2.0, int(size[1]) / 2.0
    d = (h[6] * v + h[7] * u) + h[8]
    if not d > 0.0:
        raise ValueError(f'homography denominator {d} <= 0 at the output centre: the horizon crosses the output')
    y, x = ((h[0] * v + h[1] * u) + h[2]) / d, ((h[3] * v + h[4] * u) + h[5]) / d
    return (math.hypot((h[0] - y * h[6]) / d, (h[1] - y * h[7]) / d), math.hypot((h[3] - x * h[6]) / d, (h[4] - x * h[7]) / d))


def _footprint(footprint):
    try:
        fp = tuple(float(v) for v in footprint)
    except TypeError:
        fp = ()
    if len(fp) != 2 or not all(math.isfinite(v) and v > 0.0 for v in fp):
        raise ValueError(f'a footprint is two finite positive numbers (f_y, f_x): the LR extent of an output pixel, got {footprint!r}')
    return fp


def warp_cell(footprint, th, tw):
    """(cell_y, cell_x) of a warp in a th x tw frame, the fp32 values the kernels write: f * 2 / t, `view_cell`'s operations.  ValueError
    for a footprint that is not finite and positive and for a cell component >= 1 (the reference divides by 1 - cell)."""
    fp = _footprint(footprint)
    cell = (_f32(fp[0] * 2.0 / th), _f32(fp[1] * 2.0 / tw))
    if max(cell) >= 1.0:
        raise ValueError(f'warp cell {cell} >= 1 in a {th} x {tw} frame: an output pixel may span less than half the frame '
                         f'(the reference divides by 1 - cell)')
    return cell


def warp_max_scale(footprint):
    """Output pixels per LR pixel along the finer of the two LR axes: what `encode`'s max_scale is set to by a first warp render
    (`view_max_scale`'s value when the warp is affine)."""
    fp = _footprint(footprint)
    return max(1.0 / fp[0], 1.0 / fp[1])


def map_footprint(map):
    """A footprint for a coordinate map [Hv, Wv, 2] from central differences at its centre pixel (i, j) = (Hv // 2, Wv // 2):
    f_y = hypot(dy/dv, dy/du), f_x = hypot(dx/dv, dx/du), one-sided where the centre lies on the border of the grid.  Costs ONE small
    device-to-host copy (the centre's 3 x 3 neighbourhood), which synchronises: call it once per map, not per render.  ValueError where
    the neighbourhood is not finite or the differences vanish -- give the footprint yourself then."""
    shape = tuple(map.shape)
    if len(shape) != 3 or shape[2] != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f'a warp map is [Hv, Wv, 2] of (y_lr, x_lr), got {shape}')
    ci, cj = shape[0] // 2, shape[1] // 2
    i0, i1, j0, j1 = max(ci - 1, 0), min(ci + 1, shape[0] - 1), max(cj - 1, 0), min(cj + 1, shape[1] - 1)
    nb = map[i0:i1 + 1, j0:j1 + 1].cpu().double().tolist()             # the one copy
    out = []
    for c in range(2):
        dv = (nb[i1 - i0][cj - j0][c] - nb[0][cj - j0][c]) / (i1 - i0) if i1 > i0 else 0.0
        du = (nb[ci - i0][j1 - j0][c] - nb[ci - i0][0][c]) / (j1 - j0) if j1 > j0 else 0.0
        out.append(math.hypot(dv, du))
    if not all(math.isfinite(v) and v > 0.0 for v in out):
        raise ValueError(f'map_footprint: the central differences at pixel {(ci, cj)} give {tuple(out)}; pass footprint=(f_y, f_x)')
    return tuple(out)


# ---- per-pixel warps (include/ciaosr_hip.h, "per-pixel warps") -----------------------------------------------------------------------
# A per-pixel warp is a warp whose footprint is a function of the output pixel.  Positions, membership, frame coordinates, tile plan,
# blend, `fill`, `as_u8` / `as_u16` / grey / RGBA, and the one device-to-host copy are the existing warp's, unchanged.  The raw footprint
# (g_y, g_x) of output pixel (i, j) is computed in fp64, every operation rounded on its own, from one of three sources: the Jacobian of
# the homography (`footprint='per-pixel'`): g_y = sqrt(a a + b b), a = (h00 - y_lr h20) / D, b = (h01 - y_lr h21) / D, g_x likewise with
# h10, h11, x_lr; differences of the map (`footprint='per-pixel'`): central where both neighbours lie in the grid and are finite, else
# one-sided, else the pixel has no footprint; or a device tensor [Hv, Wv, 2] of (g_y, g_x).  Clamp: f = min(max(g, lo), hi) per axis with
# `footprint_range=(lo, hi)`, default hi = 1.0 (no minification: the model was never trained below x1) and lo = 1 / M, M = the encode's
# max_scale when it is set, else what `encode` would default it to (`test_cfg`'s scale).  A NaN component, or no footprint, makes the pixel
# a non-member: it holds `fill` and A = 0, exactly as a NaN position does; +inf clamps to hi.  The cell of a member in a th x tw frame is
# fp32(f_y 2 / th), fp32(f_x 2 / tw); the warp's max_scale is 1 / lo; the head is queried with chunk = 1, so the shift radius of a query
# comes from its own cell.  A per-pixel warp whose footprints happen to be constant is the single-footprint warp of that constant.
FP_JACOBIAN, FP_DIFFERENCES, FP_TENSOR = 1, 2, 3


class PerPixel:
    """The resolved footprint of a per-pixel warp: `mode` (FP_JACOBIAN, FP_DIFFERENCES or FP_TENSOR), `range` = (lo, hi) and, in mode
    FP_TENSOR, the caller's `tensor` [Hv, Wv, 2].  `samples`: 0, or the `max_samples` of an area-sampled warp (`minify='area'`)."""
    __slots__ = ('mode', 'range', 'tensor', 'samples')

    def __init__(self, mode, range, tensor=None, samples=0):
        self.mode, self.range, self.tensor, self.samples = mode, range, tensor, samples

    def __repr__(self):
        area = f', samples={self.samples}' if self.samples else ''
        return f'PerPixel(mode={self.mode}, range={self.range!r}{area})'


def resolve_range(range=None, max_scale=None):
    """(lo, hi) of a per-pixel warp: `range`, two finite doubles 0 < lo <= hi, default (1 / max_scale, 1.0)."""
    if range is None:
        if max_scale is None or not (math.isfinite(float(max_scale)) and float(max_scale) >= 1.0):
            raise ValueError(f'a per-pixel footprint needs footprint_range=(lo, hi): the default lo = 1 / max_scale needs the encode\'s '
                             f'max_scale or test_cfg.scale (>= 1), got {max_scale!r}')
        return (1.0 / float(max_scale), 1.0)
    try:
        rg = tuple(float(v) for v in range)
    except (TypeError, ValueError):
        rg = ()
    if len(rg) != 2 or not all(math.isfinite(v) for v in rg) or not 0.0 < rg[0] <= rg[1]:
        raise ValueError(f'footprint_range is (lo, hi), two finite numbers with 0 < lo <= hi, got {range!r}')
    return rg


def _per_pixel(footprint, range_, max_scale, has_map, hv, wv, frame):
    """`check_warp`'s per-pixel branch: -> PerPixel.  `footprint`: 'per-pixel' or a tensor."""
    if isinstance(footprint, str):
        if footprint != 'per-pixel':
            raise ValueError(f"footprint is (f_y, f_x), 'per-pixel' or a device tensor [Hv, Wv, 2], got {footprint!r}")
        if has_map and (hv < 2 or wv < 2):
            raise ValueError(f'a per-pixel footprint from the differences of a map needs two pixels along each grid axis, got {hv} x {wv}')
        mode, tensor = (FP_DIFFERENCES if has_map else FP_JACOBIAN), None
    else:
        shape = tuple(footprint.shape)
        if shape != (hv, wv, 2) or str(footprint.dtype) not in ('torch.float64', 'torch.float32'):
            raise ValueError(f'a footprint tensor is a float64 (or float32) tensor [Hv, Wv, 2] = [{hv}, {wv}, 2] of (g_y, g_x), got '
                             f'{footprint.dtype} {shape}')
        if not footprint.is_cuda:
            from ._lib import CiaoSRHipError
            raise CiaoSRHipError('a footprint tensor lives on the MI355X: got a CPU tensor (no CPU fallback; move it to cuda)')
        mode, tensor = FP_TENSOR, footprint
    lo, hi = resolve_range(range_, max_scale)
    cell = (_f32(hi * 2.0 / frame[2]), _f32(hi * 2.0 / frame[3]))
    if max(cell) >= 1.0:
        raise ValueError(f'warp cell {cell} >= 1 at the upper end hi = {hi} of footprint_range in a {frame[2]} x {frame[3]} frame: an '
                         f'output pixel may span less than half the frame (the reference divides by 1 - cell)')
    return PerPixel(mode, (lo, hi), tensor)


def warp_footprints(homography, size, footprint_range):
    """The clamped per-pixel footprints of a homography on an Hv x Wv (`size`) output, [Hv, Wv, 2] float64 on the host: the definition
    above restated in plain Python doubles, one rounded operation at a time -- what `hip_ops.warp_footprints` computes on the device,
    bit for bit.  For small grids and for checks: NOT a fast path (a Python loop over the pixels)."""
    import torch
    h = _h9(homography)
    hv, wv = int(size[0]), int(size[1])
    lo, hi = resolve_range(footprint_range)
    out = []
    for i in range(hv):
        for j in range(wv):
            v, u = i + 0.5, j + 0.5
            d = (h[6] * v + h[7] * u) + h[8]
            y, x = ((h[0] * v + h[1] * u) + h[2]) / d, ((h[3] * v + h[4] * u) + h[5]) / d
            for c, p in ((0, y), (3, x)):
                a, b = (h[c] - p * h[6]) / d, (h[c + 1] - p * h[7]) / d
                g = math.sqrt(a * a + b * b)
                out.append(g if g != g else min(max(g, lo), hi))
    return torch.tensor(out, dtype=torch.float64).view(hv, wv, 2)


# ---- area-sampled warps (include/ciaosr_hip.h, "area-sampled warps") -------------------------------------------------------------------
# `minify='area'` on a per-pixel homography warp: where the raw footprint g of an output pixel exceeds hi, the pixel is answered by
# n_y x n_x point samples spread over it, n = `area_samples(g, hi, N)` per axis with N = `max_samples`, each with the footprint
# f = min(max(g / n, lo), hi), and holds the mean of their finished values (the box filter).  Sample s = a n_x + b of pixel (i, j) sits at
# v = i + (2a + 1) / (2 n_y), u = j + (2b + 1) / (2 n_x); its LR position is the homography's formula there; membership, frame coordinate
# and cell follow the warp's rules per sample.  Sample ids run through the pixels in row-major order (`first` = the exclusive prefix sum of
# n_y n_x, S the total); a pixel whose raw footprint has a NaN component has no samples and holds `fill`.  Where g > N hi the pixel stays
# under-sampled (f = hi).  `minify='clamp'`, the default, is the per-pixel warp as it was.
MAX_SAMPLES = (1, 2, 4, 8)
INT_MAX = 2 ** 31 - 1


def area_samples(g, hi, max_samples):
    """Samples per axis of a pixel whose raw footprint along the axis is `g`: n = 1; while n < max_samples and g > hi n: n = 2 n.  A
    footprint of exactly hi n stays at n; +inf gives max_samples; NaN gives 0 (the pixel has no samples)."""
    g, hi, n_max = float(g), float(hi), int(max_samples)
    if g != g:
        return 0
    n = 1
    while n < n_max and g > hi * n:
        n *= 2
    return n


def check_minify(minify='clamp', max_samples=4):
    """-> 0 for 'clamp', `max_samples` for 'area'.  ValueError for another `minify` and for a `max_samples` outside 1, 2, 4, 8."""
    if minify not in ('clamp', 'area'):
        raise ValueError(f"minify is 'clamp' (a footprint above the range is clamped: one query per pixel) or 'area' (supersample where "
                         f"the warp minifies), got {minify!r}")
    if isinstance(max_samples, bool) or max_samples not in MAX_SAMPLES:
        raise ValueError(f'max_samples is one of {MAX_SAMPLES} (samples per axis and pixel, a power of two), got {max_samples!r}')
    return int(max_samples) if minify == 'area' else 0


def warp_area_table(homography, size, footprint_range, max_samples, tensor=None):
    """The sample table of an area-sampled homography warp on an Hv x Wv (`size`) output, in plain Python doubles: -> (first, n, f) with
    first a list of Hv Wv + 1 ints, n a list of (n_y, n_x) -- (0, 0) without samples -- and f a list of the samples' (f_y, f_x) or None,
    per pixel in row-major order -- what `hip_ops.warp_area_table` computes on the device.  `tensor`: the raw footprints as nested lists
    [Hv][Wv][2] (default: the Jacobian).  For small grids and for checks: a Python loop over the pixels."""
    h = _h9(homography)
    hv, wv = int(size[0]), int(size[1])
    lo, hi = resolve_range(footprint_range)
    n_max = check_minify('area', max_samples)
    first, ns, fs = [0], [], []
    for i in range(hv):
        for j in range(wv):
            if tensor is not None:
                g = [float(tensor[i][j][0]), float(tensor[i][j][1])]
            else:
                v, u = i + 0.5, j + 0.5
                d = (h[6] * v + h[7] * u) + h[8]
                y, x = ((h[0] * v + h[1] * u) + h[2]) / d, ((h[3] * v + h[4] * u) + h[5]) / d
                g = []
                for c, p in ((0, y), (3, x)):
                    a, b = (h[c] - p * h[6]) / d, (h[c + 1] - p * h[7]) / d
                    g.append(math.sqrt(a * a + b * b))
            n = (area_samples(g[0], hi, n_max), area_samples(g[1], hi, n_max))
            if 0 in n:
                n = (0, 0)
            ns.append(n)
            fs.append(None if n == (0, 0) else tuple(min(max(gc / nc, lo), hi) for gc, nc in zip(g, n)))
            first.append(first[-1] + n[0] * n[1])
    return first, ns, fs


def check_warp(homography, map, size, footprint, fill, h, w, tile=None, overlap=None, any_scale=False, footprint_range=None,
               max_scale=None, minify='clamp', max_samples=4):
    """The arguments of a warp render, checked in `CiaoSR.render_warp`'s order, all on the host: -> (h9 or None, map or None, (hv, wv),
    (f_y, f_x), fill3, frames) with frames = `plan_view`'s list.  ValueError for: not exactly one point source; an empty grid; tiles
    without `tile_any_scale`; a non-finite homography entry; a denominator <= 0 at a corner (0, 0), (Hv, 0), (0, Wv), (Hv, Wv) of the grid
    (D is affine in (v, u): positive corners mean positive everywhere -- the horizon must not cross the output); a map that is not a
    float64 / float32 tensor [Hv, Wv, 2]; a map without a footprint; a footprint that is not finite and positive; a cell >= 1; a fill
    outside [0, 1].  A map on the host is a CiaoSRHipError: there is no CPU fallback.
    `footprint` = 'per-pixel' or a device tensor [Hv, Wv, 2] makes a per-pixel warp: the fourth result is then a `PerPixel` record with
    `footprint_range` resolved (default (1 / `max_scale`, 1.0), `max_scale` = the encode's or `test_cfg.scale`).  ValueError as well for:
    an unknown string; a tensor of the wrong shape or dtype; `footprint_range` without a per-pixel footprint; a range that is not
    0 < lo <= hi and finite; an upper end whose cell is >= 1; differences on a grid axis of length 1.  A host tensor is a CiaoSRHipError.
    `minify='area'` with `max_samples` = N makes it an area-sampled warp (`PerPixel.samples` = N).  ValueError as well for: a `minify`
    that is neither 'clamp' nor 'area'; N outside 1, 2, 4, 8; 'area' with a single footprint (given or defaulted) or with a map (the
    sub-pixel positions of a map would need an interpolation rule); Hv Wv N N > 2^31 - 1."""
    samples = check_minify(minify, max_samples)
    per_pixel = isinstance(footprint, str) or (hasattr(footprint, 'shape') and hasattr(footprint, 'dtype') and tuple(footprint.shape) != (2,))
    if footprint_range is not None and not per_pixel:
        raise ValueError("footprint_range=(lo, hi) clamps a per-pixel footprint: give footprint='per-pixel' or a footprint tensor with it")
    if samples and not per_pixel:
        raise ValueError("minify='area' supersamples a per-pixel warp: give footprint='per-pixel' or a footprint tensor with it (one "
                         "footprint for the whole warp says nothing about where it minifies)")
    if (homography is None) == (map is None):
        raise ValueError('a warp has exactly one point source: give homography=(nine numbers) or map=(device tensor [Hv, Wv, 2])')
    if samples and map is not None:
        raise ValueError("minify='area' needs a homography: the sub-pixel positions of a map would need an interpolation rule")
    if map is not None:
        shape = tuple(getattr(map, 'shape', ()))
        if len(shape) != 3 or shape[2] != 2 or str(getattr(map, 'dtype', None)) not in ('torch.float64', 'torch.float32'):
            raise ValueError(f'a warp map is a float64 (or float32) tensor [Hv, Wv, 2] of (y_lr, x_lr), got '
                             f'{getattr(map, "dtype", type(map).__name__)} {shape}')
        if size is None:
            size = shape[:2]
    if size is None:
        raise ValueError('a homography warp needs size=(Hv, Wv)')
    hv, wv = int(size[0]), int(size[1])
    if hv < 1 or wv < 1:
        raise ValueError(f'empty warp grid {hv} x {wv}')
    if samples and hv * wv * samples * samples > INT_MAX:
        raise ValueError(f"minify='area': {hv} x {wv} pixels of up to {samples} x {samples} samples are more than 2^31 - 1 samples")
    frames = plan_view(h, w, tile, overlap, any_scale)
    if map is not None:
        if shape[:2] != (hv, wv):
            raise ValueError(f'a warp map is [Hv, Wv, 2] = [{hv}, {wv}, 2] for size {(hv, wv)}, got {shape}')
        if not map.is_cuda:
            from ._lib import CiaoSRHipError
            raise CiaoSRHipError('a warp map lives on the MI355X: got a CPU tensor (no CPU fallback; move the map to cuda)')
        if footprint is None:
            raise ValueError('a map warp needs footprint=(f_y, f_x), the LR extent of an output pixel (scene.map_footprint(map) offers one)')
        h9 = None
    else:
        h9 = _h9(homography)
        for v, u in ((0.0, 0.0), (float(hv), 0.0), (0.0, float(wv)), (float(hv), float(wv))):
            d = (h9[6] * v + h9[7] * u) + h9[8]
            if not d > 0.0:
                raise ValueError(f'homography denominator {d} <= 0 at the grid corner (v, u) = {(v, u)}: the horizon must not cross '
                                 f'the {hv} x {wv} output')
        if footprint is None:
            footprint = warp_footprint(h9, (hv, wv))
    if per_pixel:
        fp = _per_pixel(footprint, footprint_range, max_scale, map is not None, hv, wv, frames[0])
        fp.samples = samples
    else:
        fp = _footprint(footprint)
        warp_cell(fp, frames[0][2], frames[0][3])                 # ValueError: a cell >= 1
    fill = tuple(float(v) for v in fill) if hasattr(fill, '__len__') else (float(fill),) * 3
    if len(fill) != 3 or not all(0.0 <= v <= 1.0 for v in fill):
        raise ValueError(f'fill is one number or three in [0, 1], got {fill}')
    return h9, map, (hv, wv), fp, fill, frames


# ---- many targets from one walk over the tiles (CiaoSR.render_many / prefetch) --------------------------------------------------------
class Grid:
    """One target of `CiaoSR.render_many`: the arguments of `CiaoSR.render`."""
    __slots__ = ('size', 'scale', 'window')

    def __init__(self, size=None, scale=None, window=None):
        self.size, self.scale, self.window = size, scale, window

    def resolve(self, h, w):
        """(ht, wt, (i0, j0, hh, ww)) on an h x w image, with `render`'s ValueErrors."""
        ht, wt = target_size(h, w, self.size, self.scale)
        return ht, wt, check_window(ht, wt, self.window)

    def __repr__(self):
        return f'Grid(size={self.size!r}, scale={self.scale!r}, window={self.window!r})'


class View:
    """One target of `CiaoSR.render_many`: the arguments of `CiaoSR.render_view`."""
    __slots__ = ('matrix', 'size', 'fill')

    def __init__(self, matrix, size, fill=0.0):
        self.matrix, self.size, self.fill = matrix, size, fill

    def resolve(self, h, w, tile=None, overlap=None, any_scale=False):
        """`check_view` of the record: (m, (hv, wv), fill3, frames), with `render_view`'s ValueErrors."""
        return check_view(self.matrix, self.size, self.fill, h, w, tile, overlap, any_scale)

    def __repr__(self):
        return f'View({self.matrix!r}, size={self.size!r}, fill={self.fill!r})'


class Warp:
    """One target of `CiaoSR.render_many`: the arguments of `CiaoSR.render_warp`."""
    __slots__ = ('homography', 'map', 'size', 'footprint', 'fill', 'footprint_range', 'minify', 'max_samples')

    def __init__(self, homography=None, map=None, size=None, footprint=None, fill=0.0, footprint_range=None, minify='clamp',
                 max_samples=4):
        self.homography, self.map, self.size, self.footprint, self.fill = homography, map, size, footprint, fill
        self.footprint_range, self.minify, self.max_samples = footprint_range, minify, max_samples

    def resolve(self, h, w, tile=None, overlap=None, any_scale=False, max_scale=None):
        """`check_warp` of the record: (h9 or None, map or None, (hv, wv), footprint, fill3, frames), with `render_warp`'s errors; the
        footprint is (f_y, f_x) or, for a per-pixel warp, a `PerPixel` record (`max_scale`: the default of its range)."""
        return check_warp(self.homography, self.map, self.size, self.footprint, self.fill, h, w, tile, overlap, any_scale,
                          self.footprint_range, max_scale, self.minify, self.max_samples)

    def __repr__(self):
        source = f'homography={self.homography!r}' if self.map is None else f'map=<{tuple(getattr(self.map, "shape", ()))}>'
        fp = self.footprint if not hasattr(self.footprint, 'shape') else f'<{tuple(self.footprint.shape)}>'
        rg = '' if self.footprint_range is None else f', footprint_range={self.footprint_range!r}'
        if self.minify != 'clamp':
            rg += f', minify={self.minify!r}, max_samples={self.max_samples!r}'
        return f'Warp({source}, size={self.size!r}, footprint={fp!r}{rg}, fill={self.fill!r})'


def plan_union(touched):
    """touched[k]: the tile indices target k touches.  -> (union, users): the union in ascending (row-major) index order, and per tile
    of it the targets that touch it, in list order.  Walking the union and serving users[tile] shows every target its own tiles in
    ascending order: the reference's blend order."""
    users = {}
    for k, tiles in enumerate(touched):
        for t in tiles:
            users.setdefault(int(t), [])
            if k not in users[int(t)]:
                users[int(t)].append(k)
    union = sorted(users)
    return union, {t: users[t] for t in union}


def group_missing(union, cached, n):
    """The tiles of `union` (in its order) that are not in `cached`, cut into groups of `n` consecutive missing tiles (the last group may
    be shorter): what one trunk call encodes."""
    n = max(1, int(n))
    missing = [t for t in union if t not in cached]
    return [missing[i:i + n] for i in range(0, len(missing), n)]


class SceneCache:
    """Least-recently-used cache of built scenes under a byte budget.  `build(key)` returns an object with `.nbytes`.  The entry `get`
    returns is never evicted by that call, so the smallest budget still works, by rebuilding; `builds` counts every build, rebuilt
    entries included.  A caller that builds entries itself (several tiles' trunks in one call) asks `make_room()` before each build and
    hands the entry to `put`: the same rule.  `hold`: keys a walk in progress still needs -- evicted only when nothing else is left."""

    def __init__(self, budget_bytes, build):
        self.budget = int(budget_bytes)
        self.build = build
        self.entries = OrderedDict()
        self.nbytes = 0
        self.builds = 0
        self.hold = set()
        self._last = 0                  # bytes of the last build: what the next one is expected to take (tiles are equally sized)

    def _evict(self, room, keep=None):
        for held in (False, True):       # least recently used first; the keys on hold only after every other entry
            for key in list(self.entries):
                if self.nbytes + room <= self.budget:
                    return
                if key != keep and (key in self.hold) == held:
                    self.nbytes -= self.entries.pop(key).nbytes

    def get(self, key):
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit
        self.make_room()
        return self.put(key, self.build(key))

    def make_room(self):
        """Before a build, so that the peak stays at the budget: evict for an entry of the last build's size."""
        self._evict(self._last)

    def put(self, key, entry):
        """Take a freshly built entry: counted in `builds`, never evicted by this call."""
        self.builds += 1
        self._last = entry.nbytes
        self.entries[key] = entry
        self.nbytes += entry.nbytes
        self._evict(0, keep=key)
        return entry

    def room(self):
        """How many more entries of the last build's size fit without evicting; None before the first build."""
        return max(0, (self.budget - self.nbytes) // self._last) if self._last else None

    def clear(self):
        self.entries.clear()
        self.nbytes = 0


class EncodedImage:
    """What `CiaoSR.encode` returns: the normalised LR batch, the Options and max_scale its scenes are planned with, and the scenes -- the
    whole image's (no `test_cfg.tile`), or a SceneCache of one per (batch item, LR tile), built when a render first touches the tile."""

    def __init__(self, x, options, max_scale, budget_bytes, build, tile=None):
        self.x = x
        self.tile = tile                # side of the LR tiles the scenes are keyed by (b, (y0, x0)); None: one scene per item, (b, None)
        self.options = options
        self.max_scale = max_scale
        self.cache = SceneCache(budget_bytes, build)
        self.view_tiles = None          # render_view's frame list on the device, uploaded by the first view render
        self.alpha = False              # CiaoSR.encode_rgba: the batch is (colour, alpha as grey) of ONE RGBA image
        self.grey = False               # CiaoSR.encode_grey: the colour image (v, v, v) of a grey input; `as_u8` renders are [H, W]

    @property
    def shape(self):
        return tuple(self.x.shape[-2:])

    @property
    def scene_bytes(self):
        return self.cache.nbytes


class EnsembleEncoded:
    """What `CiaoSR.encode(..., self_ensemble=...)` returns: `members[i]` is the plain `encode` of T_k(lq), k = `ids[i]`, each with an
    even share of `test_cfg.scene_cache_mb`; `shape` is the ORIGINAL image's.  `render` / `render_many` render every member's
    transformed window and average them back (hip_ops.dihedral_accum); views, pyramids and prefetch are refused."""

    def __init__(self, ids, members, shape):
        self.ids = tuple(ids)
        self.members = list(members)
        self._shape = tuple(shape)
        self.alpha = False
        self.grey = False               # CiaoSR.encode_grey with self_ensemble

    @property
    def shape(self):
        return self._shape

    @property
    def scene_bytes(self):
        return sum(m.scene_bytes for m in self.members)
