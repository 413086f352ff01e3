"""Affine views, host side (no GPU): scene.view_matrix / view_of_window / view_cell / plan_view against the definition restated in numpy
(tests/view_reference.py), and the new entries' declarations."""
import ctypes as C

import numpy as np
import pytest

from ciaosr_amd import _lib, scene
from ciaosr_amd.coords import make_coord
from tests import view_reference as vr

WINDOW = (9, 41, 61, 35)        # tests/test_scene_restorer_gpu.py: crosses both seams of the 2 x 2 tiles of the 40 x 56 image at x2.7


def _grid_coord(m, hv, wv, h, w):
    y, x = vr.lr_points(m, hv, wv)
    return vr.coord_in(y, x, (0, 0, h, w))


@pytest.mark.parametrize('h,w,ht,wt', [(24, 24, 79, 79), (24, 24, 96, 96), (40, 56, 108, 151)])
def test_axis_aligned_view_is_make_coord_within_2_pow_minus_22(h, w, ht, wt):
    """make_coord rounds three times in fp32 (v0 + r, 2 r, the product and the sum: 2^-24 relative each on values up to 1), a view's
    coordinate once from fp64 (2^-25 at most): together under 2^-22."""
    want = make_coord((ht, wt)).numpy()
    m, size = scene.view_of_window(h, w, ht, wt)
    assert size == (ht, wt)
    assert np.abs(_grid_coord(m, ht, wt, h, w).astype(np.float64) - want).max() <= 2.0 ** -22
    if h * wt == w * ht:                                          # one zoom for both axes: view_matrix can say it too
        m = scene.view_matrix((h / 2, w / 2), ht / h, 0, (ht, wt))
        assert m[1] == 0.0 and m[3] == 0.0
        assert np.abs(_grid_coord(m, ht, wt, h, w).astype(np.float64) - want).max() <= 2.0 ** -22
        cell = vr.cell_in(m, (0, 0, h, w))
        assert abs(float(cell[0]) - 2 / ht) <= 2.0 ** -24 * (2 / ht) * 2 and scene.view_cell(m, h, w) == (float(cell[0]), float(cell[1]))


def test_quarter_turns_are_exact():
    zoom = 2.7
    inv = 1.0 / zoom
    for angle, (c, s) in ((0, (1, 0)), (90, (0, 1)), (180, (-1, 0)), (270, (0, -1)), (-90, (0, -1)), (450, (0, 1))):
        m = scene.view_matrix((10.0, 12.0), zoom, angle, (31, 17))
        assert (m[0], m[1], m[3], m[4]) == (c * inv, -s * inv, s * inv, c * inv), (angle, m)
        assert all(v == 0.0 or abs(v) == inv for v in (m[0], m[1], m[3], m[4]))
    # the norm of a row -- the cell -- does not change under rotation
    cells = {scene.view_cell(scene.view_matrix((10.0, 12.0), zoom, a, (31, 17)), 24, 24) for a in (0, 90, 180, 270)}
    assert len(cells) == 1
    for a in (13, 30, -32, 211.5):
        got = scene.view_cell(scene.view_matrix((10.0, 12.0), zoom, a, (31, 17)), 24, 24)
        assert max(abs(g - c) for g, c in zip(got, next(iter(cells)))) <= 2.0 ** -23 * got[0]


def test_corners_of_a_quarter_turn_follow_the_documented_convention():
    """A positive angle turns the picture clockwise on the screen: at 90 degrees the view's top-left corner shows the image's bottom-left
    and walking right in the view walks up the image (scene.view_matrix)."""
    hv, wv, zoom, cy, cx = 8, 12, 2.0, 20.0, 30.0
    m = scene.view_matrix((cy, cx), zoom, 90, (hv, wv))
    y, x = vr.lr_points(m, hv, wv)
    y, x = y.reshape(hv, wv), x.reshape(hv, wv)
    half_v, half_u = (hv - 1) / 2 / zoom, (wv - 1) / 2 / zoom          # centre-to-centre half extents in LR pixels
    # view corner -> LR point: top-left -> bottom-left, top-right -> top-left, bottom-left -> bottom-right, bottom-right -> top-right;
    # the view's width runs along the image's height
    want = {(0, 0): (cy + half_u, cx - half_v), (0, wv - 1): (cy - half_u, cx - half_v),
            (hv - 1, 0): (cy + half_u, cx + half_v), (hv - 1, wv - 1): (cy - half_u, cx + half_v)}
    for (i, j), (wy, wx) in want.items():
        assert abs(y[i, j] - wy) < 1e-12 and abs(x[i, j] - wx) < 1e-12, ((i, j), y[i, j], x[i, j], wy, wx)
    assert y[0, 1] < y[0, 0] and x[0, 1] == x[0, 0]                  # right in the view = up in the image
    # the centre of the view looks at `center`, at every angle
    for a in (0, 90, 33.0, -32):
        m = scene.view_matrix((cy, cx), zoom, a, (hv, wv))
        assert abs(m[0] * hv / 2 + m[1] * wv / 2 + m[2] - cy) < 1e-12 and abs(m[3] * hv / 2 + m[4] * wv / 2 + m[5] - cx) < 1e-12
    # a small positive angle: walking right in the view drifts up the image (y falls), walking down drifts right
    m = scene.view_matrix((cy, cx), zoom, 10, (hv, wv))
    assert m[1] < 0 < m[3] and m[0] > 0 and m[4] > 0


def test_view_of_window_reproduces_the_window_planner():
    h, w, tile, overlap, ht, wt = 40, 56, 32, 8, 108, 151
    m, (hv, wv) = scene.view_of_window(h, w, ht, wt, WINDOW)
    assert (hv, wv) == WINDOW[2:]
    frames = scene.plan_view(h, w, tile, overlap, any_scale=True)
    assert frames == [(0, 0, 32, 32), (0, 24, 32, 32), (8, 0, 32, 32), (8, 24, 32, 32)]
    y, x = vr.lr_points(m, hv, wv)
    # precondition: no centre on (or within rounding of) a tile edge, so membership cannot hinge on the last bit
    assert vr.edge_distance(y, x, frames) > 1e-3
    planned = scene.plan_window(h, w, tile, overlap, ht, wt, WINDOW, any_scale=True)
    assert len(planned) == 4 and [(t['y0'], t['x0'], t['th'], t['tw']) for t in planned] == frames
    for t, frame in zip(planned, frames):
        got = vr.members(y, x, frame).reshape(hv, wv)
        want = np.zeros((hv, wv), dtype=bool)
        want[t['a0'] - WINDOW[0]:t['a1'] - WINDOW[0], t['b0'] - WINDOW[1]:t['b1'] - WINDOW[1]] = True
        assert np.array_equal(got, want), frame
        # and the coordinates in the tile's frame are the planner's window grid within the bound
        gh, gw, r0, r1, c0, c1, fr = t['grid']
        from ciaosr_amd import tile_plan
        cy = tile_plan.axis_local(frame[0], tile, h, ht)
        cx = tile_plan.axis_local(frame[1], tile, w, wt)
        ref_y = cy[2][r0 - cy[0]:r1 - cy[0]].numpy().astype(np.float64)
        ref_x = cx[2][c0 - cx[0]:c1 - cx[0]].numpy().astype(np.float64)
        mine = vr.coord_in(y, x, frame).reshape(hv, wv, 2)[got].reshape(r1 - r0, c1 - c0, 2).astype(np.float64)
        # the frame stretches the image's [-1, 1] by n_lr / tile: the fp32 error of the global coordinate grows by that factor
        assert np.abs(mine[..., 0] - ref_y[:, None]).max() <= 2.0 ** -22 * h / tile
        assert np.abs(mine[..., 1] - ref_x[None, :]).max() <= 2.0 ** -22 * w / tile
    # the whole grid by default
    m, size = scene.view_of_window(h, w, ht, wt)
    assert size == (ht, wt) and m == (h / ht, 0.0, 0.0, 0.0, w / wt, 0.0)


def test_view_refusals():
    with pytest.raises(ValueError, match='singular'):
        scene.view_cell((0.5, 0.25, 1.0, 1.0, 0.5, 2.0), 24, 24)
    with pytest.raises(ValueError, match='singular'):
        scene.view_cell((0.0, 0.0, 1.0, 0.0, 0.5, 2.0), 24, 24)
    with pytest.raises(ValueError):
        scene.view_cell((float('nan'), 0.0, 1.0, 0.0, 0.5, 2.0), 24, 24)
    # cell >= 1: an output pixel spans half of the frame or more
    assert scene.view_cell((11.9, 0.0, 0.0, 0.0, 0.5, 0.0), 24, 24)[0] < 1.0
    for m in ((12.0, 0.0, 0.0, 0.0, 0.5, 0.0), (0.5, 0.0, 0.0, 9.0, 9.0, 0.0)):
        with pytest.raises(ValueError, match='cell'):
            scene.view_cell(m, 24, 24)
    with pytest.raises(ValueError, match='tile_any_scale'):
        scene.plan_view(40, 56, 32, 8, any_scale=False)
    assert scene.plan_view(40, 56) == [(0, 0, 40, 56)]
    assert scene.plan_view(24, 40, 32, 8, any_scale=True) == [(0, 0, 24, 24), (0, 16, 24, 24)]          # the tile shrinks to the image
    for bad in (dict(zoom=0.0), dict(zoom=-1.0), dict(size=(0, 4))):
        kw = dict(center=(1.0, 1.0), zoom=2.0, angle_deg=0.0, size=(4, 4))
        kw.update(bad)
        with pytest.raises(ValueError):
            scene.view_matrix(**kw)
    assert abs(scene.view_max_scale(scene.view_matrix((3.0, 3.0), 2.7, 30, (9, 9))) - 2.7) < 1e-12


def test_render_view_refuses_tiles_without_tile_any_scale():
    """CiaoSR.render_view raises before it touches the device."""
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR

    class _Enc:
        max_scale, view_tiles = None, None

        def __init__(self):
            import torch
            self.x = torch.zeros(1, 3, 40, 56)

    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[16, 16])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=8, num_blocks=1),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=2, tile=32, tile_overlap=8)).eval()
    m = scene.view_matrix((20.0, 28.0), 2.0, 30, (16, 16))
    with pytest.raises(ValueError, match='tile_any_scale'):
        model.render_view(_Enc(), m, (16, 16))
    model.test_cfg = dict(scale=2)
    with pytest.raises(ValueError, match='singular'):
        model.render_view(_Enc(), (0.5, 0.5, 0.0, 0.5, 0.5, 0.0), (16, 16))
    with pytest.raises(ValueError, match='cell'):
        model.render_view(_Enc(), (30.0, 0.0, 0.0, 0.0, 0.5, 0.0), (16, 16))
    with pytest.raises(ValueError, match='fill'):
        model.render_view(_Enc(), m, (16, 16), fill=1.5)


def test_view_exports_are_declared():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 250
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for name, res, n_args in (('ciaosr_view_block_queries', C.c_int, 0), ('ciaosr_view_workspace_bytes', C.c_size_t, 3),
                              ('ciaosr_view_coord_cell_f32', C.c_int, 7), ('ciaosr_view_count_i32', C.c_int, 9),
                              ('ciaosr_view_select_f32', C.c_int, 13), ('ciaosr_view_blend_f32', C.c_int, 7),
                              ('ciaosr_view_finalize_f32', C.c_int, 8)):
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert _lib.SIGNATURES['ciaosr_view_count_i32'][1][0] is D and _lib.SIGNATURES['ciaosr_view_select_f32'][1][3] is I
    # the header declares them with the same arity
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ciaosr_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in (n for n in _lib.SIGNATURES if n.startswith('ciaosr_view_')):
        args = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', header).group(1).strip()
        assert (0 if args == 'void' else len(args.split(','))) == len(_lib.SIGNATURES[name][1]), name
    # sizes: one int per tile and workgroup; refusals are 0
    chunk = lib.ciaosr_view_block_queries()
    assert chunk >= 64 and chunk % 64 == 0
    assert lib.ciaosr_view_workspace_bytes(1, 1, 1) == 4
    assert lib.ciaosr_view_workspace_bytes(3, chunk, 5) == 3 * 5 * 4 and lib.ciaosr_view_workspace_bytes(3, chunk + 1, 5) == 4 * 5 * 4
    assert lib.ciaosr_view_workspace_bytes(0, 4, 1) == 0 and lib.ciaosr_view_workspace_bytes(4, 4, 0) == 0
    assert lib.ciaosr_view_workspace_bytes(65536, 65536, 1) == 0              # more than 2^31 - 1 queries
