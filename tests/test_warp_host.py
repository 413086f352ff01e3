"""Warps, host side (no GPU): scene.py's warp helpers against the definition restated in numpy (tests/warp_reference.py), the refusals
of CiaoSR.render_warp before any library call, the fixed cases of tests/test_warp_gpu.py pinned, and the new entries' declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ciaosr_amd import _lib, scene
from tests import view_reference as vr
from tests import warp_reference as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_LR, A_SIZE, A_ARGS = (40, 56), (61, 83), ((31.0, 42.5), 2.7, -32)
B_LR, B_SIZE, B_ARGS = (24, 24), (40, 52), ((15.5, 17.25), 2.7, 30)
PERSPECTIVE = (0.0025, -0.002, 1.0)             # the last row of warps A and B
M_CENTRE, M_K, M_NAN = (20, 28), 2e-4, (28, 38, 5, 7)


def warp_a():
    return (*scene.view_matrix(*A_ARGS, A_SIZE), *PERSPECTIVE)


def warp_b():
    return (*scene.view_matrix(*B_ARGS, B_SIZE), *PERSPECTIVE)


def frames_a():
    return scene.plan_view(*A_LR, 32, 8, any_scale=True)


def map_m():
    """Map M, numpy [61, 83, 2] float64, and its footprint (view A's)."""
    m = scene.view_matrix(*A_ARGS, A_SIZE)
    y, x = vr.lr_points(m, *A_SIZE)
    return wr.radial_map(y, x, M_CENTRE, M_K, *A_SIZE, nan_patch=M_NAN), (float(np.hypot(m[0], m[1])), float(np.hypot(m[3], m[4])))


def test_the_fixed_cases_are_the_ones_the_issue_describes():
    """The inputs of the GPU tests cannot drift into an easy case."""
    frames = frames_a()
    assert frames == [(0, 0, 32, 32), (0, 24, 32, 32), (8, 0, 32, 32), (8, 24, 32, 32)]
    h = warp_a()
    y, x = wr.lr_points(h, *A_SIZE)
    d = wr.denominators(h, *A_SIZE)
    assert 0.836 < d.min() < 0.837 and 1.150 < d.max() < 1.151
    assert [int(wr.members(y, x, f).sum()) for f in frames] == [757, 2456, 860, 3614]
    cover = sum(wr.members(y, x, f).astype(int) for f in frames)
    assert [int((cover == k).sum()) for k in range(5)] == [1355, 1055, 1990, 0, 663] and abs((cover == 0).mean() - 0.268) < 5e-4
    assert np.array_equal(cover == 0, ~wr.members(y, x, (0, 0, *A_LR)))
    assert 2.6e-4 < wr.edge_distance(y, x, frames + [(0, 0, *A_LR)]) < 2.8e-4
    fy, fx = wr.centre_footprint(h, *A_SIZE)
    assert abs(fy - 0.3526) < 5e-5 and abs(fx - 0.5051) < 5e-5
    corners = [f for v in (0, A_SIZE[0]) for u in (0, A_SIZE[1]) for f in wr.footprint(h, v, u)]
    assert 0.30 < min(corners) < 0.31 and 0.71 < max(corners) < 0.72
    assert y.size == 5063 > 4 * 1024 and y.size % 1024                        # more than four count workgroups, the last one ragged
    # warp B: whole image
    hb = warp_b()
    yb, xb = wr.lr_points(hb, *B_SIZE)
    inside = wr.members(yb, xb, (0, 0, *B_LR))
    assert int(inside.sum()) == 1766 and wr.edge_distance(yb, xb, [(0, 0, *B_LR)]) > 5e-3
    db = wr.denominators(hb, *B_SIZE)
    assert 0.89 < db.min() and db.max() < 1.10
    # map M: its member counts, and a NaN patch that would otherwise be covered
    mm, fp = map_m()
    my, mx = mm[..., 0].ravel(), mm[..., 1].ravel()
    assert int(np.isnan(my).sum()) == 35 and np.array_equal(np.isnan(my), np.isnan(mx))
    assert [int(wr.members(my, mx, f).sum()) for f in frames] == [375, 2312, 577, 3506]
    cover = sum(wr.members(my, mx, f).astype(int) for f in frames)
    assert [int((cover == k).sum()) for k in range(5)] == [1554, 998, 2136, 0, 375]
    fin = np.isfinite(my)
    assert wr.edge_distance(my[fin], mx[fin], frames + [(0, 0, *A_LR)]) > 6e-4
    m = scene.view_matrix(*A_ARGS, A_SIZE)
    whole = wr.radial_map(*vr.lr_points(m, *A_SIZE), M_CENTRE, M_K, *A_SIZE)
    patch = (slice(M_NAN[0], M_NAN[0] + M_NAN[2]), slice(M_NAN[1], M_NAN[1] + M_NAN[3]))
    assert wr.members(whole[patch][..., 0], whole[patch][..., 1], (0, 0, *A_LR)).all()
    assert fp == (wr.centre_footprint(scene.homography_of_view(m), *A_SIZE))


@pytest.mark.parametrize('args,size', [(A_ARGS, A_SIZE), (B_ARGS, B_SIZE), (((10.0, 12.0), 2.7, 90), (31, 17))])
def test_an_affine_homography_is_the_view_bitwise(args, size):
    m = scene.view_matrix(*args, size)
    h = scene.homography_of_view(m)
    assert h == (*m, 0.0, 0.0, 1.0)
    fp = scene.warp_footprint(h, size)
    assert fp == (float(np.hypot(m[0], m[1])), float(np.hypot(m[3], m[4]))) == wr.centre_footprint(h, *size)
    for th, tw in ((32, 32), (24, 24), (40, 56)):
        assert scene.warp_cell(fp, th, tw) == scene.view_cell(m, th, tw)
        assert scene.warp_cell(fp, th, tw) == tuple(float(c) for c in wr.cell_in(fp, (0, 0, th, tw)))
    assert scene.warp_max_scale(fp) == scene.view_max_scale(m) == wr.max_scale(fp)
    # and the points: identical doubles
    yh, xh = wr.lr_points(h, *size)
    yv, xv = vr.lr_points(m, *size)
    assert np.array_equal(yh.view(np.int64), yv.view(np.int64)) and np.array_equal(xh.view(np.int64), xv.view(np.int64))


def test_footprint_of_a_projective_homography_is_the_reference():
    for h, size in ((warp_a(), A_SIZE), (warp_b(), B_SIZE)):
        assert scene.warp_footprint(h, size) == wr.centre_footprint(h, *size)
        tg = scene.Warp(homography=h, size=size).resolve(*A_LR)
        assert tg[0] == tuple(float(v) for v in h) and tg[1] is None and tg[2] == size and tg[3] == wr.centre_footprint(h, *size)
        assert tg[4] == (0.0, 0.0, 0.0) and tg[5] == [(0, 0, *A_LR)]
    # a caller's own footprint overrides the default
    assert scene.Warp(homography=warp_a(), size=A_SIZE, footprint=(0.4, 0.5)).resolve(*A_LR)[3] == (0.4, 0.5)


def test_homography_from_points():
    h = warp_a()
    pts = [(0.0, 0.0), (0.0, 83.0), (61.0, 83.0), (61.0, 0.0)]
    lr = []
    for v, u in pts:
        d = h[6] * v + h[7] * u + h[8]
        lr.append(((h[0] * v + h[1] * u + h[2]) / d, (h[3] * v + h[4] * u + h[5]) / d))
    got = scene.homography_from_points(pts, lr)
    assert len(got) == 9 and got[8] == 1.0 and max(abs(a - b) for a, b in zip(got, h)) < 1e-12          # the known matrix
    for (v, u), (y, x) in zip(pts, lr):                                                                   # and its four points
        d = got[6] * v + got[7] * u + got[8]
        assert abs((got[0] * v + got[1] * u + got[2]) / d - y) < 1e-9 and abs((got[3] * v + got[4] * u + got[5]) / d - x) < 1e-9
    # a keystone: the output rectangle looks at a trapezoid of the LR image
    quad = [(2.0, 6.0), (3.0, 50.0), (38.0, 55.0), (36.0, 1.0)]
    got = scene.homography_from_points(pts, quad)
    for (v, u), (y, x) in zip(pts, quad):
        d = got[6] * v + got[7] * u + got[8]
        assert abs((got[0] * v + got[1] * u + got[2]) / d - y) < 1e-9 and abs((got[3] * v + got[4] * u + got[5]) / d - x) < 1e-9
    assert scene.Warp(homography=got, size=A_SIZE).resolve(*A_LR)[0] == got
    with pytest.raises(ValueError):
        scene.homography_from_points([(0, 0), (1, 1), (2, 2), (3, 3)], quad)                             # on a line
    with pytest.raises(ValueError):
        scene.homography_from_points(pts[:3], quad[:3])


class _Map:
    """What check_warp reads of a tensor: nothing of it touches a device."""

    def __init__(self, shape, dtype='torch.float64', is_cuda=True):
        self.shape, self.dtype, self.is_cuda = shape, dtype, is_cuda


def test_warp_refusals():
    h = warp_a()
    ok = dict(homography=h, map=None, size=A_SIZE, footprint=None, fill=0.0, h=40, w=56)
    assert scene.check_warp(**ok)[2] == A_SIZE

    def refused(match, **kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            scene.check_warp(**args)

    refused('exactly one', homography=None)
    refused('exactly one', map=_Map((61, 83, 2)))
    for k in range(9):                                                                  # a non-finite entry
        for bad in (float('nan'), float('inf')):
            refused('finite', homography=tuple(bad if i == k else v for i, v in enumerate(h)))
    refused('nine', homography=h[:6])
    # D <= 0 at a corner: each of the four on its own, and D = 0 exactly
    refused('denominator', homography=(*h[:6], 0.0, 0.0, 0.0))
    refused('denominator', homography=(*h[:6], 0.0, 0.0, -1.0))
    refused('denominator', homography=(*h[:6], -1.0 / 61, 0.0, 1.0))                    # D = 0 at (Hv, 0)
    refused('denominator', homography=(*h[:6], 0.0, -1.0 / 80, 1.0))                    # D < 0 at (0, Wv)
    refused('denominator', homography=(*h[:6], -0.01, -0.01, 1.0))                      # only at (Hv, Wv)
    assert scene.check_warp(**dict(ok, homography=(*h[:6], -1.0 / 62, 0.0, 1.0)))       # the horizon just outside the output
    for bad in ((0.0, 0.5), (0.5, -1.0), (float('nan'), 0.5), (0.5, float('inf')), (0.5,), 0.5):
        refused('footprint', footprint=bad)
    refused('cell', footprint=(20.0, 0.5))                                              # 20 * 2 / 40 = 1
    assert scene.check_warp(**dict(ok, footprint=(19.9, 0.5)))
    refused('cell', footprint=(0.5, 16.0), tile=32, overlap=8, any_scale=True)          # 16 * 2 / 32 = 1 in a tile's frame
    refused('empty', size=(0, 4))
    refused('empty', size=(3, 0))
    refused('size', size=None)
    for bad in (1.5, -0.1, (0.1, 0.2), (0.1, 0.2, 1.01)):
        refused('fill', fill=bad)
    refused('tile_any_scale', tile=32, overlap=8, any_scale=False)
    # maps
    fp = (0.37, 0.37)
    good = dict(homography=None, map=_Map((61, 83, 2)), size=None, footprint=fp)
    assert scene.check_warp(**dict(ok, **good))[2] == (61, 83)                          # the size is the map's
    assert scene.check_warp(**dict(ok, **dict(good, map=_Map((61, 83, 2), 'torch.float32'))))[1] is not None
    for shape in ((61, 83), (61, 83, 3), (5063, 2), (61, 83, 2, 1)):
        refused('map', **dict(good, map=_Map(shape)))
    for dtype in ('torch.float16', 'torch.int32', 'torch.bfloat16'):
        refused('map', **dict(good, map=_Map((61, 83, 2), dtype)))
    refused('map', **dict(good, map=[[0.0, 0.0]]))
    refused('map', **dict(good, size=(61, 84)))                                         # a size that is not the map's
    refused('footprint', **dict(good, footprint=None))                                  # required for a map
    with pytest.raises(_lib.CiaoSRHipError, match='CPU'):                               # no CPU fallback
        scene.check_warp(**dict(ok, **dict(good, map=_Map((61, 83, 2), is_cuda=False))))
    with pytest.raises(_lib.CiaoSRHipError, match='CPU'):
        scene.check_warp(**dict(ok, **dict(good, map=torch.zeros(61, 83, 2, dtype=torch.float64))))


def test_render_warp_refuses_before_any_library_call(monkeypatch):
    """CiaoSR.render_warp, render_many and prefetch raise on the host: the library is not even asked for an entry."""
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR

    def no_call(*a, **kw):
        raise AssertionError('a library call before the refusal')

    monkeypatch.setattr(_lib, 'call', no_call)
    monkeypatch.setattr(_lib, 'load', no_call)

    class _Enc:
        max_scale, view_tiles, tile = None, None, None

        def __init__(self):
            self.x = torch.zeros(1, 3, 40, 56)

    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[16, 16])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=8, num_blocks=1),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=2, tile=32, tile_overlap=8)).eval()
    h = warp_a()
    with pytest.raises(ValueError, match='tile_any_scale'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE)
    model.test_cfg = dict(scale=2)
    with pytest.raises(ValueError, match='denominator'):
        model.render_warp(_Enc(), homography=(*h[:6], -0.02, 0.0, 1.0), size=A_SIZE)
    with pytest.raises(ValueError, match='finite'):
        model.render_warp(_Enc(), homography=(float('nan'), *h[1:]), size=A_SIZE)
    with pytest.raises(ValueError, match='footprint'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint=(0.0, 1.0))
    with pytest.raises(ValueError, match='cell'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint=(30.0, 0.5))
    with pytest.raises(ValueError, match='empty'):
        model.render_warp(_Enc(), homography=h, size=(0, 3))
    with pytest.raises(ValueError, match='fill'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, fill=1.5)
    with pytest.raises(ValueError, match='map'):
        model.render_warp(_Enc(), map=torch.zeros(61, 83, 3, dtype=torch.float64), footprint=(0.4, 0.4))
    with pytest.raises(ValueError, match='map'):
        model.render_warp(_Enc(), map=torch.zeros(61, 83, 2, dtype=torch.int32), footprint=(0.4, 0.4))
    with pytest.raises(_lib.CiaoSRHipError, match='CPU'):
        model.render_warp(_Enc(), map=torch.zeros(61, 83, 2, dtype=torch.float64), footprint=(0.4, 0.4))
    with pytest.raises(ValueError, match='exactly one'):
        model.render_warp(_Enc())
    with pytest.raises(ValueError, match='as_u8 and as_u16'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, as_u8=True, as_u16=True)
    for call in (model.render_many, model.prefetch):
        with pytest.raises(ValueError, match='denominator'):
            call(_Enc(), [scene.Grid(scale=2), scene.Warp(homography=(*h[:6], 0.0, 0.0, 0.0), size=A_SIZE)])
    # a self-ensemble encode is refused as a view is
    ens = scene.EnsembleEncoded((0, 1), [_Enc(), _Enc()], (40, 56))
    with pytest.raises(ValueError, match='self-ensemble'):
        model.render_warp(ens, homography=h, size=A_SIZE)
    with pytest.raises(ValueError, match='self-ensemble'):
        model.render_many(ens, [scene.Warp(homography=h, size=A_SIZE)])


def test_map_footprint_is_central_differences_at_the_centre():
    m = scene.view_matrix(*A_ARGS, A_SIZE)
    y, x = vr.lr_points(m, *A_SIZE)
    grid = torch.from_numpy(np.stack([y, x], 1).reshape(*A_SIZE, 2))
    fy, fx = scene.map_footprint(grid)                                                   # (a host tensor is fine here: no kernel runs)
    want = scene.warp_footprint(scene.homography_of_view(m), A_SIZE)
    assert abs(fy - want[0]) < 1e-12 and abs(fx - want[1]) < 1e-12                       # exact up to rounding on an affine map
    with pytest.raises(ValueError, match='footprint'):                                   # map M's NaN patch covers its centre pixel
        scene.map_footprint(torch.from_numpy(map_m()[0]))
    mm = wr.radial_map(y, x, M_CENTRE, M_K, *A_SIZE)
    ci, cj = A_SIZE[0] // 2, A_SIZE[1] // 2
    dv, du = (mm[ci + 1, cj] - mm[ci - 1, cj]) / 2, (mm[ci, cj + 1] - mm[ci, cj - 1]) / 2
    got = scene.map_footprint(torch.from_numpy(mm))
    assert got == (float(np.hypot(dv[0], du[0])), float(np.hypot(dv[1], du[1])))
    assert scene.map_footprint(grid[:1]) is not None and scene.map_footprint(grid[:, :1]) is not None      # one-sided on a border
    with pytest.raises(ValueError):
        scene.map_footprint(grid[:1, :1])
    nan = grid.clone()
    nan[ci, cj + 1] = float('nan')
    with pytest.raises(ValueError, match='footprint'):
        scene.map_footprint(nan)
    with pytest.raises(ValueError, match='map'):
        scene.map_footprint(grid[..., 0])


def test_warp_exports_are_declared():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 370
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    names = {'ciaosr_warp_workspace_bytes': (C.c_size_t, 3), 'ciaosr_warp_count_i32': (C.c_int, 11),
             'ciaosr_warp_select_f32': (C.c_int, 15), 'ciaosr_warp_coord_cell_f32': (C.c_int, 9)}
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name, (res, n_args) in names.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
        args = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', header).group(1)
        assert len(args.split(',')) == n_args, name
        assert name in integration, name
    assert {n for n in _lib.SIGNATURES if n.startswith('ciaosr_warp_')} == set(names)
    sig = _lib.SIGNATURES['ciaosr_warp_count_i32'][1]
    assert sig[0] is D and sig[1] is C.c_void_p and sig[2] is D and _lib.SIGNATURES['ciaosr_warp_select_f32'][1][5] is I
    # sizes: the view's layout, one int per tile and workgroup; refusals are 0
    chunk = lib.ciaosr_view_block_queries()
    assert lib.ciaosr_warp_workspace_bytes(1, 1, 1) == 4
    assert lib.ciaosr_warp_workspace_bytes(3, chunk, 5) == 3 * 5 * 4 and lib.ciaosr_warp_workspace_bytes(3, chunk + 1, 5) == 4 * 5 * 4
    assert lib.ciaosr_warp_workspace_bytes(61, 83, 4) == lib.ciaosr_view_workspace_bytes(61, 83, 4)
    assert lib.ciaosr_warp_workspace_bytes(0, 4, 1) == 0 and lib.ciaosr_warp_workspace_bytes(4, 0, 1) == 0
    assert lib.ciaosr_warp_workspace_bytes(4, 4, 0) == 0 and lib.ciaosr_warp_workspace_bytes(-1, 4, 1) == 0
    assert lib.ciaosr_warp_workspace_bytes(65536, 65536, 1) == 0                    # more than 2^31 - 1 queries


def test_warp_entries_refuse_bad_arguments_without_a_launch(capfd):
    """Argument checks run on the host before anything is launched: every call below returns the error code with null device pointers."""
    lib = _lib.load()
    h9 = (C.c_double * 9)(*warp_a())
    fp = (C.c_double * 2)(0.35, 0.5)
    frame = (C.c_int * 4)(0, 0, 40, 56)
    one = C.c_void_p(16)                                                            # a non-null, aligned pointer that is never read

    def count(h=h9, mp=None, f=fp, hv=61, wv=83, n_tiles=4):
        return lib.ciaosr_warp_count_i32(h, mp, f, hv, wv, one, n_tiles, one, one, 1 << 20, None)

    codes = [count(h=None), count(mp=one), count(f=None), count(hv=0), count(wv=0), count(hv=65536, wv=65536), count(n_tiles=0),
             count(f=(C.c_double * 2)(0.0, 0.5)), count(f=(C.c_double * 2)(float('nan'), 0.5)),
             count(h=(C.c_double * 9)(*warp_a()[:8], float('inf'))), count(h=(C.c_double * 9)(*warp_a()[:6], -0.02, 0.0, 1.0)),
             count(h=None, mp=C.c_void_p(24)),                                      # a map that is not 16-byte aligned
             lib.ciaosr_warp_coord_cell_f32(one, one, None, None, fp, 61, 83, frame, None),
             lib.ciaosr_warp_coord_cell_f32(one, one, h9, None, fp, 61, 83, (C.c_int * 4)(0, 0, 0, 56), None),
             lib.ciaosr_warp_select_f32(h9, one, fp, 61, 83, frame, 0, 1, one, 1 << 20, 5, one, one, one, None),
             lib.ciaosr_warp_select_f32(h9, None, fp, 61, 83, frame, 1, 1, one, 1 << 20, 5, one, one, one, None),
             lib.ciaosr_warp_select_f32(h9, None, fp, 61, 83, frame, 0, 1, one, 1 << 20, 0, one, one, one, None)]
    assert all(c == codes[0] and c != 0 for c in codes), codes
    assert lib.ciaosr_error_string(codes[0]).decode().startswith('bad argument')
    short = lib.ciaosr_warp_count_i32(h9, None, fp, 61, 83, one, 4, one, one, 8, None)        # a workspace that is too small
    assert short != 0 and short != codes[0] and lib.ciaosr_error_string(short).decode().startswith('workspace')
    capfd.readouterr()
