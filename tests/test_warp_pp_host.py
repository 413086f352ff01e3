"""Per-pixel warps, host side (no GPU): the fixed cases of tests/test_warp_pp_gpu.py pinned, scene.warp_footprints against the definition
restated in numpy (tests/warp_pp_reference.py) bit for bit, the refusals of check_warp / CiaoSR.render_warp before any library call, and
the new entries' declarations and argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from ciaosr_amd import _lib, scene
from tests import warp_pp_reference as pr
from tests import warp_reference as wr
from tests.test_warp_host import A_ARGS, A_LR, A_SIZE, B_ARGS, B_LR, B_SIZE, _Map, frames_a, map_m, warp_a, warp_b

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = (0.32, 0.6)                             # what the GPU tests clamp to: both ends act on warp A
# Consequence (ii)'s eight member pixels of warp A: 4980 and 48 are the inside minimum and maximum of BOTH axes (the footprint grows
# along one diagonal of the output); 4980 and 3403 are clamped at lo in y, 48 is the one pixel clamped at hi in x; 3403, 3499 and 2000
# are covered by four frames, 3377 and 4200 by one, the others by two.
PIXELS_II = (4980, 48, 3403, 3499, 3377, 1521, 2000, 4200)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_fixed_cases_are_the_ones_the_issue_describes():
    frames = frames_a()
    h = warp_a()
    y, x = wr.lr_points(h, *A_SIZE)
    inside = wr.members(y, x, (0, 0, *A_LR))
    gy, gx = pr.raw_jacobian(h, *A_SIZE)
    assert gy.size == 5063
    assert abs(gy.min() - 0.3051) < 5e-5 and abs(gy.max() - 0.4180) < 5e-5 and abs(gx.min() - 0.3767) < 5e-5 and abs(gx.max() - 0.7136) < 5e-5
    assert abs(gy[inside].min() - 0.3051) < 5e-5 and abs(gy[inside].max() - 0.3892) < 5e-5
    assert abs(gx[inside].min() - 0.3767) < 5e-5 and abs(gx[inside].max() - 0.6001) < 5e-5
    assert len(np.unique((gy * 2.0 / 32).astype(np.float32))) == 5060           # an own cell for nearly every query
    assert [int((gy[inside] < RANGE[0]).sum()), int((gy[inside] > RANGE[1]).sum())] == [314, 0]
    assert [int((gx[inside] < RANGE[0]).sum()), int((gx[inside] > RANGE[1]).sum())] == [0, 1]
    # the pixels of consequence (ii)
    cover = sum(wr.members(y, x, f).astype(int) for f in frames)
    idx = np.flatnonzero(inside)
    assert int(idx[gy[inside].argmin()]) == int(idx[gx[inside].argmin()]) == 4980
    assert int(idx[gy[inside].argmax()]) == int(idx[gx[inside].argmax()]) == 48
    assert np.flatnonzero(inside & (gx > RANGE[1])).tolist() == [48] and gy[3403] < RANGE[0] and gy[4980] < RANGE[0]
    assert [int(cover[q]) for q in PIXELS_II] == [2, 2, 4, 4, 1, 2, 4, 1], [int(cover[q]) for q in PIXELS_II]
    assert len(set(PIXELS_II)) == 8
    # the affine degenerate of A: one value everywhere, and the sqrt form rounds to the cell hypot gives (the same double here)
    for args, size in ((A_ARGS, A_SIZE), (B_ARGS, B_SIZE)):
        m = scene.view_matrix(*args, size)
        ay, ax = pr.raw_jacobian(scene.homography_of_view(m), *size)
        assert len(np.unique(ay)) == 1 and len(np.unique(ax)) == 1
        assert (float(ay[0]), float(ax[0])) == (math.sqrt(m[0] * m[0] + m[1] * m[1]), math.sqrt(m[3] * m[3] + m[4] * m[4]))
        for t in (24, 32, 40, 56):
            assert scene.warp_cell((float(ay[0]), float(ax[0])), t, t) == scene.warp_cell((math.hypot(m[0], m[1]), math.hypot(m[3], m[4])), t, t)
    # warp B
    hb = warp_b()
    yb, xb = wr.lr_points(hb, *B_SIZE)
    ins_b = wr.members(yb, xb, (0, 0, *B_LR))
    by, bx = pr.raw_jacobian(hb, *B_SIZE)
    assert abs(by.min() - 0.2681) < 5e-5 and abs(by.max() - 0.3946) < 5e-5 and abs(bx.min() - 0.3441) < 5e-5 and abs(bx.max() - 0.4339) < 5e-5
    assert int(ins_b.sum()) == 1766 and int((by[ins_b] < RANGE[0]).sum()) == 910
    assert int((by[ins_b] > RANGE[1]).sum()) == int((bx[ins_b] < RANGE[0]).sum()) == int((bx[ins_b] > RANGE[1]).sum()) == 0
    # map M: the pixels without a footprint.  31 pixels of the 5 x 7 NaN patch have both neighbours along an axis missing; its four
    # corners have a finite neighbour on each axis, and their one-sided difference with the NaN centre is NaN: 35 non-members, exactly
    # the NaN positions.  The ring around the patch keeps a footprint from its one-sided differences.
    mm, _ = map_m()
    my, mx = mm[..., 0].ravel(), mm[..., 1].ravel()
    dy, dx, has = pr.raw_differences(mm)
    assert int((~has).sum()) == 31 and int(np.isnan(dy[has]).sum()) == 4
    fy, fx, has_c = pr.clamp(dy, dx, RANGE)
    assert int((~has_c).sum()) == 35 and np.array_equal(~has_c, np.isnan(my))
    assert [int((wr.members(my, mx, f) & has_c).sum()) for f in frames] == [375, 2312, 577, 3506]
    assert 0.3712 < np.nanmin(dy) < 0.3713 and 0.5895 < np.nanmax(dy) < 0.5896 and 0.3717 < np.nanmin(dx) < 0.3718 and 0.6222 < np.nanmax(dx) < 0.6223
    assert int((dx[has_c] > RANGE[1]).sum()) > 0                                 # the upper clamp acts on the map as well
    ring = np.zeros(A_SIZE, dtype=bool)
    ring[27:34, 37:46] = True
    ring[28:33, 38:45] = False
    assert has_c[ring.ravel()].all() and int(ring.sum()) == 28


@pytest.mark.parametrize('h,size', [(warp_a(), A_SIZE), (warp_b(), B_SIZE), (scene.homography_of_view(scene.view_matrix(*A_ARGS, A_SIZE)), (7, 5))])
@pytest.mark.parametrize('rng', [RANGE, (0.25, 1.0), (0.4, 0.4)])
def test_scene_warp_footprints_is_the_reference_bitwise(h, size, rng):
    got = scene.warp_footprints(h, size, rng)
    assert got.shape == (*size, 2) and got.dtype == torch.float64 and not got.is_cuda
    fy, fx, has = pr.clamp(*pr.raw_jacobian(h, *size), rng)
    assert has.all()
    got = got.numpy().reshape(-1, 2)
    assert np.array_equal(_bits64(got[:, 0]), _bits64(fy)) and np.array_equal(_bits64(got[:, 1]), _bits64(fx))
    assert got.min() >= rng[0] and got.max() <= rng[1]


def test_the_reference_differences_rule():
    """Central where both neighbours are in the grid and finite, one-sided beside a border or a missing neighbour, nothing where both
    are missing."""
    p = np.array([[0.0, 1.0, 4.0, 9.0], [1.0, np.nan, 5.0, 10.0], [2.0, 3.0, np.inf, 11.0]])
    dv, ok_v = pr._derivative(p, 0)
    du, ok_u = pr._derivative(p, 1)
    miss_u, miss_v = {(1, 0), (2, 3)}, {(0, 1), (2, 1)}                         # a border on one side, a non-finite value on the other
    assert {(i, j) for i in range(3) for j in range(4) if not ok_u[i, j]} == miss_u
    assert {(i, j) for i in range(3) for j in range(4) if not ok_v[i, j]} == miss_v
    assert [du[0, j] for j in range(4)] == [1.0, 2.0, 4.0, 5.0]                 # forward, central, central, backward
    assert du[1, 1] == 2.0 and du[1, 2] == 5.0 and du[1, 3] == 5.0              # the NaN's own: central; left is NaN: forward; backward
    assert du[2, 0] == 1.0 and du[2, 1] == 1.0 and du[2, 2] == 4.0              # (2, 1): right is inf: backward
    assert [dv[i, 0] for i in range(3)] == [1.0, 1.0, 1.0] and dv[1, 1] == 1.0
    assert dv[0, 2] == 1.0 and dv[1, 2] == 1.0 and dv[2, 2] == np.inf           # (1, 2): below is inf: backward; the inf's own: inf
    gy, gx, has = pr.raw_differences(np.stack([p, p], -1))
    assert {(i, j) for i in range(3) for j in range(4) if not has.reshape(3, 4)[i, j]} == miss_u | miss_v
    assert np.isnan(gy[~has]).all() and gy.reshape(3, 4)[2, 2] == np.inf and np.isnan(gy.reshape(3, 4)[1, 1]) == False
    fy, fx, has_c = pr.clamp(gy, gx, (0.5, 3.0))
    assert np.array_equal(has_c, has) and fy.reshape(3, 4)[2, 2] == 3.0 and fy.reshape(3, 4)[0, 0] == np.sqrt(2.0)
    lone = np.full((3, 3, 2), np.nan)
    lone[1, 1] = 1.0
    assert not pr.raw_differences(lone)[2].any()


def test_check_warp_resolves_a_per_pixel_footprint():
    h = warp_a()
    ok = dict(homography=h, map=None, size=A_SIZE, footprint='per-pixel', fill=0.0, h=40, w=56)
    fp = scene.check_warp(**ok, footprint_range=RANGE)[3]
    assert isinstance(fp, scene.PerPixel) and (fp.mode, fp.range, fp.tensor) == (scene.FP_JACOBIAN, RANGE, None)
    assert scene.check_warp(**ok, max_scale=4)[3].range == (0.25, 1.0)           # default: (1 / max_scale, 1.0)
    assert scene.check_warp(**ok, footprint_range=(0.4, 0.4))[3].range == (0.4, 0.4)
    mp = _Map((61, 83, 2))
    via_map = dict(ok, homography=None, map=mp, size=None)
    assert scene.check_warp(**via_map, max_scale=2.5)[3].mode == scene.FP_DIFFERENCES
    t = _Map((61, 83, 2), 'torch.float32')
    for source in (ok, via_map):
        fp = scene.check_warp(**dict(source, footprint=t), footprint_range=RANGE)[3]
        assert fp.mode == scene.FP_TENSOR and fp.tensor is t and fp.range == RANGE
    # the record carries the range; a single footprint resolves as before
    w = scene.Warp(homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=RANGE)
    assert w.resolve(*A_LR)[3].range == RANGE and 'per-pixel' in repr(w) and '0.32' in repr(w)
    assert scene.Warp(homography=h, size=A_SIZE).resolve(*A_LR)[3] == wr.centre_footprint(h, *A_SIZE)
    assert scene.check_warp(**dict(ok, footprint=np.array([0.4, 0.5])))[3] == (0.4, 0.5)       # two numbers in an array: one footprint

    def refused(match, exc=ValueError, **kw):
        args = dict(ok, max_scale=4)
        args.update(kw)
        with pytest.raises(exc, match=match):
            scene.check_warp(**args)

    refused('per-pixel', footprint='per_pixel')                                  # an unknown string
    refused('per-pixel', footprint='')
    for shape in ((61, 83), (61, 83, 3), (61, 84, 2), (5063, 2)):
        refused('footprint tensor', footprint=_Map(shape))
    for dtype in ('torch.float16', 'torch.int64'):
        refused('footprint tensor', footprint=_Map((61, 83, 2), dtype))
    refused('CPU', exc=_lib.CiaoSRHipError, footprint=_Map((61, 83, 2), is_cuda=False))
    refused('CPU', exc=_lib.CiaoSRHipError, footprint=torch.zeros(61, 83, 2, dtype=torch.float64))
    refused('footprint_range', footprint=None, footprint_range=RANGE)            # a range without a per-pixel footprint
    refused('footprint_range', footprint=(0.4, 0.5), footprint_range=RANGE)
    for bad in ((0.0, 0.5), (-0.1, 0.5), (0.6, 0.5), (float('nan'), 0.5), (0.3, float('inf')), (0.3,), 0.3, (0.1, 0.2, 0.3)):
        refused('footprint_range', footprint_range=bad)
    refused('footprint_range', max_scale=None)                                   # nothing to default lo from
    refused('cell', footprint_range=(0.3, 20.0))                                 # 20 * 2 / 40 = 1
    assert scene.check_warp(**dict(ok, footprint_range=(0.3, 19.9)))
    refused('cell', footprint_range=(0.3, 16.0), tile=32, overlap=8, any_scale=True)
    refused('grid axis', homography=None, map=_Map((1, 83, 2)), size=None)       # differences need two pixels along each axis
    refused('grid axis', homography=None, map=_Map((61, 1, 2)), size=None)
    assert scene.check_warp(**dict(ok, homography=None, map=_Map((1, 83, 2)), size=None, footprint=_Map((1, 83, 2)), max_scale=4))
    with pytest.raises(ValueError, match='footprint_range'):
        scene.warp_footprints(h, A_SIZE, (0.5, 0.4))


def test_render_warp_refuses_before_any_library_call(monkeypatch):
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
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=2)).eval()
    h = warp_a()
    host = torch.zeros(61, 83, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match='per-pixel'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint='jacobian')
    with pytest.raises(ValueError, match='footprint tensor'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint=torch.zeros(61, 83, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='footprint tensor'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint=torch.zeros(61, 83, 2, dtype=torch.int32))
    with pytest.raises(_lib.CiaoSRHipError, match='CPU'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint=host)
    with pytest.raises(ValueError, match='footprint_range'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint_range=RANGE)
    with pytest.raises(ValueError, match='footprint_range'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=(0.6, 0.32))
    with pytest.raises(ValueError, match='cell'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=(0.3, 30.0))
    model.test_cfg = dict()                                                      # no scale and an open max_scale: no default lo
    with pytest.raises(ValueError, match='footprint_range'):
        model.render_warp(_Enc(), homography=h, size=A_SIZE, footprint='per-pixel')
    model.test_cfg = dict(scale=2)
    for call in (model.render_many, model.prefetch):
        with pytest.raises(ValueError, match='footprint_range'):
            call(_Enc(), [scene.Grid(scale=2), scene.Warp(homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=(0.0, 1.0))])
    ens = scene.EnsembleEncoded((0, 1), [_Enc(), _Enc()], (40, 56))
    with pytest.raises(ValueError, match='self-ensemble'):
        model.render_warp(ens, homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=RANGE)
    with pytest.raises(ValueError, match='self-ensemble'):
        model.render_many(ens, [scene.Warp(homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=RANGE)])


def test_the_generator_render_takes_a_chunk_override():
    import inspect
    from ciaosr_amd.implicit_net import LocalImplicitSRNet
    sig = inspect.signature(LocalImplicitSRNet.render)
    assert sig.parameters['chunk'].default is None


NAMES = {'ciaosr_ppwarp_count_i32': 13, 'ciaosr_ppwarp_select_f32': 17, 'ciaosr_ppwarp_coord_cell_f32': 11, 'ciaosr_ppwarp_footprints_f64': 9}


def test_per_pixel_warp_exports_are_declared():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 371
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == n_args, name
        args = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', header).group(1)
        assert len(args.split(',')) == n_args, name
        assert name in integration, name
    assert {n for n in _lib.SIGNATURES if n.startswith('ciaosr_ppwarp_')} == set(NAMES)


def test_per_pixel_warp_entries_refuse_bad_arguments_without_a_launch(capfd):
    """Argument checks run on the host before anything is launched: every call below returns the error code with device pointers that
    are never read."""
    lib = _lib.load()
    h9 = (C.c_double * 9)(*warp_a())
    rng = (C.c_double * 2)(*RANGE)
    frame = (C.c_int * 4)(0, 0, 40, 56)
    one = C.c_void_p(16)

    def count(h=h9, mp=None, mode=1, r=rng, t=None, hv=61, wv=83, n_tiles=4):
        return lib.ciaosr_ppwarp_count_i32(h, mp, mode, r, t, hv, wv, one, n_tiles, one, one, 1 << 20, None)

    def r2(lo, hi):
        return (C.c_double * 2)(lo, hi)

    codes = [count(mode=0), count(mode=4), count(mode=2),                         # differences need the map
             count(h=None, mp=one, mode=1),                                        # the Jacobian needs the homography
             count(mode=3), count(mode=3, t=C.c_void_p(24)),                       # a null and a misaligned tensor
             count(h=None, mp=one, mode=3, t=C.c_void_p(8)),
             count(r=None), count(r=r2(0.0, 0.5)), count(r=r2(-1.0, 0.5)), count(r=r2(0.6, 0.5)), count(r=r2(float('nan'), 0.5)),
             count(r=r2(0.3, float('inf'))), count(r=r2(0.3, float('nan'))),
             count(h=None, mp=one, mode=2, hv=1), count(h=None, mp=one, mode=2, wv=1),            # a grid axis of 1 with differences
             count(h=None), count(mp=one), count(hv=0), count(n_tiles=0), count(h=None, mp=C.c_void_p(24), mode=2),
             count(h=(C.c_double * 9)(*warp_a()[:6], -0.02, 0.0, 1.0)),
             lib.ciaosr_ppwarp_coord_cell_f32(one, one, h9, None, 2, rng, None, 61, 83, frame, None),
             lib.ciaosr_ppwarp_coord_cell_f32(one, one, h9, None, 1, rng, None, 61, 83, (C.c_int * 4)(0, 0, 0, 56), None),
             lib.ciaosr_ppwarp_coord_cell_f32(None, one, h9, None, 1, rng, None, 61, 83, frame, None),
             lib.ciaosr_ppwarp_select_f32(h9, None, 1, r2(0.5, 0.4), None, 61, 83, frame, 0, 1, one, 1 << 20, 5, one, one, one, None),
             lib.ciaosr_ppwarp_select_f32(h9, None, 1, rng, None, 61, 83, frame, 1, 1, one, 1 << 20, 5, one, one, one, None),
             lib.ciaosr_ppwarp_select_f32(h9, None, 1, rng, None, 61, 83, frame, 0, 1, one, 1 << 20, 0, one, one, one, None),
             lib.ciaosr_ppwarp_select_f32(h9, None, 3, rng, None, 61, 83, frame, 0, 1, one, 1 << 20, 5, one, one, one, None),
             lib.ciaosr_ppwarp_footprints_f64(None, h9, None, 1, rng, None, 61, 83, None),
             lib.ciaosr_ppwarp_footprints_f64(C.c_void_p(24), h9, None, 1, rng, None, 61, 83, None),
             lib.ciaosr_ppwarp_footprints_f64(one, h9, None, 2, rng, None, 61, 83, None),
             lib.ciaosr_ppwarp_footprints_f64(one, None, one, 2, rng, None, 1, 83, None),
             lib.ciaosr_ppwarp_footprints_f64(one, h9, None, 1, r2(0.0, 1.0), None, 61, 83, None)]
    assert all(c == codes[0] and c != 0 for c in codes), codes
    assert lib.ciaosr_error_string(codes[0]).decode().startswith('bad argument')
    short = lib.ciaosr_ppwarp_count_i32(h9, None, 1, rng, None, 61, 83, one, 4, one, one, 8, None)
    assert short != 0 and short != codes[0] and lib.ciaosr_error_string(short).decode().startswith('workspace')
    capfd.readouterr()
