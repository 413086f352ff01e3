"""Area-sampled warps, host side (no GPU): warp C of tests/test_warp_area_gpu.py pinned, scene.area_samples and scene.warp_area_table
against the definition restated in numpy (tests/warp_area_reference.py), the refusals of check_warp / CiaoSR.render_warp / tools/render.py
before any library call, and the new entries' declarations and argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ciaosr_amd import _lib, scene
from tests import warp_area_reference as ar
from tests import warp_pp_reference as pr
from tests import warp_reference as wr
from tests.test_warp_host import A_LR, A_SIZE, _Map, warp_a

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_LR, C_SIZE, C_ARGS = (40, 56), (24, 34), ((21.0, 27.5), 0.7, -32)
C_RANGE = (0.25, 1.0)                           # hi = 1: the default upper end
C_N = 4


def warp_c():
    """Warp C: a zoomed-out (x0.7), turned and keystoned look at a 40 x 56 image: it minifies everywhere but in one corner."""
    return (*scene.view_matrix(*C_ARGS, C_SIZE), 0.02, -0.012, 1.0)


def frames_c():
    return scene.plan_view(*C_LR, 32, 8, any_scale=True)


def _hist(n, values=(1, 2, 4)):
    return [int((n == v).sum()) for v in values]


def test_warp_c_is_the_case_the_issue_describes():
    """The fixture cannot quietly stop exercising a case: both axes take all three counts, they differ on more than half of the pixels,
    and 37 pixels stay under-sampled."""
    h = warp_c()
    hv, wv = C_SIZE
    gy, gx = pr.raw_jacobian(h, hv, wv)
    assert abs(gy.min() - 0.89) < 5e-3 and abs(gy.max() - 2.10) < 5e-3 and abs(gx.min() - 0.96) < 5e-3 and abs(gx.max() - 5.74) < 5e-3
    first, ny, nx, fy, fx = ar.table(gy, gx, C_RANGE, C_N)
    assert _hist(ny) == [70, 742, 4] and _hist(nx) == [3, 436, 377]
    assert int((ny != nx).sum()) == 440 and int((gx > 4.0).sum()) == 37 and int(first[-1]) == 4661
    assert (fx[gx > 4.0] == 1.0).all() and (fx[gx <= 4.0] < 1.0).sum() > 700
    y, x = wr.lr_points(h, hv, wv)
    assert int(wr.members(y, x, (0, 0, *C_LR)).sum()) == 684
    assert frames_c() == [(0, 0, 32, 32), (0, 24, 32, 32), (8, 0, 32, 32), (8, 24, 32, 32)]
    # fewer samples with a smaller N, one per pixel with N = 1
    assert int(ar.table(gy, gx, C_RANGE, 2)[0][-1]) == 3121
    assert int(ar.table(gy, gx, C_RANGE, 1)[0][-1]) == hv * wv


def test_area_samples_is_the_reference():
    hi = 0.75
    edge = [hi * n for n in (1, 2, 4, 8)]                                        # g == hi n exactly: stays at n
    g = np.array(edge + [np.nextafter(e, np.inf) for e in edge] + [np.nextafter(e, 0.0) for e in edge]
                 + [0.0, -1.0, 1e-300, 5.99, 6.0, 6.01, 1e300, np.inf, np.nan])
    for n_max in (1, 2, 4, 8):
        want = ar.counts(g, hi, n_max)
        got = [scene.area_samples(v, hi, n_max) for v in g]
        assert got == want.tolist(), (n_max, got, want.tolist())
    assert [scene.area_samples(e, hi, 8) for e in edge] == [1, 2, 4, 8]
    assert [scene.area_samples(np.nextafter(e, np.inf), hi, 8) for e in edge] == [2, 4, 8, 8]
    assert scene.area_samples(float('inf'), hi, 4) == 4 and scene.area_samples(float('inf'), hi, 1) == 1
    assert scene.area_samples(float('nan'), hi, 4) == 0 and scene.area_samples(-3.0, hi, 4) == 1


@pytest.mark.parametrize('n_max', [1, 2, 4, 8])
def test_scene_warp_area_table_is_the_reference_bitwise(n_max):
    h = warp_c()
    hv, wv = C_SIZE
    first, ns, fs = scene.warp_area_table(h, C_SIZE, C_RANGE, n_max)
    w_first, ny, nx, fy, fx = ar.table(*pr.raw_jacobian(h, hv, wv), C_RANGE, n_max)
    assert first == w_first.tolist() and ns == list(zip(ny.tolist(), nx.tolist()))
    got = np.array(fs, dtype=np.float64)
    assert np.array_equal(got[:, 0].view(np.int64), fy.view(np.int64)) and np.array_equal(got[:, 1].view(np.int64), fx.view(np.int64))
    # a tensor with a NaN, a +inf, a value below lo n and a negative entry
    raw = tensor_c()
    first, ns, fs = scene.warp_area_table(h, C_SIZE, C_RANGE, n_max, tensor=raw.tolist())
    w_first, ny, nx, fy, fx = ar.table(raw[..., 0].ravel(), raw[..., 1].ravel(), C_RANGE, n_max)
    assert first == w_first.tolist() and ns == list(zip(ny.tolist(), nx.tolist()))
    assert ns[Q_NAN] == (0, 0) and fs[Q_NAN] is None and ns[Q_INF][1] == n_max and fs[Q_INF][1] == 1.0
    assert ns[Q_LOW][0] == 1 and fs[Q_LOW][0] == C_RANGE[0] and ns[Q_NEG][0] == 1 and fs[Q_NEG][0] == C_RANGE[0]
    for q, f in enumerate(fs):
        if f is not None:
            assert (f[0], f[1]) == (fy[q], fx[q]), q


Q_NAN, Q_INF, Q_LOW, Q_NEG = 400, 300, 500, 200


def tensor_c():
    """The Jacobian footprints of warp C with four entries replaced: a NaN (no samples), a +inf (N samples, f = hi), a value below lo
    (n = 1, f = lo; under the range (0.7, 1.0) many split pixels have g / n below lo as well) and a negative entry (n = 1, f = lo)."""
    hv, wv = C_SIZE
    raw = np.stack(pr.raw_jacobian(warp_c(), hv, wv), 1).reshape(hv, wv, 2).copy()
    flat = raw.reshape(-1, 2)
    flat[Q_NAN, 0] = np.nan
    flat[Q_INF, 1] = np.inf
    flat[Q_LOW, 0] = 0.1
    flat[Q_NEG, 0] = -1.0
    return raw


def test_a_sample_footprint_below_lo_is_raised_to_lo():
    """With lo = 0.7 and hi = 1 a footprint of 1.2 is split in two and 0.6 < lo: f = lo."""
    first, ny, nx, fy, fx = ar.table(np.array([1.2, 1.0, 2.5]), np.array([0.5, 1.0, np.inf]), (0.7, 1.0), 4)
    assert ny.tolist() == [2, 1, 4] and nx.tolist() == [1, 1, 4] and first.tolist() == [0, 2, 3, 19]
    assert fy.tolist() == [0.7, 1.0, 0.7] and fx.tolist() == [0.7, 1.0, 1.0]
    f2, ns, fs = scene.warp_area_table(warp_c(), (1, 3), (0.7, 1.0), 4, tensor=[[[1.2, 0.5], [1.0, 1.0], [2.5, float('inf')]]])
    assert f2 == [0, 2, 3, 19] and ns == [(2, 1), (1, 1), (4, 4)] and fs == [(0.7, 0.7), (1.0, 1.0), (0.7, 1.0)]


def test_the_reference_samples():
    """Sample ids run through the pixels in row-major order, a pixel's samples through its rows; the positions are exact."""
    h = scene.homography_of_view((1.0, 0.0, 0.0, 0.0, 1.0, 0.0))                 # the identity: (y_lr, x_lr) = (v, u)
    first, ny, nx, fy, fx = ar.table(np.array([2.0, np.nan, 1.0]), np.array([4.0, 1.0, 1.0]), (0.25, 1.0), 4)
    pix, y, x, sfy, sfx = ar.samples(h, 1, 3, first, ny, nx, fy, fx)
    assert first.tolist() == [0, 8, 8, 9] and pix.tolist() == [0] * 8 + [2]
    assert y.tolist() == [0.25] * 4 + [0.75] * 4 + [0.5] and x.tolist() == [0.125, 0.375, 0.625, 0.875] * 2 + [2.5]
    assert sfy.tolist() == [1.0] * 9 and sfx.tolist() == [1.0] * 9


def test_check_warp_resolves_an_area_warp():
    h = warp_c()
    ok = dict(homography=h, map=None, size=C_SIZE, footprint='per-pixel', fill=0.0, h=40, w=56, footprint_range=C_RANGE)
    assert scene.check_warp(**ok)[3].samples == 0                                # 'clamp' is the default
    assert scene.check_warp(**ok, minify='clamp', max_samples=8)[3].samples == 0
    fp = scene.check_warp(**ok, minify='area')[3]
    assert isinstance(fp, scene.PerPixel) and (fp.mode, fp.range, fp.samples) == (scene.FP_JACOBIAN, C_RANGE, 4)
    for n in (1, 2, 4, 8):
        assert scene.check_warp(**ok, minify='area', max_samples=n)[3].samples == n
    t = _Map((24, 34, 2))
    fp = scene.check_warp(**dict(ok, footprint=t), minify='area', max_samples=2)[3]
    assert (fp.mode, fp.samples) == (scene.FP_TENSOR, 2) and fp.tensor is t
    w = scene.Warp(homography=h, size=C_SIZE, footprint='per-pixel', footprint_range=C_RANGE, minify='area', max_samples=8)
    assert w.resolve(*C_LR)[3].samples == 8 and "minify='area'" in repr(w) and 'max_samples=8' in repr(w)
    assert 'minify' not in repr(scene.Warp(homography=h, size=C_SIZE, footprint='per-pixel', footprint_range=C_RANGE))
    assert scene.check_minify() == 0 and scene.check_minify('area', 2) == 2

    def refused(match, **kw):
        args = dict(ok, minify='area')
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            scene.check_warp(**args)

    for bad in ('box', 'Area', '', None, 4):
        refused('minify', minify=bad)
    for bad in (0, 3, 5, 16, -2, 2.5, None, True, '4'):
        refused('max_samples', max_samples=bad)
        refused('max_samples', max_samples=bad, minify='clamp')
    refused('per-pixel', footprint=(1.0, 1.0), footprint_range=None)             # a single footprint
    refused('per-pixel', footprint=None, footprint_range=None)                   # the defaulted single footprint
    refused('homography', homography=None, map=_Map((24, 34, 2)), size=None)     # a map point source
    refused('homography', homography=None, map=_Map((24, 34, 2)), size=None, footprint=_Map((24, 34, 2)))
    refused('2\\^31', size=(8192, 16385), footprint_range=(0.25, 1.0))           # 8192 * 16385 * 16 = 2^31 + 2^17
    flat = scene.homography_of_view((1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    assert scene.check_warp(**dict(ok, homography=flat, size=(8192, 16383)), minify='area')[2] == (8192, 16383)
    refused('2\\^31', size=(8192, 4096), max_samples=8)
    # the existing refusals stay as they are
    refused('cell', footprint_range=(0.3, 20.0))
    refused('footprint_range', footprint_range=(0.6, 0.5))
    refused('denominator', homography=(*h[:6], -0.05, 0.0, 1.0))


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
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=4)).eval()
    h = warp_c()
    pp = dict(homography=h, size=C_SIZE, footprint='per-pixel')
    with pytest.raises(ValueError, match='minify'):
        model.render_warp(_Enc(), minify='box', **pp)
    with pytest.raises(ValueError, match='max_samples'):
        model.render_warp(_Enc(), minify='area', max_samples=3, **pp)
    with pytest.raises(ValueError, match='per-pixel'):
        model.render_warp(_Enc(), homography=h, size=C_SIZE, footprint=(1.0, 1.0), minify='area')
    with pytest.raises(ValueError, match='per-pixel'):
        model.render_warp(_Enc(), homography=h, size=C_SIZE, minify='area')
    with pytest.raises(ValueError, match='homography'):
        model.render_warp(_Enc(), map=_Map((24, 34, 2)), footprint='per-pixel', minify='area')
    with pytest.raises(ValueError, match='2\\^31'):
        model.render_warp(_Enc(), homography=h, size=(8192, 16385), footprint='per-pixel', minify='area')
    with pytest.raises(ValueError, match='cell'):
        model.render_warp(_Enc(), minify='area', footprint_range=(0.3, 30.0), **pp)
    for call in (model.render_many, model.prefetch):
        with pytest.raises(ValueError, match='max_samples'):
            call(_Enc(), [scene.Grid(scale=2), scene.Warp(minify='area', max_samples=16, **pp)])
        with pytest.raises(ValueError, match='homography'):
            call(_Enc(), [scene.Warp(map=_Map((24, 34, 2)), footprint='per-pixel', minify='area')])
    ens = scene.EnsembleEncoded((0, 1), [_Enc(), _Enc()], (40, 56))
    with pytest.raises(ValueError, match='self-ensemble'):
        model.render_warp(ens, minify='area', **pp)


def test_the_render_tool_refuses_minify_without_a_per_pixel_footprint(tmp_path):
    from tools import render
    base = ['cfg.py', 'w.pth', 'img.png', '--homography', *[repr(v) for v in warp_c()], '--size', '24', '34', '--out', str(tmp_path)]
    args = render.parse_args(base + ['--footprint', 'per-pixel', '--minify', 'area'])
    assert (args.minify, args.max_samples) == ('area', None)
    args = render.parse_args(base + ['--footprint', 'per-pixel', '--minify', 'area', '--max-samples', '8'])
    assert (args.minify, args.max_samples) == ('area', 8)
    assert render.parse_args(base + ['--footprint', 'per-pixel']).minify is None
    assert render.parse_args(base + ['--footprint', 'per-pixel', '--minify', 'clamp']).minify == 'clamp'
    for bad in (['--minify', 'area'], ['--minify', 'clamp'], ['--footprint', 'per-pixel', '--minify', 'box'],
                ['--footprint', 'per-pixel', '--minify', 'area', '--max-samples', '3'],
                ['--footprint', 'per-pixel', '--max-samples', '4'], ['--footprint', 'per-pixel', '--minify', 'clamp', '--max-samples', '4'],
                ['--minify', 'area', '--footprint-range', '0.25', '1.0']):
        with pytest.raises(SystemExit):
            render.parse_args(base + bad)


NAMES = {'ciaosr_areawarp_count_i32': 13, 'ciaosr_areawarp_select_f32': 15, 'ciaosr_areawarp_resolve_f32': 14,
         'ciaosr_areawarp_table_i32': 13}


def test_area_warp_exports_are_declared():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 372
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name, n_args in dict(NAMES, ciaosr_areawarp_workspace_bytes=4).items():
        assert hasattr(lib, name), name
        res = C.c_size_t if name.endswith('_bytes') else C.c_int
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
        args = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', header).group(1)
        assert len(args.split(',')) == n_args, name
        assert name in integration, name
    assert {n for n in _lib.SIGNATURES if n.startswith('ciaosr_areawarp_')} == set(NAMES) | {'ciaosr_areawarp_workspace_bytes'}


def test_area_warp_workspace_bytes():
    lib = _lib.load()
    size = lib.ciaosr_areawarp_workspace_bytes
    assert size(24, 34, 4, 4) > 24 * 34 * 24 and size(24, 34, 4, 4) % 4 == 0
    assert size(24, 34, 8, 4) > size(24, 34, 4, 4) and size(24, 34, 4, 8) >= size(24, 34, 4, 4) >= size(24, 34, 4, 1)
    for bad in ((0, 34, 4, 4), (24, 0, 4, 4), (24, 34, 0, 4), (24, 34, 4, 0), (24, 34, 4, 3), (24, 34, 4, 16), (-1, 34, 4, 4),
                (8192, 16385, 4, 4), (46341, 46341, 1, 1), (8192, 4096, 1, 8)):
        assert size(*bad) == 0, bad
    assert size(8192, 16383, 1, 4) > 0


def test_area_warp_entries_refuse_bad_arguments_without_a_launch(capfd):
    """Argument checks run on the host before anything is launched: every call below returns the error code with device pointers that
    are never read."""
    lib = _lib.load()
    h9 = (C.c_double * 9)(*warp_c())
    rng = (C.c_double * 2)(*C_RANGE)
    frame = (C.c_int * 4)(0, 0, 32, 32)
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    one, odd = C.c_void_p(16), C.c_void_p(24)
    big = 1 << 22

    def r2(lo, hi):
        return (C.c_double * 2)(lo, hi)

    def count(h=h9, mode=1, r=rng, t=None, n=4, hv=24, wv=34, tiles=one, n_tiles=4, counts=one, ws=one, nbytes=big):
        return lib.ciaosr_areawarp_count_i32(h, mode, r, t, n, hv, wv, tiles, n_tiles, counts, ws, nbytes, None)

    def select(h=h9, n_max=4, hv=24, wv=34, fr=frame, index=0, n_tiles=4, ws=one, nbytes=big, S=4661, n=10, si=one, co=one, ce=one):
        return lib.ciaosr_areawarp_select_f32(h, n_max, hv, wv, fr, index, n_tiles, ws, nbytes, S, n, si, co, ce, None)

    def resolve(E=one, Wt=one, out=one, S=4661, n_max=4, hv=24, wv=34, n_tiles=4, ws=one, nbytes=big, fill=f3, mean=f3, std=f3):
        return lib.ciaosr_areawarp_resolve_f32(E, Wt, out, S, n_max, hv, wv, n_tiles, ws, nbytes, fill, mean, std, None)

    def table(first=one, n=one, h=h9, mode=1, r=rng, t=None, n_max=4, hv=24, wv=34, ws=one, nbytes=big):
        return lib.ciaosr_areawarp_table_i32(first, n, h, mode, r, t, n_max, hv, wv, 1, ws, nbytes, None)

    zero3, bad3 = (C.c_float * 3)(0.5, 0.0, 0.5), (C.c_float * 3)(0.5, 1.5, 0.5)
    codes = [count(h=None), count(mode=0), count(mode=2), count(mode=4), count(mode=3), count(mode=3, t=odd),
             count(r=None), count(r=r2(0.0, 1.0)), count(r=r2(1.5, 1.0)), count(r=r2(0.25, float('inf'))), count(r=r2(float('nan'), 1.0)),
             count(n=0), count(n=3), count(n=16), count(n=-4), count(hv=0), count(wv=-1), count(hv=8192, wv=16385),
             count(tiles=None), count(tiles=odd), count(n_tiles=0), count(counts=None), count(ws=None), count(ws=odd),
             count(h=(C.c_double * 9)(*warp_c()[:6], -0.05, 0.0, 1.0)), count(h=(C.c_double * 9)(*warp_c()[:8], float('nan'))),
             select(h=None), select(n_max=5), select(hv=0), select(fr=None), select(fr=(C.c_int * 4)(0, 0, 0, 32)), select(index=4),
             select(index=-1), select(n_tiles=0), select(ws=None), select(ws=odd), select(S=0), select(S=24 * 34 * 16 + 1), select(n=0),
             select(n=4662), select(si=None), select(co=None), select(ce=None),
             resolve(E=None), resolve(Wt=None), resolve(out=None), resolve(S=-1), resolve(S=24 * 34 * 16 + 1), resolve(n_max=3),
             resolve(hv=0), resolve(n_tiles=0), resolve(ws=None), resolve(ws=odd), resolve(fill=None), resolve(mean=None),
             resolve(std=None), resolve(fill=bad3), resolve(std=zero3),
             table(first=None), table(n=None), table(h=None), table(mode=2), table(mode=3), table(r=r2(0.5, 0.25)), table(n_max=6),
             table(hv=0), table(ws=None), table(ws=odd)]
    assert all(c == codes[0] and c != 0 for c in codes), codes
    assert lib.ciaosr_error_string(codes[0]).decode().startswith('bad argument')
    short = [count(nbytes=64), select(nbytes=64), resolve(nbytes=64), table(nbytes=64)]
    assert all(c == short[0] and c != 0 and c != codes[0] for c in short), short
    assert lib.ciaosr_error_string(short[0]).decode().startswith('workspace')
    capfd.readouterr()


def test_warp_a_minifies_nowhere_under_a_wide_range():
    """What consequence (i) of the GPU tests rests on: with hi above every raw footprint of warps A and B every n is 1."""
    gy, gx = pr.raw_jacobian(warp_a(), *A_SIZE)
    first, ny, nx, _, _ = ar.table(gy, gx, (0.1, 0.9), 4)
    assert max(gy.max(), gx.max()) < 0.9 and (ny == 1).all() and (nx == 1).all() and int(first[-1]) == A_SIZE[0] * A_SIZE[1]
    assert A_LR == C_LR
