"""Per-pixel warps on the GPU: the count / select / coordinate / footprint kernels of the three footprint sources against the definition in
numpy float64 (tests/warp_pp_reference.py), bit for bit; a per-pixel warp with constant footprints against the single-footprint warp
and render_view (consequence (i)); single pixels against the single-footprint warp of their own footprint (consequence (ii), fp32);
the torch-CPU oracle with one query per batch item, which gives every query the shift radius of its own cell; f16 against fp32;
render_many; fill and the quantised, grey and RGBA outputs; tools/render.py --footprint per-pixel."""
import math
import os

import numpy as np
import pytest
import torch

from tests import view_reference as vr
from tests import warp_pp_reference as pr
from tests import warp_reference as wr
from tests.helpers import SQRT6
from tests.test_view_gpu import A_ONE_TILE_SHIFT, _bits, _lq, _model, _params, _tiles, _view
from tests.test_warp_gpu import TILED, _count_copies, _points_map, _shift
from tests.test_warp_host import A_ARGS, A_LR, A_SIZE, B_ARGS, B_LR, B_SIZE, frames_a, map_m, warp_a, warp_b
from tests.test_warp_pp_host import PIXELS_II, RANGE

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SCALE = 1.0 / RANGE[0]                       # what a per-pixel warp with RANGE plans for: every encode below is made with it


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same64(a, b):
    """Equal doubles bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits64(a[~nan]), _bits64(b[~nan]))


def _check_kernels(h, mp, spec, y, x, fy, fx, has, hv, wv, frames, dev):
    """Count, select, the whole grid's coordinates and cells, and the footprints of one per-pixel warp whose points are (y, x) and whose
    clamped footprints are (fy, fx) where `has`: counts and q_index equal, coord, cell and the doubles bitwise; everything run twice."""
    from ciaosr_amd import hip_ops
    tiles = _tiles(frames, dev)
    want_counts = [int((wr.members(y, x, f) & has).sum()) for f in frames]
    runs = []
    for _ in range(2):
        counts, ws = hip_ops.warp_pp_count(h, mp, spec, hv, wv, tiles)
        counts = counts.tolist()
        assert counts == want_counts, (counts, want_counts)
        out = []
        for k, (frame, n) in enumerate(zip(frames, counts)):
            if n == 0:
                continue
            q_index, coord, cell = hip_ops.warp_pp_select(h, mp, spec, hv, wv, frame, k, len(frames), ws, n)
            mem = wr.members(y, x, frame) & has
            assert np.array_equal(q_index.cpu().numpy(), np.flatnonzero(mem).astype(np.int32)), frame
            want = wr.coord_in(y[mem], x[mem], frame)
            assert np.array_equal(coord.cpu().numpy().view(np.int32), want.view(np.int32)), frame
            want_cell = pr.cells_in(fy[mem], fx[mem], frame)
            assert np.array_equal(cell.cpu().numpy().view(np.int32), want_cell.view(np.int32)), (frame, np.abs(cell.cpu().numpy() - want_cell).max())
            assert hip_ops.grid_width_of(coord) == 0
            out += [q_index, coord, cell]
        coord, cell = hip_ops.make_coord_cell_warp_pp(h, mp, spec, hv, wv, frames[-1], dev)     # the whole grid, without selection
        fin = np.isfinite(y)
        want = wr.coord_in(np.where(fin, y, 0.0), np.where(fin, x, 0.0), frames[-1])
        got = coord.cpu().numpy()
        assert np.array_equal(got.view(np.int32)[fin], want.view(np.int32)[fin]) and np.isnan(got[~fin]).all()
        got_cell = cell.cpu().numpy()
        want_cell = pr.cells_in(np.where(has, fy, 0.0), np.where(has, fx, 0.0), frames[-1])
        assert np.array_equal(got_cell.view(np.int32)[has], want_cell.view(np.int32)[has]) and np.isnan(got_cell[~has]).all()
        assert hip_ops.grid_width_of(coord) == wv
        fps = hip_ops.warp_footprints(h, mp, spec, hv, wv, dev)
        assert fps.shape == (hv, wv, 2) and fps.dtype == torch.float64
        got_fp = fps.cpu().numpy().reshape(-1, 2)
        assert _same64(got_fp[:, 0], np.where(has, fy, np.nan)) and _same64(got_fp[:, 1], np.where(has, fx, np.nan))
        runs.append((counts, out + [coord, cell, fps.view(torch.int64)]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8)) for a, b in zip(runs[0][1], runs[1][1]))
    return counts


def test_kernels_against_the_definition(dev):
    """Test 1: Jacobian, differences and tensor footprints with both clamps acting, bit for bit."""
    from ciaosr_amd import hip_ops, scene
    frames = frames_a()
    hv, wv = A_SIZE
    # the Jacobian of warp A
    h = warp_a()
    y, x = wr.lr_points(h, hv, wv)
    fy, fx, has = pr.clamp(*pr.raw_jacobian(h, hv, wv), RANGE)
    assert has.all() and (fy == RANGE[0]).sum() > 300 and (fx == RANGE[1]).sum() >= 1
    spec = scene.PerPixel(scene.FP_JACOBIAN, RANGE)
    assert _check_kernels(h, None, spec, y, x, fy, fx, has, hv, wv, frames, dev) == [757, 2456, 860, 3614]
    assert _same64(hip_ops.warp_footprints(h, None, spec, hv, wv, dev).cpu().numpy(), scene.warp_footprints(h, A_SIZE, RANGE).numpy())
    # differences on map M: the borders of the grid and the ring around the NaN patch are one-sided, the patch has no footprint
    mm, _ = map_m()
    my, mx = mm[..., 0].ravel(), mm[..., 1].ravel()
    dy, dx, _ = pr.raw_differences(mm)
    fy, fx, has = pr.clamp(dy, dx, RANGE)
    grid = has.reshape(hv, wv)
    assert grid[0].all() and grid[-1].all() and grid[:, 0].all() and grid[:, -1].all() and grid[27, 38:45].all() and grid[28:33, 37].all()
    assert not grid[28:33, 38:45].any() and int((~has).sum()) == 35 and (fx == RANGE[1]).sum() > 0
    mdev = torch.from_numpy(mm).to(dev)
    spec = scene.PerPixel(scene.FP_DIFFERENCES, RANGE)
    assert _check_kernels(None, mdev, spec, my, mx, fy, fx, has, hv, wv, frames, dev) == [375, 2312, 577, 3506]
    # a tensor with a NaN entry and a +inf entry at two members of tile (8, 24), over both point sources; a negative entry clamps to lo
    raw = np.stack(pr.raw_jacobian(h, hv, wv), 1).reshape(hv, wv, 2).copy()
    q_nan, q_inf, q_neg = 3499, 3403, 2000
    raw.reshape(-1, 2)[q_nan, 0] = np.nan
    raw.reshape(-1, 2)[q_inf, 1] = np.inf
    raw.reshape(-1, 2)[q_neg, 0] = -1.0
    fy, fx, has = pr.clamp(raw[..., 0].ravel(), raw[..., 1].ravel(), RANGE)
    assert not has[q_nan] and int((~has).sum()) == 1 and fx[q_inf] == RANGE[1] and fy[q_neg] == RANGE[0]
    tdev = torch.from_numpy(raw).to(dev)
    spec = scene.PerPixel(scene.FP_TENSOR, RANGE, tdev)
    assert _check_kernels(h, None, spec, y, x, fy, fx, has, hv, wv, frames, dev) == [756, 2455, 859, 3613]       # q_nan is covered by all four frames
    has_m = has & ~np.isnan(my)
    counts = _check_kernels(None, mdev, spec, my, mx, fy, fx, has, hv, wv, frames, dev)
    assert counts == [int((wr.members(my, mx, f) & has_m).sum()) for f in frames]
    # the wrappers refuse a float32 or a host tensor
    with pytest.raises(ValueError):
        hip_ops.warp_pp_count(h, None, scene.PerPixel(scene.FP_TENSOR, RANGE, tdev.float()), hv, wv, _tiles(frames, dev))
    with pytest.raises(hip_ops.CiaoSRHipError):
        hip_ops.warp_pp_count(h, None, scene.PerPixel(scene.FP_TENSOR, RANGE, tdev.cpu()), hv, wv, _tiles(frames, dev))


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_constant_footprints_are_the_single_footprint_warp_bitwise(dev, precision):
    """Consequence (i): the affine degenerate with 'per-pixel' is render_view, and a constant tensor is the single-footprint warp of
    that constant -- A tiled, B whole-image, view A shifted into one tile (a member list), and a 30 x 30 warp inside tile (0, 0) that is
    walked as a grid."""
    from ciaosr_amd import scene
    model = _model('rdn', dev, 3)
    small = _view(((12, 12), 2.0, 12), (30, 30))
    cases = [('B whole', dict(precision=precision), B_LR, _view(B_ARGS, B_SIZE), B_SIZE, warp_b()),
             ('A tiled', dict(TILED, precision=precision), A_LR, _view(A_ARGS, A_SIZE), A_SIZE, warp_a()),
             ('A in one tile', dict(TILED, precision=precision), A_LR, _shift(_view(A_ARGS, A_SIZE), A_ONE_TILE_SHIFT), A_SIZE, None),
             ('a grid in one tile', dict(TILED, precision=precision), A_LR, small, (30, 30), None)]
    wide = (0.1, 0.9)                                                            # a range that clamps nothing here
    for name, cfg, (h, w), m, size, hom in cases:
        model.test_cfg = dict(cfg)
        lq = _lq(h, w, dev)
        fill = (0.25, 0.5, 1.0)
        enc = model.encode(lq, max_scale=MAX_SCALE)
        want = model.render_view(enc, m, size, fill=fill)
        affine = scene.homography_of_view(m)
        got = model.render_warp(enc, homography=affine, size=size, footprint='per-pixel', footprint_range=wide, fill=fill)
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, 'jacobian', (got - want).abs().max().item())
        # the sqrt form of the footprint, what the kernel computes: the same fp32 cell as hypot's (pinned on the host)
        const = (math.sqrt(m[0] * m[0] + m[1] * m[1]), math.sqrt(m[3] * m[3] + m[4] * m[4]))
        y, x = vr.lr_points(m, *size)
        tensor = torch.tensor(const, dtype=torch.float64, device=dev).expand(*size, 2)
        for source in (dict(homography=affine, size=size), dict(map=_points_map(y, x, *size, dev))):
            got = model.render_warp(enc, footprint=tensor, footprint_range=wide, fill=fill, **source)
            assert torch.equal(_bits(got), _bits(want)), (name, 'tensor', sorted(source))
            single = model.render_warp(enc, footprint=const, fill=fill, **source)
            assert torch.equal(_bits(single), _bits(want)), (name, 'single', sorted(source))
        if 'map' in source and size[0] > 1:                                      # differences of an affine map: constant up to rounding,
            got = model.render_warp(enc, footprint='per-pixel', footprint_range=(const[0], const[0]), fill=fill, **source)
            iso = model.render_warp(enc, footprint=(const[0], const[0]), fill=fill, **source)
            assert torch.equal(_bits(got), _bits(iso)), (name, 'differences pinned by the clamp')
        if hom is not None:                                                      # a projective warp with a constant tensor
            c = (0.4, 0.5)
            single = model.render_warp(enc, homography=hom, size=size, footprint=c, fill=fill)
            got = model.render_warp(enc, homography=hom, size=size, footprint=torch.tensor(c, dtype=torch.float64, device=dev).expand(*size, 2),
                                    footprint_range=wide, fill=fill)
            assert torch.equal(_bits(got), _bits(single)) and not torch.equal(_bits(got), _bits(want)), name
            clamped = model.render_warp(enc, homography=hom, size=size, footprint='per-pixel', footprint_range=(0.4, 0.4), fill=fill)
            iso = model.render_warp(enc, homography=hom, size=size, footprint=(0.4, 0.4), fill=fill)
            assert torch.equal(_bits(clamped), _bits(iso)), name


def test_a_pixel_is_the_single_footprint_warp_of_its_own_footprint(dev):
    """Consequence (ii), fp32: eight member pixels of warp A -- the inside extremes of both axes, pixels clamped at lo and at hi, covered
    by four frames, by two and by one."""
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED)
    h = warp_a()
    fy, fx, _ = pr.clamp(*pr.raw_jacobian(h, *A_SIZE), RANGE)
    enc = model.encode(_lq(*A_LR, dev), max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=h, size=A_SIZE, footprint='per-pixel', footprint_range=RANGE).view(3, -1)
    assert enc.max_scale == MAX_SCALE and enc.cache.builds == 4
    assert fy[4980] == RANGE[0] and fy[3403] == RANGE[0] and fx[48] == RANGE[1]
    other = model.encode(_lq(*A_LR, dev), max_scale=MAX_SCALE)                    # an encode of its own with the same explicit max_scale
    for q in PIXELS_II:
        want = model.render_warp(other, homography=h, size=A_SIZE, footprint=(float(fy[q]), float(fx[q]))).view(3, -1)
        assert torch.equal(_bits(got[:, q]), _bits(want[:, q])), (q, (got[:, q] - want[:, q]).abs().max().item())
        assert not torch.equal(_bits(got), _bits(want)), q                       # and only there: the other pixels have other footprints


def _oracle_per_query(feature, nonlocal_map, x, coord, cell, params, step=64):
    """oracle.ciaosr_oracle.query_rgb + bilinear_residual with the queries along the BATCH axis, one query per item: the oracle reads the
    shift radius from cell[:, 0] per batch item, so every query is answered with the radius of its own cell.  The 3 x 3 unfold that
    query_rgb would repeat for every item of the expanded batch is taken once (`feat_unfold=False` on the unfolded map: the same
    numbers).  coord, cell [n, 2] -> [n, 3]."""
    import torch.nn.functional as F
    from oracle import ciaosr_oracle as orc
    _, c_, h_, w_ = feature.shape
    unfolded = F.unfold(feature, 3, padding=1).view(1, c_ * 9, h_, w_)
    outs = []
    for s in range(0, coord.shape[0], step):
        c, l = coord[s:s + step].unsqueeze(1), cell[s:s + step].unsqueeze(1)
        b = c.shape[0]
        pred = orc.query_rgb(unfolded.expand(b, -1, -1, -1), c, l, params, feat_unfold=False, nonlocal_map=nonlocal_map.expand(b, -1, -1, -1))
        outs.append((pred + orc.bilinear_residual(x.expand(b, -1, -1, -1), c))[:, 0])
    return torch.cat(outs)


def _oracle_scene(xn, params):
    from oracle import ciaosr_oracle as orc
    with torch.no_grad():
        feature = orc.encoder_features(xn, params)
        return feature, orc.cross_scale_attention(feature, params)


def test_whole_image_per_pixel_warp_vs_oracle(dev):
    """Test 4, warp B: all 1766 inside queries against the oracle, each with its own cell and radius; bound 2e-4 (the single-footprint
    warp's on this fixture)."""
    model = _model('edsr', dev, 2)
    model.test_cfg = dict()
    h, w = B_LR
    hv, wv = B_SIZE
    hom = warp_b()
    y, x = wr.lr_points(hom, hv, wv)
    fy, fx, _ = pr.clamp(*pr.raw_jacobian(hom, hv, wv), RANGE)
    inside = wr.members(y, x, (0, 0, h, w))
    assert int(inside.sum()) == 1766 and int((fy[inside] == RANGE[0]).sum()) == 910
    coord = torch.from_numpy(wr.coord_in(y[inside], x[inside], (0, 0, h, w)))
    cell = torch.from_numpy(pr.cells_in(fy[inside], fx[inside], (0, 0, h, w)))
    lq = _lq(h, w, dev)
    params = _params(model)
    mean = torch.tensor(model.rgb_mean).view(1, 3)
    xn = lq.cpu() - mean.view(1, 3, 1, 1)
    with torch.no_grad():
        want = (_oracle_per_query(*_oracle_scene(xn, params), xn, coord, cell, params) + mean).clamp(0, 1).t()
    fill = (0.75, 0.125, 0.5)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=hom, size=(hv, wv), footprint='per-pixel', footprint_range=RANGE, fill=fill).cpu().view(3, hv * wv)
    err = (got[:, torch.from_numpy(inside)] - want).abs().max().item()
    centre = model.render_warp(enc, homography=hom, size=(hv, wv), fill=fill).cpu().view(3, hv * wv)
    print(f'per-pixel warp B vs oracle: max |diff| = {err:.3e}; per-pixel vs centre footprint: max |diff| = {(got - centre).abs().max().item():.3e}')
    assert err < 2e-4, err
    assert not torch.equal(_bits(got), _bits(centre))
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(~inside)], torch.full((hv * wv - 1766,), fill[c]))


def test_tiled_per_pixel_warp_vs_oracle_composition(dev):
    """Test 4, warp A: every 5th member of each frame, and for those pixels every frame that covers them, composed and blended per tile
    in tile order; bound 1e-4."""
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED)
    h, w = A_LR
    hv, wv = A_SIZE
    n_q = hv * wv
    frames = frames_a()
    hom = warp_a()
    y, x = wr.lr_points(hom, hv, wv)
    fy, fx, _ = pr.clamp(*pr.raw_jacobian(hom, hv, wv), RANGE)
    chosen = np.zeros(n_q, dtype=bool)
    for f in frames:
        chosen[np.flatnonzero(wr.members(y, x, f))[::5]] = True
    assert int(chosen.sum()) == 1131 and chosen[np.flatnonzero(wr.members(y, x, frames[0]))[0]]
    lq = _lq(h, w, dev)
    params = _params(model)
    mean = torch.tensor(model.rgb_mean).view(3, 1)
    xn = lq.cpu() - mean.view(1, 3, 1, 1)
    E, Wt = torch.zeros(3, n_q), torch.zeros(n_q)
    with torch.no_grad():
        for y0, x0, th, tw in frames:                                           # tile order
            mem = wr.members(y, x, (y0, x0, th, tw)) & chosen
            coord = torch.from_numpy(wr.coord_in(y[mem], x[mem], (y0, x0, th, tw)))
            cell = torch.from_numpy(pr.cells_in(fy[mem], fx[mem], (y0, x0, th, tw)))
            patch = xn[..., y0:y0 + th, x0:x0 + tw]
            out = _oracle_per_query(*_oracle_scene(patch, params), patch, coord, cell, params)
            idx = torch.from_numpy(np.flatnonzero(mem))
            E[:, idx] += out.t()
            Wt[idx] += 1
    sel = torch.from_numpy(chosen)
    want = (E[:, sel] / Wt[sel] + mean).clamp(0, 1)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=hom, size=(hv, wv), footprint='per-pixel', footprint_range=RANGE).cpu().view(3, n_q)
    err = (got[:, sel] - want).abs().max().item()
    centre = model.render_warp(enc, homography=hom, size=(hv, wv)).cpu().view(3, n_q)
    print(f'per-pixel warp A vs oracle composition: max |diff| = {err:.3e}; per-pixel vs centre footprint: max |diff| = '
          f'{(got - centre).abs().max().item():.3e}')
    assert err < 1e-4, err
    assert not torch.equal(_bits(got), _bits(centre))


def test_f16_against_fp32(dev):
    """Test 5: the f16 per-pixel render of B and of A against the fp32 one may differ by twice what the single-footprint warp (code from
    before per-pixel warps) differs by on the same fixture -- other cells move the products, not the rounding.  The figures measured on
    an MI355X (the test prints them): B per-pixel 1.079e-4 against single 1.075e-4; A 1.009e-4 against 1.042e-4."""
    model = _model('rdn', dev, 3)
    for name, cfg, lr, hom, size in (('B', dict(), B_LR, warp_b(), B_SIZE), ('A', dict(TILED), A_LR, warp_a(), A_SIZE)):
        lq = _lq(*lr, dev)
        outs = {}
        for precision in ('fp32', 'f16'):
            model.test_cfg = dict(cfg, precision=precision)
            enc = model.encode(lq, max_scale=MAX_SCALE)
            outs[precision] = (model.render_warp(enc, homography=hom, size=size, footprint='per-pixel', footprint_range=RANGE),
                               model.render_warp(enc, homography=hom, size=size))
        gap_pp = (outs['f16'][0] - outs['fp32'][0]).abs().max().item()
        gap_single = (outs['f16'][1] - outs['fp32'][1]).abs().max().item()
        print(f'warp {name}: f16 - fp32 per-pixel {gap_pp:.3e}, single footprint {gap_single:.3e}')
        assert gap_single > 0.0 and gap_pp <= 2.0 * gap_single, (name, gap_pp, gap_single)


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_render_many_with_per_pixel_warps_is_the_single_calls(dev, precision, monkeypatch):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.scene import Grid, View, Warp
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*A_LR, dev)
    h = warp_a()
    mm, fpm = map_m()
    mdev = torch.from_numpy(mm).to(dev)
    m = _view(A_ARGS, A_SIZE)
    pp = dict(footprint='per-pixel', footprint_range=RANGE)
    targets = [Grid(size=(80, 112)), View(m, A_SIZE, fill=0.25), Warp(homography=h, size=A_SIZE, fill=(0.25, 0.5, 1.0)),
               Warp(homography=h, size=A_SIZE, fill=0.75, **pp), Warp(map=mdev, fill=0.5, **pp)]
    ref = model.encode(lq, max_scale=MAX_SCALE)
    wants = [model.render(ref, size=(80, 112)), model.render_view(ref, m, A_SIZE, fill=0.25),
             model.render_warp(ref, homography=h, size=A_SIZE, fill=(0.25, 0.5, 1.0)),
             model.render_warp(ref, homography=h, size=A_SIZE, fill=0.75, **pp), model.render_warp(ref, map=mdev, fill=0.5, **pp)]
    enc = model.encode(lq, max_scale=MAX_SCALE)
    torch.cuda.synchronize()
    copies = _count_copies(monkeypatch)
    with hip_ops.profile():
        outs = model.render_many(enc, targets)
    n_copies = list(copies)
    monkeypatch.undo()
    prof = hip_ops.profile.results()
    assert n_copies == ['tolist'], n_copies                                     # ONE copy for the view and the three warps together
    assert prof['warp_pp_count']['launches'] == 2 and prof['warp_count']['launches'] == 1 and prof['view_count_many']['launches'] == 1, sorted(prof)
    assert enc.cache.builds == 4 and len(outs) == 5
    for k, (got, want) in enumerate(zip(outs, wants)):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (k, (got - want).abs().max().item())
    assert not torch.equal(_bits(outs[2]), _bits(outs[3]))
    u8 = model.render_many(enc, targets, as_u8=True)
    assert torch.equal(u8[3], model.render_warp(ref, homography=h, size=A_SIZE, fill=0.75, as_u8=True, **pp)) and enc.cache.builds == 4
    # an open max_scale: a per-pixel warp asks for 1 / lo
    open_ = model.encode(lq)
    model.render_many(open_, targets[1:4])
    assert open_.max_scale == MAX_SCALE


def test_fill_and_outputs(dev):
    """Test 7: outside pixels, NaN positions and pixels without a footprint hold `fill` exactly; as_u8, as_u16, grey and RGBA."""
    from ciaosr_amd import metrics_hip
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED)
    lq = _lq(*A_LR, dev)
    hv, wv = A_SIZE
    n_q = hv * wv
    fill = (0.25, 0.5, 1.0)
    pp = dict(footprint_range=RANGE, fill=fill)
    h = warp_a()
    y, x = wr.lr_points(h, hv, wv)
    out = ~wr.members(y, x, (0, 0, *A_LR))
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=h, size=A_SIZE, footprint='per-pixel', **pp).cpu().view(3, n_q)
    assert int(out.sum()) == 1355 and not torch.isnan(got).any()
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(out)], torch.full((1355,), fill[c])), c
    assert (got[:, torch.from_numpy(~out)] != torch.tensor(fill).view(3, 1)).any(0).float().mean() > 0.99
    # map M with differences: outside the image, and the NaN patch
    mm, _ = map_m()
    my, mx = mm[..., 0].ravel(), mm[..., 1].ravel()
    out_m = ~wr.members(my, mx, (0, 0, *A_LR))
    got = model.render_warp(enc, map=torch.from_numpy(mm).to(dev), footprint='per-pixel', **pp).cpu().view(3, n_q)
    assert int(out_m.sum()) == 1554 and not torch.isnan(got).any()
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(out_m)], torch.full((1554,), fill[c])), c
    assert (got[:, torch.from_numpy(~out_m)] != torch.tensor(fill).view(3, 1)).any(0).float().mean() > 0.99
    # a tensor with NaN entries at pixels inside the image: no footprint, so they hold fill although their position is fine
    raw = torch.from_numpy(np.stack(pr.raw_jacobian(h, hv, wv), 1).reshape(hv, wv, 2).copy())
    holes = [3499, 3377, 1521]
    for k, q in enumerate(holes):
        raw.view(-1, 2)[q, k % 2] = float('nan')
    raw32 = raw.float()                                                         # a float32 tensor is widened exactly
    out_t = out.copy()
    out_t[holes] = True
    tens = model.render_warp(enc, homography=h, size=A_SIZE, footprint=raw32.to(dev), **pp)
    flat = tens.cpu().view(3, n_q)
    assert torch.equal(_bits(tens), _bits(model.render_warp(enc, homography=h, size=A_SIZE, footprint=raw32.double().to(dev), **pp)))
    for c in range(3):
        assert torch.equal(flat[c, torch.from_numpy(out_t)], torch.full((1358,), fill[c])), c
    assert (flat[:, torch.from_numpy(~out_t)] != torch.tensor(fill).view(3, 1)).any(0).float().mean() > 0.99
    # quantised, grey and RGBA outputs of that warp
    src = dict(homography=h, size=A_SIZE, footprint=raw32.to(dev), **pp)
    u8, u16 = model.render_warp(enc, as_u8=True, **src), model.render_warp(enc, as_u16=True, **src)
    assert u8.dtype == torch.uint8 and u8.shape == (*A_SIZE, 3) and torch.equal(u8, metrics_hip.tensor2img_u8(tens))
    assert u16.dtype == torch.uint16 and torch.equal(u16.view(torch.int16), metrics_hip.tensor2img_u16(tens).view(torch.int16))
    grey = model.encode_grey(lq[:, :1].contiguous(), max_scale=MAX_SCALE)
    g32, g8 = model.render_warp(grey, **src), model.render_warp(grey, as_u8=True, **src)
    assert g32.shape == (1, 3, *A_SIZE) and g8.shape == A_SIZE and torch.equal(g8, metrics_hip.tensor2img_grey_u8(g32))
    rgba = model.encode_rgba(torch.cat([lq, torch.full((1, 1, *A_LR), 0.9, device=dev)], 1), max_scale=MAX_SCALE)
    b8 = model.render_warp(rgba, as_u8=True, **src)
    assert b8.shape == (*A_SIZE, 4) and torch.equal(b8[..., :3], u8)
    a = b8[..., 3].cpu().view(-1)
    assert (a[torch.from_numpy(out_t)] == 0).all() and (a[torch.from_numpy(~out_t)] > 0).float().mean() > 0.5


def test_render_cli_per_pixel_footprint(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_rgb01
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=SQRT6)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray((_lq(24, 24, 'cpu', seed=8)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(png)
    h = warp_b()
    flags = ['--homography', *[repr(v) for v in h], '--size', str(B_SIZE[0]), str(B_SIZE[1])]
    paths = render.main([config, ckpt, png, *flags, '--footprint', 'per-pixel', '--footprint-range', '0.32', '0.6', '--out', str(tmp_path / 'out')])
    assert [os.path.basename(p) for p in paths] == ['img_warp0.png']
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                                           # what the tool sets
    enc = model.encode(imread_rgb01(png).unsqueeze(0).to(dev), max_scale=MAX_SCALE)
    want = model.render_warp(enc, homography=h, size=B_SIZE, footprint='per-pixel', footprint_range=RANGE, as_u8=True).cpu().numpy()    # B G R
    got = np.asarray(Image.open(paths[0]).convert('RGB'))
    assert got.shape == (*B_SIZE, 3) and np.array_equal(got[..., ::-1], want)
    plain = render.main([config, ckpt, png, *flags, '--max-scale', repr(MAX_SCALE), '--out', str(tmp_path / 'plain')])
    assert open(plain[0], 'rb').read() != open(paths[0], 'rb').read()
    for bad in (['--footprint-range', '0.32', '0.6'], ['--footprint', 'per-pixel', '--footprint-range', '0.6', '0.32'], ['--footprint', 'centre']):
        with pytest.raises(SystemExit):
            render.parse_args([config, ckpt, png, *flags, *bad, '--out', str(tmp_path / 'no')])
    with pytest.raises(SystemExit):
        render.parse_args([config, ckpt, png, '--scale', '2', '--footprint', 'per-pixel', '--out', str(tmp_path / 'no')])
