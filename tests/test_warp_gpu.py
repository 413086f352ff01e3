"""Warps of an encoded scene on the GPU: the count / select / coordinate kernels of both point sources against the definition in numpy
float64 (tests/warp_reference.py); CiaoSR.render_warp of an affine warp bitwise against render_view (the yardstick), of a map against
its homography, against the torch-CPU oracle, its fill, its quantised outputs, render_many / prefetch with warps, `view_blocks`, and
tools/render.py --homography."""
import os

import numpy as np
import pytest
import torch

from tests import view_reference as vr
from tests import warp_reference as wr
from tests.helpers import SQRT6
from tests.test_view_gpu import A_ONE_TILE_SHIFT, _bits, _lq, _model, _params, _tiles, _view
from tests.test_warp_host import A_ARGS, A_LR, A_SIZE, B_ARGS, B_LR, B_SIZE, frames_a, map_m, warp_a, warp_b

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED = dict(tile=32, tile_overlap=8, tile_any_scale=True)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _view_fp(m):
    from ciaosr_amd import scene
    return scene.warp_footprint(scene.homography_of_view(m), (1, 1))


def _points_map(y, x, hv, wv, dev):
    return torch.from_numpy(np.ascontiguousarray(np.stack([y, x], 1).reshape(hv, wv, 2))).to(dev)


def _check_kernels_against_numpy(h, mp, fp, y, x, hv, wv, frames, dev):
    """Count, select and the whole grid's coordinates of one warp (`h` or the device map `mp`) whose points are (y, x): counts and
    q_index equal, coord and cell bitwise; everything run twice."""
    from ciaosr_amd import hip_ops
    tiles = _tiles(frames, dev)
    want_counts = [int(wr.members(y, x, f).sum()) for f in frames]
    runs = []
    for _ in range(2):
        counts, ws = hip_ops.warp_count(h, mp, fp, hv, wv, tiles)
        counts = counts.tolist()
        assert counts == want_counts, (counts, want_counts)
        out = []
        for k, (frame, n) in enumerate(zip(frames, counts)):
            if n == 0:
                continue
            q_index, coord, cell = hip_ops.warp_select(h, mp, fp, hv, wv, frame, k, len(frames), ws, n)
            mem = wr.members(y, x, frame)
            assert np.array_equal(q_index.cpu().numpy(), np.flatnonzero(mem).astype(np.int32)), frame
            want = wr.coord_in(y[mem], x[mem], frame)
            assert np.array_equal(coord.cpu().numpy().view(np.int32), want.view(np.int32)), (frame, np.abs(coord.cpu().numpy() - want).max())
            want_cell = np.ascontiguousarray(np.broadcast_to(wr.cell_in(fp, frame), (n, 2)))
            assert np.array_equal(cell.cpu().numpy().view(np.int32), want_cell.view(np.int32)), frame
            assert hip_ops.grid_width_of(coord) == 0
            out += [q_index, coord, cell]
        coord, cell = hip_ops.make_coord_cell_warp(h, mp, fp, hv, wv, frames[-1], dev)        # the whole grid, without selection
        fin = np.isfinite(y)
        want = wr.coord_in(np.where(fin, y, 0.0), np.where(fin, x, 0.0), frames[-1])
        got = coord.cpu().numpy()
        assert np.array_equal(got.view(np.int32)[fin], want.view(np.int32)[fin]) and np.isnan(got[~fin]).all()
        assert np.array_equal(cell.cpu().numpy().view(np.int32),
                              np.ascontiguousarray(np.broadcast_to(wr.cell_in(fp, frames[-1]), (hv * wv, 2))).view(np.int32))
        assert hip_ops.grid_width_of(coord) == wv
        runs.append((counts, out + [coord, cell]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0][1], runs[1][1]))
    return counts


def test_count_select_and_coordinates_against_the_definition(dev):
    from ciaosr_amd import hip_ops, scene
    chunk = hip_ops.view_block_queries()
    frames = frames_a()
    # warp A
    h = warp_a()
    fp = scene.warp_footprint(h, A_SIZE)
    y, x = wr.lr_points(h, *A_SIZE)
    assert A_SIZE[0] * A_SIZE[1] > 4 * chunk                                   # several workgroups, the last one ragged
    assert _check_kernels_against_numpy(h, None, fp, y, x, *A_SIZE, frames, dev) == [757, 2456, 860, 3614]
    # map M, with its NaN patch
    mm, fpm = map_m()
    assert _check_kernels_against_numpy(None, torch.from_numpy(mm).to(dev), fpm, mm[..., 0].ravel(), mm[..., 1].ravel(), *A_SIZE, frames,
                                        dev) == [375, 2312, 577, 3506]
    # one query: near LR point (5, 30), in the two upper tiles -- as a homography and as a map
    h1 = (*scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1)), 0.0025, -0.002, 1.0)
    y1, x1 = wr.lr_points(h1, 1, 1)
    assert _check_kernels_against_numpy(h1, None, (0.37, 0.37), y1, x1, 1, 1, frames, dev) == [1, 1, 0, 0]
    assert _check_kernels_against_numpy(None, _points_map(y1, x1, 1, 1, dev), (0.37, 0.37), y1, x1, 1, 1, frames, dev) == [1, 1, 0, 0]
    # three very wide rows: more than one workgroup per row pair, members of all four tiles, some outside
    wide = 700
    assert 3 * wide > 2 * chunk and wide < chunk
    hw = (*scene.view_matrix((20.0, 28.0), 11.0, 7, (3, wide)), 0.0, 0.0004, 1.0)
    yw, xw = wr.lr_points(hw, 3, wide)
    fpw = scene.warp_footprint(hw, (3, wide))
    counts = _check_kernels_against_numpy(hw, None, fpw, yw, xw, 3, wide, frames, dev)
    assert all(c > 0 for c in counts) and max(counts) < 3 * wide
    assert _check_kernels_against_numpy(None, _points_map(yw, xw, 3, wide, dev), fpw, yw, xw, 3, wide, frames, dev) == counts
    # a float64 map is required here: the wrappers refuse anything else, and a host map
    with pytest.raises(ValueError):
        hip_ops.warp_count(None, torch.zeros(3, wide, 2, device=dev), fpw, 3, wide, _tiles(frames, dev))
    with pytest.raises(hip_ops.CiaoSRHipError):
        hip_ops.warp_count(None, torch.zeros(3, wide, 2, dtype=torch.float64), fpw, 3, wide, _tiles(frames, dev))


def _shift(m, shift):
    m = list(m)
    m[2] += shift[0]
    m[5] += shift[1]
    return tuple(m)


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_an_affine_warp_is_render_view_bitwise(dev, precision):
    """The yardstick: the affine-degenerate homography, and the map holding the view's own points, are render_view of the matrix."""
    from ciaosr_amd import hip_ops, scene
    model = _model('rdn', dev, 3)
    cases = [('B whole', dict(precision=precision), B_LR, _view(B_ARGS, B_SIZE), B_SIZE, 1),
             ('A tiled', dict(TILED, precision=precision), A_LR, _view(A_ARGS, A_SIZE), A_SIZE, 4),
             ('A in one tile', dict(TILED, precision=precision), A_LR, _shift(_view(A_ARGS, A_SIZE), A_ONE_TILE_SHIFT), A_SIZE, 1)]
    for name, cfg, (h, w), m, size, builds in cases:
        model.test_cfg = dict(cfg)
        lq = _lq(h, w, dev)
        fill = (0.25, 0.5, 1.0)
        ref = model.encode(lq)
        want = model.render_view(ref, m, size, fill=fill)
        assert ref.cache.builds == builds, name
        y, x = vr.lr_points(m, *size)
        for source in (dict(homography=scene.homography_of_view(m), size=size), dict(map=_points_map(y, x, *size, dev), footprint=_view_fp(m))):
            enc = model.encode(lq)
            got = model.render_warp(enc, fill=fill, **source)
            assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, sorted(source), (got - want).abs().max().item())
            assert enc.cache.builds == builds and enc.max_scale == ref.max_scale, name
    # The shifted view A has its 515 members in tile (0, 0) alone, but most of its pixels lie outside the image: a member list.  The
    # branch "the frame owns every query" needs a warp wholly inside a tile: this one lies inside tile (0, 0), which walks it as a grid
    # with the grid-width hint, as the view does, while tile (8, 0) sees a part of it as a list.
    frames = frames_a()
    size = (30, 30)
    m = _view(((12, 12), 2.0, 12), size)
    y, x = vr.lr_points(m, *size)
    assert vr.members(y, x, (0, 0, 32, 32)).all() and not vr.members(y, x, (0, 24, 32, 32)).any() and not vr.members(y, x, (8, 0, 32, 32)).all()
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*A_LR, dev)
    want = model.render_view(model.encode(lq, max_scale=30 / 32), m, size)
    for source in (dict(homography=scene.homography_of_view(m), size=size), dict(map=_points_map(y, x, *size, dev), footprint=_view_fp(m))):
        enc = model.encode(lq, max_scale=30 / 32)
        got = model.render_warp(enc, **source)
        assert torch.equal(_bits(got), _bits(want)), sorted(source)
    coord_v, cell_v = hip_ops.make_coord_cell_view(m, *size, frames[0], dev)
    coord_w, cell_w = hip_ops.make_coord_cell_warp(scene.homography_of_view(m), None, _view_fp(m), *size, frames[0], dev)
    assert hip_ops.grid_width_of(coord_w) == hip_ops.grid_width_of(coord_v) == 30
    assert torch.equal(_bits(coord_w), _bits(coord_v)) and torch.equal(_bits(cell_w), _bits(cell_v))


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_a_map_of_the_homography_points_is_the_homography_render(dev, precision):
    from ciaosr_amd import scene
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*A_LR, dev)
    h = warp_a()
    y, x = wr.lr_points(h, *A_SIZE)
    enc = model.encode(lq)
    want = model.render_warp(enc, homography=h, size=A_SIZE, fill=0.5)
    assert enc.cache.builds == 4 and enc.max_scale == wr.max_scale(wr.centre_footprint(h, *A_SIZE))
    enc_m = model.encode(lq)
    got = model.render_warp(enc_m, map=_points_map(y, x, *A_SIZE, dev), footprint=scene.warp_footprint(h, A_SIZE), fill=0.5)
    assert torch.equal(_bits(got), _bits(want)) and enc_m.cache.builds == 4 and enc_m.max_scale == enc.max_scale
    assert torch.equal(_bits(model.render_warp(enc, homography=h, size=A_SIZE, fill=0.5)), _bits(want)) and enc.cache.builds == 4
    # a float32 map is widened exactly: the render of the float64 map that holds the same numbers
    m32 = _points_map(y, x, *A_SIZE, dev).float()
    fp = scene.warp_footprint(h, A_SIZE)
    assert torch.equal(_bits(model.render_warp(enc, map=m32, footprint=fp)), _bits(model.render_warp(enc, map=m32.double(), footprint=fp)))


def test_tiled_warp_vs_oracle_composition(dev):
    """Warp A against the per-tile composition of the torch-CPU oracle (tests/test_view_gpu.py's, with the warp's points and cell)."""
    from oracle import ciaosr_oracle as orc
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED)
    h, w = A_LR
    hv, wv = A_SIZE
    n_q = hv * wv
    frames = frames_a()
    hom = warp_a()
    fp = wr.centre_footprint(hom, hv, wv)
    y, x = wr.lr_points(hom, hv, wv)
    lq = _lq(h, w, dev)
    params = _params(model)
    mean = torch.tensor(model.rgb_mean).view(3, 1)
    xn = lq.cpu() - mean.view(1, 3, 1, 1)
    E, Wt = torch.zeros(3, n_q), torch.zeros(n_q)
    for y0, x0, th, tw in frames:                                               # tile order
        mem = wr.members(y, x, (y0, x0, th, tw))
        coord = torch.from_numpy(wr.coord_in(y[mem], x[mem], (y0, x0, th, tw))).unsqueeze(0)
        cell = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(wr.cell_in(fp, (y0, x0, th, tw)), (int(mem.sum()), 2)))).unsqueeze(0)
        out = orc.generator_forward(xn[..., y0:y0 + th, x0:x0 + tw], coord, cell, params)
        idx = torch.from_numpy(np.flatnonzero(mem))
        E[:, idx] += out[0].t()
        Wt[idx] += 1
    claimed = Wt > 0
    want = (E / Wt + mean).clamp(0, 1)
    enc = model.encode(lq)
    got = model.render_warp(enc, homography=hom, size=(hv, wv))
    assert got.shape == (1, 3, hv, wv) and enc.cache.builds == 4
    flat = got.cpu().view(3, n_q)
    err = (flat[:, claimed] - want[:, claimed]).abs().max().item()
    print(f'warp A vs oracle composition: max |diff| = {err:.3e}')
    assert err < 1e-4, err
    assert int((~claimed).sum()) == 1355 and torch.equal(flat[:, ~claimed], torch.zeros(3, 1355))


def test_whole_image_warp_vs_oracle(dev):
    """Warp B against the oracle's forward_test on the inside queries, padded to a square as tests/test_view_gpu.py pads them."""
    from oracle import ciaosr_oracle as orc
    model = _model('edsr', dev, 2)
    model.test_cfg = dict()
    h, w = B_LR
    hv, wv = B_SIZE
    hom = warp_b()
    fp = wr.centre_footprint(hom, hv, wv)
    y, x = wr.lr_points(hom, hv, wv)
    inside = wr.members(y, x, (0, 0, h, w))
    n = int(inside.sum())
    side = int(np.ceil(np.sqrt(n)))
    assert n == 1766 and side == 43 and round(h * np.sqrt(side * side / (h * w))) == side
    coord = torch.from_numpy(wr.coord_in(y[inside], x[inside], (0, 0, h, w)))
    cell = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(wr.cell_in(fp, (0, 0, h, w)), (n, 2))))
    pad = side * side - n
    lq = _lq(h, w, dev)
    want = orc.forward_test(lq.cpu(), torch.cat([coord, coord[:pad]]).unsqueeze(0), torch.cat([cell, cell[:pad]]).unsqueeze(0), _params(model))
    want = want.view(3, side * side)[:, :n]
    fill = (0.75, 0.125, 0.5)
    enc = model.encode(lq)
    got = model.render_warp(enc, homography=hom, size=(hv, wv), fill=fill).cpu()
    assert got.shape == (1, 3, hv, wv) and enc.max_scale == wr.max_scale(fp) and enc.cache.builds == 1
    got = got.view(3, hv * wv)
    err = (got[:, torch.from_numpy(inside)] - want).abs().max().item()
    print(f'warp B vs oracle: max |diff| = {err:.3e}')
    assert err < 2e-4, err
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(~inside)], torch.full((hv * wv - n,), fill[c]))


@pytest.mark.parametrize('fill', [0.0, (0.25, 0.5, 1.0)])
def test_outside_pixels_and_nan_hold_fill_exactly(dev, fill):
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED)
    lq = _lq(*A_LR, dev)
    fill3 = fill if isinstance(fill, tuple) else (fill,) * 3
    n_q = A_SIZE[0] * A_SIZE[1]
    # warp A: the pixels outside the image
    h = warp_a()
    y, x = wr.lr_points(h, *A_SIZE)
    out = ~wr.members(y, x, (0, 0, *A_LR))
    got = model.render_warp(model.encode(lq), homography=h, size=A_SIZE, fill=fill).cpu().view(3, n_q)
    assert int(out.sum()) == 1355 and not torch.isnan(got).any()
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(out)], torch.full((1355,), fill3[c])), c
    assert (got[:, torch.from_numpy(~out)] != torch.tensor(fill3).view(3, 1)).any(0).float().mean() > 0.99        # the model's answer elsewhere
    # map M: outside the image, and the NaN patch
    mm, fpm = map_m()
    my, mx = mm[..., 0].ravel(), mm[..., 1].ravel()
    out = ~wr.members(my, mx, (0, 0, *A_LR))
    nan = np.isnan(my)
    assert int(out.sum()) == 1554 and int(nan.sum()) == 35 and out[nan].all()
    got = model.render_warp(model.encode(lq), map=torch.from_numpy(mm).to(dev), footprint=fpm, fill=fill).cpu().view(3, n_q)
    assert not torch.isnan(got).any()
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(out)], torch.full((1554,), fill3[c])), c
    assert (got[:, torch.from_numpy(~out)] != torch.tensor(fill3).view(3, 1)).any(0).float().mean() > 0.99


def test_quantised_grey_and_rgba_outputs(dev):
    from ciaosr_amd import metrics_hip
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED)
    lq = _lq(*A_LR, dev)
    h = warp_a()
    fill = (0.25, 0.5, 1.0)
    y, x = wr.lr_points(h, *A_SIZE)
    out = torch.from_numpy(~wr.members(y, x, (0, 0, *A_LR))).view(*A_SIZE)
    enc = model.encode(lq)
    f32 = model.render_warp(enc, homography=h, size=A_SIZE, fill=fill)
    u8 = model.render_warp(enc, homography=h, size=A_SIZE, fill=fill, as_u8=True)
    u16 = model.render_warp(enc, homography=h, size=A_SIZE, fill=fill, as_u16=True)
    assert u8.dtype == torch.uint8 and u8.shape == (*A_SIZE, 3) and torch.equal(u8, metrics_hip.tensor2img_u8(f32))
    assert u16.dtype == torch.uint16 and u16.shape == (*A_SIZE, 3) and torch.equal(u16.view(torch.int16), metrics_hip.tensor2img_u16(f32).view(torch.int16))
    # a grey record: 2-D images
    grey = model.encode_grey(lq[:, :1].contiguous())
    g32 = model.render_warp(grey, homography=h, size=A_SIZE, fill=0.5)
    g8 = model.render_warp(grey, homography=h, size=A_SIZE, fill=0.5, as_u8=True)
    g16 = model.render_warp(grey, homography=h, size=A_SIZE, fill=0.5, as_u16=True)
    assert g32.shape == (1, 3, *A_SIZE) and g8.shape == A_SIZE and g8.dtype == torch.uint8 and g16.shape == A_SIZE and g16.dtype == torch.uint16
    assert torch.equal(g8, metrics_hip.tensor2img_grey_u8(g32)) and torch.equal(g16.view(torch.int16), metrics_hip.tensor2img_grey_u16(g32).view(torch.int16))
    # an RGBA record: A = 0 exactly where no frame claims the pixel, the colour bytes those of the colour render
    alpha = torch.full((1, 1, *A_LR), 0.9, device=dev)
    rgba = model.encode_rgba(torch.cat([lq, alpha], 1))
    b8 = model.render_warp(rgba, homography=h, size=A_SIZE, fill=fill, as_u8=True)
    assert b8.shape == (*A_SIZE, 4) and b8.dtype == torch.uint8
    assert torch.equal(b8[..., :3], u8)
    pair = model.render_warp(rgba, homography=h, size=A_SIZE, fill=fill)
    assert pair.shape == (2, 3, *A_SIZE) and torch.equal(pair[0], f32[0]) and (pair[1].cpu()[:, out] == 0).all()
    assert torch.equal(b8, metrics_hip.tensor2img_bgra_u8(pair))
    a = b8[..., 3].cpu()
    assert (a[out] == 0).all() and (a[~out] > 0).float().mean() > 0.5
    with pytest.raises(ValueError, match='as_u16'):
        model.render_warp(rgba, homography=h, size=A_SIZE, as_u16=True)


def _count_copies(monkeypatch):
    """Every way a device tensor reaches the host: the synchronising copies of a call."""
    copies = []
    for name in ('tolist', 'cpu', 'item', 'numpy'):
        inner = getattr(torch.Tensor, name)

        def counted(self, *a, _inner=inner, _name=name, **kw):
            if self.is_cuda:
                copies.append(_name)
            return _inner(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, name, counted)
    return copies


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_render_many_with_warps_is_the_single_calls(dev, precision, monkeypatch):
    from ciaosr_amd import hip_ops, scene
    from ciaosr_amd.scene import Grid, View, Warp
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*A_LR, dev)
    h = warp_a()
    mm, fpm = map_m()
    mdev = torch.from_numpy(mm).to(dev)
    m = _view(A_ARGS, A_SIZE)
    targets = [Grid(size=(80, 112)), View(m, A_SIZE, fill=0.25), Warp(homography=h, size=A_SIZE, fill=(0.25, 0.5, 1.0)),
               Warp(map=mdev, footprint=fpm, fill=0.5)]
    ref = model.encode(lq, max_scale=2.7)
    wants = [model.render(ref, size=(80, 112)), model.render_view(ref, m, A_SIZE, fill=0.25),
             model.render_warp(ref, homography=h, size=A_SIZE, fill=(0.25, 0.5, 1.0)), model.render_warp(ref, map=mdev, footprint=fpm, fill=0.5)]
    enc = model.encode(lq, max_scale=2.7)
    torch.cuda.synchronize()
    copies = _count_copies(monkeypatch)
    with hip_ops.profile():
        outs = model.render_many(enc, targets)
    n_copies = list(copies)
    monkeypatch.undo()
    prof = hip_ops.profile.results()
    assert n_copies == ['tolist'], n_copies                                     # ONE copy for the view and both warps together
    assert prof['warp_count']['launches'] == 2 and prof['view_count_many']['launches'] == 1 and 'view_count' not in prof, sorted(prof)
    assert enc.cache.builds == 4 and len(outs) == 4
    for k, (got, want) in enumerate(zip(outs, wants)):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (k, (got - want).abs().max().item())
    u8 = model.render_many(enc, targets, as_u8=True)
    assert torch.equal(u8[2], model.render_warp(ref, homography=h, size=A_SIZE, fill=(0.25, 0.5, 1.0), as_u8=True)) and enc.cache.builds == 4
    # warps alone; prefetch builds the scenes the render then finds cached
    fresh = model.encode(lq, max_scale=2.7)
    assert model.prefetch(fresh, targets[2:]) == 4 and fresh.cache.builds == 4
    alone = model.render_many(fresh, targets[2:])
    assert fresh.cache.builds == 4 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(alone, wants[2:]))
    assert model.prefetch(fresh, targets) == 0
    one = model.encode(lq, max_scale=2.7)                                       # members in tile (0, 0) alone: that scene alone
    shifted = scene.homography_of_view(_shift(m, A_ONE_TILE_SHIFT))
    assert model.prefetch(one, [Warp(homography=shifted, size=A_SIZE)]) == 1 and list(one.cache.entries) == [(0, (0, 0))]
    # an open max_scale is the largest any target needs
    open_ = model.encode(lq)
    model.render_many(open_, targets[1:3])
    assert open_.max_scale == max(scene.view_max_scale(m), wr.max_scale(wr.centre_footprint(h, *A_SIZE)))


def test_view_blocks_is_ignored_for_warps(dev):
    model = _model('rdn', dev, 3)
    lq = _lq(*A_LR, dev)
    h = warp_a()
    mm, fpm = map_m()
    outs = []
    for blocks in (False, True):
        model.test_cfg = dict(TILED, precision='f16', view_blocks=blocks)
        enc = model.encode(lq, max_scale=2.7)
        outs.append((model.render_warp(enc, homography=h, size=A_SIZE), model.render_warp(enc, map=torch.from_numpy(mm).to(dev), footprint=fpm)))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


def test_render_cli_homography(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model, scene
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
    paths = render.main([config, ckpt, png, *flags, '--out', str(tmp_path / 'out')])
    assert [os.path.basename(p) for p in paths] == ['img_warp0.png']
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                                           # what the tool sets
    fp = scene.warp_footprint(h, B_SIZE)
    enc = model.encode(imread_rgb01(png).unsqueeze(0).to(dev), max_scale=scene.warp_max_scale(fp))
    want = model.render_warp(enc, homography=h, size=B_SIZE, as_u8=True).cpu().numpy()             # B G R
    got = np.asarray(Image.open(paths[0]).convert('RGB'))
    assert got.shape == (*B_SIZE, 3) and np.array_equal(got[..., ::-1], want)
    # alongside a scale and a view: the sizes are the views' first, and the other outputs do not change
    both = render.main([config, ckpt, png, '--scale', '2', '--view', '12', '12', '2.5', '30', '--size', '40', '52', *flags, '--out', str(tmp_path / 'both')])
    assert [os.path.basename(p) for p in both] == ['img_x2.png', 'img_view0.png', 'img_warp0.png']
    plain = render.main([config, ckpt, png, '--scale', '2', '--view', '12', '12', '2.5', '30', '--size', '40', '52', '--out', str(tmp_path / 'plain')])
    for a, b in zip(plain, both):
        assert open(a, 'rb').read() == open(b, 'rb').read(), a
    for bad in (['--self-ensemble', '--scale', '2'], ['--tiff', '--scale', '2']):
        with pytest.raises(SystemExit):
            render.parse_args([config, ckpt, png, *flags, *bad, '--out', str(tmp_path / 'no')])
