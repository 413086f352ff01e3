"""Area-sampled warps on the GPU: the table, count and select kernels against the definition in numpy float64
(tests/warp_area_reference.py), bit for bit; (i) where nothing minifies `minify='area'` is `minify='clamp'`; (ii) uniform sample counts
are the box mean of the finer single-footprint warp, bit for bit in fp32; the torch-CPU oracle asked one query per batch item and
averaged in float64; f16 against fp32; render_many with one copy; the quantised, grey and RGBA outputs, prefetch and tools/render.py."""
import os

import numpy as np
import pytest
import torch

from tests import warp_area_reference as ar
from tests import warp_pp_reference as pr
from tests import warp_reference as wr
from tests.helpers import SQRT6
from tests.test_view_gpu import _bits, _lq, _model, _params, _tiles, _view
from tests.test_warp_area_host import C_LR, C_N, C_RANGE, C_SIZE, Q_INF, Q_LOW, Q_NAN, Q_NEG, frames_c, tensor_c, warp_c
from tests.test_warp_gpu import TILED, _count_copies
from tests.test_warp_host import A_ARGS, A_LR, A_SIZE, B_LR, B_SIZE, warp_a, warp_b
from tests.test_warp_pp_gpu import _oracle_per_query, _oracle_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SCALE = 1.0 / C_RANGE[0]
WHOLE = (0, 0, *C_LR)
AREA = dict(footprint='per-pixel', footprint_range=C_RANGE, minify='area')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _check_kernels(h, spec, gy, gx, rng, n_max, hv, wv, frames, dev):
    """The table, the per-tile counts and every tile's list of one area-sampled warp with the raw footprints (gy, gx): integers equal,
    coord and cell bitwise; everything run twice.  -> (S, counts)."""
    from ciaosr_amd import hip_ops
    first, ny, nx, fy, fx = ar.table(gy, gx, rng, n_max)
    pix, y, x, sfy, sfx = ar.samples(h, hv, wv, first, ny, nx, fy, fx)
    tiles = _tiles(frames, dev)
    want_counts = [int(wr.members(y, x, f).sum()) for f in frames] + [int(first[-1]), int((ny * nx == 1).sum())]
    runs = []
    for _ in range(2):
        got_first, got_n = hip_ops.warp_area_table(h, spec, hv, wv, dev)
        assert got_first.dtype == torch.int32 and got_first.shape == (hv * wv + 1,) and got_n.shape == (hv, wv, 2)
        assert np.array_equal(got_first.cpu().numpy(), first) and np.array_equal(got_n.cpu().numpy().reshape(-1, 2), np.stack([ny, nx], 1))
        counts, ws = hip_ops.warp_area_count(h, spec, hv, wv, tiles)
        counts = counts.tolist()
        assert counts == want_counts, (counts, want_counts)
        out = [got_first, got_n]
        for k, (frame, n) in enumerate(zip(frames, counts[:len(frames)])):
            if n == 0:
                continue
            s_index, coord, cell = hip_ops.warp_area_select(h, n_max, hv, wv, frame, k, len(frames), ws, counts[len(frames)], n)
            mem = wr.members(y, x, frame)
            assert np.array_equal(s_index.cpu().numpy(), np.flatnonzero(mem).astype(np.int32)), frame
            want = wr.coord_in(y[mem], x[mem], frame)
            assert np.array_equal(coord.cpu().numpy().view(np.int32), want.view(np.int32)), frame
            want_cell = pr.cells_in(sfy[mem], sfx[mem], frame)
            assert np.array_equal(cell.cpu().numpy().view(np.int32), want_cell.view(np.int32)), frame
            assert hip_ops.grid_width_of(coord) == 0
            out += [s_index, coord, cell]
        runs.append((counts, out))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8)) for a, b in zip(runs[0][1], runs[1][1]))
    return int(first[-1]), counts[:len(frames)]


def test_kernels_against_the_definition(dev):
    """Test 1: warp C (Jacobian) with max_samples 1, 2, 4 and the tensor variant (a NaN, a +inf, a value below lo, a negative entry) with
    8 as well, over the four tiles and over the whole image; and under a range whose lo raises the footprint of split pixels."""
    from ciaosr_amd import hip_ops, scene
    h = warp_c()
    hv, wv = C_SIZE
    gy, gx = pr.raw_jacobian(h, hv, wv)
    totals = {}
    for n_max in (1, 2, 4):
        spec = scene.PerPixel(scene.FP_JACOBIAN, C_RANGE, None, n_max)
        totals[n_max], counts = _check_kernels(h, spec, gy, gx, C_RANGE, n_max, hv, wv, frames_c(), dev)
        assert sum(counts) > totals[n_max] // 2                                  # overlapping tiles: most samples are in one at least
        _check_kernels(h, spec, gy, gx, C_RANGE, n_max, hv, wv, [WHOLE], dev)
    assert totals == {1: hv * wv, 2: 3121, 4: 4661}
    raw = tensor_c()
    tdev = torch.from_numpy(raw).to(dev)
    ty, tx = raw[..., 0].ravel(), raw[..., 1].ravel()
    for n_max in (1, 2, 4, 8):
        for rng in (C_RANGE, (0.7, 1.0)):
            spec = scene.PerPixel(scene.FP_TENSOR, rng, tdev, n_max)
            _check_kernels(h, spec, ty, tx, rng, n_max, hv, wv, frames_c(), dev)
    first, ny, nx, fy, fx = ar.table(ty, tx, (0.7, 1.0), 8)
    assert ny[Q_NAN] == 0 and nx[Q_INF] == 8 and fx[Q_INF] == 1.0 and fy[Q_LOW] == 0.7 and fy[Q_NEG] == 0.7
    assert int(((ny > 1) & (fy == 0.7)).sum()) > 100                             # split pixels whose g / n fell below lo
    # the device table is scene.py's restatement
    got_first, got_n = hip_ops.warp_area_table(h, scene.PerPixel(scene.FP_JACOBIAN, C_RANGE, None, C_N), hv, wv, dev)
    s_first, s_n, _ = scene.warp_area_table(h, C_SIZE, C_RANGE, C_N)
    assert got_first.tolist() == s_first and [tuple(v) for v in got_n.view(-1, 2).tolist()] == s_n
    # the wrappers refuse a map source, a float32 and a host tensor
    with pytest.raises(ValueError):
        hip_ops.warp_area_count(None, scene.PerPixel(scene.FP_JACOBIAN, C_RANGE, None, 4), hv, wv, _tiles(frames_c(), dev))
    with pytest.raises(ValueError):
        hip_ops.warp_area_count(h, scene.PerPixel(scene.FP_TENSOR, C_RANGE, tdev.float(), 4), hv, wv, _tiles(frames_c(), dev))
    with pytest.raises(hip_ops.CiaoSRHipError):
        hip_ops.warp_area_count(h, scene.PerPixel(scene.FP_TENSOR, C_RANGE, tdev.cpu(), 4), hv, wv, _tiles(frames_c(), dev))


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_where_nothing_minifies_area_is_clamp_bitwise(dev, precision):
    """Test 2, consequence (i): warps A (tiled) and B (whole image) with hi above every raw footprint, the 30 x 30 warp inside one tile
    that stays a grid walk, and warp C with max_samples = 1."""
    from ciaosr_amd import hip_ops, scene
    model = _model('rdn', dev, 3)
    wide = (0.25, 0.9)
    small = scene.homography_of_view(_view(((12, 12), 2.0, 12), (30, 30)))
    cases = [('B whole', dict(precision=precision), B_LR, warp_b(), B_SIZE, wide, 4),
             ('A tiled', dict(TILED, precision=precision), A_LR, warp_a(), A_SIZE, wide, 4),
             ('a grid in one tile', dict(TILED, precision=precision), A_LR, small, (30, 30), wide, 4),
             ('C, one sample', dict(TILED, precision=precision), C_LR, warp_c(), C_SIZE, C_RANGE, 1)]
    fill = (0.25, 0.5, 1.0)
    for name, cfg, (h, w), hom, size, rng, n_max in cases:
        model.test_cfg = dict(cfg)
        enc = model.encode(_lq(h, w, dev), max_scale=MAX_SCALE)
        src = dict(homography=hom, size=size, footprint='per-pixel', footprint_range=rng, fill=fill)
        want = model.render_warp(enc, **src)
        with hip_ops.profile():
            got = model.render_warp(enc, minify='area', max_samples=n_max, **src)
        prof = hip_ops.profile.results()
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, (got - want).abs().max().item())
        assert 'warp_area_resolve' not in prof and prof['warp_area_count']['launches'] == 1, (name, sorted(prof))
        if name == 'a grid in one tile':
            assert prof['warp_pp_coord_cell']['launches'] == 1, sorted(prof)     # tile (0, 0) owns every pixel: walked as a grid
        tensor = torch.from_numpy(np.stack(pr.raw_jacobian(hom, *size), 1).reshape(*size, 2).copy()).to(dev)
        got = model.render_warp(enc, minify='area', max_samples=n_max, **dict(src, footprint=tensor))
        assert torch.equal(_bits(got), _bits(want)), (name, 'tensor')


def _fine(h, ny, nx):
    """The homography of the (ny Hv) x (nx Wv) grid whose pixel centres are the samples of ny x nx per pixel: the first column over ny,
    the second over nx (exact)."""
    return (h[0] / ny, h[1] / nx, h[2], h[3] / ny, h[4] / nx, h[5], h[6] / ny, h[7] / nx, h[8])


@pytest.mark.parametrize('tiled', [True, False])
def test_uniform_counts_are_the_box_mean_of_the_fine_grid_bitwise(dev, tiled):
    """Test 3, consequence (ii), fp32: every pixel has the same n_y x n_x, so the samples are the pixel centres of the finer grid and
    their footprint is (1, 1): the render is the box mean, in sample order, of the single-footprint warp on that grid -- seams, cut
    border pixels and `fill` included."""
    from ciaosr_amd import scene
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED) if tiled else dict()
    size = (24, 34)
    lq = _lq(*C_LR, dev)
    fill = (0.25, 0.5, 1.0)
    zoom_out = scene.homography_of_view(scene.view_matrix((21.0, 27.5), 0.5, 0, size))
    turned = scene.homography_of_view(scene.view_matrix((21.0, 27.5), 0.5, -32, size))

    def const(gy, gx):
        return torch.tensor((gy, gx), dtype=torch.float64, device=dev).expand(*size, 2)

    cases = [('g = 2 from the Jacobian', zoom_out, 'per-pixel', (2, 2)), ('turned, tensor (2, 2)', turned, const(2.0, 2.0), (2, 2)),
             ('turned, tensor (1, 4)', turned, const(1.0, 4.0), (1, 4)), ('warp C, tensor (4, 2)', warp_c(), const(4.0, 2.0), (4, 2))]
    for name, hom, footprint, (ny, nx) in cases:
        if footprint == 'per-pixel':
            gy, gx = pr.raw_jacobian(hom, *size)
            assert (gy == 2.0).all() and (gx == 2.0).all()
        enc = model.encode(lq, max_scale=MAX_SCALE)
        got = model.render_warp(enc, homography=hom, size=size, footprint=footprint, footprint_range=C_RANGE, minify='area', fill=fill)
        other = model.encode(lq, max_scale=MAX_SCALE)                            # an encode of its own, the same explicit max_scale
        fine = model.render_warp(other, homography=_fine(hom, ny, nx), size=(ny * size[0], nx * size[1]), footprint=(1.0, 1.0), fill=fill)
        want = ar.box_mean(fine, ny, nx)
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, (got - want).abs().max().item())
        y, x = wr.lr_points(_fine(hom, ny, nx), ny * size[0], nx * size[1])
        inside = wr.members(y, x, WHOLE).reshape(size[0], ny, size[1], nx).sum((1, 3))
        assert ((inside > 0) & (inside < ny * nx)).sum() > 10 and (inside == 0).sum() > 10, name      # cut border pixels, and fill
        clamp = model.render_warp(enc, homography=hom, size=size, footprint=footprint, footprint_range=C_RANGE, fill=fill)
        assert not torch.equal(_bits(got), _bits(clamp)), name


def _sample_values(model, h, n_max, frames, chosen, dev, fill):
    """Warp C's render from the oracle: per frame the chosen pixels' inside samples asked one query per batch item, blended in tile
    order, finished per sample (`fill` where no frame holds it), then averaged per pixel in float64.  -> [3, chosen pixels]."""
    hv, wv = C_SIZE
    first, ny, nx, fy, fx = ar.table(*pr.raw_jacobian(h, hv, wv), C_RANGE, n_max)
    pix, y, x, sfy, sfx = ar.samples(h, hv, wv, first, ny, nx, fy, fx)
    take = chosen[pix]
    n_s = int(first[-1])
    lq = _lq(*C_LR, dev)
    params = _params(model)
    mean = torch.tensor(model.rgb_mean, dtype=torch.float64).view(3, 1)
    xn = lq.cpu() - mean.float().view(1, 3, 1, 1)
    E, Wt = torch.zeros(3, n_s, dtype=torch.float64), torch.zeros(n_s, dtype=torch.float64)
    asked = 0
    with torch.no_grad():
        for y0, x0, th, tw in frames:                                           # tile order
            mem = wr.members(y, x, (y0, x0, th, tw)) & take
            coord = torch.from_numpy(wr.coord_in(y[mem], x[mem], (y0, x0, th, tw)))
            cell = torch.from_numpy(pr.cells_in(sfy[mem], sfx[mem], (y0, x0, th, tw)))
            patch = xn[..., y0:y0 + th, x0:x0 + tw]
            out = _oracle_per_query(*_oracle_scene(patch, params), patch, coord, cell, params)
            idx = torch.from_numpy(np.flatnonzero(mem))
            E[:, idx] += out.t().double()
            Wt[idx] += 1
            asked += int(mem.sum())
    value = torch.where(Wt > 0, (E / Wt.clamp(min=1) + mean).clamp(0, 1), torch.tensor(fill, dtype=torch.float64).view(3, 1).expand(3, n_s))
    sums = torch.zeros(3, hv * wv, dtype=torch.float64).index_add_(1, torch.from_numpy(pix), value)
    sel = torch.from_numpy(chosen)
    return sums[:, sel] / torch.from_numpy((ny * nx)[chosen]).double(), lq, asked


def test_whole_image_area_warp_vs_oracle(dev):
    """Test 4, warp C whole-image, fp32, max_samples = 2 (3121 samples, the inside ones asked of the oracle one per batch item); bound
    2e-4, the single-footprint and per-pixel warps' on these fixtures: a mean cannot exceed its largest sample error, and the at most
    four fp32 additions add 4 x 2^-24."""
    model = _model('edsr', dev, 2)
    model.test_cfg = dict()
    fill = (0.75, 0.125, 0.5)
    chosen = np.ones(C_SIZE[0] * C_SIZE[1], dtype=bool)
    want, lq, asked = _sample_values(model, warp_c(), 2, [WHOLE], chosen, dev, fill)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=warp_c(), size=C_SIZE, max_samples=2, fill=fill, **AREA).cpu().view(3, -1).double()
    err = (got - want).abs().max().item()
    clamp = model.render_warp(enc, homography=warp_c(), size=C_SIZE, footprint='per-pixel', footprint_range=C_RANGE, fill=fill).cpu().view(3, -1)
    print(f'area warp C vs oracle, whole image: {asked} samples asked, max |diff| = {err:.3e}; area vs clamp: max |diff| = '
          f'{(got - clamp.double()).abs().max().item():.3e}')
    assert asked > 2000 and err < 2e-4, err


def test_tiled_area_warp_vs_oracle_composition(dev):
    """Test 4, warp C tiled, fp32, max_samples = 2: every third pixel, all of its samples in every frame that holds them, composed and
    blended per tile in tile order; bound 1e-4."""
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED)
    chosen = np.zeros(C_SIZE[0] * C_SIZE[1], dtype=bool)
    chosen[::3] = True
    fill = (0.75, 0.125, 0.5)
    want, lq, asked = _sample_values(model, warp_c(), 2, frames_c(), chosen, dev, fill)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=warp_c(), size=C_SIZE, max_samples=2, fill=fill, **AREA).cpu().view(3, -1).double()
    err = (got[:, torch.from_numpy(chosen)] - want).abs().max().item()
    print(f'area warp C vs oracle composition: {asked} samples asked, max |diff| = {err:.3e}')
    assert asked > 1000 and err < 1e-4, err


def test_tiled_area_warp_with_mixed_counts_vs_oracle(dev):
    """Test 4 at max_samples = 4 on a subset, tiled, fp32, bound 1e-4: every fifth pixel with n_y != n_x -- (1, 2), (2, 4) among them --,
    the pixels with n_y = 4, and the 37 under-sampled pixels (g_x > 4): those lie outside the image on warp C, so the oracle side says
    that each of their 16 samples holds `fill`."""
    model = _model('edsr', dev, 4)
    model.test_cfg = dict(TILED)
    hv, wv = C_SIZE
    gy, gx = pr.raw_jacobian(warp_c(), hv, wv)
    _, ny, nx, _, _ = ar.table(gy, gx, C_RANGE, 4)
    chosen = (gx > 4.0) | (ny == 4)
    chosen[np.flatnonzero(ny != nx)[::5]] = True
    assert int((gx > 4.0).sum()) == 37 and {(1, 2), (2, 4), (4, 4)} <= set(zip(ny[chosen].tolist(), nx[chosen].tolist()))
    fill = (0.75, 0.125, 0.5)
    want, lq, asked = _sample_values(model, warp_c(), 4, frames_c(), chosen, dev, fill)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, homography=warp_c(), size=C_SIZE, max_samples=4, fill=fill, **AREA).cpu().view(3, -1).double()
    err = (got[:, torch.from_numpy(chosen)] - want).abs().max().item()
    print(f'area warp C, max_samples 4, {int(chosen.sum())} pixels vs oracle composition: {asked} samples asked, max |diff| = {err:.3e}')
    assert asked > 500 and err < 1e-4, err
    under = got[:, torch.from_numpy(gx > 4.0)]
    assert torch.equal(under, torch.tensor(fill, dtype=torch.float32).double().view(3, 1).expand(3, 37))


def test_f16_against_fp32(dev):
    """Test 5: on warp C the f16 area render may differ from the fp32 one by at most twice what the `clamp` per-pixel render of the same
    warp differs by (the rule of the per-pixel warps' test).  The test prints both gaps."""
    model = _model('rdn', dev, 3)
    for name, cfg in (('whole', dict()), ('tiled', dict(TILED))):
        lq = _lq(*C_LR, dev)
        outs = {}
        for precision in ('fp32', 'f16'):
            model.test_cfg = dict(cfg, precision=precision)
            enc = model.encode(lq, max_scale=MAX_SCALE)
            src = dict(homography=warp_c(), size=C_SIZE, footprint='per-pixel', footprint_range=C_RANGE)
            outs[precision] = (model.render_warp(enc, minify='area', **src), model.render_warp(enc, **src))
        gap_area = (outs['f16'][0] - outs['fp32'][0]).abs().max().item()
        gap_clamp = (outs['f16'][1] - outs['fp32'][1]).abs().max().item()
        print(f'warp C {name}: f16 - fp32 area {gap_area:.3e}, clamp {gap_clamp:.3e}')
        assert gap_clamp > 0.0 and gap_area <= 2.0 * gap_clamp, (name, gap_area, gap_clamp)


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_render_many_with_an_area_warp_is_the_single_calls(dev, precision, monkeypatch):
    """Test 6: [Grid, View, Warp(clamp), Warp(area)] from one walk equals the single calls bit for bit, with one device-to-host copy."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.scene import Grid, View, Warp
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*C_LR, dev)
    h = warp_c()
    m = _view(A_ARGS, A_SIZE)
    pp = dict(footprint='per-pixel', footprint_range=C_RANGE)
    targets = [Grid(size=(80, 112)), View(m, A_SIZE, fill=0.25), Warp(homography=h, size=C_SIZE, fill=0.75, **pp),
               Warp(homography=h, size=C_SIZE, fill=(0.25, 0.5, 1.0), minify='area', **pp)]
    ref = model.encode(lq, max_scale=MAX_SCALE)
    wants = [model.render(ref, size=(80, 112)), model.render_view(ref, m, A_SIZE, fill=0.25),
             model.render_warp(ref, homography=h, size=C_SIZE, fill=0.75, **pp),
             model.render_warp(ref, homography=h, size=C_SIZE, fill=(0.25, 0.5, 1.0), minify='area', **pp)]
    enc = model.encode(lq, max_scale=MAX_SCALE)
    torch.cuda.synchronize()
    copies = _count_copies(monkeypatch)
    with hip_ops.profile():
        outs = model.render_many(enc, targets)
    n_copies = list(copies)
    monkeypatch.undo()
    prof = hip_ops.profile.results()
    assert n_copies == ['tolist'], n_copies
    assert prof['warp_area_count']['launches'] == 1 and prof['warp_pp_count']['launches'] == 1 and prof['warp_area_resolve']['launches'] == 1
    assert prof['warp_area_select']['launches'] == 4 and enc.cache.builds == 4 and len(outs) == 4, sorted(prof)
    for k, (got, want) in enumerate(zip(outs, wants)):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (k, (got - want).abs().max().item())
    assert not torch.equal(_bits(outs[2]), _bits(outs[3]))
    # the single call makes one copy as well
    torch.cuda.synchronize()
    copies = _count_copies(monkeypatch)
    model.render_warp(enc, homography=h, size=C_SIZE, minify='area', **pp)
    n_copies = list(copies)
    monkeypatch.undo()
    assert n_copies == ['tolist'], n_copies
    # prefetch builds what the render touches
    fresh = model.encode(lq, max_scale=MAX_SCALE)
    assert model.prefetch(fresh, targets[3:]) == 4 and fresh.cache.builds == 4
    again = model.render_many(fresh, targets[3:])
    assert fresh.cache.builds == 4 and torch.equal(_bits(again[0]), _bits(wants[3]))


def test_outputs(dev):
    """Test 7: a pixel without samples holds `fill` (A = 0); as_u8, as_u16 and grey quantise the resolved tensor; the alpha of an RGBA
    record is the coverage-weighted mean: at a border pixel with k of n samples inside, the quantised mean of the inside alphas and
    zeros."""
    from ciaosr_amd import metrics_hip, scene
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(TILED)
    lq = _lq(*C_LR, dev)
    hv, wv = C_SIZE
    fill = (0.25, 0.5, 1.0)
    h = warp_c()
    raw = tensor_c()
    first, ny, nx, fy, fx = ar.table(raw[..., 0].ravel(), raw[..., 1].ravel(), C_RANGE, C_N)
    pix, y, x, _, _ = ar.samples(h, hv, wv, first, ny, nx, fy, fx)
    inside = np.bincount(pix[wr.members(y, x, WHOLE)], minlength=hv * wv)       # per pixel: samples inside the image
    none = torch.from_numpy(inside == 0)
    assert inside[Q_NAN] == 0 and ny[Q_NAN] == 0 and int(none.sum()) > 100
    src = dict(homography=h, size=C_SIZE, footprint=torch.from_numpy(raw).to(dev), footprint_range=C_RANGE, minify='area', fill=fill)
    enc = model.encode(lq, max_scale=MAX_SCALE)
    got = model.render_warp(enc, **src)
    flat = got.cpu().view(3, -1)
    assert not torch.isnan(flat).any()
    for c in range(3):
        assert torch.equal(flat[c, none], torch.full((int(none.sum()),), fill[c])), c
    assert (flat[:, ~none] != torch.tensor(fill).view(3, 1)).any(0).float().mean() > 0.99
    u8, u16 = model.render_warp(enc, as_u8=True, **src), model.render_warp(enc, as_u16=True, **src)
    assert u8.dtype == torch.uint8 and u8.shape == (*C_SIZE, 3) and torch.equal(u8, metrics_hip.tensor2img_u8(got))
    assert u16.dtype == torch.uint16 and torch.equal(u16.view(torch.int16), metrics_hip.tensor2img_u16(got).view(torch.int16))
    grey = model.encode_grey(lq[:, :1].contiguous(), max_scale=MAX_SCALE)
    g32, g8 = model.render_warp(grey, **src), model.render_warp(grey, as_u8=True, **src)
    assert g32.shape == (1, 3, *C_SIZE) and g8.shape == C_SIZE and torch.equal(g8, metrics_hip.tensor2img_grey_u8(g32))
    rgba = model.encode_rgba(torch.cat([lq, torch.full((1, 1, *C_LR), 0.9, device=dev)], 1), max_scale=MAX_SCALE)
    b8 = model.render_warp(rgba, as_u8=True, **src)
    assert b8.shape == (*C_SIZE, 4) and torch.equal(b8[..., :3], u8)
    a = b8[..., 3].cpu().view(-1)
    assert (a[none] == 0).all() and a[Q_NAN] == 0 and (a[~none] > 0).float().mean() > 0.9
    # uniform 2 x 2 samples: the alpha plane is the box mean of the fine warp's alpha, whose outside samples are 0
    size = (24, 34)
    hom = scene.homography_of_view(scene.view_matrix((21.0, 27.5), 0.5, -32, size))
    two = dict(homography=hom, size=size, footprint='per-pixel', footprint_range=C_RANGE, minify='area', fill=fill)
    b8 = model.render_warp(rgba, as_u8=True, **two)
    fine_h = (hom[0] / 2, hom[1] / 2, hom[2], hom[3] / 2, hom[4] / 2, hom[5], 0.0, 0.0, 1.0)
    other = model.encode_rgba(torch.cat([lq, torch.full((1, 1, *C_LR), 0.9, device=dev)], 1), max_scale=MAX_SCALE)
    fine = model.render_warp(other, homography=fine_h, size=(48, 68), footprint=(1.0, 1.0), fill=fill)
    assert fine.shape == (2, 3, 48, 68) and torch.equal(b8, metrics_hip.tensor2img_bgra_u8(ar.box_mean(fine, 2, 2)))
    # a border pixel with k of 4 samples inside: the outside samples of the fine alpha are exactly 0, so A is the quantised mean of the k
    # inside alphas and 4 - k zeros
    yf, xf = wr.lr_points(fine_h, 48, 68)
    ins4 = torch.from_numpy(wr.members(yf, xf, WHOLE).reshape(24, 2, 34, 2)).permute(0, 2, 1, 3).reshape(24 * 34, 4)
    k_in = ins4.sum(1)
    cut, full = (k_in > 0) & (k_in < 4), k_in == 4
    assert int(cut.sum()) > 20 and set(k_in[cut].tolist()) == {1, 2, 3}
    box = fine[1].cpu().view(3, 24, 2, 34, 2).permute(0, 1, 3, 2, 4).reshape(3, 24 * 34, 4)     # the alpha item as grey, per pixel
    assert (box[:, ~ins4] == 0).all()
    grey8 = metrics_hip.tensor2img_u8(ar.box_mean(fine, 2, 2)[1:2].contiguous()).cpu().view(-1, 3).long()     # B G R of the mean
    a8 = b8[..., 3].cpu().view(-1).long()
    assert torch.equal(a8, (4899 * grey8[:, 2] + 9617 * grey8[:, 1] + 1868 * grey8[:, 0] + 8192) >> 14)
    assert (a8[k_in == 0] == 0).all() and a8[cut].float().mean() < a8[full].float().mean()


def test_render_cli_minify_area(dev, tmp_path):
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
    Image.fromarray((_lq(*C_LR, 'cpu', seed=8)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(png)
    h = warp_c()
    flags = ['--homography', *[repr(v) for v in h], '--size', str(C_SIZE[0]), str(C_SIZE[1]), '--footprint', 'per-pixel',
             '--footprint-range', '0.25', '1.0']
    paths = render.main([config, ckpt, png, *flags, '--minify', 'area', '--max-samples', '2', '--out', str(tmp_path / 'out')])
    assert [os.path.basename(p) for p in paths] == ['img_warp0.png']
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                                           # what the tool sets
    enc = model.encode(imread_rgb01(png).unsqueeze(0).to(dev), max_scale=MAX_SCALE)
    want = model.render_warp(enc, homography=h, size=C_SIZE, as_u8=True, max_samples=2, **AREA).cpu().numpy()    # B G R
    got = np.asarray(Image.open(paths[0]).convert('RGB'))
    assert got.shape == (*C_SIZE, 3) and np.array_equal(got[..., ::-1], want)
    plain = render.main([config, ckpt, png, *flags, '--out', str(tmp_path / 'plain')])
    assert open(plain[0], 'rb').read() != open(paths[0], 'rb').read()
