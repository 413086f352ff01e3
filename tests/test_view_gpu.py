"""Affine views of an encoded scene on the GPU: the count / select / blend / finalize kernels against the definition in numpy float64
(tests/view_reference.py), CiaoSR.render_view against the torch-CPU oracle and against the library's own query path, the scene cache
under views, the axis-aligned view against the window render, and tools/render.py --view."""
import os

import numpy as np
import pytest
import torch

from tests import view_reference as vr
from tests.helpers import SQRT6, randn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = (0.4488, 0.4371, 0.4040)
# view A: 40 x 56 LR, tile 32, overlap 8 (2 x 2 tiles); view B: 24 x 24 LR, whole image
A_LR, A_SIZE, A_ARGS = (40, 56), (61, 83), ((31.0, 42.5), 2.7, -32)
B_LR, B_SIZE, B_ARGS = (24, 24), (40, 52), ((15.5, 17.25), 2.7, 30)
A_ONE_TILE_SHIFT = (-40.75, -30.5)          # added to (t_y, t_x): every member of view A then lies in tile (0, 0) alone


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_models = {}


def _model(kind, dev, blocks):
    if (kind, blocks) not in _models:
        from ciaosr_amd.init_utils import seeded_init_
        from tests.test_hip_parity import _restorer
        model = _restorer(kind, 4, dev, dict(), blocks=blocks, layers=4)
        seeded_init_(model, seed=17, gain=1.2, head_gain=SQRT6)
        _models[(kind, blocks)] = model.to(dev)
    return _models[(kind, blocks)]


def _params(model):
    return {k[len('generator.'):]: v.detach().clone().cpu() for k, v in model.state_dict().items()}


def _lq(h, w, dev, seed=5):
    return (randn((1, 3, h, w), seed) * 0.2 + 0.45).clamp(0, 1).to(dev)


def _view(args, size):
    from ciaosr_amd import scene
    return scene.view_matrix(args[0], args[1], args[2], size)


def _frames_a():
    from ciaosr_amd import scene
    return scene.plan_view(*A_LR, 32, 8, any_scale=True)


def _tiles(frames, dev):
    return torch.tensor(frames, dtype=torch.int32).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _view_a_numpy():
    m = _view(A_ARGS, A_SIZE)
    y, x = vr.lr_points(m, *A_SIZE)
    return m, y, x


def test_view_a_is_the_case_the_issue_describes():
    """Host-only guard (no GPU needed, kept here with the views it guards): the input cannot drift into an easy case."""
    m, y, x = _view_a_numpy()
    frames = _frames_a()
    inside = vr.members(y, x, (0, 0, *A_LR))
    cover = sum(vr.members(y, x, f).astype(int) for f in frames)
    assert y.size == 5063 and abs(1 - inside.mean() - 0.171) < 5e-4
    assert [int(vr.members(y, x, f).sum()) for f in frames] == [397, 2642, 589, 4197]
    assert [int((cover == k).sum()) for k in range(5)] == [864, 1367, 2435, 0, 397]
    assert np.array_equal(cover == 0, ~inside)
    assert vr.edge_distance(y, x, frames + [(0, 0, *A_LR)]) > 4e-3
    mb = _view(B_ARGS, B_SIZE)
    yb, xb = vr.lr_points(mb, *B_SIZE)
    assert abs(1 - vr.members(yb, xb, (0, 0, *B_LR)).mean() - 0.143) < 5e-4 and vr.edge_distance(yb, xb, [(0, 0, *B_LR)]) > 3e-3
    m1 = list(m)
    m1[2] += A_ONE_TILE_SHIFT[0]
    m1[5] += A_ONE_TILE_SHIFT[1]
    y1, x1 = vr.lr_points(m1, *A_SIZE)
    assert [int(vr.members(y1, x1, f).sum()) for f in frames] == [515, 0, 0, 0] and vr.edge_distance(y1, x1, frames + [(0, 0, *A_LR)]) > 4e-3


def _check_kernels_against_numpy(m, hv, wv, frames, dev):
    from ciaosr_amd import hip_ops
    y, x = vr.lr_points(m, hv, wv)
    tiles = _tiles(frames, dev)
    runs = []
    for _ in range(2):
        counts, ws = hip_ops.view_count(m, hv, wv, tiles)
        counts = counts.tolist()
        want_counts = [int(vr.members(y, x, f).sum()) for f in frames]
        assert counts == want_counts, (counts, want_counts)
        out = []
        for k, (frame, n) in enumerate(zip(frames, counts)):
            if n == 0:
                continue
            q_index, coord, cell = hip_ops.view_select(m, hv, wv, frame, k, len(frames), ws, n)
            mem = vr.members(y, x, frame)
            assert np.array_equal(q_index.cpu().numpy(), np.flatnonzero(mem).astype(np.int32)), frame
            want = vr.coord_in(y[mem], x[mem], frame)
            assert np.array_equal(coord.cpu().numpy().view(np.int32), want.view(np.int32)), (frame, np.abs(coord.cpu().numpy() - want).max())
            want_cell = np.broadcast_to(vr.cell_in(m, frame), (n, 2))
            assert np.array_equal(cell.cpu().numpy().view(np.int32), np.ascontiguousarray(want_cell).view(np.int32)), frame
            out += [q_index, coord, cell]
        runs.append((counts, out))
    assert runs[0][0] == runs[1][0] and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0][1], runs[1][1]))
    # the whole grid in one frame, without selection
    coord, cell = hip_ops.make_coord_cell_view(m, hv, wv, frames[-1], dev)
    assert np.array_equal(coord.cpu().numpy().view(np.int32), vr.coord_in(y, x, frames[-1]).view(np.int32))
    assert np.array_equal(cell.cpu().numpy().view(np.int32),
                          np.ascontiguousarray(np.broadcast_to(vr.cell_in(m, frames[-1]), (hv * wv, 2))).view(np.int32))
    assert hip_ops.grid_width_of(coord) == wv
    return counts


def test_count_and_select_against_the_definition(dev):
    from ciaosr_amd import hip_ops, scene
    chunk = hip_ops.view_block_queries()
    frames = _frames_a()
    m = _view(A_ARGS, A_SIZE)
    assert A_SIZE[0] * A_SIZE[1] > 4 * chunk                                   # several workgroups, the last one ragged
    assert _check_kernels_against_numpy(m, *A_SIZE, frames, dev) == [397, 2642, 589, 4197]
    # one query: LR point (5, 30), in the two upper tiles
    assert _check_kernels_against_numpy(scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1)), 1, 1, frames, dev) == [1, 1, 0, 0]
    # three very wide rows: more than one workgroup per row pair, members of all four tiles, some outside
    wide = 700
    assert 3 * wide > 2 * chunk and wide < chunk
    counts = _check_kernels_against_numpy(scene.view_matrix((20.0, 28.0), 11.0, 7, (3, wide)), 3, wide, frames, dev)
    assert all(c > 0 for c in counts) and max(counts) < 3 * wide


@pytest.mark.parametrize('mean,std', [(MEAN, (1.0, 1.0, 1.0)), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
def test_blend_and_finalize_against_index_add(dev, mean, std):
    from ciaosr_amd import hip_ops
    m, y, x = _view_a_numpy()
    hv, wv = A_SIZE
    n_q = hv * wv
    frames = _frames_a()
    fill = (0.25, 0.5, 1.0)
    E = torch.zeros(3, n_q, device=dev)
    Wt = torch.zeros(n_q, device=dev)
    E_ref, Wt_ref = torch.zeros(3, n_q), torch.zeros(n_q)
    for k, frame in enumerate(frames):                                          # tile order
        idx = torch.from_numpy(np.flatnonzero(vr.members(y, x, frame)))
        rgb = randn((idx.numel(), 3), 40 + k)
        hip_ops.view_blend(E, Wt, idx.to(torch.int32).to(dev), rgb.to(dev))
        E_ref.index_add_(1, idx, rgb.t().contiguous())
        Wt_ref.index_add_(0, idx, torch.ones(idx.numel()))
    assert torch.equal(_bits(E), _bits(E_ref)) and torch.equal(_bits(Wt), _bits(Wt_ref))
    claimed = Wt_ref > 0
    assert int((~claimed).sum()) == 864 and Wt_ref.max() == 4
    pred = hip_ops.view_finalize(E, Wt, fill, mean, std)
    assert pred.shape == (n_q, 3) and not torch.isnan(pred).any()
    assert torch.equal(_bits(pred[claimed.to(dev)]), _bits((E_ref / Wt_ref).t()[claimed]))
    out = hip_ops.denorm_clamp(pred, hv, wv, mean, std).cpu().view(3, n_q)
    assert not torch.isnan(out).any()
    want = ((E_ref / Wt_ref) * torch.tensor(std).view(3, 1) + torch.tensor(mean).view(3, 1)).clamp(0, 1)
    assert torch.equal(_bits(out[:, claimed]), _bits(want[:, claimed]))
    for c in range(3):
        assert torch.equal(out[c, ~claimed], torch.full((864,), fill[c])), c          # exactly
    # a whole-view tile skips the index list
    E2, W2 = torch.zeros(3, n_q, device=dev), torch.zeros(n_q, device=dev)
    rgb = randn((n_q, 3), 50).to(dev)
    hip_ops.view_blend(E2, W2, None, rgb)
    assert torch.equal(E2, rgb.t()) and torch.equal(W2, torch.ones(n_q, device=dev))
    zeros = hip_ops.denorm_clamp(hip_ops.view_finalize(torch.zeros_like(E2), torch.zeros_like(W2), (0.0,) * 3, mean, std), hv, wv, mean, std)
    assert torch.equal(zeros, torch.zeros_like(zeros))                                # the default fill, nothing claimed: no NaN from 0 / 0


def test_whole_image_view_vs_oracle(dev):
    """View B through render_view against the torch-CPU oracle's forward_test on the inside queries, coordinates from the numpy formula.
    forward_test shapes its output as the round(h s) x round(w s) image of s = sqrt(Q / hw): the 1782 inside queries are padded with
    copies of the first ones to 43 x 43 (s = 43 / 24), and the padding is dropped from the result."""
    from oracle import ciaosr_oracle as orc
    model = _model('edsr', dev, 2)
    model.test_cfg = dict()
    h, w = B_LR
    hv, wv = B_SIZE
    m = _view(B_ARGS, B_SIZE)
    y, x = vr.lr_points(m, hv, wv)
    inside = vr.members(y, x, (0, 0, h, w))
    n = int(inside.sum())
    side = int(np.ceil(np.sqrt(n)))
    assert n == 1782 and side == 43 and round(h * np.sqrt(side * side / (h * w))) == side
    coord = torch.from_numpy(vr.coord_in(y[inside], x[inside], (0, 0, h, w)))
    cell = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(vr.cell_in(m, (0, 0, h, w)), (n, 2))))
    pad = side * side - n
    lq = _lq(h, w, dev)
    want = orc.forward_test(lq.cpu(), torch.cat([coord, coord[:pad]]).unsqueeze(0), torch.cat([cell, cell[:pad]]).unsqueeze(0), _params(model))
    want = want.view(3, side * side)[:, :n]
    fill = (0.75, 0.125, 0.5)
    enc = model.encode(lq)
    got = model.render_view(enc, m, (hv, wv), fill=fill).cpu()
    assert got.shape == (1, 3, hv, wv) and abs(enc.max_scale - 2.7) < 1e-12 and enc.cache.builds == 1
    got = got.view(3, hv * wv)
    err = (got[:, torch.from_numpy(inside)] - want).abs().max().item()
    print(f'view B vs oracle: max |diff| = {err:.3e}')
    assert err < 2e-4, err
    for c in range(3):
        assert torch.equal(got[c, torch.from_numpy(~inside)], torch.full((hv * wv - n,), fill[c]))


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_whole_image_view_is_the_scene_query(dev, precision):
    from ciaosr_amd import hip_ops, metrics_hip
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(precision=precision)
    h, w = B_LR
    lq = _lq(h, w, dev)
    # view B: the inside pixels are the head's answer to exactly those queries
    hv, wv = B_SIZE
    m = _view(B_ARGS, B_SIZE)
    y, x = vr.lr_points(m, hv, wv)
    inside = torch.from_numpy(vr.members(y, x, (0, 0, h, w))).to(dev)
    enc = model.encode(lq)
    got = model.render_view(enc, m, (hv, wv))
    coord, cell = hip_ops.make_coord_cell_view(m, hv, wv, (0, 0, h, w), dev)
    n = int(inside.sum())
    rgb = model.generator.render(enc.cache.get((0, None)), coord[inside].contiguous(), cell[inside].contiguous())[0]
    want = hip_ops.denorm_clamp(rgb.contiguous(), 1, n, model.rgb_mean, model.rgb_std).view(3, n)
    assert torch.equal(got.view(3, hv * wv)[:, inside], want)
    assert torch.equal(got.view(3, hv * wv)[:, ~inside], torch.zeros(3, hv * wv - n, device=dev))       # fill = 0
    assert enc.cache.builds == 1
    # a view that lies inside the image is `restore` on its coordinates: one tile owns every query, the view is walked as a grid (in f16
    # the chained head kernel takes that hint; without it the 128-row kernel would answer, with other summation orders).  The scene is
    # planned for the 30 x 30 queries `restore` sees, so both run the same route.
    size = (30, 30)
    m = _view(((12, 12), 2.0, 12), size)
    y, x = vr.lr_points(m, *size)
    assert vr.members(y, x, (0, 0, h, w)).all()
    enc = model.encode(lq, max_scale=30 / 24)
    got = model.render_view(enc, m, size)
    coord, cell = hip_ops.make_coord_cell_view(m, *size, (0, 0, h, w), dev)
    assert hip_ops.grid_width_of(coord) == 30
    want = model.restore(lq, coord.unsqueeze(0), cell.unsqueeze(0))
    assert got.shape == want.shape == (1, 3, 30, 30)
    assert torch.equal(got, want), (got - want).abs().max().item()
    u8 = model.render_view(enc, m, size, as_u8=True)
    assert u8.dtype == torch.uint8 and torch.equal(u8, metrics_hip.tensor2img_u8(got))


def test_tiled_view_vs_oracle_composition(dev):
    from oracle import ciaosr_oracle as orc
    model = _model('edsr', dev, 4)
    cfg = dict(tile=32, tile_overlap=8, tile_any_scale=True)
    model.test_cfg = dict(cfg)
    h, w = A_LR
    hv, wv = A_SIZE
    n_q = hv * wv
    frames = _frames_a()
    m, y, x = _view_a_numpy()
    lq = _lq(h, w, dev)
    params = _params(model)
    mean = torch.tensor(model.rgb_mean).view(3, 1)
    xn = lq.cpu() - mean.view(1, 3, 1, 1)
    E, Wt = torch.zeros(3, n_q), torch.zeros(n_q)
    for y0, x0, th, tw in frames:                                               # tile order
        mem = vr.members(y, x, (y0, x0, th, tw))
        coord = torch.from_numpy(vr.coord_in(y[mem], x[mem], (y0, x0, th, tw))).unsqueeze(0)
        cell = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(vr.cell_in(m, (y0, x0, th, tw)), (int(mem.sum()), 2)))).unsqueeze(0)
        out = orc.generator_forward(xn[..., y0:y0 + th, x0:x0 + tw], coord, cell, params)
        idx = torch.from_numpy(np.flatnonzero(mem))
        E[:, idx] += out[0].t()
        Wt[idx] += 1
    claimed = Wt > 0
    want = (E / Wt + mean).clamp(0, 1)
    enc = model.encode(lq)
    assert enc.cache.builds == 0
    got = model.render_view(enc, m, (hv, wv))
    assert got.shape == (1, 3, hv, wv) and enc.cache.builds == 4 and abs(enc.max_scale - 2.7) < 1e-12
    flat = got.cpu().view(3, n_q)
    err = (flat[:, claimed] - want[:, claimed]).abs().max().item()
    print(f'view A vs oracle composition: max |diff| = {err:.3e}')
    assert err < 1e-4, err
    assert torch.equal(flat[:, ~claimed], torch.zeros(3, 864))
    # a second view whose members all lie in tile (0, 0) builds nothing, and touches nothing else
    m1 = list(m)
    m1[2] += A_ONE_TILE_SHIFT[0]
    m1[5] += A_ONE_TILE_SHIFT[1]
    y1, x1 = vr.lr_points(m1, hv, wv)
    assert [int(vr.members(y1, x1, f).sum()) for f in frames] == [515, 0, 0, 0]
    one = model.render_view(enc, m1, (hv, wv))
    assert enc.cache.builds == 4 and list(enc.cache.entries)[-1] == (0, (0, 0))
    assert int((one.view(3, n_q) != 0).any(0).sum()) <= 515
    fresh = model.encode(lq)
    assert torch.equal(model.render_view(fresh, m1, (hv, wv)), one) and fresh.cache.builds == 1 and list(fresh.cache.entries) == [(0, (0, 0))]
    # room for one tile scene, not for two: the same image, by rebuilding
    model.test_cfg = dict(cfg, scene_cache_mb=20)
    small = model.encode(lq)
    assert torch.equal(model.render_view(small, m, (hv, wv)), got)
    assert torch.equal(model.render_view(small, m, (hv, wv)), got)
    assert small.cache.builds > 4 and len(small.cache.entries) == 1 and small.scene_bytes <= 20 << 20


def test_axis_aligned_view_vs_window_render(dev):
    """Not bitwise: the window's coordinates round three times in fp32, the view's once from fp64 (<= 2^-22 apart).  Where that moves a
    query or one of its four shifted samples across an LR pixel boundary the head reads another feature vector, so the image is compared
    only where all five nearest indices agree -- and those pixels must be all but a per cent of the window."""
    from ciaosr_amd import hip_ops, scene
    from oracle import ciaosr_oracle as orc
    h = w = 24
    ht = wt = 96
    win = (3, 50, 70, 41)
    m, (hv, wv) = scene.view_of_window(h, w, ht, wt, win)
    cw, lw = hip_ops.make_coord_cell_window(ht, wt, win[0], win[0] + hv, win[1], win[1] + wv, dev)
    cv, lv = hip_ops.make_coord_cell_view(m, hv, wv, (0, 0, h, w), dev)
    cw, lw, cv, lv = (t.cpu() for t in (cw, lw, cv, lv))
    assert (cw.double() - cv.double()).abs().max().item() <= 2.0 ** -22 and (lw.double() - lv.double()).abs().max().item() <= 2.0 ** -26
    index_map = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)

    def nearest(coord, cell):
        """[Q, 5]: LR index of the query and of its four shifted samples (oracle query_rgb's arithmetic, local_size 2)."""
        coord, cell = coord.unsqueeze(0), cell.unsqueeze(0)
        cols = [orc._nearest(index_map, coord)]
        ty, tx = (h - 1) / (1 - cell[:, 0, 0]), (w - 1) / (1 - cell[:, 0, 1])
        for vy, vx in orc.shift_list(2):
            c_ = coord.clone()
            c_[:, :, 0] += vy / abs(vy) * ((2 * abs(vy) - 1) / ty) + 1e-6
            c_[:, :, 1] += vx / abs(vx) * ((2 * abs(vx) - 1) / tx) + 1e-6
            c_.clamp_(-1 + 1e-6, 1 - 1e-6)
            cols.append(orc._nearest(index_map, c_))
        return torch.cat(cols, -1)[0]

    same = (nearest(cw, lw) == nearest(cv, lv)).all(-1)
    left_out = 1 - same.float().mean().item()
    print(f'axis-aligned view vs window: {left_out:.3%} of the pixels left out')
    assert left_out < 0.01, left_out
    model = _model('rdn', dev, 3)
    model.test_cfg = dict(scale=4)
    enc = model.encode(_lq(h, w, dev))
    a = model.render(enc, size=(ht, wt), window=win).cpu().view(3, hv * wv)
    b = model.render_view(enc, m, (hv, wv)).cpu().view(3, hv * wv)
    err = (a[:, same] - b[:, same]).abs().max().item()
    print(f'axis-aligned view vs window: max |diff| = {err:.3e} on the compared pixels')
    assert enc.cache.builds == 1 and err < 2e-4, err


def test_render_cli_views(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, metrics, scene
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_rgb01, imwrite
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=SQRT6)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray((_lq(24, 24, 'cpu', seed=8)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(png)
    views = [((12.0, 12.0), 2.5, 30.0, (40, 52)), ((7.25, 15.5), 3.0, -90.0, (33, 21))]
    flags = [v for (c, z, a, s) in views for v in ('--view', str(c[0]), str(c[1]), str(z), str(a), '--size', str(s[0]), str(s[1]))]
    with hip_ops.profile():
        paths = render.main([config, ckpt, png, '--scale', '2', '3.3', *flags, '--out', str(tmp_path / 'both')])
    prof = hip_ops.profile.results()
    assert prof['head_unfold']['launches'] == 1, prof['head_unfold']                  # one encode in total
    assert prof['view_count']['launches'] == 2 and prof['view_finalize']['launches'] == 2
    assert [os.path.basename(p) for p in paths] == ['img_x2.png', 'img_x3p3.png', 'img_view0.png', 'img_view1.png']
    # the --scale outputs are the files the tool writes without --view
    alone = render.main([config, ckpt, png, '--scale', '2', '3.3', '--out', str(tmp_path / 'scales')])
    assert [os.path.basename(p) for p in alone] == ['img_x2.png', 'img_x3p3.png']
    for a, b in zip(alone, paths):
        assert open(a, 'rb').read() == open(b, 'rb').read(), a
    # the views are render_view + tensor2img + imwrite
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                                           # what the tool sets
    enc = model.encode(imread_rgb01(png).unsqueeze(0).to(dev), max_scale=3.3)
    for path, (c, z, a, s) in zip(paths[2:], views):
        ref = str(tmp_path / ('ref_' + os.path.basename(path)))
        imwrite(metrics.tensor2img(model.render_view(enc, scene.view_matrix(c, z, a, s), s)), ref)
        assert open(path, 'rb').read() == open(ref, 'rb').read(), path
    only = render.main([config, ckpt, png, *flags[:8], '--out', str(tmp_path / 'views')])
    assert [os.path.basename(p) for p in only] == ['img_view0.png']
