"""CiaoSR.render_many / prefetch on the GPU: every output bitwise the single call's (`render`, `render_view`) on a fresh encode, the scene
builds, trunk calls and synchronising copies a call may make, and ciaosr_view_count_many_i32 against the definition in numpy float64
(tests/view_reference.py) and against the single-view count."""
import math
import os

import numpy as np
import pytest
import torch

from tests import view_reference as vr
from tests.helpers import SQRT6, randn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = (40, 56)                                   # tile 32, overlap 8: 2 x 2 tiles
TILED = dict(tile=32, tile_overlap=8, tile_any_scale=True)
HR = (108, 151)                                 # x2.7
WINDOW = (9, 41, 61, 35)                        # crosses both seams at x2.7
A_SIZE, A_ARGS = (61, 83), ((31.0, 42.5), 2.7, -32)
A_ONE_TILE_SHIFT = (-40.75, -30.5)              # added to (t_y, t_x): every member of view A then lies in tile (0, 0) alone
ONE_SCENE = 32 * 32 * 13968                     # bytes of a 32 x 32 tile scene at C = 64


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_models = {}


def _model(kind, dev):
    """Random-init restorers as in tests/test_scene_restorer_gpu.py; test_cfg is set per test."""
    if kind not in _models:
        from ciaosr_amd.init_utils import seeded_init_
        from tests.test_hip_parity import _restorer
        model = _restorer(kind, 4, dev, dict(), blocks=3, layers=4)
        seeded_init_(model, seed=17, gain=1.2, head_gain=SQRT6)
        _models[kind] = model.to(dev)
    return _models[kind]


def _lq(h, w, dev, seed=5):
    return (randn((1, 3, h, w), seed) * 0.2 + 0.45).clamp(0, 1).to(dev)


def _view_a(shift=(0.0, 0.0)):
    from ciaosr_amd import scene
    m = list(scene.view_matrix(*A_ARGS, A_SIZE))
    m[2] += shift[0]
    m[5] += shift[1]
    return tuple(m)


def _frames():
    from ciaosr_amd import scene
    return scene.plan_view(*LR, 32, 8, any_scale=True)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _targets():
    from ciaosr_amd.scene import Grid, View
    return [Grid(size=(80, 112)), Grid(size=HR, window=WINDOW), View(_view_a(), A_SIZE), View(_view_a(A_ONE_TILE_SHIFT), A_SIZE, fill=(0.25, 0.5, 1.0))]


def _single(model, enc, target, as_u8=False):
    from ciaosr_amd.scene import Grid
    if isinstance(target, Grid):
        return model.render(enc, size=target.size, scale=target.scale, window=target.window, as_u8=as_u8)
    return model.render_view(enc, target.matrix, target.size, target.fill, as_u8=as_u8)


def _singles(model, lq, targets, max_scale=2.7, as_u8=False):
    enc = model.encode(lq, max_scale=max_scale)
    return [_single(model, enc, t, as_u8) for t in targets], enc


def test_count_many_against_the_definition(dev):
    from ciaosr_amd import _lib, hip_ops, scene
    frames = _frames()
    tiles = torch.tensor(frames, dtype=torch.int32).to(dev)
    n_max = _lib.load().ciaosr_view_count_many_max_views()
    views = [(_view_a(), A_SIZE), (_view_a(A_ONE_TILE_SHIFT), A_SIZE), (scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1)), (1, 1))]
    for k in range(n_max + 1):                                   # tiny views: the list crosses a launch group
        size = (2 + k % 3, 3 + k % 5)
        views.append((scene.view_matrix((4.0 + 0.9 * k, 50.0 - 1.3 * k), 0.3 + 0.05 * k, 11 * k, size), size))
    assert len(views) > n_max + 3
    ms, sizes = [v[0] for v in views], [v[1] for v in views]
    want = []
    for m, (hv, wv) in views:
        y, x = vr.lr_points(m, hv, wv)
        want.append([int(vr.members(y, x, f).sum()) for f in frames])
    assert want[:3] == [[397, 2642, 589, 4197], [515, 0, 0, 0], [1, 1, 0, 0]]
    assert sum(1 for w in want[3:] if sum(w)) > n_max // 2 and any(sum(1 for n in w if n) > 1 for w in want[3:])
    runs = []
    for _ in range(2):
        counts, ws, offsets = hip_ops.view_count_many(ms, sizes, tiles)
        assert counts.shape == (len(views), len(frames)) and counts.dtype == torch.int32
        assert counts.tolist() == want
        lists = [counts]
        for v, ((m, (hv, wv)), off) in enumerate(zip(views, offsets)):
            one, ws1 = hip_ops.view_count(m, hv, wv, tiles)
            assert one.tolist() == want[v], v
            nbytes = _lib.load().ciaosr_view_workspace_bytes(hv, wv, len(frames))
            assert off % 256 == 0 and torch.equal(ws[off:off + nbytes], ws1[:nbytes]), v              # the part array, bitwise
            for k, n in enumerate(want[v]):
                if n == 0:
                    continue
                got = hip_ops.view_select(m, hv, wv, frames[k], k, len(frames), ws[off:], n)
                ref = hip_ops.view_select(m, hv, wv, frames[k], k, len(frames), ws1, n)
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, ref)), (v, k)
                y, x = vr.lr_points(m, hv, wv)
                assert np.array_equal(got[0].cpu().numpy(), np.flatnonzero(vr.members(y, x, frames[k])).astype(np.int32)), (v, k)
                lists += list(got)
        runs.append(lists)
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_render_many_is_the_single_calls(dev, precision):
    from ciaosr_amd import hip_ops
    model = _model('rdn', dev)
    model.test_cfg = dict(TILED, precision=precision)
    lq = _lq(*LR, dev)
    targets = _targets()
    wants, ref = _singles(model, lq, targets)
    assert ref.cache.builds == 4
    enc = model.encode(lq, max_scale=2.7)
    with hip_ops.profile():
        outs = model.render_many(enc, targets)
    prof = hip_ops.profile.results()
    assert len(outs) == 4 and [tuple(o.shape) for o in outs] == [(1, 3, 80, 112), (1, 3, 61, 35), (1, 3, *A_SIZE), (1, 3, *A_SIZE)]
    for k, (got, want) in enumerate(zip(outs, wants)):
        assert got.dtype == torch.float32 and torch.equal(got, want), (k, (got - want).abs().max().item())
    assert enc.cache.builds == 4 and len(enc.cache.entries) == 4
    assert prof['view_count_many']['launches'] == 1 and 'view_count' not in prof, sorted(prof)
    assert prof['head_unfold']['launches'] == 4
    u8 = model.render_many(enc, targets, as_u8=True)
    want_u8, _ = _singles(model, lq, targets, as_u8=True)
    assert enc.cache.builds == 4
    for k, (got, want) in enumerate(zip(u8, want_u8)):
        assert got.dtype == torch.uint8 and torch.equal(got, want), k


def test_an_open_max_scale_is_the_largest_any_target_needs(dev):
    from ciaosr_amd.scene import Grid, View
    model = _model('rdn', dev)
    model.test_cfg = dict(TILED)
    lq = _lq(*LR, dev)
    targets = [Grid(size=(80, 112)), View(_view_a(), A_SIZE), Grid(size=HR, window=WINDOW)]
    enc = model.encode(lq)
    assert enc.max_scale is None
    outs = model.render_many(enc, targets)
    assert abs(enc.max_scale - 2.7) < 1e-12                     # 108 / 40, 151 / 56 and the view's zoom: the largest
    wants, _ = _singles(model, lq, targets, max_scale=enc.max_scale)
    assert all(torch.equal(a, b) for a, b in zip(outs, wants))


def test_a_budget_of_one_scene_builds_every_tile_once(dev):
    from ciaosr_amd.scene import Grid, View
    model = _model('rdn', dev)
    model.test_cfg = dict(TILED, scene_cache_mb=20)
    assert ONE_SCENE < 20 << 20 < 2 * ONE_SCENE
    lq = _lq(*LR, dev)
    targets = [Grid(size=(80, 112)), Grid(size=HR), View(_view_a(), A_SIZE)]                  # each touches all four tiles
    enc = model.encode(lq, max_scale=2.7)
    outs = model.render_many(enc, targets)
    assert enc.cache.builds == 4 and len(enc.cache.entries) == 1 and 0 < enc.scene_bytes <= 20 << 20
    wants, ref = _singles(model, lq, targets)
    assert ref.cache.builds > 4                                                                # the single calls evict what the next one needs
    assert all(torch.equal(a, b) for a, b in zip(outs, wants))


def test_only_touched_tiles_are_built(dev):
    from ciaosr_amd.scene import Grid
    model = _model('rdn', dev)
    model.test_cfg = dict(TILED)
    lq = _lq(*LR, dev)
    enc = model.encode(lq, max_scale=2.7)
    targets = [Grid(size=HR, window=(0, 0, 5, 7)), Grid(size=HR, window=(0, 0, 20, 151))]
    outs = model.render_many(enc, targets)
    assert enc.cache.builds == 2 and sorted(enc.cache.entries) == [(0, (0, 0)), (0, (0, 24))]
    full = model.render_many(enc, [Grid(size=HR)])[0]
    assert enc.cache.builds == 4
    want = model.render(model.encode(lq, max_scale=2.7), size=HR)
    assert torch.equal(full, want)
    assert torch.equal(outs[0], want[..., :5, :7]) and torch.equal(outs[1], want[..., :20, :])


def test_scenes_are_built_from_batched_trunk_calls(dev, monkeypatch):
    from ciaosr_amd.scene import Grid, View
    model = _model('rdn', dev)
    lq = _lq(*LR, dev)
    targets = [Grid(size=HR), View(_view_a(), A_SIZE)]
    trunk = model.generator._encoder_hip
    inner = trunk.forward_hwc_batch
    calls = []

    def counted(x, *args, **kw):
        calls.append(x.shape[0])
        return inner(x, *args, **kw)

    monkeypatch.setattr(trunk, 'forward_hwc_batch', counted)
    first = None
    for n_batch, sizes in ((3, [3, 1]), (1, [1, 1, 1, 1]), (4, [4])):
        for ahead in (True, False):
            model.test_cfg = dict(TILED, tile_batch=n_batch, encoder_ahead=ahead)
            enc = model.encode(lq, max_scale=2.7)
            del calls[:]
            outs = model.render_many(enc, targets)
            assert calls == sizes and sum(sizes) == 4 and len(sizes) == math.ceil(4 / n_batch), (n_batch, ahead, calls)
            assert enc.cache.builds == 4
            if first is None:
                first = outs
            assert all(torch.equal(a, b) for a, b in zip(outs, first)), (n_batch, ahead)
    monkeypatch.undo()
    model.test_cfg = dict(TILED)
    wants, _ = _singles(model, lq, targets)
    assert all(torch.equal(a, b) for a, b in zip(first, wants))


def test_f16_keeps_the_grid_hint_of_more_than_64_coordinate_tensors(dev):
    """hip_ops keeps the grid width of the last 64 coordinate tensors; the 16-bit head answers a grid it does not know with another
    kernel and other sums.  68 (tile, target) pairs, each made right before its query: every one is still a known grid."""
    from ciaosr_amd import scene
    from ciaosr_amd.scene import Grid
    model = _model('rdn', dev)
    model.test_cfg = dict(TILED, precision='f16')
    lq = _lq(*LR, dev)
    windows = [(20 + 4 * k, 45 + k, 6, 40) for k in range(17)]
    pairs = sum(len(scene.plan_window(*LR, 32, 8, *HR, w, any_scale=True)) for w in windows)
    assert pairs == 68 > 64
    enc = model.encode(lq, max_scale=2.7)
    outs = model.render_many(enc, [Grid(size=HR, window=w) for w in windows])
    assert enc.cache.builds == 4
    ref = model.encode(lq, max_scale=2.7)
    for w, got in zip(windows, outs):
        want = model.render(ref, size=HR, window=w)
        assert got.shape == (1, 3, 6, 40) and torch.equal(got, want), (w, (got - want).abs().max().item())


def test_whole_image_batch_of_two(dev):
    from ciaosr_amd import scene
    from ciaosr_amd.scene import Grid, View
    model = _model('rdn', dev)
    model.test_cfg = dict()
    lq = torch.cat([_lq(24, 24, dev), _lq(24, 24, dev, seed=6)])
    size = (40, 52)
    targets = [Grid(scale=2.7, window=(0, 11, 37, 53)), View(scene.view_matrix((15.5, 17.25), 2.7, 30, size), size, fill=0.5)]
    enc = model.encode(lq, max_scale=2.7)
    outs = model.render_many(enc, targets)
    assert enc.cache.builds == 2                                                               # one scene per item
    wants, ref = _singles(model, lq, targets)
    assert [tuple(o.shape) for o in outs] == [(2, 3, 37, 53), (2, 3, 40, 52)] and ref.cache.builds == 2
    assert all(torch.equal(a, b) for a, b in zip(outs, wants))
    assert not torch.equal(outs[0][0], outs[0][1])
    assert model.prefetch(enc, targets) == 0
    fresh = model.encode(lq)                                                                   # nothing built yet, max_scale open
    assert fresh.cache.builds == 0 and model.prefetch(fresh, targets) == 2 and fresh.max_scale == 65 / 24      # the grid's, above the view's 2.7
    wants, _ = _singles(model, lq, targets, max_scale=65 / 24)
    assert all(torch.equal(a, b) for a, b in zip(model.render_many(fresh, targets), wants)) and fresh.cache.builds == 2


def test_other_trunk(dev):
    from ciaosr_amd.scene import Grid
    model = _model('edsr', dev)
    model.test_cfg = dict(scale=3.3)
    lq = _lq(24, 24, dev)
    want = model.render(model.encode(lq), scale=3.3)
    enc = model.encode(lq)
    assert torch.equal(model.render_many(enc, [Grid(scale=3.3)])[0], want) and enc.cache.builds == 1


def test_prefetch(dev):
    model = _model('rdn', dev)
    lq = _lq(*LR, dev)
    targets = _targets()
    model.test_cfg = dict(TILED)
    enc = model.encode(lq, max_scale=2.7)
    assert model.prefetch(enc, targets) == 4 and enc.cache.builds == 4 and len(enc.cache.entries) == 4
    outs = model.render_many(enc, targets)
    assert enc.cache.builds == 4                                                               # nothing left to build
    wants, _ = _singles(model, lq, targets)
    assert all(torch.equal(a, b) for a, b in zip(outs, wants))
    assert model.prefetch(enc, targets) == 0
    part = model.encode(lq, max_scale=2.7)
    assert model.prefetch(part, targets[3:]) == 1 and list(part.cache.entries) == [(0, (0, 0))]   # the shifted view: tile (0, 0) alone
    model.test_cfg = dict(TILED, scene_cache_mb=20)                                            # room for one scene: it stops there
    small = model.encode(lq, max_scale=2.7)
    assert model.prefetch(small, targets) == 1 and small.cache.builds == 1 and list(small.cache.entries) == [(0, (0, 0))]
    assert model.prefetch(small, targets) == 0 and small.cache.builds == 1                     # never evicts


def test_render_cli_many(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, metrics, scene
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_rgb01, imwrite
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    base = os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    text = open(base).read()
    assert text.count('tile=192, tile_overlap=32') == 1
    config = str(tmp_path / 'tiled.py')
    with open(config, 'w') as f:
        f.write(text.replace('tile=192, tile_overlap=32', 'tile=32, tile_overlap=8'))
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=SQRT6)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray((_lq(*LR, 'cpu', seed=8)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(png)
    view = ['--view', '31.0', '42.5', '2.7', '-32', '--size', '61', '83']
    with hip_ops.profile():
        paths = render.main([config, ckpt, png, '--scale', '2', '2.7', *view, '--out', str(tmp_path / 'out')])
    prof = hip_ops.profile.results()
    assert [os.path.basename(p) for p in paths] == ['img_x2.png', 'img_x2p7.png', 'img_view0.png']
    assert prof['head_unfold']['launches'] == 4, prof['head_unfold']                           # one scene per tile for the three outputs
    assert prof['view_count_many']['launches'] == 1 and 'view_count' not in prof
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True
    lq = imread_rgb01(png).unsqueeze(0).to(dev)
    enc = model.encode(lq, max_scale=2.7)
    wants = [model.render(enc, scale=2), model.render(enc, scale=2.7), model.render_view(enc, scene.view_matrix(*A_ARGS, A_SIZE), A_SIZE)]
    for path, want in zip(paths, wants):
        ref = str(tmp_path / ('ref_' + os.path.basename(path)))
        imwrite(metrics.tensor2img(want), ref)
        assert open(path, 'rb').read() == open(ref, 'rb').read(), path
