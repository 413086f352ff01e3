"""CiaoSR.encode / render against CiaoSR.restore under the same test_cfg (bitwise: the same kernels on the same operands), whole-image
and tiled, and tools/render.py against the files `restore` gives."""
import os

import pytest
import torch

from tests.helpers import SQRT6, randn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = (9, 41, 61, 35)        # crosses both seams of the 2 x 2 tiles of the 40 x 56 image at x2 and at x2.7


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_models = {}


def _model(kind, dev):
    """Random-init restorers (explicit seed) on the smallest trunks the tests of the trunks themselves use; test_cfg is set per test."""
    if kind not in _models:
        from ciaosr_amd.init_utils import seeded_init_
        if kind == 'swinir':
            from tests.test_host_logic import _swinir_ciaosr
            model = _swinir_ciaosr(dict())
        else:
            from tests.test_hip_parity import _restorer
            model = _restorer(kind, 4, dev, dict(), blocks=3, layers=4)
        seeded_init_(model, seed=17, gain=1.2, head_gain=SQRT6)
        _models[kind] = model.to(dev)
    return _models[kind]


def _lq(h, w, dev, seed=5):
    return (randn((1, 3, h, w), seed) * 0.2 + 0.45).clamp(0, 1).to(dev)


def _grid(ht, wt, dev):
    from ciaosr_amd.coords import make_cell, make_coord
    return make_coord((ht, wt)).unsqueeze(0).to(dev), make_cell((ht, wt)).unsqueeze(0).to(dev)


def _device_grid(ht, wt, dev):
    """The grid as the library makes it for itself (clip_test, the device dataset): the same values as `_grid`, and known to the 16-bit
    chained head kernel as a row-major grid.  That kernel walks a known grid in 16 x 4 blocks; queries in index order put the keys of 8
    consecutive queries of a row outside a row tile's 4 x 4 key-pixel window below about x3, and the whole launch is then redone by the
    128-row kernel, with other fp32 summation orders (tests/test_hip_parity.py, test_chained_16bit_head_kernel_vs_the_128_row_kernels).
    `render` always knows its grid, so it is `restore` on a grid that `restore` knows too."""
    from ciaosr_amd import hip_ops
    coord, cell = hip_ops.make_coord_cell(ht, wt, dev)
    return coord.unsqueeze(0), cell.unsqueeze(0)


def _crop(img, window):
    i0, j0, hh, ww = window
    return img[..., i0:i0 + hh, j0:j0 + ww]


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_whole_image_render_is_restore(dev, precision):
    model = _model('rdn', dev)
    model.test_cfg = dict(scale=4, precision=precision)
    lq = _lq(24, 24, dev)
    enc = model.encode(lq)
    assert enc.cache.builds == 1 and enc.scene_bytes >= 24 * 24 * 13968       # max_scale from test_cfg.scale: built by encode, with the logit table
    for s, window in ((4, (3, 50, 70, 41)), (2.7, (0, 11, 37, 53))):
        ht, wt = round(24 * s), round(24 * s)
        assert all(torch.equal(a, b) for a, b in zip(_grid(ht, wt, dev), _device_grid(ht, wt, dev)))
        want = model.restore(lq, *(_grid if precision == 'fp32' else _device_grid)(ht, wt, dev))
        got = model.render(enc, scale=s)
        assert got.shape == want.shape == (1, 3, ht, wt)
        assert torch.equal(got, want), (s, (got - want).abs().max().item())
        assert torch.equal(model.render(enc, size=(ht, wt), window=window), _crop(want, window))
    assert enc.cache.builds == 1
    u8 = model.render(enc, scale=2.7, as_u8=True)
    from ciaosr_amd import metrics_hip
    assert u8.dtype == torch.uint8 and torch.equal(u8, metrics_hip.tensor2img_u8(want))
    with pytest.raises(ValueError):
        model.render(enc, scale=2.7, window=(0, 0, 66, 10))


@pytest.mark.parametrize('kind', ['edsr', 'swinir'])
def test_whole_image_render_other_trunks(dev, kind):
    model = _model(kind, dev)
    model.test_cfg = dict(scale=3.3)
    lq = _lq(24, 24, dev)
    ht = wt = round(24 * 3.3)
    want = model.restore(lq, *_grid(ht, wt, dev))
    enc = model.encode(lq)
    assert torch.equal(model.render(enc, scale=3.3), want)


def test_first_render_sets_the_plan_without_a_configured_scale(dev):
    model = _model('rdn', dev)
    model.test_cfg = dict()
    lq = _lq(24, 24, dev)
    enc = model.encode(lq)
    assert enc.cache.builds == 0 and enc.max_scale is None
    want = model.restore(lq, *_grid(79, 79, dev))
    assert torch.equal(model.render(enc, scale=3.3), want) and enc.cache.builds == 1 and abs(enc.max_scale - 79 / 24) < 1e-12


def test_tiled_render_is_restore(dev):
    model = _model('rdn', dev)
    lq = _lq(40, 56, dev)
    for cache_mb, any_scale, (ht, wt) in ((None, False, (80, 112)), (None, True, (108, 151)), (20, False, (80, 112)), (20, True, (108, 151))):
        cfg = dict(scale=2, tile=32, tile_overlap=8)
        if any_scale:
            cfg['tile_any_scale'] = True
        if cache_mb:
            cfg['scene_cache_mb'] = cache_mb
        model.test_cfg = cfg
        want = model.restore(lq, *_grid(ht, wt, dev))
        enc = model.encode(lq, max_scale=2.7 if any_scale else None)
        assert enc.cache.builds == 0                                # tile scenes are built when a render first touches them
        corner = model.render(enc, size=(ht, wt), window=(0, 0, 5, 7))
        assert enc.cache.builds == 1 and torch.equal(corner, _crop(want, (0, 0, 5, 7)))
        got = model.render(enc, size=(ht, wt))
        assert got.shape == want.shape == (1, 3, ht, wt)
        assert torch.equal(got, want), (cfg, (got - want).abs().max().item())
        assert torch.equal(model.render(enc, size=(ht, wt), window=WINDOW), _crop(want, WINDOW))
        one_scene = 32 * 32 * 13968
        if cache_mb:                                                # room for one tile scene (14.3 MB), not for two: works by rebuilding
            assert one_scene < cache_mb << 20 < 2 * one_scene
            assert enc.cache.builds > 4 and len(enc.cache.entries) == 1 and enc.scene_bytes <= cache_mb << 20
        else:
            assert enc.cache.builds == 4 and len(enc.cache.entries) == 4
    model.test_cfg = dict(scale=2, tile=32, tile_overlap=8)
    enc = model.encode(lq)
    with pytest.raises(ValueError):                                 # `restore` cannot make this image either
        model.render(enc, size=(108, 151))


def test_render_cli_writes_the_files_restore_gives(dev, tmp_path):
    import numpy as np
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, metrics
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_rgb01, imwrite
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=SQRT6)
    ckpt, png, out = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png'), str(tmp_path / 'out')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray((_lq(24, 24, 'cpu', seed=8)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(png)
    with hip_ops.profile():
        paths = render.main([config, ckpt, png, '--scale', '2', '3.3', '--out', out])
    prof = hip_ops.profile.results()
    assert prof['make_coord_cell_window']['launches'] == 2
    assert prof['head_unfold']['launches'] == 1, prof['head_unfold']      # one encode in total: the per-image stages ran once ...
    trunk = {k: v['launches'] for k, v in prof.items() if k.startswith('enc_')}
    assert trunk, sorted(prof)
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                               # what the tool sets: the configs tile integer scales only
    lq = imread_rgb01(png).unsqueeze(0).to(dev)
    with hip_ops.profile():
        wants = [model.restore(lq, *_grid(round(24 * s), round(24 * s), dev)) for s in (2, 3.3)]
    twice = {k: v['launches'] for k, v in hip_ops.profile.results().items() if k.startswith('enc_')}
    assert twice == {k: 2 * n for k, n in trunk.items()}                  # ... and so did the trunk: half of what two restores launch
    assert [os.path.basename(p) for p in paths] == ['img_x2.png', 'img_x3p3.png']
    for path, want in zip(paths, wants):
        ref = str(tmp_path / ('ref_' + os.path.basename(path)))
        imwrite(metrics.tensor2img(want), ref)
        assert open(path, 'rb').read() == open(ref, 'rb').read(), path
