"""Deep Zoom pyramids end to end on the GPU (ciaosr_amd/pyramid.py, CiaoSR.render_pyramid, tools/render.py --dzi): the written tree read
back with Pillow, the model levels against the single `render` calls, the coarse levels against Pillow's own BICUBIC resize.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from tests.test_png_host import make_image

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _model(test_cfg, dev, kind='tiny'):
    """'tiny': the restorer of tests/test_png_gpu.py (head MLPs 64 wide: fp32 only -- the 16-bit head exists for the fused kernels,
    which take 256-wide MLPs).  'wide': a small EDSR restorer with the 256-wide head, which every precision runs."""
    if kind == 'tiny':
        from tests.test_png_gpu import _restorer
        return _restorer(test_cfg).to(dev)
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_hip_parity import _restorer
    model = _restorer('edsr', 4, dev, test_cfg, mid=64, blocks=2)
    seeded_init_(model, seed=17, gain=1.2, head_gain=6 ** 0.5)
    return model.to(dev)


def _lq(h, w, dev, seed=5):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(seed)).to(dev)


def _read_tree(out_dir, name, tile_size, overlap):
    """The levels of the written tree as RGB arrays, reassembled from the tiles without their overlaps; every tile -- overlaps
    included -- must show the reassembled level's pixels, so the strips two tiles share agree.  Also the files seen and their bytes."""
    from PIL import Image
    from ciaosr_amd.pyramid import dzi_plan
    root = ET.parse(os.path.join(out_dir, name + '.dzi')).getroot()
    assert root.tag == '{http://schemas.microsoft.com/deepzoom/2008}Image' and root.get('Format') == 'png'
    assert (int(root.get('TileSize')), int(root.get('Overlap'))) == (tile_size, overlap)
    size = root.find('{http://schemas.microsoft.com/deepzoom/2008}Size')
    height, width = int(size.get('Height')), int(size.get('Width'))
    plan = dzi_plan(height, width, tile_size, overlap)
    tree = os.path.join(out_dir, name + '_files')
    assert sorted(os.listdir(tree), key=int) == [str(lv['level']) for lv in plan]
    levels, files, nbytes = [], 1, os.path.getsize(os.path.join(out_dir, name + '.dzi'))
    for lv in plan:
        folder = os.path.join(tree, str(lv['level']))
        assert sorted(os.listdir(folder)) == sorted(f'{t[0]}_{t[1]}.png' for t in lv['tiles'])
        canvas = np.zeros((lv['height'], lv['width'], 3), dtype=np.uint8)
        tiles = []
        for col, row, y0, x0, h, w in lv['tiles']:
            path = os.path.join(folder, f'{col}_{row}.png')
            im = Image.open(path)
            assert im.mode == 'RGB' and im.size == (w, h)
            px = np.asarray(im)
            dy, dx = (overlap if row > 0 else 0), (overlap if col > 0 else 0)
            y1, x1 = min((row + 1) * tile_size, lv['height']), min((col + 1) * tile_size, lv['width'])
            canvas[y0 + dy:y1, x0 + dx:x1] = px[dy:y1 - y0, dx:x1 - x0]
            tiles.append((y0, x0, px))
            files += 1
            nbytes += os.path.getsize(path)
        for y0, x0, px in tiles:
            assert np.array_equal(canvas[y0:y0 + px.shape[0], x0:x0 + px.shape[1]], px), (lv['level'], y0, x0)
        levels.append(canvas)
    return (height, width), levels, files, nbytes


def _rgb(u8_bgr):
    return np.ascontiguousarray(u8_bgr.cpu().numpy()[:, :, ::-1])


@pytest.mark.parametrize('kind,precision', [('tiny', 'fp32'), ('wide', 'fp32'), ('wide', 'f16')])
def test_pyramid_untiled(dev, tmp_path, kind, precision):
    from PIL import Image
    from ciaosr_amd.pyramid import level_sizes, write_dzi
    model = _model(dict(precision=precision), dev, kind)
    lq = _lq(12, 10, dev)
    enc = model.encode(lq, max_scale=4)
    res = write_dzi(model, enc, str(tmp_path), 'img', scale=4, tile_size=16, overlap=1)
    sizes = [(1, 1), (2, 2), (3, 3), (6, 5), (12, 10), (24, 20), (48, 40)]
    assert level_sizes(48, 40) == sizes and res['levels'] == sizes and res['model_levels'] == [4, 5, 6]
    top, levels, files, nbytes = _read_tree(str(tmp_path), 'img', 16, 1)
    assert top == (48, 40) and [lv.shape[:2] for lv in levels] == sizes
    assert (res['files'], res['bytes']) == (files, nbytes) and files == 1 + 5 + 4 + 9              # the manifest; five one-tile levels, 2 x 2 and 3 x 3 tiles
    ref = model.encode(lq, max_scale=4)
    for k in res['model_levels']:
        want = model.render(ref, size=sizes[k], as_u8=True)
        assert np.array_equal(levels[k], _rgb(want)), k
    base = Image.fromarray(levels[4])                           # the smallest model level, 12 x 10
    for k in range(4):
        want = np.asarray(base.resize((sizes[k][1], sizes[k][0]), Image.BICUBIC))
        assert np.array_equal(levels[k], want), k
    # the images themselves: level 0 first, the same pixels as the files
    imgs = model.render_pyramid(model.encode(lq, max_scale=4), scale=4)
    assert [tuple(im.shape) for im in imgs] == [s + (3,) for s in sizes] and all(im.dtype == torch.uint8 and im.is_cuda for im in imgs)
    for k, im in enumerate(imgs):
        assert np.array_equal(_rgb(im), levels[k]), k


def test_pyramid_tiled_builds_every_scene_once(dev):
    from ciaosr_amd.pyramid import level_sizes
    cfg = dict(tile=12, tile_overlap=4, tile_any_scale=True)
    model = _model(cfg, dev)
    lq = _lq(20, 28, dev, seed=7)
    probe = model.encode(lq, max_scale=4)
    model.render(probe, scale=4, window=(0, 0, 2, 2))
    assert probe.cache.builds == 1
    one = probe.scene_bytes                                     # bytes of one tile's scene
    enc = model.encode(lq, max_scale=4)
    enc.cache.budget = 2 * one + one // 2                       # room for two scenes, not for three
    imgs = model.render_pyramid(enc, scale=4)
    sizes = level_sizes(80, 112)
    assert [tuple(im.shape[:2]) for im in imgs] == sizes and sizes[-3:] == [(20, 28), (40, 56), (80, 112)]
    assert enc.cache.builds == 6 and len(enc.cache.entries) == 2 and enc.scene_bytes <= enc.cache.budget      # 2 x 3 LR tiles, each once
    ref = model.encode(lq, max_scale=4)
    for k in range(len(sizes) - 3, len(sizes)):
        assert torch.equal(imgs[k], model.render(ref, size=sizes[k], as_u8=True)), k
    from PIL import Image
    base = Image.fromarray(imgs[-3].cpu().numpy())
    for k in range(len(sizes) - 3):
        want = np.asarray(base.resize((sizes[k][1], sizes[k][0]), Image.BICUBIC))
        assert np.array_equal(imgs[k].cpu().numpy(), want), k


def test_render_cli_dzi(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model
    from ciaosr_amd.config import Config
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray(make_image(12, 10, 'smooth')).save(png)
    argv = [config, ckpt, png, '--scale', '4']
    plain = render.main(argv + ['--out', str(tmp_path / 'plain')])
    both = render.main(argv + ['--dzi', '4', '--dzi-tile', '16', '--out', str(tmp_path / 'dzi')])
    assert [os.path.basename(p) for p in both] == [os.path.basename(p) for p in plain] == ['img_x4.png']
    assert open(both[0], 'rb').read() == open(plain[0], 'rb').read()                       # the scale output is unchanged
    assert sorted(os.listdir(tmp_path / 'plain')) == ['img_x4.png']
    assert sorted(os.listdir(tmp_path / 'dzi')) == ['img.dzi', 'img_files', 'img_x4.png']
    top, levels, files, _ = _read_tree(str(tmp_path / 'dzi'), 'img', 16, 1)
    assert top == (48, 40) and len(levels) == 7 and files == 1 + 5 + 4 + 9
    assert np.array_equal(levels[-1], np.asarray(Image.open(plain[0]).convert('RGB')))     # the top level shows the x4 render
