"""CPU tests of the GT -> LR degradation (ciaosr_amd/degrade.py) and the GT-only test dataset: the Pillow coefficient tables, the
RandomDownSampling size arithmetic, pipeline validation and dataset selection.  No GPU needed."""
import math

import numpy as np
import pytest

# sizes (H, W) x scales of the Pillow comparison; the GPU tests reuse them
GRID_SIZES = [(20, 37), (64, 64), (123, 200), (400, 311)]
GRID_SCALES = [2, 3, 4, 6, 8, 12, 18, 24, 30, 2.5, 3.3, 7.1]


def valid_pipeline(scale):
    """The reference's valid_pipeline (configs/001_*.py), restated."""
    return [dict(type='LoadImageFromFile', io_backend='disk', key='gt', flag='color', channel_order='rgb'),
            dict(type='RandomDownSampling', scale_min=scale, scale_max=scale),
            dict(type='RescaleToZeroOne', keys=['lq', 'gt']),
            dict(type='ImageToTensor', keys=['lq', 'gt']),
            dict(type='GenerateCoordinateAndCell', scale=scale),
            dict(type='Collect', keys=['lq', 'gt', 'coord', 'cell'], meta_keys=['gt_path'])]


def grid_image(h, w, kind, seed):
    if kind == 'random':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    return np.stack([127.5 + 127 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 + 0.3 * c) for c in range(3)], -1).astype(np.uint8)


def grid_cases():
    """(H, W, w_out, h_out, kind): the size x scale grid, 1-pixel outputs and the no-resize case."""
    cases = []
    for (h, w) in GRID_SIZES:
        for s in GRID_SCALES:
            for kind in ('random', 'smooth'):
                cases.append((h, w, max(1, math.floor(w / s + 1e-9)), max(1, math.floor(h / s + 1e-9)), kind))
    cases += [(37, 41, 1, 1, 'random'), (37, 41, 1, 9, 'smooth'), (37, 41, 9, 1, 'random'), (1, 1, 1, 1, 'random'),
              (45, 33, 33, 45, 'random'), (45, 33, 33, 20, 'smooth'), (45, 33, 10, 45, 'random')]
    return cases


def _filter(x):
    # the bicubic kernel as the issue restates it: a = -0.5
    a, x = -0.5, abs(x)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def scalar_tables(n_in, n_out):
    """Scalar restatement of Pillow's precompute_coeffs + normalize_coeffs_8bpc."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * math.ceil(support) + 1
    bounds, coef = [], []
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_filter((t + xmin - center + 0.5) * (1.0 / fs)) for t in range(xmax)]
        tot = sum(w)
        w = [v / tot for v in w] if tot != 0 else w
        row = [math.trunc(v * 4194304.0 + (0.5 if v >= 0 else -0.5)) for v in w]
        coef.append(row + [0] * (ksize - len(row)))
        bounds.append((xmin, xmax))
    return np.array(bounds, np.int64), np.array(coef, np.int64), ksize


def apply_tables(img, bounds, coef, axis):
    """Pillow's 8-bit pass along `axis` (1 = horizontal, 0 = vertical) with the given tables, in numpy int64."""
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for o, (xmin, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, np.int64)
        for t in range(n):
            acc += a[xmin + t] * int(coef[o, t])
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def numpy_resize(img, w_out, h_out):
    from ciaosr_amd.degrade import pillow_bicubic_tables
    h, w = img.shape[:2]
    x = img
    if w_out != w:
        b, k, _ = pillow_bicubic_tables(w, w_out)
        x = apply_tables(x, b, k, 1)
    if h_out != h:
        b, k, _ = pillow_bicubic_tables(h, h_out)
        x = apply_tables(x, b, k, 0)
    return x.copy()


def pil_resize(img, w_out, h_out):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((w_out, h_out), Image.BICUBIC))


@pytest.mark.parametrize('n_in,n_out', [(2040, 68), (1356, 113), (1356, 452), (400, 311), (100, 30), (37, 1), (20, 6), (200, 28),
                                        (64, 64), (5, 17)])
def test_tables_equal_scalar_restatement(n_in, n_out):
    from ciaosr_amd.degrade import pillow_bicubic_tables
    b, k, ks = pillow_bicubic_tables(n_in, n_out)
    rb, rk, rks = scalar_tables(n_in, n_out)
    assert ks == rks and b.dtype == np.int32 and k.dtype == np.int32
    assert np.array_equal(b, rb) and np.array_equal(k, rk)
    # every tap lies in the input, and the fixed-point weights sum to about 1
    assert (b[:, 0] >= 0).all() and (b.sum(1) <= n_in).all() and (b[:, 1] <= ks).all()
    assert (np.abs(k.sum(1) - (1 << 22)) <= ks).all()


def test_tables_at_x30_reach_121_taps():
    from ciaosr_amd.degrade import pillow_bicubic_tables
    b, k, ks = pillow_bicubic_tables(1350, 45)
    assert ks == 121 and b[:, 1].max() <= 121
    # |acc| < 255 sum |coef| + 2^21 < 2^31: the int32 sum is exact in any order
    assert 255 * np.abs(k.astype(np.int64)).sum(1).max() + (1 << 21) < 2 ** 31


@pytest.mark.parametrize('case', grid_cases(), ids=lambda c: '%dx%d-%dx%d-%s' % c)
def test_numpy_apply_of_tables_equals_pillow(case):
    h, w, w_out, h_out, kind = case
    img = grid_image(h, w, kind, seed=h * 1000 + w + w_out)
    assert np.array_equal(numpy_resize(img, w_out, h_out), pil_resize(img, w_out, h_out))


@pytest.mark.parametrize('h,w,scale,want', [
    (1356, 2040, 12, (113, 170, 1356, 2040)),
    (1350, 2040, 30, (45, 68, 1350, 2040)),
    (100, 100, 3.3, (30, 30, 99, 99)),
    (1356, 2040, 30, (45, 68, 1350, 2040)),
    (76, 100, 6, (12, 16, 72, 96)),
    (76, 100, 12, (6, 8, 72, 96)),
])
def test_random_down_sampling_sizes_and_crop(h, w, scale, want):
    from ciaosr_amd.degrade import RandomDownSampling, down_size
    assert down_size(h, w, scale) == want
    assert RandomDownSampling(scale_min=scale, scale_max=scale).sizes(h, w) == want


@pytest.mark.parametrize('kw,what', [(dict(patch_size=48), 'patch_size'), (dict(scale_max=8), 'scale'),
                                     (dict(interpolation='bilinear'), 'bicubic'), (dict(backend='cv2'), 'pillow')])
def test_random_down_sampling_refuses_training_forms(kw, what):
    from ciaosr_amd.degrade import RandomDownSampling
    args = dict(scale_min=6, scale_max=6)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        RandomDownSampling(**args)


def test_gt_dataset_accepts_reference_pipeline(tmp_path):
    from ciaosr_amd.dataset import SRFolderGTDataset
    from PIL import Image
    Image.fromarray(grid_image(30, 40, 'smooth', 0)).save(tmp_path / 'a.png')
    (tmp_path / 'notes.txt').write_text('not an image')
    ds = SRFolderGTDataset(tmp_path, valid_pipeline(12), scale=12, device='cpu')
    assert len(ds) == 1 and ds.down.scale == 12.0
    assert ds.paths[0].endswith('a.png')


def _bad(step, **changes):
    p = valid_pipeline(6)
    p[step] = dict(p[step], **changes)
    return p


@pytest.mark.parametrize('pipeline,match', [
    (valid_pipeline(6)[:2] + [dict(type='Flip', keys=['lq', 'gt'])] + valid_pipeline(6)[2:], "'Flip'"),
    (valid_pipeline(6)[:2] + [dict(type='PairedRandomCrop', gt_patch_size=96)] + valid_pipeline(6)[3:], "'PairedRandomCrop'"),
    (_bad(1, patch_size=48), 'patch_size'),
    (_bad(1, scale_min=1, scale_max=4), 'scale'),
    (_bad(1, interpolation='lanczos'), 'bicubic'),
    (_bad(0, channel_order='bgr'), 'channel_order'),
    (_bad(0, key='lq'), 'key'),
    (_bad(4, sample_quantity=2304), 'sample_quantity'),
    (valid_pipeline(6)[:1] + valid_pipeline(6)[2:], 'in this order'),
    ([valid_pipeline(6)[1], valid_pipeline(6)[0]] + valid_pipeline(6)[2:], 'in this order'),
])
def test_gt_dataset_refuses_other_pipelines(tmp_path, pipeline, match):
    from ciaosr_amd.dataset import SRFolderGTDataset
    with pytest.raises(ValueError, match=match):
        SRFolderGTDataset(tmp_path, pipeline, scale=6, device='cpu')


def test_build_test_dataset_chooses_class_by_type(tmp_path):
    from ciaosr_amd.config import ConfigDict
    from ciaosr_amd.dataset import SRFolderDataset, SRFolderGTDataset, build_test_dataset
    (tmp_path / 'gt').mkdir()
    (tmp_path / 'lq').mkdir()
    paired = ConfigDict(type='SRFolderDataset', lq_folder=str(tmp_path / 'lq'), gt_folder=str(tmp_path / 'gt'), scale=4,
                        filename_tmpl='{}')
    gt_only = ConfigDict(type='SRFolderGTDataset', gt_folder=str(tmp_path / 'gt'), pipeline=valid_pipeline(12), scale=12)
    assert type(build_test_dataset(paired, 'cpu')) is SRFolderDataset
    ds = build_test_dataset(gt_only, 'cpu')
    assert type(ds) is SRFolderGTDataset and ds.down.scale == 12.0
    with pytest.raises(ValueError, match='LQ folder'):
        build_test_dataset(gt_only, 'cpu', lq_folder=str(tmp_path / 'lq'))
    with pytest.raises(ValueError, match='RepeatDataset'):
        build_test_dataset(ConfigDict(type='RepeatDataset', gt_folder=str(tmp_path / 'gt')), 'cpu')


@pytest.mark.parametrize('val_scale', [4, 6, 12, 30])
def test_configs_switch_to_gt_only_above_x4(tmp_path, val_scale):
    import glob
    import os
    from ciaosr_amd.config import Config
    from ciaosr_amd.dataset import check_gt_pipeline
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = sorted(glob.glob(os.path.join(repo, 'configs', '001_*.py')))
    assert len(paths) == 3
    for p in paths:
        text = open(p).read()
        assert '\nval_scale = 4\n' in text
        cfg_path = tmp_path / os.path.basename(p)
        cfg_path.write_text(text.replace('\nval_scale = 4\n', f'\nval_scale = {val_scale}\n'))
        t = Config.fromfile(str(cfg_path)).data.test
        if val_scale <= 4:
            assert t.type == 'SRFolderDataset' and t.lq_folder.endswith(f'LRbicx{val_scale}')
        else:
            assert t.type == 'SRFolderGTDataset' and 'lq_folder' not in t and t.gt_folder.endswith('GTmod12')
            assert t.scale == val_scale and check_gt_pipeline(t.pipeline).scale == val_scale


def test_imread_u8_returns_hwc_uint8(tmp_path):
    from ciaosr_amd.imageio import imread_u8
    from PIL import Image
    img = grid_image(9, 13, 'random', 1)
    Image.fromarray(img).save(tmp_path / 'x.png')
    Image.fromarray(img[:, :, 0]).save(tmp_path / 'gray.png')
    got = imread_u8(str(tmp_path / 'x.png'))
    assert got.dtype == np.uint8 and got.shape == (9, 13, 3) and np.array_equal(got, img)
    assert imread_u8(str(tmp_path / 'gray.png')).shape == (9, 13, 3)
