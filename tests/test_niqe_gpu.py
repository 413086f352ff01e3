"""NIQE on the device (csrc/niqe_f32.hip, ciaosr_amd/niqe_hip.py) against the float64 restatement tests/niqe_ref.py and the reference's
own runs in tests/golden/niqe_cases.npz -- never the device against itself.

Tolerance.  The yardstick is the reference's own noise G: per fixture case the gap between its run as written (float32 plane) and the
same code on the float64 plane, recorded by tools/make_niqe_golden.py: features (relative, non-alpha columns) up to 2.232e-05, NIQE up
to 3.013e-06.  The device gets 2 x the largest G over the cases (one G for keeping float32 where the reference does, one for another
summation order and FMA in the windows).  The kernels keep every map in fp64 in the restatement's operation order, so the measured
device gaps are far inside: see DESIGN 4.1i-f.  Alpha columns: at most 1 % of the entries may differ from the float64 run, each by
exactly one grid step.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import niqe_ref
from tests.test_niqe_host import GOLDEN, REPO, load_cases

pytestmark = pytest.mark.gpu

ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
OTHER_COLS = [c for c in range(36) if c not in ALPHA_COLS]
GRID_STEP = 0.001


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return load_cases()


@pytest.fixture(scope='module')
def params():
    from ciaosr_amd import niqe_hip
    return niqe_hip.load_params(os.path.join(GOLDEN, 'niqe_pris_params.npz'))


@pytest.fixture(scope='module')
def tol(cases):
    """(features, NIQE): 2 x the largest gap between the reference's float32 and float64 runs over the fixture cases."""
    return 2 * max(c['g_feat'] for c in cases), 2 * max(c['g_niqe'] for c in cases)


def exact_luma(img, crop):
    """(rounding of the exact Y, mask of the pixels whose exact Y is farther than 1e-4 from a half) in integer arithmetic:
    Y = 16 + t / 255000, t = 24966 B + 128553 G + 65481 R."""
    p = img.astype(np.int64)
    t = 24966 * p[:, :, 0] + 128553 * p[:, :, 1] + 65481 * p[:, :, 2]
    q, rem = t // 255000, t % 255000
    low = 16 + q
    want = np.where(rem > 127500, low + 1, low)
    decided = np.abs(rem - 127500) > 1e-4 * 255000
    if crop:
        low, want, decided = (a[crop:-crop, crop:-crop] for a in (low, want, decided))
    return low, want, decided


def check_luma(y, img, crop, what):
    low, want, decided = exact_luma(img, crop)
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == want.shape, what
    assert np.array_equal(y[decided], want[decided]), what
    assert ((y == low) | (y == low + 1))[~decided].all(), what
    return int((~decided).sum())


def device_run(img, params, crop, dev):
    """(luma, features, NIQE) of the device for a uint8 BGR array or tensor."""
    from ciaosr_amd import niqe_hip
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    m, luma = niqe_hip.moments_u8(t, params, crop, return_luma=True)
    feats = niqe_hip.features(m)
    return luma.cpu().numpy(), feats, niqe_hip.finish(feats, params), m


def compare(feats, q, want, q_want, tol, what):
    """Device features / NIQE against a float64 run: the bound on the non-alpha columns and on NIQE, the alpha rule.  Prints the gaps."""
    assert feats.shape == want.shape and np.array_equal(np.isnan(feats), np.isnan(want)), what
    a, b = feats[:, OTHER_COLS], want[:, OTHER_COLS]
    ok = ~np.isnan(b)
    gf = float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))
    gq = abs(q - q_want) / abs(q_want)
    da = np.abs(feats[:, ALPHA_COLS] - want[:, ALPHA_COLS])
    moved = da > GRID_STEP / 2
    print(f'{what}: features {gf:.3e} (bound {tol[0]:.3e}), NIQE {gq:.3e} (bound {tol[1]:.3e}), alpha entries moved {int(moved.sum())} of {da.size}')
    assert gf <= tol[0] and gq <= tol[1], what
    assert (da[moved] < 1.5 * GRID_STEP).all() and moved.sum() <= 0.01 * da.size, what
    return gf, gq


def test_luma_plane_is_the_exact_rounding(dev, cases, params):
    for c in cases:
        assert check_luma(c['y'], c['img'], c['crop'], 'fixture ' + c['name']) >= 0          # the fixture's own plane obeys the rule
        luma = device_run(c['img'], params, c['crop'], dev)[0]
        assert luma.dtype == np.float32
        ties = check_luma(luma, c['img'], c['crop'], 'device ' + c['name'])
        print(f"{c['name']}: {ties} pixels within 1e-4 of a half; device plane differs from the fixture's in "
              f"{int((luma != c['y']).sum())} pixels")
    # every byte value of every channel, and the pixels nearest to a tie
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (192, 192, 3), dtype=np.uint8)
    img[0, :, :] = np.arange(192)[:, None]
    img[1, :64] = (255, 255, 255)
    img[1, 64:128] = (0, 0, 0)
    check_luma(device_run(img, params, 0, dev)[0], img, 0, 'random')


def test_features_and_niqe_of_the_fixture_cases(dev, cases, params, tol):
    worst = [0.0, 0.0]
    for c in cases:
        luma, feats, q, m = device_run(c['img'], params, c['crop'], dev)
        assert feats.dtype == np.float64 and type(q) is float
        want, q_want = niqe_ref.niqe(luma, params)                       # the restatement on the DEVICE's luma plane
        g = compare(feats, q, want, q_want, tol, c['name'] + ' vs restatement')
        worst = [max(worst[0], g[0]), max(worst[1], g[1])]
        gq = abs(q - c['niqe64']) / c['niqe64']
        print(f"{c['name']}: device NIQE {q:.9f}, reference float64 run {c['niqe64']:.9f} (gap {gq:.3e}), float32 run {c['niqe32']:.9f}")
        assert gq <= tol[1]
        if np.array_equal(luma, c['y']):
            compare(feats, q, c['feat64'], c['niqe64'], tol, c['name'] + ' vs reference float64 run')
        # the sign of every sample is the restatement's: the counts of negatives and positives agree exactly
        m_ref = niqe_ref.moments(luma, params['gaussian_window'])
        assert np.array_equal(m.cpu().numpy()[..., [0, 2]], m_ref[..., [0, 2]])
        # bitwise repeatable
        m2 = device_run(c['img'], params, c['crop'], dev)[3]
        assert torch.equal(m.view(torch.int64), m2.view(torch.int64))
    print(f'worst device gap to the restatement: features {worst[0]:.3e}, NIQE {worst[1]:.3e}')
    flat = device_run(cases[4]['img'], params, 0, dev)[1]
    assert np.isnan(flat).any(axis=1).tolist() == [False, False, True, False, False, False] and flat[2, 0] == 0.2


def test_pitched_crop_view(dev, params, tol):
    from ciaosr_amd import niqe_hip
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:230, 0:330]
    base = 110 + 60 * np.sin(yy / 9.0) * np.cos(xx / 13.0)
    big = np.clip(np.rint(base[:, :, None] + rng.normal(0, 6, (230, 330, 3))), 0, 255).astype(np.uint8)
    t = torch.from_numpy(big).to(dev)
    view = t[13:13 + 200, 17:17 + 301]
    assert not view.is_contiguous()
    luma, feats, q, m = device_run(view, params, 3, dev)
    m2 = niqe_hip.moments_u8(view.contiguous(), params, 3)
    assert torch.equal(m.view(torch.int64), m2.view(torch.int64))          # independent of the pitch, bit for bit
    check_luma(luma, big[13:213, 17:318], 3, 'view')
    want, q_want = niqe_ref.niqe(luma, params)
    compare(feats, q, want, q_want, tol, 'pitched view 200x301 crop 3')
    assert abs(niqe_hip.niqe_u8(view, params, 3) - q) == 0


def test_wrap_borders_and_transposition(dev, params, tol):
    """Blocks that differ strongly from their neighbours: a roll into the neighbouring block, or a clamp at the block border, changes the
    product maps; a transposed image has another block order and another order of the two resample passes."""
    rng = np.random.default_rng(9)
    means = np.array([[50, 190, 70], [200, 60, 180]], dtype=np.float64)           # checkerboard of block means, 2 x 3 blocks
    sig = np.array([[3, 14, 6], [12, 4, 9]], dtype=np.float64)
    y = np.kron(means, np.ones((96, 96))) + np.kron(sig, np.ones((96, 96))) * rng.normal(0, 1, (192, 288))
    img = np.clip(np.rint(y[:, :, None] + rng.normal(0, 2, (192, 288, 3))), 0, 255).astype(np.uint8)
    scores = []
    for name, im in (('checkerboard', img), ('checkerboard transposed', np.ascontiguousarray(img.transpose(1, 0, 2)))):
        luma, feats, q, _ = device_run(im, params, 0, dev)
        want, q_want = niqe_ref.niqe(luma, params)
        compare(feats, q, want, q_want, tol, name)
        scores.append(q)
    assert abs(scores[0] - scores[1]) / scores[0] > 10 * tol[1]


def _restorer(test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    from ciaosr_amd.init_utils import seeded_init_
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[32, 32])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=16, num_blocks=2),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                   test_cfg=test_cfg).eval()
    seeded_init_(model, seed=3, gain=2.0, head_gain=6 ** 0.5)
    return model


NIQE_KERNELS = ('niqe_luma', 'niqe_mscn', 'niqe_half', 'niqe_moments')


def test_evaluate_and_forward_test(dev, params):
    from ciaosr_amd import hip_ops, metrics, metrics_hip, niqe_hip
    from ciaosr_amd.coords import make_cell, make_coord
    g = torch.Generator().manual_seed(4)
    gt = torch.rand(1, 3, 192, 192, generator=g)
    out = (gt + 0.05 * torch.randn(1, 3, 192, 192, generator=g)).clamp(0, 1)
    path = os.path.join(GOLDEN, 'niqe_pris_params.npz')
    for gpu_metrics in (False, True):
        cfg = dict(metrics=['PSNR', 'NIQE'], crop_border=0, convert_to='y', niqe_params=path, gpu_metrics=gpu_metrics)
        model = _restorer(cfg).to(dev)
        with hip_ops.profile():
            res = model.evaluate(out.to(dev), gt.to(dev))
        prof = hip_ops.profile.results()
        assert list(res) == ['PSNR', 'NIQE'] and type(res['NIQE']) is float
        assert type(res['PSNR']) is (float if gpu_metrics else np.float32)      # the host PSNR is numpy's, as before
        assert [prof[k]['launches'] for k in NIQE_KERNELS] == [1, 2, 1, 1]
        assert res['NIQE'] == niqe_hip.niqe_u8(metrics_hip.tensor2img_u8(out.to(dev)), params, 0)
        if not gpu_metrics:
            assert res['PSNR'] == metrics.psnr(metrics.tensor2img(out), metrics.tensor2img(gt), 0, 'y')
        # without niqe_params: no launch of these kernels, the same PSNR
        plain = _restorer(dict(metrics=['PSNR'], crop_border=0, convert_to='y', gpu_metrics=gpu_metrics)).to(dev)
        with hip_ops.profile():
            res0 = plain.evaluate(out.to(dev), gt.to(dev))
        assert not any(k.startswith('niqe') for k in hip_ops.profile.results()) and res0 == {'PSNR': res['PSNR']}
    # forward_test without a ground truth
    model = _restorer(dict(scale=2, metrics=['NIQE'], crop_border=0, niqe_params=path)).to(dev)
    lq = torch.rand(1, 3, 48, 96, generator=g)
    coord, cell = make_coord((96, 192)).unsqueeze(0), make_cell((96, 192)).unsqueeze(0)
    res = model(lq=lq.to(dev), gt=None, test_mode=True, coord=coord.to(dev), cell=cell.to(dev))['eval_result']
    want = niqe_hip.niqe_u8(metrics_hip.tensor2img_u8(model.restore(lq.to(dev), coord.to(dev), cell.to(dev))), params)
    assert list(res) == ['NIQE'] and type(res['NIQE']) is float and res['NIQE'] == want
    model.test_cfg['metrics'] = ['NIQE', 'PSNR']
    with pytest.raises(AssertionError):
        model(lq=lq.to(dev), gt=None, test_mode=True, coord=coord.to(dev), cell=cell.to(dev))


def test_render_cli_niqe(dev, tmp_path, params):
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, niqe_hip
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_u8
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    rng = np.random.default_rng(2)
    Image.fromarray(rng.integers(0, 256, (24, 50, 3), dtype=np.uint8)).save(png)
    argv = [config, ckpt, png, '--scale', '4', '--view', '11.0', '14.5', '2.2', '20', '--size', '37', '45']
    plain = render.main(argv + ['--out', str(tmp_path / 'plain')])
    assert not os.path.exists(tmp_path / 'plain' / 'niqe.json')
    with hip_ops.profile():
        scored = render.main(argv + ['--niqe', os.path.join(GOLDEN, 'niqe_pris_params.npz'), '--out', str(tmp_path / 'scored')])
    prof = hip_ops.profile.results()
    assert prof['niqe_moments']['launches'] == 1                      # the view is too small for two blocks: never launched
    for a, b in zip(plain, scored):
        assert open(a, 'rb').read() == open(b, 'rb').read()             # the outputs do not change
    scores = json.load(open(tmp_path / 'scored' / 'niqe.json'))
    assert list(scores) == ['img_x4.png', 'img_view0.png'] and scores['img_view0.png'] is None
    pixels = imread_u8(scored[0])
    assert pixels.shape == (96, 200, 3)
    bgr = torch.from_numpy(np.ascontiguousarray(pixels[:, :, ::-1])).to(dev)
    assert type(scores['img_x4.png']) is float and scores['img_x4.png'] == niqe_hip.niqe_u8(bgr, params)
