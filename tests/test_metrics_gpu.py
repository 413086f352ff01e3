"""GPU tests of the device evaluation path (csrc/metrics_u8.hip, ciaosr_amd/metrics_hip.py, `test_cfg.gpu_metrics`) against the
HOST code (ciaosr_amd/metrics.py) and the float64 restatement of tests/test_metrics_host.py -- never the device against itself.
Tolerances and their derivation: tests/test_metrics_host.py.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_metrics_host import (CONVERT, CROPS, PSNR_TOL_DB, SIGMAS, SIZES, SSIM_TOL, image_pair, psnr64, ssim64)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bits(res):
    return {k: np.float64(v).tobytes() for k, v in res.items()}


# ---- 5: the quantiser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(1, 1), (37, 53), (768, 768)])
def test_tensor2img_u8_is_bitwise_the_host_quantiser(dev, h, w):
    from ciaosr_amd import metrics
    from ciaosr_amd.metrics_hip import tensor2img_u8
    g = torch.Generator().manual_seed(h * 1000 + w)
    ties = ((torch.arange(255, dtype=torch.float64) + 0.5) / 255).float()          # every exact tie (k + 0.5) / 255 as fp32
    special = torch.cat([ties, torch.tensor([0.0, 1.0, -0.0])])
    inputs = [torch.rand(1, 3, h, w, generator=g) * 1.4 - 0.2]
    n = 3 * h * w
    inputs.append(special.repeat(n // special.numel() + 1)[:n].view(1, 3, h, w).clone())
    inputs.append(inputs[0][0].clone())                                           # [3, H, W] form
    for t in inputs:
        want = metrics.tensor2img(t)
        got = tensor2img_u8(t.to(dev))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.device == dev
        assert np.array_equal(got.cpu().numpy(), want), int(np.abs(got.cpu().numpy().astype(int) - want).max())


# ---- 6: the metric kernel against the host functions -------------------------------------------------------------------------------
@pytest.mark.parametrize('convert_to', CONVERT)
@pytest.mark.parametrize('h,w', SIZES)
def test_psnr_ssim_u8_against_the_host_functions(dev, h, w, convert_to):
    from ciaosr_amd import metrics
    from ciaosr_amd.metrics_hip import psnr_ssim_u8
    worst = [0.0, 0.0, 0.0, 0.0]
    for sigma in SIGMAS:
        a, b = image_pair(h, w, sigma)
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        for crop in CROPS:
            both = psnr_ssim_u8(da, db, crop, convert_to)
            assert list(both) == ['PSNR', 'SSIM'] and all(type(v) is float for v in both.values())
            only_p = psnr_ssim_u8(da, db, crop, convert_to, want=('PSNR',))
            only_s = psnr_ssim_u8(da, db, crop, convert_to, want=('SSIM',))
            assert _bits(only_p) == {'PSNR': _bits(both)['PSNR']} and _bits(only_s) == {'SSIM': _bits(both)['SSIM']}
            hp, hs = float(metrics.psnr(a, b, crop, convert_to)), metrics.ssim(a, b, crop, convert_to)
            dp, ds = abs(both['PSNR'] - hp), abs(both['SSIM'] - hs)
            worst[0], worst[1] = max(worst[0], dp), max(worst[1], ds)
            if (h, w) != SIZES[-1]:                                      # the float64 restatement (its cost keeps it off 768x768)
                worst[2] = max(worst[2], abs(both['PSNR'] - psnr64(a, b, crop, convert_to)))
                worst[3] = max(worst[3], abs(both['SSIM'] - ssim64(a, b, crop, convert_to)))
            print(f'{h}x{w} sigma {sigma} crop {crop} {convert_to}: PSNR {both["PSNR"]:.6f} (host {hp:.6f}, d {dp:.3g}) '
                  f'SSIM {both["SSIM"]:.9f} (d {ds:.3g})')
            assert dp <= PSNR_TOL_DB and ds <= SSIM_TOL, (h, w, sigma, crop, convert_to, both, hp, hs)
    print(f'{h}x{w} {convert_to}: max |dPSNR| {worst[0]:.3g} dB, max |dSSIM| {worst[1]:.3g} vs host; '
          f'{worst[2]:.3g} dB, {worst[3]:.3g} vs float64')
    assert worst[2] <= PSNR_TOL_DB and worst[3] <= SSIM_TOL


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_identical_images_and_one_level_difference(dev):
    from ciaosr_amd import metrics
    from ciaosr_amd.metrics_hip import psnr_ssim_u8
    a, _ = image_pair(150, 210, 3.0)
    da = torch.from_numpy(a).to(dev)
    for conv in CONVERT:
        res = psnr_ssim_u8(da, da.clone(), 4, conv)
        assert res['PSNR'] == float('inf') and abs(res['SSIM'] - 1.0) <= 1e-12, res
    a, _ = image_pair(300, 300, 3.0)
    b = a.copy()
    b[150, 160, 1] = int(a[150, 160, 1]) + (1 if a[150, 160, 1] < 255 else -1)
    res = psnr_ssim_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), 4, None, want=('PSNR',))
    host = float(metrics.psnr(a, b, 4, None))
    exact = 10 * math.log10(255 ** 2 * 3 * 292 * 292)
    print(f'one level: device {res["PSNR"]:.10f} host {host:.10f} exact {exact:.10f}')
    assert abs(res['PSNR'] - host) <= PSNR_TOL_DB and abs(res['PSNR'] - exact) <= 1e-9


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('convert_to', CONVERT)
def test_pitched_view_repeat_and_poisoned_workspace_are_bitwise_equal(dev, convert_to):
    from ciaosr_amd import hip_ops, metrics
    from ciaosr_amd.metrics_hip import psnr_ssim_u8
    a, b = image_pair(211, 333, 12.0)
    big_a, big_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    va, vb = big_a[3:-5, 7:-2], big_b[3:-5, 7:-2]
    assert not va.is_contiguous() and va.stride(0) == 3 * 333
    ref = psnr_ssim_u8(va.contiguous(), vb.contiguous(), 4, convert_to)
    assert _bits(psnr_ssim_u8(va, vb, 4, convert_to)) == _bits(ref)
    assert _bits(psnr_ssim_u8(va, vb.contiguous(), 4, convert_to)) == _bits(ref)
    assert _bits(psnr_ssim_u8(va.contiguous(), vb.contiguous(), 4, convert_to)) == _bits(ref)
    hip_ops.poison_workspaces()
    assert _bits(psnr_ssim_u8(va, vb, 4, convert_to)) == _bits(ref)
    ha, hb = np.ascontiguousarray(a[3:-5, 7:-2]), np.ascontiguousarray(b[3:-5, 7:-2])
    assert abs(ref['PSNR'] - float(metrics.psnr(ha, hb, 4, convert_to))) <= PSNR_TOL_DB
    assert abs(ref['SSIM'] - metrics.ssim(ha, hb, 4, convert_to)) <= SSIM_TOL


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_too_small_for_ssim_and_argument_errors(dev):
    from ciaosr_amd import hip_ops, metrics
    from ciaosr_amd._lib import CiaoSRHipError
    from ciaosr_amd.metrics_hip import psnr_ssim_u8
    a, b = image_pair(20, 20, 12.0)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    with hip_ops.profile():
        with pytest.raises(ValueError):
            psnr_ssim_u8(da, db, 5, 'y')
        with pytest.raises(ValueError):
            psnr_ssim_u8(da, db, 5, 'y', want=('SSIM',))
        with pytest.raises(ValueError):
            psnr_ssim_u8(da, db, 10, 'y', want=('PSNR',))
        with pytest.raises(ValueError, match='Wrong color model'):
            psnr_ssim_u8(da, db, 0, 'ycbcr')
        with pytest.raises(AssertionError, match='Image shapes are different'):
            psnr_ssim_u8(da, db[:19], 0, 'y')
        with pytest.raises(CiaoSRHipError):
            psnr_ssim_u8(da.cpu(), db, 0, 'y')
    assert not hip_ops.profile.results(), hip_ops.profile.results()          # nothing was launched
    for conv in CONVERT:
        res = psnr_ssim_u8(da, db, 5, conv, want=('PSNR',))
        assert list(res) == ['PSNR'] and abs(res['PSNR'] - float(metrics.psnr(a, b, 5, conv))) <= PSNR_TOL_DB


# ---- 10: restorer level -------------------------------------------------------------------------------------------------------------
def _edsr_restorer(scale, test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[256] * 4)
    gen = dict(type=LocalImplicitSREDSR,
               encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=64, num_blocks=16),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    return CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss', loss_weight=1.0, reduction='mean'),
                  rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.), test_cfg=test_cfg).eval()


def test_restorer_evaluates_on_the_device_when_asked(dev):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.coords import make_cell, make_coord
    from ciaosr_amd.init_utils import seeded_init_, synthetic_pair
    scale = 2
    lq, gt = synthetic_pair(48, 48, scale)
    h, w = gt.shape[-2:]
    gt_q3 = gt[0].permute(1, 2, 0).reshape(1, h * w, 3).contiguous()
    coord, cell = make_coord((h, w)).unsqueeze(0), make_cell((h, w)).unsqueeze(0)
    res = {}
    for on in (False, True):
        cfg = dict(scale=scale, metrics=['PSNR', 'SSIM'], crop_border=2, convert_to='y')
        if on:
            cfg['gpu_metrics'] = True
        model = _edsr_restorer(scale, cfg)
        seeded_init_(model, seed=11, gain=1.25, head_gain=2.0)
        model = model.to(dev)
        with hip_ops.profile():
            res[on] = model(lq=lq.to(dev), gt=gt_q3.to(dev), test_mode=True, coord=coord.to(dev), cell=cell.to(dev))['eval_result']
        assert ('psnr_ssim_u8' in hip_ops.profile.results()) is on
    print('restorer host', res[False], 'device', res[True])
    assert list(res[True]) == list(res[False]) == ['PSNR', 'SSIM']
    assert all(type(v) is float for v in res[True].values())
    assert abs(res[True]['PSNR'] - res[False]['PSNR']) <= PSNR_TOL_DB and abs(res[True]['SSIM'] - res[False]['SSIM']) <= SSIM_TOL
    # a GT that arrives on the host is moved; an output on the host is refused
    from ciaosr_amd._lib import CiaoSRHipError
    out = torch.rand(1, 3, 40, 40)
    got = model.evaluate(out.to(dev), gt[..., :40, :40])
    assert list(got) == ['PSNR', 'SSIM']
    with pytest.raises(CiaoSRHipError):
        model.evaluate(out, gt[..., :40, :40].to(dev))
    model.test_cfg['metrics'] = ['PSNR', 'NIQE']
    with pytest.raises(KeyError):
        model.evaluate(out.to(dev), gt[..., :40, :40].to(dev))


# ---- 11: tools/test.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('val_scale', [4, 6])
def test_cli_gpu_metrics_same_results_and_same_pngs(dev, tmp_path, capsys, val_scale):
    """RDN config, x4 from LQ + GT folders and x6 from a GT-only folder, with and without --gpu-metrics: per-image results within
    the tolerances, saved PNGs identical."""
    import ciaosr_amd
    import tools.test as cli
    from ciaosr_amd import metrics
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_u8, imwrite
    from ciaosr_amd.init_utils import seeded_init_, synthetic_gt
    (tmp_path / 'gt').mkdir()
    (tmp_path / 'lq').mkdir()
    sizes = [(19, 23), (13, 30), (25, 17)]                       # LR sizes; not multiples of the tile
    for i, (h, w) in enumerate(sizes):
        if val_scale == 4:
            gt = synthetic_gt(4 * h, 4 * w, seed=300 + i)
            lq = torch.nn.functional.interpolate(gt, size=(h, w), mode='bicubic', antialias=True, align_corners=False).clamp(0, 1)
            imwrite(metrics.tensor2img(lq), str(tmp_path / 'lq' / f'img{i}.png'))
        else:
            gt = synthetic_gt(6 * h + 1 + i, 6 * w + 2, seed=300 + i)
        imwrite(metrics.tensor2img(gt), str(tmp_path / 'gt' / f'img{i}.png'))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs',
                            '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')).read()
    assert '\nval_scale = 4\n' in src
    cfg_path = tmp_path / 'cfg.py'
    assert 'tile=192, tile_overlap=32' in src
    cfg_path.write_text(src.replace('\nval_scale = 4\n', f'\nval_scale = {val_scale}\n')
                        .replace('tile=192, tile_overlap=32', 'tile=16, tile_overlap=4'))      # several tiles on these small images
    cfg = Config.fromfile(str(cfg_path))
    assert 'gpu_metrics' not in cfg.test_cfg and (cfg.test_cfg.get('tile') == 16) == (val_scale == 4)
    model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=8, gain=1.25, head_gain=2.0)
    torch.save({'state_dict': model.state_dict()}, tmp_path / 'ck.pth')
    folders = ['--gt-folder', str(tmp_path / 'gt')] + (['--lq-folder', str(tmp_path / 'lq')] if val_scale == 4 else [])
    runs = {}
    for tag, extra in (('host', []), ('gpu', ['--gpu-metrics'])):
        runs[tag] = cli.main([str(cfg_path), str(tmp_path / 'ck.pth'), '--save-path', str(tmp_path / tag)] + folders + extra)
        assert 'Eval-PSNR' in capsys.readouterr().out
    assert len(runs['host']) == len(runs['gpu']) == 3
    for i in range(3):
        h, g = runs['host'][i]['eval_result'], runs['gpu'][i]['eval_result']
        print(f'x{val_scale} img{i}: host {h} device {g}')
        assert list(h) == list(g) and all(type(v) is float for v in g.values())
        assert abs(h['PSNR'] - g['PSNR']) <= PSNR_TOL_DB and abs(h['SSIM'] - g['SSIM']) <= SSIM_TOL
        assert np.array_equal(imread_u8(str(tmp_path / 'host' / f'img{i}.png')), imread_u8(str(tmp_path / 'gpu' / f'img{i}.png')))
