"""Host-side tests of the opt-in device evaluation (`test_cfg.gpu_metrics`): the switch and its refusal of CPU tensors, the
unchanged default, the CLI flag, and the float64 restatement of PSNR / SSIM that tests/test_metrics_gpu.py uses as second oracle.

Tolerances (shared with the GPU tests): |dPSNR| <= 1e-4 dB and |dSSIM| <= 1e-6.  They come from the spread between two legitimate
evaluation orders of the same formulas -- the committed host functions against the float64 restatement below differ by at most
1.8e-5 dB and 6.8e-8 over the grid of this file (most of the PSNR figure is fp32 carried through `metrics.psnr`) -- times 5 / 15.
"""
import math
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PSNR_TOL_DB = 1e-4
SSIM_TOL = 1e-6

SIZES = [(23, 31), (150, 210), (257, 300), (768, 768)]
CROPS = [0, 2, 4, 6]
SIGMAS = [40.0, 12.0, 3.0, 0.6]
CONVERT = ['y', None]


def image_pair(h, w, sigma, seed=0):
    """Two uint8 [h, w, 3] BGR images: a smooth image and the same plus Gaussian noise of `sigma` grey levels."""
    rng = np.random.RandomState(seed * 7919 + h * 131 + w)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    base = np.stack([127.5 + 60.0 * np.sin(xx / (9.0 + 4 * c) + 0.7 * c) * np.cos(yy / (13.0 - 3 * c)) +
                     35.0 * np.sin((xx + 2 * yy) / (31.0 + 7 * c)) for c in range(3)], axis=-1)
    a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(base + sigma * rng.standard_normal(base.shape)), 0, 255).astype(np.uint8)
    return a, b


def _channels64(img, convert_to):
    """float64 [h, w, C] of a uint8 BGR image: exact-arithmetic Y (C = 1) or the three channels."""
    v = img.astype(np.float64)
    if convert_to == 'y':
        return ((v[..., 0] * 24.966 + v[..., 1] * 128.553 + v[..., 2] * 65.481) / 255.0 + 16.0)[..., None]
    return v


def _crop(x, c):
    return x[c:x.shape[0] - c, c:x.shape[1] - c] if c else x


def psnr64(a, b, crop_border=0, convert_to=None):
    x, y = _crop(_channels64(a, convert_to), crop_border), _crop(_channels64(b, convert_to), crop_border)
    mse = np.mean((x - y) ** 2)
    return float('inf') if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


def ssim64(a, b, crop_border=0, convert_to=None):
    from scipy.signal import correlate2d
    x, y = _crop(_channels64(a, convert_to), crop_border), _crop(_channels64(b, convert_to), crop_border)
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()
    win = np.outer(k, k)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    vals = []
    for ch in range(x.shape[2]):
        p, q = x[..., ch], y[..., ch]
        f = lambda m: correlate2d(m, win, mode='valid')
        mp, mq = f(p), f(q)
        spp, sqq, spq = f(p * p) - mp * mp, f(q * q) - mq * mq, f(p * q) - mp * mq
        m = ((2 * mp * mq + c1) * (2 * spq + c2)) / ((mp * mp + mq * mq + c1) * (spp + sqq + c2))
        vals.append(m.mean())
    return float(np.mean(vals))


def _restorer(test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[16, 16])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=8, num_blocks=1),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    return CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                  test_cfg=test_cfg).eval()


def _tensors(seed=3, h=40, w=52):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(1, 3, h, w, generator=g)
    out = (gt + 0.03 * torch.randn(1, 3, h, w, generator=g)).clamp(-0.1, 1.1)
    return out, gt


def test_gpu_metrics_refuses_cpu_tensors():
    """With the switch on there is no host fallback: CPU tensors raise.  (Without this feature the key is ignored and the host
    computes a result.)"""
    from ciaosr_amd._lib import CiaoSRHipError
    model = _restorer(dict(metrics=['PSNR', 'SSIM'], crop_border=2, convert_to='y', gpu_metrics=True))
    out, gt = _tensors()
    with pytest.raises(CiaoSRHipError):
        model.evaluate(out, gt)
    from ciaosr_amd import metrics_hip
    with pytest.raises(CiaoSRHipError):
        metrics_hip.tensor2img_u8(out)
    u8 = torch.zeros(20, 20, 3, dtype=torch.uint8)
    with pytest.raises(CiaoSRHipError):
        metrics_hip.psnr_ssim_u8(u8, u8)


@pytest.mark.parametrize('extra', [{}, {'gpu_metrics': False}])
@pytest.mark.parametrize('convert', [{'convert_to': 'y'}, {}])
def test_default_evaluate_is_the_host_code(extra, convert):
    from ciaosr_amd import metrics
    model = _restorer(dict(metrics=['PSNR', 'SSIM'], crop_border=2, **convert, **extra))
    out, gt = _tensors()
    res = model.evaluate(out, gt)
    a, b = metrics.tensor2img(out), metrics.tensor2img(gt)
    assert list(res) == ['PSNR', 'SSIM']
    assert res['PSNR'] == metrics.psnr(a, b, 2, convert.get('convert_to'))
    assert res['SSIM'] == metrics.ssim(a, b, 2, convert.get('convert_to'))


@pytest.mark.slow
def test_float64_restatement_agrees_with_the_host_functions():
    """Pins the second oracle: psnr64 / ssim64 against metrics.psnr / metrics.ssim within the tolerances, sizes up to 257x300."""
    from ciaosr_amd import metrics
    worst = [0.0, 0.0]
    for (h, w) in SIZES[:3]:
        for sigma in SIGMAS:
            a, b = image_pair(h, w, sigma)
            for crop in CROPS:
                for conv in CONVERT:
                    dp = abs(metrics.psnr(a, b, crop, conv) - psnr64(a, b, crop, conv))
                    ds = abs(metrics.ssim(a, b, crop, conv) - ssim64(a, b, crop, conv))
                    worst = [max(worst[0], dp), max(worst[1], ds)]
                    assert dp <= PSNR_TOL_DB and ds <= SSIM_TOL, (h, w, sigma, crop, conv, dp, ds)
    print(f'host vs float64 restatement: max |dPSNR| {worst[0]:.3g} dB, max |dSSIM| {worst[1]:.3g}')


def test_cli_flag_reaches_the_models_test_cfg():
    import ciaosr_amd
    import tools.test as cli
    from ciaosr_amd.config import Config
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    for argv, want in ([], False), (['--gpu-metrics'], True):
        args = cli.parse_args([path, 'None'] + argv)
        assert args.gpu_metrics is want
        cfg = cli.apply_overrides(Config.fromfile(path), args)
        model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        assert bool(model.test_cfg.get('gpu_metrics', False)) is want
        assert model.gpu_metrics() is want
