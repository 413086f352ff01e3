"""GPU tests of the GT -> LR degradation: ciaosr_resample_u8 against Pillow (bitwise), the GT-only test dataset on the device, and
tools/test.py on a GT-only config at x6 and x12 against the CPU oracle's pipeline.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import os

import numpy as np
import pytest
import torch

from tests.test_degrade_host import grid_cases, grid_image, pil_resize, valid_pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _div255(u8):
    """RescaleToZeroOne: numpy's float32 division."""
    return np.asarray(u8, dtype=np.float32) / np.float32(255.0)


def _check(img_dev, img_np, w_out, h_out):
    from ciaosr_amd.degrade import resample_u8
    u8, chw = resample_u8(img_dev, (w_out, h_out), want_u8=True, want_chw=True)
    want = pil_resize(img_np, w_out, h_out)
    got = u8.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    assert chw.shape == (3, h_out, w_out)
    assert np.array_equal(chw.cpu().numpy(), _div255(got).transpose(2, 0, 1))
    # either output alone gives the same bytes
    only_chw = resample_u8(img_dev, (w_out, h_out), want_u8=False, want_chw=True)[1]
    assert torch.equal(only_chw, chw)


def test_resample_grid_equals_pillow(dev):
    for case in grid_cases():
        h, w, w_out, h_out, kind = case
        img = grid_image(h, w, kind, seed=h * 1000 + w + w_out)
        _check(torch.from_numpy(img).to(dev), img, w_out, h_out)


@pytest.mark.parametrize('scale', [4, 12, 30])
def test_resample_div2k_size_equals_pillow(dev, scale):
    from ciaosr_amd.degrade import down_size, resize_bicubic_u8
    img = grid_image(1356, 2040, 'random', seed=scale)
    img[::3] = grid_image(1356, 2040, 'smooth', 0)[::3]
    h_lr, w_lr, hc, wc = down_size(1356, 2040, scale)
    crop = np.ascontiguousarray(img[:hc, :wc])
    _check(torch.from_numpy(crop).to(dev), crop, w_lr, h_lr)
    got = resize_bicubic_u8(torch.from_numpy(crop).to(dev), (w_lr, h_lr))
    assert np.array_equal(got.cpu().numpy(), pil_resize(crop, w_lr, h_lr))


@pytest.mark.parametrize('x0', [0, 1, 5])
def test_resample_crop_passed_with_pitch(dev, x0):
    """A crop of a wider image reaches the kernel through its row pitch, at any byte alignment, and reads nothing outside it."""
    img = grid_image(131, 257, 'random', seed=7)
    full = torch.from_numpy(img).to(dev)
    view = full[3:3 + 100, x0:x0 + 233, :]
    assert view.stride(0) == 257 * 3 and not view.is_contiguous()
    crop = np.ascontiguousarray(img[3:103, x0:x0 + 233])
    for w_out, h_out in [(19, 8), (233, 33), (29, 100), (1, 1)]:
        _check(view, crop, w_out, h_out)


def test_resample_refuses_cpu_and_bad_layouts(dev):
    from ciaosr_amd._lib import CiaoSRHipError
    from ciaosr_amd.degrade import resize_bicubic_u8
    img = torch.zeros(20, 30, 3, dtype=torch.uint8)
    with pytest.raises(CiaoSRHipError, match='no CPU fallback'):
        resize_bicubic_u8(img, (10, 5))
    with pytest.raises(CiaoSRHipError, match='uint8'):
        resize_bicubic_u8(img.to(dev).float(), (10, 5))
    with pytest.raises(CiaoSRHipError, match='HWC'):
        resize_bicubic_u8(img.to(dev).permute(1, 0, 2), (10, 5))


@pytest.mark.parametrize('scale', [6, 12])
def test_gt_dataset_on_device_equals_pillow_pipeline(dev, tmp_path, scale):
    from PIL import Image
    from ciaosr_amd.coords import make_cell, make_coord
    from ciaosr_amd.dataset import SRFolderGTDataset
    from ciaosr_amd.degrade import down_size
    imgs = [grid_image(76, 100, 'smooth', 0), grid_image(81, 64, 'random', 1)]
    for i, img in enumerate(imgs):
        Image.fromarray(img).save(tmp_path / f'img{i}.png')
    ds = SRFolderGTDataset(tmp_path, valid_pipeline(scale), scale=scale, device=dev)
    assert len(ds) == 2
    for i, img in enumerate(imgs):
        d = ds[i]
        h_lr, w_lr, hc, wc = down_size(img.shape[0], img.shape[1], scale)
        crop = img[:hc, :wc]
        for k in ('lq', 'gt', 'coord', 'cell'):
            assert d[k].device == dev and d[k].dtype == torch.float32, k
        assert np.array_equal(d['lq'].cpu().numpy(), _div255(pil_resize(np.ascontiguousarray(crop), w_lr, h_lr)).transpose(2, 0, 1))
        assert np.array_equal(d['gt'].cpu().numpy(), _div255(crop).reshape(hc * wc, 3))
        assert torch.equal(d['coord'].cpu(), make_coord((hc, wc))) and torch.equal(d['cell'].cpu(), make_cell((hc, wc)))
        assert d['meta']['gt_path'].endswith(f'img{i}.png')


@pytest.mark.parametrize('val_scale', [6, 12])
def test_tools_test_cli_gt_only_config(dev, tmp_path, capsys, val_scale):
    """tools/test.py CONFIG CHECKPOINT on a folder of GT PNGs with a GT-only data.test: Eval-PSNR within 0.01 dB of the CPU
    oracle's pipeline (Pillow down-sampling -> oracle forward_test without tiles -> Y-channel PSNR with crop_border)."""
    import tools.test as cli
    from PIL import Image
    import ciaosr_amd
    from ciaosr_amd import metrics
    from ciaosr_amd.config import Config
    from ciaosr_amd.coords import make_cell, make_coord
    from ciaosr_amd.degrade import down_size
    from ciaosr_amd.imageio import imread_u8, imwrite
    from ciaosr_amd.init_utils import seeded_init_, synthetic_gt
    from oracle import ciaosr_oracle as orc
    (tmp_path / 'gt').mkdir()
    for i, (h, w) in enumerate([(76, 100), (81, 64)]):
        imwrite(metrics.tensor2img(synthetic_gt(h, w, seed=200 + i)), str(tmp_path / 'gt' / f'img{i}.png'))
    cfg_path = tmp_path / 'cfg.py'
    cfg_path.write_text(
        "from mmedited.models.restorers.ciaosr import CiaoSR\n"
        "from mmedited.models.backbones.sr_backbones.ciaosr_net import LocalImplicitSREDSR\n"
        f"val_scale = {val_scale}\n"
        "mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[256, 256, 256, 256])\n"
        "model = dict(type=CiaoSR, generator=dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3,"
        " out_channels=3, mid_channels=64, num_blocks=4), imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64),"
        " feat_unfold=True, eval_bsize=30000), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),"
        " pixel_loss=dict(type='L1Loss', loss_weight=1.0, reduction='mean'))\n"
        "test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=val_scale, scale=val_scale, convert_to='y')\n"
        f"valid_pipeline = {valid_pipeline(val_scale)!r}\n"
        f"data = dict(test=dict(type='SRFolderGTDataset', gt_folder={str(tmp_path / 'gt')!r}, pipeline=valid_pipeline,"
        " scale=val_scale))\n"
        "dist_params = dict(backend='nccl')\n")
    cfg = Config.fromfile(str(cfg_path))
    model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=8, gain=1.25, head_gain=2.0)
    torch.save({'state_dict': model.state_dict()}, tmp_path / 'ck.pth')
    with pytest.raises(SystemExit, match='LQ folder'):
        cli.main([str(cfg_path), str(tmp_path / 'ck.pth'), '--lq-folder', str(tmp_path / 'gt')])
    results = cli.main([str(cfg_path), str(tmp_path / 'ck.pth'), '--save-path', str(tmp_path / 'out')])
    printed = capsys.readouterr().out
    assert 'Eval-PSNR' in printed and 'Eval-SSIM' in printed
    assert len(results) == 2
    P = {k[len('generator.'):]: v.detach().cpu() for k, v in model.state_dict().items()}
    for i in range(2):
        gt_u8 = imread_u8(str(tmp_path / 'gt' / f'img{i}.png'))
        h_lr, w_lr, hc, wc = down_size(gt_u8.shape[0], gt_u8.shape[1], val_scale)
        crop = np.ascontiguousarray(gt_u8[:hc, :wc])
        assert os.path.exists(tmp_path / 'out' / f'img{i}.png')
        assert Image.open(tmp_path / 'out' / f'img{i}.png').size == (wc, hc)
        lq = torch.from_numpy(_div255(pil_resize(crop, w_lr, h_lr))).permute(2, 0, 1).unsqueeze(0).contiguous()
        want = orc.forward_test(lq, make_coord((hc, wc)).unsqueeze(0), make_cell((hc, wc)).unsqueeze(0), P)
        gt = torch.from_numpy(_div255(crop)).permute(2, 0, 1).unsqueeze(0)
        ref_psnr = metrics.psnr(metrics.tensor2img(want), metrics.tensor2img(gt), crop_border=val_scale, convert_to='y')
        assert abs(results[i]['eval_result']['PSNR'] - ref_psnr) <= 0.01, (results[i]['eval_result'], ref_psnr)
