"""The opt-in SwinIR trunk with f16 linears (Options.swin_h16 -> ciaosr_swinir_forward_batch_f16, csrc/swinir_h16.hip) on the GPU, through
the C ABI: against the PyTorch checker with an error budget taken from the CPU emulation of tests/test_swinir_h16_host.py, batch
independence, the 0.01 dB gate on the swinir_c5_48 fixture, the option off / ignored = the fp32 trunk launch for launch, and batched tiles."""
import math

import pytest
import torch

from tests.helpers import SQRT6, load_golden, randn
from tests.test_swinir_h16_host import GT30_SEED, emulated_features

pytestmark = pytest.mark.gpu

LIGHT = dict(embed_dim=60, depths=[2, 2], num_heads=[6, 6], mlp_ratio=2)      # ld 64, hidden 120 -> 128, head dimension 10
H16 = dict(swin_h16=1)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_cache = {}


def _trunk(dev, kind):
    """The generator of SwinIR-CiaoSR with the shipped trunk (C = 180, 36 blocks) or the light one, seeded_init_(seed=9, gain=1.3) as
    test_swinir_trunk_hip_vs_torch; built once per module."""
    if ('trunk', kind) not in _cache:
        from ciaosr_amd import CiaoSR, LocalImplicitSRSWINIR
        from ciaosr_amd.encoders import SwinIR
        from ciaosr_amd.init_utils import seeded_init_
        enc = dict(type=SwinIR, upscale=4, in_chans=3, img_size=48, window_size=8, img_range=1., depths=[6] * 6, embed_dim=180,
                   num_heads=[6] * 6, mlp_ratio=2, upsampler='pixelshuffle', resi_connection='1conv')
        if kind == 'light':
            enc.update(LIGHT)
        mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[64, 64])
        gen = dict(type=LocalImplicitSRSWINIR, window_size=8, encoder=enc, imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64),
                   feat_unfold=True, eval_bsize=30000)
        model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                       test_cfg=dict(scale=4)).eval()
        seeded_init_(model, seed=9, gain=1.3)
        g = model.generator.to(dev).eval()
        assert g._encoder_hip.supported()
        _cache[('trunk', kind)] = g
    return _cache[('trunk', kind)]


def _c5_model(dev):
    """SwinIR-CiaoSR with the swinir_c5_48 fixture's weights, built once per module; tests set and restore its test_cfg."""
    if 'c5' not in _cache:
        from ciaosr_amd.init_utils import seeded_init_
        from tests.test_host_logic import _swinir_ciaosr
        fx = load_golden('swinir_c5_48')
        model = _swinir_ciaosr(dict(scale=3.3))
        assert seeded_init_(model, seed=int(fx['weight_seed']), gain=float(fx['gain']), head_gain=SQRT6) == str(fx['sha'])
        _cache['c5'] = (model.to(dev), fx)
    return _cache['c5']


def _c5_run(dev, precision, hip_options):
    """(output image on the CPU, profile) of the fixture's forward_test under test_cfg.precision / test_cfg.hip_options."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.coords import make_coord, make_cell
    model, fx = _c5_model(dev)
    ht, wt = [int(v) for v in fx['target']]
    coord, cell = make_coord((ht, wt)).unsqueeze(0).to(dev), make_cell((ht, wt)).unsqueeze(0).to(dev)
    keep = dict(model.test_cfg)
    model.test_cfg['precision'] = precision
    if hip_options:
        model.test_cfg['hip_options'] = dict(hip_options)
    try:
        with hip_ops.profile():
            out = model(lq=torch.from_numpy(fx['lq']).to(dev), gt=None, test_mode=True, coord=coord, cell=cell)['output']
        prof = hip_ops.profile.results()
    finally:
        model.test_cfg.clear()
        model.test_cfg.update(keep)
    return out.cpu(), prof


@pytest.mark.parametrize('hw', [(48, 48), (45, 51), (8, 20)])
@pytest.mark.parametrize('kind', ['shipped', 'light'])
def test_trunk_vs_checker(dev, kind, hw):
    """ciaosr_swinir_forward_batch_f16 (B = 1) against the PyTorch trunk: maps that need reflect padding and a single window row.
    Bound = the fp32 trunk's own, 2e-4 * max(scale, 1), + twice the max abs error of the CPU emulation (operands of the four linears
    rounded to half, fp64 accumulation) on the same weights and input."""
    from ciaosr_amd import hip_ops
    gen = _trunk(dev, kind)
    x = (randn((1, 3) + hw, 91) * 0.3).to(dev)
    want, emu = emulated_features(gen, x)
    opt = hip_ops.Options('f16', **H16)
    with hip_ops.profile():
        got = gen.gen_feature(x, opt)[0]
    prof = hip_ops.profile.results()
    scale = want.abs().max().item()
    t_fp32, t_emu = 2e-4 * max(scale, 1.0), 2 * (emu - want).abs().max().item()
    err = (got - want).abs().max().item()
    print(f'swinir h16 trunk {kind} {hw}: max|d| {err:.3e} (scale {scale:.3f}); bound {t_fp32:.3e} (fp32 trunk) + {t_emu:.3e} (2 x emulation)')
    assert 'swin_qkv_f16' in prof and 'swin_window_attention' in prof, sorted(prof)
    n_blocks = sum(len(l.residual_group.blocks) for l in gen.layers)
    assert all(prof[k]['launches'] == n_blocks for k in ('swin_qkv_f16', 'swin_proj_f16', 'swin_fc1_f16', 'swin_fc2_f16', 'swin_window_attention'))
    assert prof['swin_layernorm']['launches'] <= 2 and 'swin_qkv' not in prof and 'swin_fc1' not in prof
    assert torch.isfinite(got).all()
    assert err < t_fp32 + t_emu, (err, t_fp32, t_emu)


@pytest.mark.parametrize('shape', [(3, 16, 24), (2, 45, 51)])
@pytest.mark.parametrize('kind', ['shipped', 'light'])
def test_batch_is_bitwise_the_single_images(dev, kind, shape):
    """Image b of a batch is torch.equal to the B = 1 call: no window, mask or token index bleeds across images and no tiling depends
    on the number of rows."""
    from ciaosr_amd import hip_ops
    gen = _trunk(dev, kind)
    enc = gen._encoder_hip
    opt = hip_ops.Options('f16', **H16)
    x = (randn((shape[0], 3) + shape[1:], 17) * 0.3).to(dev)
    with hip_ops.profile():
        got = enc.forward_hwc_batch(x, opt)
    prof = hip_ops.profile.results()
    n_blocks = sum(len(l.residual_group.blocks) for l in gen.layers)
    assert prof['swin_qkv_f16']['launches'] == n_blocks and prof['swin_layernorm']['launches'] == 2     # shared by the images
    assert got.shape == (shape[0],) + shape[1:] + (enc.struct().embed_dim,)
    singles = [enc.forward_hwc(x[b], opt) for b in range(shape[0])]
    for b in range(shape[0]):
        assert torch.equal(got[b], singles[b]), (kind, shape, b, (got[b] - singles[b]).abs().max().item())
    assert not torch.equal(singles[0], singles[1])
    # the fp32 trunk of the same images is another result (the option really changes what runs) and close
    f32 = enc.forward_hwc(x[0], hip_ops.Options('f16'))
    d = (f32 - singles[0]).abs().max().item()
    assert 0 < d < 1e-2 * max(f32.abs().max().item(), 1.0)


def test_c5_48_meets_the_psnr_gate_with_the_option(dev):
    """swinir_c5_48 with precision='f16', hip_options=dict(swin_h16=1): |PSNR(out, GT) - PSNR(ref, GT)| <= 0.01 dB at the fixture's own
    level and against GT' = reference + 30 dB noise; the f16 head and the f16-linear trunk both ran."""
    from ciaosr_amd.init_utils import synthetic_pair
    from ciaosr_amd.metrics import psnr_tensors
    out, prof = _c5_run(dev, 'f16', H16)
    _, fx = _c5_model(dev)
    assert 'head_kv_chain_f16' in prof and 'swin_fc1_f16' in prof and 'swin_qkv' not in prof
    ref = torch.from_numpy(fx['out'])
    err = (out - ref).abs().max().item()
    rms = (out - ref).double().pow(2).mean().sqrt().item()
    _, gt = synthetic_pair(48, 48, 3.3)
    psnr_ref = psnr_tensors(ref, gt, crop_border=3)
    assert abs(psnr_ref - float(fx['psnr_ref_gt'])) < 1e-6
    d_psnr = abs(psnr_tensors(out, gt, crop_border=3) - psnr_ref)
    gt30 = ref.double() + torch.randn(ref.shape, generator=torch.Generator().manual_seed(GT30_SEED), dtype=torch.float64) * 10 ** (-30 / 20)
    psnr30 = lambda a: -10 * math.log10((a.double() - gt30).pow(2).mean().item())
    d_psnr30 = abs(psnr30(out) - psnr30(ref))
    print(f'C5 48x48 f16 + swin_h16: max|d| {err:.3e}, rms {rms:.3e}, PSNR delta vs GT {d_psnr:.5f} dB, at 30 dB {d_psnr30:.5f} dB')
    assert torch.isfinite(out).all()
    assert d_psnr <= 0.01, d_psnr
    assert d_psnr30 <= 0.01, d_psnr30


@pytest.mark.parametrize('precision,hip_options', [('f16', None), ('f16x3', H16), ('bf16', H16)])
def test_option_off_or_ignored_is_the_fp32_trunk(dev, precision, hip_options):
    """Without the option, and with it in the modes that promise an fp32 trunk ('bf16' runs as 'bf16x3' on this head), no swin_*_f16
    kernel runs and the fp32 trunk's launches are all there: 2 LayerNorms per block + 2, one swin_qkv per block."""
    out, prof = _c5_run(dev, precision, hip_options)
    assert not any(k.startswith('swin_') and k.endswith('_f16') for k in prof), sorted(prof)
    assert prof['swin_layernorm']['launches'] == 2 * 36 + 2 and prof['swin_qkv']['launches'] == 36
    assert all(prof[k]['launches'] == 36 for k in ('swin_window_attention', 'swin_proj', 'swin_fc1', 'swin_fc2'))
    if precision == 'f16':
        out2, _ = _c5_run(dev, 'f16', dict(swin_h16=0))
        assert torch.equal(out, out2)


def test_tiles_in_batches_are_bitwise_the_single_tiles(dev):
    """A 40 x 56 LR image in 6 tiles of 24 (overlap 8) at x2 with the option: tile_batch = 3 with encoder_ahead, tile_batch = 3 without
    and tile_batch = 1 give the same image bit for bit; so does encode + render(scale=2)."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import synthetic_pair
    model, _ = _c5_model(dev)
    lq, _ = synthetic_pair(40, 56, 2)
    lq = lq.to(dev)
    keep = dict(model.test_cfg)
    try:
        model.test_cfg.clear()
        model.test_cfg.update(dict(scale=2, tile=24, tile_overlap=8, precision='f16', hip_options=dict(H16)))
        imgs = {}
        for name, extra in (('ahead', dict(tile_batch=3)), ('batched', dict(tile_batch=3, encoder_ahead=False)), ('single', dict(tile_batch=1))):
            for k in ('tile_batch', 'encoder_ahead'):
                model.test_cfg.pop(k, None)
            model.test_cfg.update(extra)
            with hip_ops.profile():
                imgs[name] = model.restore(lq).cpu()
            prof = hip_ops.profile.results()
            # 6 tiles: two trunk calls of three tiles, or six of one
            assert prof['swin_qkv_f16']['launches'] == 36 * (6 if name == 'single' else 2), (name, prof['swin_qkv_f16'])
            assert 'swin_qkv' not in prof
        assert imgs['ahead'].shape == (1, 3, 80, 112) and torch.isfinite(imgs['ahead']).all()
        assert torch.equal(imgs['ahead'], imgs['batched']) and torch.equal(imgs['batched'], imgs['single'])
        for k in ('tile_batch', 'encoder_ahead'):
            model.test_cfg.pop(k, None)
        enc = model.encode(lq)
        assert torch.equal(model.render(enc, scale=2).cpu(), imgs['single'])
    finally:
        model.test_cfg.clear()
        model.test_cfg.update(keep)
