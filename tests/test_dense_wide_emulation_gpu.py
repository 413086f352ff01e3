"""The 16-bit wide dense kernel (dense_h16_wide_kernel, csrc/dense_h16.hip: 16 x 32-pixel tiles, one persistent 512-thread workgroup per
CU) against a torch-CPU emulation of the trunk with the mode's rounding points (tests/independent_refs.py::rdn_trunk_16bit_emulation) --
not against the 12 x 12-tile kernels of the same build, whose bound (4e-2 / 6e-3 x scale) is 60 to 400 times looser and could not see
a wrong halo column on a ragged tile edge, a mis-addressed `lo` fragment or a swizzle error at a few pixel indices.

Sizes: (150, 170) ragged both ways, (192, 192) whole tiles, (24, 1040) a strip whose second tile row is half empty, (129, 257)
one-pixel remainders on both axes; each has at least 32 tiles of 16 x 32 pixels (asserted), from where the wide kernel runs whatever
`dense_min_tiles` says.  Modes: both weight forms (hi alone, hi + lo) in both element types.

Bounds.  One block of one layer: the project's bounds for this emulation (test_rdn_trunk_bf16_dense_layers), max 1e-4 x scale and mean
2e-6 x scale.  Deeper trunks (1 x 4, 2 x 8: several input groups, so the per-tile stage rotation matters): both sides round nearly equal
fp32 activations to 16 bits, the rare value that lands on the other side of a rounding boundary propagates with depth, and no absolute
bound separates that from a bug -- so the 12 x 12 kernels, which this emulation already pins on small maps, run on the same input as
the yardstick: the wide kernel's max distance to the emulation must be at most 1.5 x theirs + 1e-6 x scale, its mean distance at most
1.3 x theirs (the form of the existing `rms_new < 1.3 rms_old`).

Measured on an MI355X (in units of the feature scale, about 2): one layer, wide max f16 3.6e-5 .. 4.2e-5, f16-pairs 1.2e-5 .. 1.4e-5,
bf16 and bf16-single 4.8e-5 .. 7.7e-5, mean 1.6e-7 .. 9e-7 -- the 12 x 12 kernels within 3 % of each figure; only the batch of seven
in bf16 needed the measured max bound the 12 x 12 kernels set (BATCH_FLIP_MAX below).  Deeper trunks: wide max / 12 x 12 max 0.82 .. 1.17, mean ratio 1.00 .. 1.06 (absolute: 2 x 8 bf16 max 5.4e-4 .. 5.7e-4 on
both routes).  All four modes matched the emulation; no kernel change was needed.

Both cuts carry the profile tag `enc_dense_<type>`; that both really ran shows in their results not being bitwise equal.
That the emulation is sharp (one dropped halo column of one tap moves it by far more than the bound) is test_reference_sharpness.py's.
What the deeper-trunk yardstick (HIP against HIP) cannot bound -- layer 7 of a block, the `lo` fragments, the f16 fusion epilogue, the
second image of a batch slice -- test_trunk_h16_exact_gpu.py holds bitwise to a float64 answer on exact-arithmetic fixtures."""
import pytest
import torch

from tests import independent_refs as refs
from tests.helpers import randn
from tests.test_hip_parity import _restorer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _trunk(dev, blocks, layers):
    from ciaosr_amd.init_utils import seeded_init_
    model = _restorer('rdn', 4, dev, dict(scale=4), blocks=blocks, layers=layers)
    seeded_init_(model, seed=23, gain=1.6)
    params = {k[len('generator.'):]: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    return model.to(dev).generator._encoder_hip, params


def _emulate(x_chw, params, blocks, layers, mode):
    with torch.no_grad():
        return refs.rdn_trunk_16bit_emulation(x_chw.unsqueeze(0), params, blocks, layers, mode)[0].permute(1, 2, 0).contiguous()     # [H][W][C]


def _dist(got_hwc, want_hwc):
    """(max, mean, where) of |got - want|; where = the worst pixel, its position in the 16 x 32 tile and its channel."""
    d = (got_hwc - want_hwc).abs()
    i = int(d.argmax())
    W, C = d.shape[1], d.shape[2]
    y, rem = divmod(i, W * C)
    x, c = divmod(rem, C)
    return d.max().item(), d.mean().item(), f'pixel ({y}, {x}) = tile position ({y % 16}, {x % 32}), channel {c}'


def _routes(enc, x_chw, mode):
    """(wide result, 12 x 12 result) [H][W][C] on the CPU, with the tag of the 16-bit dense layers asserted for both."""
    from ciaosr_amd import hip_ops
    half = 'bf16' if mode.startswith('bf16') else 'f16'
    out = []
    for direct in (0, 1):
        with hip_ops.profile():
            f = enc.forward_hwc(x_chw, hip_ops.Options(mode, dense_min_tiles=1, dense_direct=direct)).cpu()
        assert f'enc_dense_{half}' in hip_ops.profile.results(), sorted(hip_ops.profile.results())
        out.append(f)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    assert not torch.equal(out[0], out[1]), 'the two cuts sum in different orders: bitwise equality means one of them did not run'
    return out


@pytest.mark.parametrize('mode', refs.WIDE_MODES)
@pytest.mark.parametrize('hw', refs.WIDE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_wide_kernel_one_layer_vs_emulation(dev, hw, mode):
    """One block of one layer: max 1e-4 x scale, mean 2e-6 x scale against the emulation, for the wide kernel and (same bound, same
    input) for the 12 x 12 kernels."""
    assert refs.wide_tiles(hw) >= 32
    enc, params = _trunk(dev, 1, 1)
    x = randn((3,) + hw, 78) * 0.3
    want = _emulate(x, params, 1, 1, mode)
    scale = want.abs().max().item()
    wide, old = _routes(enc, x.to(dev), mode)
    (mw, aw, ww), (mo, ao, wo) = _dist(wide, want), _dist(old, want)
    print(f'dense {mode} {hw} 1x1: wide vs emulation max {mw:.3e} mean {aw:.3e} at {ww}; 12x12 max {mo:.3e} mean {ao:.3e} '
          f'(bounds max {1e-4 * scale:.3e} mean {2e-6 * scale:.3e}; scale {scale:.3f})')
    assert mw < 1e-4 * scale and aw < 2e-6 * scale, (mw, aw, scale, ww)
    assert mo < 1e-4 * scale and ao < 2e-6 * scale, (mo, ao, scale, wo)


@pytest.mark.parametrize('mode', refs.WIDE_MODES)
@pytest.mark.parametrize('blocks,layers', [(1, 4), (2, 8)])
@pytest.mark.parametrize('hw', refs.WIDE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_wide_kernel_deeper_trunks_vs_emulation(dev, hw, blocks, layers, mode):
    """1 x 4 and 2 x 8 layers: the wide kernel is no further from the emulation than the 12 x 12 kernels are on the same input
    (max <= 1.5 x theirs + 1e-6 x scale, mean <= 1.3 x theirs)."""
    assert refs.wide_tiles(hw) >= 32
    enc, params = _trunk(dev, blocks, layers)
    x = randn((3,) + hw, 78) * 0.3
    want = _emulate(x, params, blocks, layers, mode)
    scale = want.abs().max().item()
    wide, old = _routes(enc, x.to(dev), mode)
    (mw, aw, ww), (mo, ao, _) = _dist(wide, want), _dist(old, want)
    print(f'dense {mode} {hw} {blocks}x{layers}: wide vs emulation max {mw:.3e} (bound {1.5 * mo + 1e-6 * scale:.3e}) mean {aw:.3e} '
          f'(bound {1.3 * ao:.3e}) at {ww}; 12x12 max {mo:.3e} mean {ao:.3e} (scale {scale:.3f})')
    assert mw <= 1.5 * mo + 1e-6 * scale, (mw, mo, scale, ww)
    assert aw <= 1.3 * ao, (aw, ao, ww)


# Max bound of the batch test in units of the feature scale.  Seven maps of 25 000 to 37 000 pixels are 11 to 17 million rounded layer
# inputs per case, and in bf16 (1 ulp = 0.4 %) one of them now and then lands on the other side of a rounding boundary than the
# emulation's (the fp32 sfe2 outputs of the two sides differ by ~1e-6): the 12 x 12 kernels, the reference route, measured
# 2.021e-4 at scale 1.590 = 1.271e-4 x scale on (150, 170) image 0 and 1.003e-4 .. 1.060e-4 x scale on three images of (24, 1040) --
# each time ONE element of 1.6 million past 1e-4 x scale, the same pixel and channel to four digits in the wide kernel's result, the mean
# ten times below its bound.  So the bf16 bound is 1.5 x that measured distance, for both routes; f16 (three more mantissa bits) stays at 1e-4.
BATCH_FLIP_MAX = {'bf16': 1.5 * 1.271e-4, 'f16': 1e-4}


@pytest.mark.parametrize('mode', refs.WIDE_MODES)
@pytest.mark.parametrize('hw', refs.WIDE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_wide_kernel_batch_of_seven_vs_emulation(dev, hw, mode):
    """Seven different images through one batched call, each against its own emulation: mean 2e-6 x scale, max 1e-4 x scale (bf16:
    BATCH_FLIP_MAX x scale, see there) for the wide kernel and for the 12 x 12 kernels on the same batch, and the wide kernel's max at
    most 1.5 x theirs + 1e-6 x scale.  A launch of seven takes the 16 x 32-pixel tile shape (R = 2) where one image takes 8 x 32 -- at
    every size here but the strip, whose 33 tile columns keep the batch on 8 x 32 too; there the test still walks persistent
    workgroups over several images."""
    from ciaosr_amd import hip_ops
    assert refs.wide_tiles(hw) >= 32
    enc, params = _trunk(dev, 1, 1)
    xs = torch.stack([randn((3,) + hw, 100 + i) * (0.2 + 0.05 * i) for i in range(7)])
    got = enc.forward_hwc_batch(xs.to(dev), hip_ops.Options(mode, dense_min_tiles=1)).cpu()
    old = enc.forward_hwc_batch(xs.to(dev), hip_ops.Options(mode, dense_min_tiles=1, dense_direct=1)).cpu()
    assert not torch.equal(got, old), 'the two cuts sum in different orders: bitwise equality means one of them did not run'
    flips = BATCH_FLIP_MAX['bf16' if mode.startswith('bf16') else 'f16']
    bad = []
    for i in range(7):
        want = _emulate(xs[i], params, 1, 1, mode)
        scale = want.abs().max().item()
        (m, a, where), (mo, ao, wo) = _dist(got[i], want), _dist(old[i], want)
        n, no = int(((got[i] - want).abs() > 1e-4 * scale).sum()), int(((old[i] - want).abs() > 1e-4 * scale).sum())
        bound = max(1e-4, flips) * scale
        print(f'dense {mode} {hw} batch image {i}: wide max {m:.3e} (bound {bound:.3e}; {n} of {want.numel()} elements past 1e-4 x scale) '
              f'mean {a:.3e} (bound {2e-6 * scale:.3e}) at {where}; 12x12 max {mo:.3e} ({no} past 1e-4 x scale) mean {ao:.3e} at {wo}')
        if not (torch.isfinite(got[i]).all() and a < 2e-6 * scale and ao < 2e-6 * scale and mo < bound and m < bound and
                m <= 1.5 * mo + 1e-6 * scale):
            bad.append((i, m, a, mo, ao, scale, where, wo))
    assert not bad, bad
