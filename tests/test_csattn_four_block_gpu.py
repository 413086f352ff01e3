"""GPU tests of the four-block attn.V route of cs_attn's composed tail (csa_attn_v4_f32.hip): the fp32 contraction over the four diagonal
tap blocks of csa_down_partial (K = 4 (Hp/2+3)(Wp/2+3)) instead of the 16 offset columns (K = L, N = 16C), with the row-0 / column-0
edge rule subtracted afterwards.  The 16C route stays reachable with Options(csa_attn_v16=1) and is the reference route here."""
import numpy as np
import pytest
import torch

from tests.helpers import SQRT6, load_golden, randn
from tests.test_hip_parity import TOL, _csattn_golden, _restorer, _tile192_checks

pytestmark = pytest.mark.gpu

ROUTE_TAGS = ('csa_gather_vedge', 'csa_attn_v', 'csa_attn_v_edge', 'csa_gather_out')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.mark.parametrize('tag,composed_min', [('64x64', 0), ('67x70', 0), ('48', 1), ('45x51', 1)])
def test_four_block_route_engages_and_matches_the_reference(dev, tag, composed_min):
    """The four csattn_c64 reference vectors (the two small ones with the composed tail forced on): the route runs and stays within TOL;
    45x51 and 67x70 are reflect-padded on one or both axes, so the edge rule is checked on even and padded maps."""
    from ciaosr_amd import hip_ops
    att, x, want = _csattn_golden(tag, dev)
    with hip_ops.profile():
        y = att(x, options=hip_ops.Options(csa_composed_min=composed_min)).cpu()
    prof = hip_ops.profile.results()
    for t in ROUTE_TAGS:
        assert t in prof, (t, sorted(prof))
    assert 'csa_gather_vprime' not in prof, sorted(prof)
    err = (y[0] - want).abs().max().item()
    print(f'cs_attn {tag} four-block route: max|hip - reference| = {err:.3e} (out scale {want.abs().max().item():.3f})')
    assert err < TOL


def _att(dev, channel, hw, seed=91):
    from ciaosr_amd.nonlocal_attn import CrossScaleAttention
    torch.manual_seed(5)
    att = CrossScaleAttention(channel=channel, scale=2).to(dev)
    x = (randn((1, channel) + hw, seed) * 0.5).to(dev)
    return att, x


@pytest.mark.parametrize('hw', [(192, 192), (190, 187)])
def test_four_block_route_against_the_16c_route(dev, hw):
    """A C3 tile's size and a reflect-padded one: the four-block route against the 16C route within 2e-5 x the output scale."""
    from ciaosr_amd import hip_ops
    att, x = _att(dev, 64, hw)
    with hip_ops.profile():
        y4 = att(x).clone()
    assert 'csa_gather_vedge' in hip_ops.profile.results()
    with hip_ops.profile():
        y16 = att(x, options=hip_ops.Options(csa_attn_v16=1)).clone()
    prof16 = hip_ops.profile.results()
    assert 'csa_gather_vprime' in prof16 and 'csa_gather_vedge' not in prof16, sorted(prof16)
    scale = y16.abs().max().item()
    err = (y4 - y16).abs().max().item()
    print(f'{hw}: max|four-block - 16C| = {err:.3e} at output scale {scale:.3f}')
    assert torch.isfinite(y4).all() and err <= 2e-5 * scale


@pytest.mark.parametrize('hw', [(192, 192), (190, 187)])
def test_four_block_tile_widths_are_bitwise_equal(dev, hw):
    """Items of one query row (default) and of half a row (csa_attn_tile128 = 1) sum every output in the same order: bitwise equal, also
    with every scratch byte poisoned first."""
    from ciaosr_amd import hip_ops
    att, x = _att(dev, 64, hw)
    with hip_ops.profile():
        big = att(x).clone()
    assert 'csa_gather_vedge' in hip_ops.profile.results()
    small = att(x, options=hip_ops.Options(csa_attn_tile128=1)).clone()
    assert torch.isfinite(big).all() and torch.equal(big, small), (big - small).abs().max().item()
    hip_ops.poison_workspaces()
    assert torch.equal(att(x), big)
    hip_ops.poison_workspaces()
    assert torch.equal(att(x, options=hip_ops.Options(csa_attn_tile128=1)), big)


def test_c180_keeps_the_16c_route(dev):
    from ciaosr_amd import hip_ops
    att, x = _att(dev, 180, (96, 96))
    with hip_ops.profile():
        y = att(x)
    prof = hip_ops.profile.results()
    assert torch.isfinite(y).all()
    assert 'csa_gather_vprime' in prof and 'csa_gather_vedge' not in prof, sorted(prof)


def test_full_c3_tile_fp32_with_the_four_block_route(dev):
    """One full C3 tile in fp32 (the route at its flagship size) against the reference's stored pixels."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import seeded_init_, synthetic_pair
    fx = load_golden('e2e_rdn_x4_tile192')
    model = _restorer('rdn', 4, dev, dict(scale=4, tile=192, tile_overlap=32))
    assert seeded_init_(model, seed=int(fx['weight_seed']), gain=float(fx['gain']), head_gain=SQRT6) == str(fx['sha'])
    model = model.to(dev)
    lq, _ = synthetic_pair(192, 192, 4)
    with hip_ops.profile():
        out = model.restore(lq.to(dev), options=hip_ops.Options('fp32')).cpu()
    prof = hip_ops.profile.results()
    for t in ROUTE_TAGS:
        assert t in prof, (t, sorted(prof))
    errs = _tile192_checks(out, fx, None)
    ref_s4 = torch.from_numpy(np.asarray(fx['out_s4']))
    rms = (out[..., ::4, ::4] - ref_s4).double().pow(2).mean().sqrt().item()
    print(f'C3 tile fp32, four-block attn.V: max|d| {errs}, rms {rms:.3e}')
    assert max(errs.values()) <= 1e-5 and rms < 1e-5, (errs, rms)
