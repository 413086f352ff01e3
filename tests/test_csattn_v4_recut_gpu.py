"""GPU tests of the wave-specialised four-block attn.V kernel (csa_attn_v4_f32.hip): producer waves stage probabilities and build the
A / U tiles of a step of 10 padded key columns while consumer waves run the MFMAs of the step before.  The sizes walk every ragged
path of that schedule: padded key columns (Wp/2 + 3) that are and are not a multiple of the step width, padded key rows (Hp/2 + 3)
that do and do not divide by the four quarters, maps narrower than an item of either width, a second ragged item per row,
reflect-padded (odd) maps, and the C3 tile's 192 x 192.  The 16C route (Options(csa_attn_v16=1)) is the reference route."""
import pytest
import torch

from tests.helpers import randn

pytestmark = pytest.mark.gpu

# (H, W) of the LR map -> padded key grid (Hp/2 + 3) x (Wp/2 + 3)
SIZES = [
    (64, 70),      # 35 x 38: columns not a multiple of 10, rows not divisible by 4, narrower than both items
    (58, 54),      # 32 x 30: columns a multiple of 10, rows divisible by 4
    (48, 40),      # 27 x 23: narrower than half a 96-wide item
    (50, 150),     # 28 x 78: a full and a ragged 96-wide item per row, one ragged 192-wide item
    (45, 51),      # reflect-padded on both axes
    (40, 200),     # 23 x 103: wider than the 192-wide item (a second item of 8 queries)
    (192, 192),    # the C3 tile: 99 x 99
]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _att(dev, hw, seed=91):
    from ciaosr_amd.nonlocal_attn import CrossScaleAttention
    torch.manual_seed(5)
    att = CrossScaleAttention(channel=64, scale=2).to(dev)
    x = (randn((1, 64) + hw, seed) * 0.5).to(dev)
    return att, x


def _opts(**kw):
    from ciaosr_amd import hip_ops
    return hip_ops.Options(csa_composed_min=1, **kw)


@pytest.mark.parametrize('hw', SIZES)
def test_recut_against_the_16c_route(dev, hw):
    """Four-block route against the 16C route within 2e-5 x the output scale (the project's bound for this comparison)."""
    from ciaosr_amd import hip_ops
    att, x = _att(dev, hw)
    hip_ops.poison_workspaces()
    with hip_ops.profile():
        y4 = att(x, options=_opts()).clone()
    prof = hip_ops.profile.results()
    assert 'csa_gather_vedge' in prof and 'csa_attn_v' in prof, sorted(prof)
    with hip_ops.profile():
        y16 = att(x, options=_opts(csa_attn_v16=1)).clone()
    prof16 = hip_ops.profile.results()
    assert 'csa_gather_vprime' in prof16 and 'csa_gather_vedge' not in prof16, sorted(prof16)
    scale = y16.abs().max().item()
    err = (y4 - y16).abs().max().item()
    print(f'{hw}: max|four-block - 16C| = {err:.3e} at output scale {scale:.3f}')
    assert torch.isfinite(y4).all() and err <= 2e-5 * scale


@pytest.mark.parametrize('hw', SIZES)
def test_recut_tile_widths_are_bitwise_equal(dev, hw):
    """192-wide and 96-wide items sum every output in the same order: bitwise equal, with every scratch byte poisoned first."""
    from ciaosr_amd import hip_ops
    att, x = _att(dev, hw)
    hip_ops.poison_workspaces()
    with hip_ops.profile():
        big = att(x, options=_opts()).clone()
    assert 'csa_gather_vedge' in hip_ops.profile.results()
    hip_ops.poison_workspaces()
    small = att(x, options=_opts(csa_attn_tile128=1)).clone()
    assert torch.isfinite(big).all() and torch.equal(big, small), (big - small).abs().max().item()


@pytest.mark.parametrize('hw', [(64, 70), (192, 192)])
@pytest.mark.parametrize('tile128', [0, 1])
def test_recut_repeats_bitwise_beside_a_second_stream(dev, hw, tile128):
    """Three calls with poisoned scratch are bitwise equal while another stream keeps the memory system busy with large copies
    (a load that lands late in a reused register, or a tile read before its barrier, shows as a difference here)."""
    from ciaosr_amd import hip_ops
    att, x = _att(dev, hw)
    opts = _opts(csa_attn_tile128=tile128)
    hip_ops.poison_workspaces()
    want = att(x, options=opts).clone()
    torch.cuda.synchronize()
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    side = torch.cuda.Stream(device=dev)
    outs = []
    for _ in range(3):
        hip_ops.poison_workspaces()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(24):
                dst.copy_(src)
        outs.append(att(x, options=opts).clone())
        torch.cuda.synchronize()
    for i, y in enumerate(outs):
        assert torch.equal(y, want), (i, (y - want).abs().max().item())
