"""cs_attn against an independent reference at the sizes where only a sibling route of the same call was compared before.

Every case computes the float64 oracle (oracle.ciaosr_oracle.cross_scale_attention on float64 tensors; 2.6e-6 .. 4.0e-6 from the four
committed `csattn_c64_*` reference outputs, pinned by test_oracle_pin.py::test_csattn_c64_float64) on the CPU, holds the fp32 result to
the suite's working tolerance TOL = 1e-4 absolute -- the whole margin belongs to the kernels -- prints max|d| beside the bound and the
output scale, and asserts through hip_ops.profile which route ran.

What the sizes reach (csrc/patch_ops.hip: the softmax kernels are register-resident for Lld/4 in (512, 2304], loops outside):
  (128, 64) L = 2048 loop kernels just before the switch | (108, 76) L = 2052 register kernels just past it |
  (90, 102) L = 2295, L % 4 = 3: the masked tail of the register kernels | (190, 187) L = 8930: their largest row here |
  (194, 192) L = 9312 > 9216: loop kernels again, and the 16-bit modes' row of that length.
`csa_composed_min = -1` takes the uncomposed tail, whose in-place softmax_rows switches at the same lengths.

Measured on an MI355X (output scale 1.66 .. 2.31), all within their bounds, no kernel change needed:
  C = 64 fp32, composed routes   1.6e-6 .. 5.4e-6 up to (128, 64); 1.3e-5 .. 1.4e-5 at (194, 192); 1.2e-5 (16C) .. 2.5e-5 (four-block) at (190, 187)
  C = 64 fp32, uncomposed tail   2.0e-6 .. 3.0e-6;   default-init (output scale 0.25)  2.2e-7 .. 3.4e-7
  C = 180                        1.2e-5 .. 1.7e-5; the bf16 / f16 entries bitwise the fp32 result
  C = 64 bf16                    5.8e-3 .. 8.0e-3 x scale, 61.5 .. 62.6 dB;   f16  5.7e-4 .. 8.4e-4 x scale, 79.7 .. 80.6 dB
  scales 3, 4, [2, 3, 4]         1.6e-6 .. 2.2e-6

That the oracle is sharp at these sizes (two swapped probabilities move it by far more than TOL) is test_reference_sharpness.py's."""
import math

import pytest
import torch

from tests import independent_refs as refs
from tests.test_hip_parity import TOL

pytestmark = pytest.mark.gpu

_want = {}      # (C, scales, hw, default_init) -> float64 oracle output: one CPU run per size, shared by the option sets


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _case(dev, C, hw, scales=(2,), default_init=False):
    att = refs.csattn_module(C, scales, default_init=default_init)
    x = refs.csattn_input(C, hw, default_init=default_init)
    key = (C, tuple(scales), tuple(hw), default_init)
    if key not in _want:
        _want[key] = refs.csattn_oracle64(att, x)
    return att.to(dev), x.to(dev), _want[key]


def _poison(dev, att, hw):
    """Grow the call's scratch to its size first, so that every byte the call will use carries the NaN pattern."""
    from ciaosr_amd import _lib, hip_ops
    hip_ops.workspace(_lib.load().ciaosr_cs_attn_workspace_bytes_scale(hw[0], hw[1], att.channel, max(att.scale)), dev)
    hip_ops.poison_workspaces()


def _run(att, x, opts, ran=(), not_ran=()):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        y = att(x, options=opts).cpu()
    prof = hip_ops.profile.results()
    missing, extra = [t for t in ran if t not in prof], [t for t in not_ran if t in prof]
    assert not missing and not extra, f'{opts}: expected tags missing {missing}, unexpected tags present {extra}; ran {sorted(prof)}'
    return y


def _check_fp32(label, y, want):
    err, where = refs.worst_element(y, want)
    scale = want.abs().max().item()
    print(f'{label}: max|hip - float64 oracle| = {err:.3e} (bound {TOL:.0e}, output scale {scale:.3f}; worst at {where})')
    assert torch.isfinite(y).all(), f'{label}: non-finite output'
    assert err < TOL, f'{label}: {err:.3e} at {where}'


# route -> (options, tags that must / must not be in the profile)
FOUR_BLOCK = dict(ran=('csa_gather_vedge', 'csa_key_norms', 'csa_attn_v_edge', 'softmax_stats'), not_ran=('csa_gather_vprime', 'csa_patch_q', 'csa_down'))
ROUTES = {
    'default': (dict(), FOUR_BLOCK),
    'tile128': (dict(csa_attn_tile128=1), FOUR_BLOCK),
    'v16': (dict(csa_attn_v16=1), dict(ran=('csa_gather_vprime', 'csa_key_norms', 'csa_attn_v_edge'), not_ran=('csa_gather_vedge', 'csa_patch_q', 'csa_down'))),
    'scores_gemm': (dict(csa_scores_gemm=1), dict(ran=('csa_patch_q', 'csa_gather_vedge', 'csa_attn_v_edge'), not_ran=('csa_key_norms', 'csa_down'))),
    'uncomposed': (dict(csa_composed_min=-1), dict(ran=('csa_down', 'softmax_rows', 'csa_key_norms'),
                                                   not_ran=('csa_attn_v_edge', 'csa_gather_vedge', 'csa_gather_vprime', 'softmax_stats'))),
}
C64_CASES = ([(hw, r) for hw in refs.C64_SIZES for r in ('default', 'v16', 'scores_gemm')] +
             [(hw, 'tile128') for hw in [(45, 51), (190, 187)]] +
             [(hw, 'uncomposed') for hw in [(128, 64), (108, 76), (90, 102), (190, 187), (194, 192)]])


def _options(hw, **kw):
    from ciaosr_amd import hip_ops
    if tuple(hw) in refs.C64_SMALL and 'csa_composed_min' not in kw:
        kw['csa_composed_min'] = 1          # below 4096 padded pixels the composed tail is forced
    return hip_ops.Options(**kw)


@pytest.mark.parametrize('hw,route', C64_CASES, ids=[f'{h}x{w}-{r}' for (h, w), r in C64_CASES])
def test_c64_fp32_routes_vs_float64_oracle(dev, hw, route):
    """C = 64, scale 2, fp32, the goldens' peaked recipe (3 to 4 effective keys per query): the four-block route (default; its 96-wide
    items on two ragged sizes), the 16C route, the patch-row score GEMM and -- on the sizes on both sides of the two softmax switches --
    the uncomposed tail, each within TOL of the float64 oracle.  The default route runs on scratch filled with NaN patterns."""
    kw, tags = ROUTES[route]
    att, x, want = _case(dev, 64, hw)
    if route == 'default':
        _poison(dev, att, hw)
    y = _run(att, x, _options(hw, **kw), **tags)
    _check_fp32(f'cs_attn C=64 {hw} {route}', y, want)


def test_c64_broad_softmax_vs_float64_oracle(dev):
    """The default-init module with randn * 0.5 of the route sweeps (80 to 150 effective keys of 2295): every key carries weight, so
    a key that the masked tail of the register softmax kernels (L % 4 = 3) dropped or counted twice would show."""
    hw = (90, 102)
    att, x, want = _case(dev, 64, hw, default_init=True)
    _poison(dev, att, hw)
    for route in ('default', 'v16', 'uncomposed'):
        kw, tags = ROUTES[route]
        _check_fp32(f'cs_attn C=64 {hw} default-init {route}', _run(att, x, _options(hw, **kw), **tags), want)


C180_ROUTE = dict(ran=('csa_gather_vprime', 'csa_patch_q', 'csa_scores', 'csa_attn_v', 'csa_attn_v_edge', 'csa_down_partial'),
                  not_ran=('csa_gather_vedge', 'csa_key_norms', 'csa_down'))


@pytest.mark.parametrize('hw', refs.C180_SIZES)
def test_c180_composed_tail_vs_float64_oracle(dev, hw):
    """C = 180 (the SwinIR head's width; what a whole-image run takes from 64 x 64 LR on): the 16C route with N = 2880, Ch = 92 and the
    patch-row score GEMM with K = 828, with the 192 x 256 attn.V kernel's choice and with the 128 x 128 kernel, against the oracle.
    9 * Ch % 8 != 0, so the 16-bit entries have no 16-bit route at this width: they must run the fp32 kernels (no `_bf16` / `_f16` tag
    in the profile) and return the fp32 result bitwise -- anything else would be a 16-bit route no reference has seen."""
    from ciaosr_amd import hip_ops
    att, x, want = _case(dev, 180, hw)
    _poison(dev, att, hw)
    y = _run(att, x, hip_ops.Options(), **C180_ROUTE)
    _check_fp32(f'cs_attn C=180 {hw} default', y, want)
    y128 = _run(att, x, hip_ops.Options(csa_attn_tile128=1), **C180_ROUTE)
    _check_fp32(f'cs_attn C=180 {hw} tile128', y128, want)
    for half in ('bf16', 'f16'):
        y16 = _run(att, x, hip_ops.Options(half), ran=C180_ROUTE['ran'],
                   not_ran=C180_ROUTE['not_ran'] + (f'csa_scores_{half}', f'csa_attn_v_{half}'))
        d = (y16 - y).abs().max().item()
        print(f'cs_attn C=180 {hw} {half} entry: max|d| to the fp32 entry {d:.3e} (must be 0: no 16-bit route at this width)')
        assert torch.equal(y16, y), d


def _localise(label, d, tile=128):
    """Where a 16-bit error sits: by row, by column, by position in the 128-row MFMA tile of the flattened queries."""
    e = d.abs()[0].amax(0)                                   # [H][W]
    H, W = e.shape
    rows, cols = e.amax(1), e.amax(0)
    flat = e.reshape(-1)
    pos = torch.zeros(tile, dtype=e.dtype).scatter_reduce(0, torch.arange(flat.numel()) % tile, flat, 'amax')
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[2:-2, 2:-2] = False
    top = lambda v: ', '.join(f'{int(i)}: {v[i].item():.2e}' for i in v.topk(min(5, v.numel())).indices)
    print(f'{label}: error by row     [{top(rows)}] (median {rows.median().item():.2e})')
    print(f'{label}: error by column  [{top(cols)}] (median {cols.median().item():.2e})')
    print(f'{label}: error by pixel index mod {tile} [{top(pos)}] (median {pos.median().item():.2e})')
    print(f'{label}: mean error in the 2-pixel border ring {e[ring].mean().item():.2e}, inside {e[~ring].mean().item():.2e}')


@pytest.mark.parametrize('half', ['bf16', 'f16'])
@pytest.mark.parametrize('hw', refs.H16_SIZES)
def test_c64_16bit_modes_vs_float64_oracle(dev, hw, half):
    """ciaosr_cs_attn_bf16 / _f16 (scores and P.V' on the 16-bit MFMA) against the float64 oracle under the project's bounds for these
    modes (test_csattn_bf16_mode_vs_reference): bf16 max < 0.01 x scale and PSNR > 58 dB, f16 max < 0.001 x scale and PSNR > 76 dB --
    at a wide map, at L % 4 = 3, at a forced composed tail with reflect padding on both axes and at L = 9312 > 9216."""
    from ciaosr_amd import hip_ops
    att, x, want = _case(dev, 64, hw)
    kw = dict(csa_composed_min=1) if tuple(hw) in refs.C64_SMALL else {}
    y = _run(att, x, hip_ops.Options(half, **kw), ran=(f'csa_scores_{half}', f'csa_attn_v_{half}', 'csa_attn_v_edge'), not_ran=('csa_down',))
    d = y.double() - want
    scale = want.abs().max().item()
    err, where = refs.worst_element(y, want)
    psnr = 10 * math.log10(scale ** 2 / max((d ** 2).mean().item(), 1e-30))
    rel, db = (0.01, 58.0) if half == 'bf16' else (0.001, 76.0)
    print(f'cs_attn C=64 {hw} {half}: max|hip - float64 oracle| = {err:.3e} = {err / scale:.2e} x scale (bound {rel:g} x scale = {rel * scale:.3e}; '
          f'worst at {where}), PSNR {psnr:.1f} dB (bound {db:.0f})')
    ok = torch.isfinite(y).all() and err < rel * scale and psnr > db
    if not ok:
        _localise(f'cs_attn C=64 {hw} {half}', d)
    assert ok, (err, scale, psnr)


@pytest.mark.parametrize('scales,hw', refs.OTHER_SCALES, ids=['s3-50x47', 's4-45x54', 's234-30x34'])
def test_c64_scales_3_and_4_vs_float64_oracle(dev, scales, hw):
    """Scale entries 3 and 4 and the list [2, 3, 4] at the model's width (they were pinned at C = 8 on 10 x 13 maps only): reflect
    mod-padding on both axes, `downsample`, (3s) x (3s) value patches, `fold_s`, downx3 / downx4 and the channel concatenation."""
    from ciaosr_amd import hip_ops
    att, x, want = _case(dev, 64, hw, scales=scales)
    _poison(dev, att, hw)
    y = _run(att, x, hip_ops.Options(), ran=('csa_down', 'fold_gather', 'csa_patch_v', 'softmax_rows'), not_ran=('csa_attn_v_edge',))
    assert y.shape == want.shape == (1, 64 * len(scales)) + tuple(hw)
    _check_fp32(f'cs_attn C=64 scales {list(scales)} {hw}', y, want)
