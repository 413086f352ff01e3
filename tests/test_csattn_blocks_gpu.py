"""GPU tests of cs_attn in bands of query rows (Options.csa_block_mb; csattn.hip): the logit matrix S (and the 16-bit
probability matrix P16) held for one band at a time under a byte budget, scores / softmax / attn.V per band, everything else once.
Against the reference vectors, bitwise against the whole-map call wherever both run the same route, the four-block route at sizes whose
whole S is past its 2 GiB, bounded scratch at 512 x 512, and one C3 tile end to end."""
import math

import pytest
import torch

from tests import independent_refs as refs
from tests.helpers import SQRT6, load_golden, randn
from tests.test_csattn_four_block_gpu import ROUTE_TAGS
from tests.test_hip_parity import TOL, _csattn_golden, _my_csattn, _restorer, _tile192_checks, csattn_shapes

pytestmark = pytest.mark.gpu

PREC = {'fp32': 0, 'bf16': 1, 'f16': 2}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bands(hw, opt, channel=64, scale=2):
    """Band count of a call, from the library's host arithmetic."""
    from ciaosr_amd import _lib
    rows = _lib.load().ciaosr_cs_attn_block_rows(hw[0], hw[1], channel, scale, PREC[opt.precision], opt.c_arg())
    assert rows > 0
    return math.ceil((hw[0] + scale - 1) // scale * scale / rows)


def _profiled(att, x, opt):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        y = att(x, options=opt).clone()
    return y, hip_ops.profile.results()


GOLDEN = [('64x64', 0), ('67x70', 0), ('48', 1), ('45x51', 1)]


@pytest.mark.parametrize('mb', [1, 2, 4])
@pytest.mark.parametrize('tag,composed_min', GOLDEN)
def test_banded_fp32_matches_the_reference_vectors(dev, tag, composed_min, mb):
    """The four csattn_c64 reference vectors under 1, 2 and 4 MiB: csa_scores is launched once per band, more than once, on the
    four-block route, and the result stays within TOL of the reference."""
    from ciaosr_amd import hip_ops
    att, x, want = _csattn_golden(tag, dev)
    opt = hip_ops.Options(csa_composed_min=composed_min, csa_block_mb=mb)
    n = _bands(x.shape[2:], opt)
    y, prof = _profiled(att, x, opt)
    for t in ROUTE_TAGS + ('csa_edge_rows',):
        assert t in prof, (t, sorted(prof))
    assert 'csa_gather_vprime' not in prof, sorted(prof)
    err = (y.cpu()[0] - want).abs().max().item()
    print(f'cs_attn {tag}, {mb} MiB: {n} bands, csa_scores launches {prof["csa_scores"]["launches"]}, max|hip - reference| = {err:.3e}')
    assert n > 1 and prof['csa_scores']['launches'] == n and prof['csa_attn_v']['launches'] == n
    assert prof['csa_key_norms']['launches'] == 1 and prof['csa_down_partial']['launches'] == 1
    assert err < TOL


@pytest.mark.parametrize('mb', [1, 2, 4])
@pytest.mark.parametrize('precision', ['bf16', 'f16'])
@pytest.mark.parametrize('tag', ['64x64', '67x70'])
def test_banded_16bit_matches_the_reference_vectors(dev, tag, precision, mb):
    """The 16-bit entries in bands, inside the bounds test_csattn_bf16_mode_vs_reference asserts for the whole-map call."""
    from ciaosr_amd import hip_ops
    att, x, want = _csattn_golden(tag, dev)
    opt = hip_ops.Options(precision, csa_block_mb=mb)
    n = _bands(x.shape[2:], opt)
    y, prof = _profiled(att, x, opt)
    assert n > 1 and prof[f'csa_scores_{precision}']['launches'] == n and prof[f'csa_attn_v_{precision}']['launches'] == n, (n, prof)
    err = (y.cpu()[0] - want).abs()
    scale = want.abs().max().item()
    psnr = 10 * math.log10(scale ** 2 / max((err ** 2).mean().item(), 1e-20))
    print(f'{precision} cs_attn {tag}, {mb} MiB: {n} bands, max|d| vs reference {err.max().item():.3e} (scale {scale:.3f}), PSNR {psnr:.1f} dB')
    if precision == 'bf16':
        assert err.max().item() < 0.01 * scale and psnr > 58.0
    else:
        assert err.max().item() < 0.001 * scale and psnr > 76.0


@pytest.mark.parametrize('scales,hw', refs.OTHER_SCALES, ids=['s3-50x47', 's4-45x54', 's234-30x34'])
def test_banded_uncomposed_tail_at_scales_3_and_4(dev, scales, hw):
    """The uncomposed tail (scales 3 and 4, and 2 below the composed tail's size) in bands against the float64 oracle, within TOL as
    test_c64_scales_3_and_4_vs_float64_oracle holds the whole-map call; bitwise the whole-map result too."""
    from ciaosr_amd import hip_ops
    att = refs.csattn_module(64, scales).to(dev)
    x = refs.csattn_input(64, hw).to(dev)
    want = refs.csattn_oracle64(att, x)
    opt = hip_ops.Options(csa_block_mb=1)
    y, prof = _profiled(att, x, opt)
    n = [_bands(hw, opt, scale=s_) for s_ in scales]
    print(f'cs_attn scales {list(scales)} {hw}, 1 MiB: bands per scale {n}, csa_scores launches {prof["csa_scores"]["launches"]}')
    assert prof['csa_scores']['launches'] == sum(n) and 'csa_down' in prof and 'csa_attn_v_edge' not in prof, sorted(prof)
    if len(scales) == 1:
        assert n[0] > 1
    err, where = refs.worst_element(y.cpu(), want)
    assert torch.isfinite(y).all() and err < TOL, (err, where)
    assert torch.equal(y, att(x))


ROUTES = {'four-block': ('fp32', {}), '16c': ('fp32', dict(csa_attn_v16=1)), 'gemm-scores': ('fp32', dict(csa_scores_gemm=1)),
          'bf16': ('bf16', {}), 'f16': ('f16', {})}
# two budgets per size with different band counts; one leaves a ragged last band
BUDGETS = {(64, 64): (2, 4), (67, 70): (3, 7), (192, 192): (256, 100), (190, 187): (256, 100)}


@pytest.mark.parametrize('route', sorted(ROUTES))
@pytest.mark.parametrize('hw', sorted(BUDGETS))
def test_banded_is_bitwise_the_whole_map_call(dev, hw, route):
    """A band's scores, statistics and attn.V sum every output in the order the whole-map call does (the launchers derive what could change
    it from the whole map's rows), so the results are bitwise equal: on every route, at a C3 tile's size, on a reflect-padded one and on the
    two reference sizes, under two budgets with different band counts, and again with every scratch byte poisoned first."""
    from ciaosr_amd import hip_ops
    precision, kw = ROUTES[route]
    att = refs.csattn_module(64, default_init=True).to(dev)
    x = refs.csattn_input(64, hw, default_init=True).to(dev)
    whole, prof0 = _profiled(att, x, hip_ops.Options(precision, **kw))
    assert torch.isfinite(whole).all()
    assert 'csa_edge_rows' not in prof0
    scores = 'csa_scores' if precision == 'fp32' else f'csa_scores_{precision}'
    assert prof0[scores]['launches'] == 1
    counts = []
    for mb in BUDGETS[hw]:
        opt = hip_ops.Options(precision, csa_block_mb=mb, **kw)
        n = _bands(hw, opt)
        y, prof = _profiled(att, x, opt)
        assert n > 1 and prof[scores]['launches'] == n, (mb, n, prof[scores])
        for t in ('csa_gather_vedge', 'csa_gather_vprime', 'csa_patch_q', 'csa_key_norms'):
            assert (t in prof) == (t in prof0), (t, sorted(prof))
        assert torch.equal(y, whole), (route, mb, n, (y - whole).abs().max().item())
        counts.append(n)
    assert counts[0] != counts[1], counts
    hip_ops.poison_workspaces()
    assert torch.equal(att(x, options=hip_ops.Options(precision, csa_block_mb=BUDGETS[hw][1], **kw)), whole)


@pytest.mark.parametrize('hw,mb', [((256, 256), 1024), ((226, 340), 512)])
def test_bands_bring_the_four_block_route_back(dev, hw, mb):
    """Sizes whose whole logit matrix is past the four-block route's 2 GiB (256 x 256: 4 GiB; 226 x 340, a DIV2K image at x6: 5.6 GiB): the
    default call takes the 16C tail on the 128 x 128 kernel in row blocks, the banded call the four-block tail.  Two routes, the same
    products in another order: within 2e-5 x max(1, scale), the bound of the existing 256 x 256 and four-block-against-16C tests."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import seeded_state_dict
    P = seeded_state_dict(csattn_shapes(64, prefix=''), 11, 1.0)
    att = _my_csattn(64, P, dev, prefix='')
    x = randn((1, 64) + hw, 12).to(dev)
    whole, prof0 = _profiled(att, x, hip_ops.Options())
    assert 'csa_gather_vprime' in prof0 and 'csa_gather_vedge' not in prof0, sorted(prof0)
    opt = hip_ops.Options(csa_block_mb=mb)
    y, prof = _profiled(att, x, opt)
    for t in ROUTE_TAGS:
        assert t in prof, (t, sorted(prof))
    assert 'csa_gather_vprime' not in prof, sorted(prof)
    assert prof['csa_scores']['launches'] == _bands(hw, opt) > 1
    scale = whole.abs().max().item()
    d = (y - whole).abs().max().item()
    ms = lambda p: sum(v['total_ms'] for v in p.values())
    print(f'{hw}: {_bands(hw, opt)} bands of the four-block route against the default call: max |delta| {d:.2e} (scale {scale:.2f}); '
          f'kernel time {ms(prof):.2f} ms against {ms(prof0):.2f} ms')
    assert torch.isfinite(y).all() and d < 2e-5 * max(1.0, scale), d
    del x, y, whole
    hip_ops.release_workspaces()
    torch.cuda.empty_cache()


def test_bounded_scratch_at_512x512(dev):
    """512 x 512 (a whole-map S of 64 GiB, which the default call should not be asked for): 1024 and 2047 MiB give bands of 5 and 12 rows,
    finite and bitwise equal results, and a workspace of exactly ciaosr_cs_attn_workspace_bytes_opt bytes."""
    from ciaosr_amd import _lib, hip_ops
    from ciaosr_amd.init_utils import seeded_state_dict
    P = seeded_state_dict(csattn_shapes(64, prefix=''), 11, 1.0)
    att = _my_csattn(64, P, dev, prefix='')
    hw = (512, 512)
    x = randn((1, 64) + hw, 12).to(dev)
    out = {}
    for mb in (1024, 2047):
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
        opt = hip_ops.Options(csa_block_mb=mb)
        y, prof = _profiled(att, x, opt)
        want_bytes = _lib.load().ciaosr_cs_attn_workspace_bytes_opt(hw[0], hw[1], 64, 2, opt.c_arg())
        ws = hip_ops.workspace(1, dev)                     # the buffer the call grew: grow-only, so a 1-byte request hands it out
        print(f'512x512, {mb} MiB: {_bands(hw, opt)} bands, workspace {ws.numel() / 2 ** 20:.0f} MiB, '
              f'kernel time {sum(v["total_ms"] for v in prof.values()):.1f} ms, peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB')
        assert ws.numel() == want_bytes, (ws.numel(), want_bytes)
        assert prof['csa_scores']['launches'] == _bands(hw, opt) and 'csa_gather_vedge' in prof
        assert torch.isfinite(y).all()
        out[mb] = y.cpu()
        del y, ws
    assert torch.equal(out[1024], out[2047])
    del x
    hip_ops.release_workspaces()
    torch.cuda.empty_cache()


def test_c3_tile_end_to_end_with_banded_cs_attn(dev):
    """One full C3 tile through the restorer with test_cfg.hip_options = dict(csa_block_mb=256): bitwise the image without the option, and
    inside the limits of test_full_c3_tile_fp32_with_the_four_block_route against the reference's stored pixels."""
    import numpy as np
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import seeded_init_, synthetic_pair
    fx = load_golden('e2e_rdn_x4_tile192')
    lq, _ = synthetic_pair(192, 192, 4)
    outs = []
    for cfg in (dict(scale=4, tile=192, tile_overlap=32, hip_options=dict(csa_block_mb=256)), dict(scale=4, tile=192, tile_overlap=32)):
        model = _restorer('rdn', 4, dev, cfg)
        assert seeded_init_(model, seed=int(fx['weight_seed']), gain=float(fx['gain']), head_gain=SQRT6) == str(fx['sha'])
        model = model.to(dev)
        with hip_ops.profile():
            outs.append(model.restore(lq.to(dev)).cpu())
        prof = hip_ops.profile.results()
        for t in ROUTE_TAGS:
            assert t in prof, (t, sorted(prof))
        assert prof['csa_scores']['launches'] == (7 if 'hip_options' in cfg else 1), prof['csa_scores']
        del model
    assert torch.equal(outs[0], outs[1])
    errs = _tile192_checks(outs[0], fx, None)
    ref_s4 = torch.from_numpy(np.asarray(fx['out_s4']))
    rms = (outs[0][..., ::4, ::4] - ref_s4).double().pow(2).mean().sqrt().item()
    print(f'C3 tile fp32, cs_attn in 7 bands: max|d| {errs}, rms {rms:.3e}')
    assert max(errs.values()) <= 1e-5 and rms < 1e-5, (errs, rms)
