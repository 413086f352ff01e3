"""Every 16-bit RDN trunk route against the float64 answer of fixtures on which its arithmetic is exact (tests/exact_trunk.py).

The routes: dense_h16_kernel<LO>, dense_h16_dma_kernel, dense_h16_wide_kernel<LO, R> (R = 1, 2) and cast_group_h16_kernel of
csrc/dense_h16.hip in both element types, and the f16 local fusion on gemm_h16.hip whose epilogue writes the next block's 16-bit input
group -- the modes 'bf16', 'bf16-single', 'f16', 'f16-pairs'.  On these fixtures every tensor such a mode rounds to bf16 / half is such a
number already, hi + lo is the weight, and every sum (the hi and the lo products of the 9 cin sums on their own and together, in any
order and any K split; lff, gff, bias and residual epilogues) consists of multiples of one power of two whose absolute values add up to
less than 2^22 of it (check_exact_h16; test_trunk_h16_exact_host.py runs it on every case below).  So no operation rounds, ONE float64
evaluation is the answer of every route, and the bound is ZERO:

    torch.equal(got.double(), want)

The unsplit fixtures are those of test_trunk_exact_gpu.py, the same answer object; their weights are bf16 and half numbers, so every
`lo` fragment is zero.  The split fixtures (probe weights w (1 + s 2^-8)) have a non-zero lo on every tap -- in half, subnormal ones --
and two answers: hi + lo for 'bf16' and 'f16-pairs', hi alone for 'bf16-single', which must not read lo.

Which kernel ran: both cuts carry the tag enc_dense_<type> and agree bitwise here, so the cut is asserted from the launcher's size rule,
restated in _kernel, and test_random_weights_tell_the_cuts_apart shows once per wide shape and mode that the two cuts are different
code.  A failure names the worst element (image, channel, row, column) with the got / want values there and the error in output units."""
import pytest
import torch

from tests import exact_trunk as et
from tests import independent_refs as refs
from tests.helpers import randn
from tests.test_trunk_exact_gpu import DENSE_TAGS, _build, _encoder, _exact, _run

pytestmark = pytest.mark.gpu

CASES = et.h16_cases()
PAIRS = [(c, m) for c in CASES for m in c.modes]
WIDE_SHAPES = [(hw, 1) for hw in et.H16_WIDE_MAPS] + [et.H16_WIDE2]
TEETH_ROUTES = {'12x12': ((21, 37), 1, 1), 'wide1': ((65, 225), 1, 0), 'wide2': et.H16_WIDE2 + (0,)}      # kernel -> (map, B, dense_direct)

_teeth, _random = {}, {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _kernel(hw, B, direct, pairs):
    """The choice of dense_layer_h16 (csrc/dense_h16.hip), restated: the wide kernel from 32 tiles of 16 x 32 pixels per image unless the
    12 x 12 cut is asked for; its tile shape by the LAUNCH -- rounds of the 256 CUs over 8 x 32 tiles (R = 1) times 1.2 against rounds
    over 16 x 32 tiles (R = 2) times 2; on the 12 x 12 cut, a batch without a lo pack takes the two-workgroups-per-CU kernel."""
    if direct or refs.wide_tiles(hw) < 32:
        return '12x12' if pairs or B < 2 else 'dma'
    tiles_x = -(-hw[1] // 32)
    n16, n8 = tiles_x * -(-hw[0] // 16) * B, tiles_x * -(-hw[0] // 8) * B
    rounds = lambda n: -(-n // 256)
    return 'wide1' if 1.2 * rounds(n8) < 2.0 * rounds(n16) else 'wide2'


def _tags(mode, nb, nl):
    """(ran, not_ran, counts) of a 16-bit trunk call: the dense layers and the casts of the element type (the f16 fusion writes the 16-bit
    input of every block after the first: one cast), the fusion's tags, none of the fp32 dense routes."""
    h = et.H16_MODES[mode]
    dense, cast = f'enc_dense_{h.half}', f'enc_cast_{h.half}'
    fuse, other = (('enc_conv1x1_f16', 'enc_gff1x1'), ('enc_conv1x1',)) if h.lff16 else (('enc_conv1x1',), ('enc_conv1x1_f16', 'enc_gff1x1'))
    wrong = 'f16' if h.half == 'bf16' else 'bf16'
    return ('enc_conv_first', 'enc_conv3x3', dense, cast) + fuse, DENSE_TAGS + other + (f'enc_dense_{wrong}', f'enc_cast_{wrong}', 'enc_edsr_resident'), \
        {dense: nb * nl, cast: 1 if h.lff16 else nb}


def _opts(mode, direct):
    return dict(precision=mode, dense_min_tiles=1, dense_direct=direct)


def _shape(fx):
    return 1 + max(int(k.split('.')[1]) for k in fx.params if k.startswith('rdbs.')), 1 + max(int(k.split('.')[3]) for k in fx.params if k.startswith('rdbs.0.layers.'))


def test_the_cases_reach_every_kernel():
    """The size rule on the chosen shapes: (81, 257) x 3 is 162 tiles of 16 x 32 against 297 of 8 x 32 -- one round against two, R = 2;
    every one-image wide map stays on R = 1; every kernel instantiation is some case's."""
    assert _kernel(et.H16_WIDE2[0], et.H16_WIDE2[1], 0, False) == 'wide2' and not 1.2 * 2 < 2.0 * 1
    for hw in et.H16_WIDE_MAPS:
        assert refs.wide_tiles(hw) >= 32 and _kernel(hw, 1, 0, True) == 'wide1' and _kernel(hw, 1, 1, True) == '12x12'
    assert refs.wide_tiles((64, 256)) == 32 and _kernel((65, 225), 2, 0, False) == 'wide1'
    for hw in et.H16_SMALL_MAPS:
        assert refs.wide_tiles(hw) < 32
    seen = set()
    for c, mode in PAIRS:
        pairs = et.H16_MODES[mode].pairs
        assert _kernel(c.hw, c.B, c.direct, pairs) == c.kernel, (c, mode)
        seen.add((c.kernel, pairs, et.H16_MODES[mode].half, c.fixture == 'split'))
    for half in ('bf16', 'f16'):
        assert {('12x12', True, half, True), ('12x12', False, half, False), ('dma', False, half, False)} <= seen
        for k in ('wide1', 'wide2'):
            assert {(k, True, half, True), (k, False, half, False)} <= seen
    assert ('12x12', False, 'bf16', True) in seen and ('wide1', False, 'bf16', True) in seen and ('wide2', False, 'bf16', True) in seen


@pytest.mark.parametrize('c,mode', PAIRS, ids=[f'{et.h16_id(c)}-{m}' for c, m in PAIRS])
def test_16_bit_routes(dev, c, mode):
    """Every case of exact_trunk.h16_cases in each of its modes: bitwise the float64 answer (the split fixtures under 'bf16-single': the
    answer with hi alone), with the element type's dense and cast tags, l + 1 dense launches per block, the fusion's tags of the mode and
    no fp32 dense route."""
    fx = et.h16_fixture(c)
    assert _kernel(c.hw, c.B, c.direct, et.H16_MODES[mode].pairs) == c.kernel
    ran, not_ran, counts = _tags(mode, *_shape(fx))
    _exact(_encoder(fx, dev), fx._replace(want=et.h16_answer(fx, mode)), dev, _opts(mode, c.direct), ran=ran, not_ran=not_ran, counts=counts,
           label=f'{et.h16_id(c)} {mode}')


@pytest.mark.parametrize('mode', et.H16_ALL)
@pytest.mark.parametrize('hw,B', WIDE_SHAPES, ids=[f'{hw[0]}x{hw[1]}-b{B}' for hw, B in WIDE_SHAPES])
def test_random_weights_tell_the_cuts_apart(dev, hw, B, mode):
    """On the exact fixtures the two cuts agree bitwise and share their tag.  With random weights they sum in different orders: on every
    wide shape and mode, dense_direct = 0 and 1 differ in some bit -- two kernels ran."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_hip_parity import _restorer
    if 'enc' not in _random:
        model = _restorer('rdn', 4, dev, dict(scale=4), blocks=1, layers=2)
        seeded_init_(model, seed=23, gain=1.6)
        _random['enc'] = model.to(dev).generator._encoder_hip
    assert _kernel(hw, B, 0, False) in ('wide1', 'wide2') and _kernel(hw, B, 1, True) == '12x12'
    x = torch.stack([randn((3,) + hw, 78 + i) * 0.3 for i in range(B)]).to(dev)
    out = []
    for direct in (0, 1):
        with hip_ops.profile():
            out.append(_random['enc'].forward_hwc_batch(x, hip_ops.Options(**_opts(mode, direct))).cpu())
        assert f'enc_dense_{et.H16_MODES[mode].half}' in hip_ops.profile.results(), sorted(hip_ops.profile.results())
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    d = (out[0] - out[1]).abs().max().item()
    print(f'random weights {mode} {hw} B = {B}: max |wide - 12x12| = {d:.3e} (feature scale {out[1].abs().max().item():.3f})')
    assert not torch.equal(out[0], out[1]), 'the two cuts sum in different orders: bitwise equality means one of them did not run'


@pytest.mark.parametrize('mode', ['bf16', 'f16-pairs'])
@pytest.mark.parametrize('kernel', list(TEETH_ROUTES))
def test_the_bound_has_teeth(dev, kernel, mode):
    """The comparison itself, on the GPU: a model whose probe lo pack lacks ONE fragment's worth of one output row (exact_trunk.lo_mutated
    'drop': those taps hold hi alone, so the pack's lo is zero there), run through each cut and held against the UNCHANGED answer, is off
    by at least one output unit -- what a kernel that skipped or mis-addressed that lo fragment would do."""
    hw, B, direct = TEETH_ROUTES[kernel]
    half = et.H16_MODES[mode].half
    fx = et.split_probe(3, hw, B)
    if half not in _teeth:
        _teeth[half] = _build(et.lo_mutated(fx, half, 'drop'), dev)
    assert _kernel(hw, B, direct, True) == kernel
    ran, not_ran, counts = _tags(mode, 1, 4)
    err, where, (g, w_), got = _run(_teeth[half], fx, dev, _opts(mode, direct), ran=ran, not_ran=not_ran, counts=counts,
                                    label=f'one lo fragment dropped, {kernel} {mode}')
    print(f'one lo fragment dropped, {kernel} {mode}: {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output scale at {where} (got {g!r}, want {w_!r})')
    assert not torch.equal(got.double(), fx.want) and err >= fx.unit, (kernel, mode, err)
