"""The exact trunk fixtures under the 16-bit trunk modes, on the CPU (tests/exact_trunk.py): that on every (fixture, map, mode)
test_trunk_h16_exact_gpu.py runs, every tensor a route of the mode rounds to bf16 / half is such a number already and every sum meets the
exactness condition (check_exact_h16: the direct 9 cin sums with the hi weights, with the lo weights and with both; stem, lff, gff and the
residual epilogues) -- so the float64 answer the fp32 routes are held to is the answer of the 16-bit routes too, and the GPU bound is
zero; that the split fixtures have a `lo` half on every probe tap; and that the answer is sharp: each defect of a 16-bit route the zero
bound is meant to catch, applied to the REFERENCE, moves the float64 answer by at least one output unit.  Nothing here needs a GPU."""
import pytest
import torch

from tests import exact_trunk as et
from tests import test_trunk_exact_host as fp32_host

CASES = et.h16_cases()
PAIRS = [(c, m) for c in CASES for m in c.modes]
_distinct = {}


@pytest.mark.parametrize('c,mode', PAIRS, ids=[f'{et.h16_id(c)}-{m}' for c, m in PAIRS])
def test_fixture_is_exact_in_16_bits(c, mode):
    fx = et.h16_fixture(c)
    fig = et.check_exact_h16(fx, mode)
    bits = {k: v for k, v in fig.items() if not k.endswith(('.max', '.alive', '.taps'))}
    print(f"{et.h16_id(c)} {mode}: log2(sum |addends| / unit), bound 22: {', '.join(f'{k} {v:.2f}' for k, v in bits.items())}; "
          f'output scale {fx.scale:.3f}, unit {fx.unit}')
    assert all(v < 22.0 for v in bits.values())
    want = et.h16_answer(fx, mode)
    if id(want) not in _distinct:                               # (once per answer: the modes of an unsplit fixture share it)
        _distinct[id(want)] = want.flatten()[:100000].unique().numel()
    assert want.dtype == torch.float64 and want.shape == (fx.B, 64) + fx.hw and _distinct[id(want)] > 30
    assert fig['dense.alive'] > 0.01, fig
    if fx.B > 1:
        assert all(not torch.equal(want[i], want[i + 1]) for i in range(fx.B - 1))
    if c.fixture == 'split':
        if et.H16_MODES[mode].pairs:
            assert fig['lo.taps'] == 64 * et.TAPS and {'dense.hi', 'dense.lo', 'dense.hi+lo'} <= set(fig)
        else:                                                    # hi alone: an answer of its own, away from the pair modes' by whole units
            err = (want - fx.want).abs().max().item()
            print(f'{et.h16_id(c)} {mode}: the lo terms are worth up to {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output scale')
            assert err >= fx.unit


def test_unsplit_answers_are_the_fp32_routes_answers():
    """On the unsplit fixtures every mode is held to fx.want itself -- the object test_trunk_exact_gpu.py holds the fp32 routes to where
    both files run a fixture, not a recomputation."""
    shared = 0
    for c in CASES:
        if c.fixture == 'split':
            continue
        fx = et.h16_fixture(c)
        assert all(et.h16_answer(fx, m) is fx.want for m in c.modes)
        name = f'probe{c.l}-{c.hw[0]}x{c.hw[1]}' if c.fixture == 'probe' and c.B == 1 else f'nb2-{c.hw[0]}x{c.hw[1]}' if c.B == 1 else None
        if name in fp32_host.FIXTURES:
            assert fp32_host.FIXTURES[name]().want is fx.want, name
            shared += 1
    assert shared >= 12          # (21, 37) probes 0 .. 7, (7, 30) probes 0, 1, 7 and the two-block fixture


@pytest.mark.parametrize('l', [0, 3, 7])
def test_split_fixtures_have_a_lo_half_on_every_tap(l):
    """w (1 + s 2^-8): hi + lo == w exactly and lo != 0 on all 1024 taps in both element types; in half, the lo of a 9/256 tap is the
    subnormal 2^-16 (probe 0 has no such tap: it reads integers with 9/16)."""
    fx, unsplit = et.split_probe(l), et.probe(l)
    err = (fx.want - unsplit.want).abs().max().item()
    print(f'split probe {l} {fx.hw}: max |answer - unsplit answer| = {err:.3e} = {err / fx.unit:.0f} output units')
    assert torch.equal(fx.x, unsplit.x) and err >= fx.unit
    w = fx.params[f'rdbs.0.layers.{l}.conv.weight'].double()
    taps = w != 0
    assert int(taps.sum()) == 64 * et.TAPS and torch.equal(taps, et.probe(l).params[f'rdbs.0.layers.{l}.conv.weight'] != 0)
    for half in ('bf16', 'f16'):
        hi, lo = et.split16(w, half)
        assert torch.equal(hi + lo, w) and torch.equal(lo != 0, taps) and not torch.equal(hi, w)
        sub = int(((lo != 0) & (lo.abs() < 2.0 ** -14)).sum())
        print(f'split probe {l} {half}: |lo| in [{lo[taps].abs().min().item()}, {lo[taps].abs().max().item()}], {sub} subnormal')
        if half == 'f16':
            assert (sub >= 1) == (l > 0), sub


@pytest.mark.parametrize('half', ['bf16', 'f16'])
@pytest.mark.parametrize('l', [0, 3, 7])
@pytest.mark.parametrize('kind', list(et.H16_MUTATIONS)[:2])
def test_lo_mutations_move_the_answer(kind, l, half):
    fx, got = et.H16_MUTATIONS[kind](l, half)
    err, where, _ = et.worst_element(got, fx.want)
    print(f'split probe {l} {fx.hw} {half}, {kind}: max |mutated - intact| = {err:.4g} = {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output '
          f'scale ({where}); {int((got != fx.want).sum())} elements differ')
    assert err >= fx.unit and err / fx.unit == round(err / fx.unit)


def test_stale_16_bit_block_input_moves_the_answer():
    kind = list(et.H16_MUTATIONS)[2]
    fx, got = et.H16_MUTATIONS[kind](None, 'f16')
    err, where, _ = et.worst_element(got, fx.want)
    print(f'NB = 2 {fx.hw}, {kind}: max |mutated - intact| = {err:.4g} = {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output scale '
          f'({where}); {int((got != fx.want).sum())} elements differ')
    assert err >= fx.unit and err / fx.unit == round(err / fx.unit)
