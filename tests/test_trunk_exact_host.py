"""The exact trunk fixtures on the CPU (tests/exact_trunk.py): that every fixture and map test_trunk_exact_gpu.py runs meets the exactness
condition (every sum a route can form: multiples of one power of two, sum |addends| below 2^22 of it -- two bits of headroom in fp32),
that the project's oracle agrees with the tap-by-tap float64 evaluation, and that the answer is sharp: each kernel defect the zero bound
is meant to catch, applied to the REFERENCE, moves the float64 answer by at least one output unit.  Nothing here needs a GPU."""
import pytest
import torch

from oracle import ciaosr_oracle as orc
from tests import exact_trunk as et

FIXTURES = et.all_fixtures()
BIG = f'probe7-{et.BIG[0]}x{et.BIG[1]}'


@pytest.mark.parametrize('name', list(FIXTURES))
def test_fixture_is_exact(name):
    """check_exact on every fixture and size of the GPU file, the bit figures per stage, and the oracle's own float64 evaluation."""
    fx = FIXTURES[name]()
    fig = et.check_exact(fx)
    bits = ', '.join(f'{k} {v:.2f}' for k, v in fig.items() if not k.endswith(('.max', '.alive')))
    print(f'{name}: log2(sum |addends| / unit), bound 22: {bits}; output scale {fx.scale:.3f}, unit {fx.unit}; '
          f'block inputs up to {max(v for k, v in fig.items() if k.endswith(".in.max")) if fx.kind == "rdn" else 0:.0f}')
    assert all(v < 22.0 for k, v in fig.items() if not k.endswith(('.max', '.alive')))
    assert fx.want.dtype == torch.float64 and fx.want.shape == (fx.B, fx.params['gff.1.weight' if fx.kind == 'rdn' else 'conv_after_body.weight'].shape[0]) + fx.hw
    assert fx.want.unique().numel() > 30, 'a degenerate output would not tell kernels apart'
    assert fx.scale >= 16 * fx.unit
    if fx.kind == 'rdn':
        assert fig['dense.alive'] > 0.01, fig
    if fx.B > 1:
        assert not torch.equal(fx.want[0], fx.want[1]) and not torch.equal(fx.want[1], fx.want[2])
    if name != BIG:                                              # (the dense float64 convolutions of the big map take a minute)
        P = {k: v.double() for k, v in fx.params.items()}
        with torch.no_grad():
            ref = orc.edsr_features(fx.x.double(), P, res_scale=fx.res_scale) if fx.kind == 'edsr' else orc.encoder_features(fx.x.double(), P)
        assert torch.equal(ref, fx.want), 'the oracle in float64 differs from the tap-by-tap evaluation'


def test_every_input_column_is_read():
    """Stem, lff, gff and the EDSR convolutions read every input column in at least one row; a probe has a tap in every input group of
    every output row and never two on one (output, input) pair; a feeder has one tap per row, on group 0."""
    for fx in (et.probe(7), et.probe(0), et.two_blocks(), et.narrow32(), et.edsr((12, 12))):
        for k, w in fx.params.items():
            if not k.endswith('.weight'):
                continue
            if '.layers.' not in k:
                assert (w != 0).flatten(1).any(0).reshape(w.shape[1:]).all(), k
                continue
            C = w.shape[0]
            l = int(k.split('.')[3])
            pairs = (w != 0).sum((2, 3))
            assert pairs.max() == 1, k
            nl = 1 + max(int(n.split('.')[3]) for n in fx.params if n.startswith(k.split('.layers.')[0] + '.layers.'))
            if l == nl - 1:
                assert (pairs.view(C, l + 1, C).sum(2) >= 1).all(), k
                if not (k.startswith('rdbs.0.') and 'rdbs.1.lff.weight' in fx.params):     # (block 0 of the NB = 2 fixture: one tap per group)
                    assert (pairs.sum(0) >= 1).all(), k                                  # every input channel is read by some row
            else:
                assert (pairs.sum(1) == 1).all() and not pairs[:, C:].any(), k


@pytest.mark.parametrize('l', [1, 3, 7])
@pytest.mark.parametrize('kind', list(et.MUTATIONS))
def test_mutations_move_the_answer(kind, l):
    """One tap's product dropped at the first column right of a tile seam (12-pixel, 8x16 and 16x32 tilings), two input channels of the
    last group swapped across 8-channel steps, the one-row partial 4x4 tile dropped: each moves the float64 answer by at least one
    output unit somewhere (the GPU bound is zero)."""
    hw, arg = et.MUTATIONS[kind]
    fx = et.probe(l, hw)
    got = et.rdn_eval(fx.params, fx.x, mutate=arg(fx))
    err, where, _ = et.worst_element(got, fx.want)
    print(f'probe {l} {hw}, {kind}: max |mutated - intact| = {err:.4g} = {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output scale ({where}); '
          f'{int((got != fx.want).sum())} elements differ')
    assert err >= fx.unit
