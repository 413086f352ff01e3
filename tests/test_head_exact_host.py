"""The exact head fixtures on the CPU (tests/exact_head.py): that they are exact, that the project's float32 oracle already agrees with
the float64 answer on them, and that the answer is sharp -- each kernel defect the GPU bound is meant to catch, applied to the REFERENCE,
moves the output past that bound by three orders of magnitude or more.  Nothing here needs a GPU."""
import pytest
import torch

from oracle import ciaosr_oracle as orc
from tests import exact_head as eh

ONE_UNIT_FLOOR = 0.20           # share of queries whose runner-up logit is exactly one unit below the winner's
SHARP = 1e3                     # a mutation must move the output by at least SHARP x the GPU bound

NAMES = list(eh.CASES)
ONEHOT = [n for n in NAMES if n.endswith('onehot')]


def _oracle32(fx):
    with torch.no_grad():
        return orc.query_rgb(fx.feat, fx.coord, fx.cell, fx.params, return_intermediates=True)


@pytest.mark.parametrize('name', NAMES + ['prefix'])
def test_fixture_is_exact(name, half='both'):
    """Every fixture the GPU file uses passes the builder's own assertions in both 16-bit types (half = 'both'; exact_head raises otherwise: U, q * key,
    hidden activations, Z representable; pre-activations, logits, table entries multiples of their unit below 2^24), and the 'onehot'
    ones keep the one-unit runner-up share above its floor."""
    fx = eh.case(eh.PREFIX[0], half, Q=eh.PREFIX[1]) if name == 'prefix' else eh.case(name, half)
    fig = fx.figures
    assert fx.want.dtype == torch.float64 and fx.want.shape == (1, fx.Q, 3) and fx.scale >= 8.0
    assert fx.want.unique().numel() > 30, 'a degenerate output would not tell kernels apart'
    for mlp in ('imnet_k', 'imnet_v', 'imnet_q'):
        if not (mlp == 'imnet_k' and fx.regime == 'uniform'):
            assert min(fig[f'{mlp}.h{i}.alive'] for i in range(4)) > 0.03, (mlp, fig)
    if fx.regime == 'onehot':
        print(f"{name} {half}: runner-up exactly one unit below the winner for {100 * fig['one_unit_share']:.1f} % of {fx.Q} queries "
              f"(floor {100 * ONE_UNIT_FLOOR:.0f} %); four distinct key pixels for {100 * fig['distinct_keys_share']:.1f} %; "
              f"winners by sample {fig['winner_hist']}; largest |logit| {fig['logit.max']:.0f} units, largest table entry {fig['table.max']:.0f}")
        assert fig['one_unit_share'] >= ONE_UNIT_FLOOR, fig
        assert min(fig['winner_hist']) > 0.1 * fx.Q, fig


@pytest.mark.parametrize('name', NAMES)
def test_float32_oracle_equals_float64(name):
    """The project's float32 CPU oracle on the fixture: within 2e-6 of the scale of the float64 answer (key selection does not hinge on
    a coordinate tie; the fixture is exact in fp32 without any GPU), and its attention is exactly one-hot / exactly 1/4 in float32."""
    fx = eh.case(name)
    out, inter = _oracle32(fx)
    assert out.dtype == torch.float32
    err = (out.double() - fx.want).abs().max().item()
    print(f'{name}: max|float32 oracle - float64| = {err:.3e} (bound {2e-6 * fx.scale:.3e}, scale {fx.scale:.2f})')
    assert err <= 2e-6 * fx.scale
    attn = inter['attn'][0]
    if fx.regime == 'uniform':
        assert torch.equal(attn, torch.full_like(attn, 0.25))
        return
    # one-hot: a single 1.0 and three 0.0 -- or, where the border clamp makes m samples read the same key pixel (same logit, same value
    # row), 1 / m on each of them and 0.0 elsewhere
    top = attn.max(1, keepdim=True).values
    m = (attn == top).sum(1)
    assert bool(((attn == top) | (attn == 0)).all()) and torch.equal(top[:, 0], 1.0 / m.float())
    strict = (m == 1).float().mean().item()
    print(f'{name}: attention exactly one-hot in float32 for {100 * strict:.1f} % of the queries, 1/m on m clamped duplicates for the rest')
    assert strict > 0.8


# ------------------------------------------------------------------------------------------------
# sharpness: mutations of the reference
# ------------------------------------------------------------------------------------------------
def _moved(label, fx, out):
    d = (out - fx.want[0]).abs().max().item()
    ratio = d / (eh.GPU_BOUND * fx.scale)
    print(f'{label}: output moves by {d:.3f} = {ratio:.2e} x the GPU bound ({eh.GPU_BOUND * fx.scale:.2e}); {int(((out - fx.want[0]).abs().amax(1) > 0).sum())} '
          f'of {fx.Q} queries change')
    assert ratio >= SHARP, (label, d)


def _mutated_params(fx, edit):
    P = {k: v.clone() for k, v in fx.params.items()}
    edit(P)
    return eh.reference64(P, fx.feat, fx.coord, fx.cell)[0][0]


@pytest.mark.parametrize('name', ['c180-dyadic-onehot', 'c180-ragged-onehot', 'c180-dyadic-uniform'])
def test_sharp_dropped_last_chunk_of_the_decode_input(name):
    """Dv = 1800 = 112 x 16 + 8: the decode input layer's last MFMA step has 8 columns.  Without them the answer moves."""
    fx = eh.case(name)

    def edit(P):
        P['imnet_q.layers.0.weight'][:, -8:] = 0
    _moved(f'{name}: last 8 input columns of imnet_q layer 0 dropped', fx, _mutated_params(fx, edit))


@pytest.mark.parametrize('name', ['c64-dyadic-onehot', 'c180-dyadic-uniform'])
def test_sharp_dropped_tail_term(name):
    fx = eh.case(name)

    def edit(P):
        P['imnet_v.layers.0.weight'][:, -4:] = 0
    _moved(f'{name}: tail term of imnet_v layer 0 dropped', fx, _mutated_params(fx, edit))


@pytest.mark.parametrize('name', ['c180-dyadic-onehot', 'c180-ragged-uniform'])
def test_sharp_removed_output_unit(name):
    """Output unit 56 of imnet_v's output layer at C = 180: the 32-row tile that holds rows 1792 .. 1799, the padded one."""
    fx = eh.case(name)

    def edit(P):
        P['imnet_v.layers.8.weight'][56 * 32:] = 0
        P['imnet_v.layers.8.bias'][56 * 32:] = 0
    _moved(f'{name}: output unit 56 of imnet_v removed', fx, _mutated_params(fx, edit))


def _recorded(name):
    fx = eh.case(name, keep_record=True)
    rec = fx.rec
    D = 9 * fx.C
    key = torch.stack([c[0][:, :D] for c in rec.mlp['imnet_k']], 1)                  # [Q, 4, D]
    kidx = torch.stack([k[0] for k in rec.key_idx], 1)                               # [Q, 4]
    return fx, rec, key, kidx


@pytest.mark.parametrize('name', ['c64-dyadic-onehot', 'c180-ragged-onehot'])
def test_sharp_logit_table_row_off_by_one_tap(name):
    """One of the nine taps of the logit fold -- the key offset most samples have -- reads the (q * key) products of the key pixel one
    column further (what a table row off by one tap does); imnet_k's activations stay those of the right key."""
    fx, rec, key, kidx = _recorded(name)
    H, W = fx.hw
    idx_map = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    qidx = orc._nearest(idx_map, fx.coord.double())[0, :, 0].long()
    off = (kidx // W - (qidx // W).unsqueeze(1)) * 3 + (kidx % W - (qidx % W).unsqueeze(1))
    tap = int(torch.mode(off.flatten()).values)
    U = torch.nn.functional.unfold(fx.feat.double(), 3, padding=1)[0].t()            # [HW, D]
    moved = (kidx // W) * W + (kidx % W + 1).clamp(max=W - 1)
    key_mut = torch.where((off == tap).unsqueeze(-1), U[moved], key)
    out = eh.finish(rec, fx.params, key=key_mut)[0]
    # only the logit's product changed: val * wv rows are the recorded ones
    _moved(f'{name}: tap {tap} of the logit fold shifted by one key pixel', fx, out)


def test_sharp_swapped_keys_in_the_last_ragged_row_tile():
    """Two adjacent queries of the last, partly filled row tile of the ragged C = 64 grid (Q = 4897: its last 33 queries) read each
    other's key, wk, value and wv rows.  Adjacent queries of a x2.8 grid often share their key pixels, and then the swap is no mutation:
    the pair is the last one whose swap can show, and there must be one."""
    name = 'c64-ragged-onehot'
    fx, rec, key, kidx = _recorded(name)
    Q = fx.Q
    pairs = [q for q in range(Q - 2, Q - 34, -1) if not torch.equal(kidx[q], kidx[q + 1])]
    assert pairs, 'no two adjacent queries with different keys among the last 33'
    best = None
    for q in pairs:
        two = torch.tensor([q, q + 1])
        out2 = eh.finish(rec, fx.params, queries=two, samples=two.flip(0))[0]
        if best is None or (out2 - fx.want[0, two]).abs().max() > (best[1] - fx.want[0, best[0]]).abs().max():
            best = (two, out2)
    out = fx.want[0].clone()
    out[best[0]] = best[1]
    _moved(f'{name}: keys of queries {int(best[0][0])} and {int(best[0][1])} swapped ({len(pairs)} candidate pairs)', fx, out)
