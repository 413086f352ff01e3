"""Every 16-bit head kernel against the float64 answer of fixtures on which 16-bit arithmetic is exact (tests/exact_head.py).

On these fixtures every tensor a kernel rounds to bf16 / half is already such a number and every fp32 sum is exact, so ONE float64
evaluation of the oracle is the answer of every precision mode, every kernel cut (head_fused_h16, head_chain_h16, head_fused_wide_h16)
and every `head_route` bit.  Everything but the final fp32 residual add is exact, so the bound is

    max |got - want| <= 1e-5 * max(1, max |want|)

-- a hundred fp32 ulps of the output scale, several thousand times tighter than the 0.05 x scale of the tests on random weights and far
below what one dropped weight unit moves (test_head_exact_host.py prints those ratios).  A failure here is a defect of a kernel or of its
packing, not noise.  Each run asserts through hip_ops.profile (and, for the wide cut, PackedHead.route_code) that the intended kernel ran.

Left out on purpose: the fp32 default route at C = 64 from 512 LR pixels on builds the logit table by Winograd transforms, which multiply
by sixths and are not exact; the fp32 control therefore runs HEAD_TABLE_GEMM, HEAD_NO_LOGIT_TABLE and HEAD_STAGED.  The x3 modes keep an
fp32 table and would take the same Winograd route at C = 64: they run with HEAD_TABLE_GEMM, and once more without it on the 'onehot'
fixture, where the transform's rounding (1e-6 of a logit) cannot move a softmax whose gaps are whole multiples of 1024."""
import pytest
import torch

from tests import exact_head as eh

pytestmark = pytest.mark.gpu

BOUND = eh.GPU_BOUND
FIXTURES = eh.CASES
PREFIX_Q = eh.PREFIX[1]                                   # 5000 % 64 = 8, and the prefix ends inside a grid row
MODES = ['bf16', 'bf16-single', 'bf16x3', 'f16', 'f16-pairs', 'f16x3', 'f16x3-fast']
CHAIN_SUFFIX = {'f16': '_f16', 'f16-pairs': '_pairs_f16', 'bf16': '_pairs_bf16', 'bf16-single': '_bf16'}
X3 = ('bf16x3', 'f16x3', 'f16x3-fast')

_gens = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _half_of(mode):
    return 'bf16' if mode.startswith('bf16') else 'f16'


def _setup(dev, name, Q=None):
    """(generator on the device, fixture checked for both 16-bit types): one generator per fixture name, shared by every test (the
    bf16-single pack calibrates once per generator)."""
    from tests.test_hip_parity import _my_generator
    fx = eh.case(name, 'both', Q)
    if name not in _gens:
        _gens[name] = _my_generator(fx.C, eh.HIDDEN, fx.params, dev, eval_bsize=30000)
    return _gens[name], fx


def _x_lr(fx, kind, dev):
    if kind is None:
        return None, None
    H, W = fx.hw
    if kind == 'zeros':
        x = torch.zeros(1, 3, H, W)
    else:
        x = torch.randint(-3, 4, (1, 3, H, W), generator=torch.Generator().manual_seed(7)).float()
    return x.to(dev), eh.residual64(x, fx.coord)


def _run(g, fx, dev, opt, x_kind=None, hinted=False, chunk=30000, ran=(), not_ran=(), label=''):
    """One _predict against the float64 expectation; returns the error.  `hinted`: the coordinates from hip_ops.make_coord_cell (the
    traversal hint of the chained kernels), else the fixture's own tensors in index order."""
    from ciaosr_amd import hip_ops
    if hinted:
        hc, hl = hip_ops.make_coord_cell(fx.target[0], fx.target[1], dev)
        coord, cell = hc.unsqueeze(0), hl.unsqueeze(0)
        assert torch.equal(coord.cpu(), fx.coord) and torch.equal(cell.cpu(), fx.cell) and hip_ops.grid_width_of(coord[0]) == fx.target[1]
    else:
        coord, cell = fx.coord.to(dev), fx.cell.to(dev)
        assert hip_ops.grid_width_of(coord[0]) == 0
    x, res = _x_lr(fx, x_kind, dev)
    with hip_ops.profile():
        got = g._predict([fx.feat.to(dev)], coord, cell, chunk, x, opt).cpu()
    prof = hip_ops.profile.results()
    starts = lambda t: any(k == t or (t.endswith('*') and k.startswith(t[:-1])) for k in prof)
    missing, extra = [t for t in ran if not starts(t)], [t for t in not_ran if starts(t)]
    assert not missing and not extra, f'{label} {opt}: expected tags missing {missing}, unexpected tags present {extra}; ran {sorted(prof)}'
    want = fx.want if res is None else fx.want + res
    scale = max(1.0, want.abs().max().item())
    err, where = eh.worst_query(got, want)
    print(f'{label} {opt}: max|hip - float64| = {err:.3e} (bound {BOUND * scale:.3e}, scale {scale:.2f}; worst at {where})')
    assert torch.isfinite(got).all(), f'{label} {opt}: non-finite output'
    assert err <= BOUND * scale, f'{label} {opt}: {err:.3e} > {BOUND * scale:.3e} at {where}: got {got[0, int(where.split()[1])].tolist()}, ' \
                                 f'want {want[0, int(where.split()[1])].tolist()}'
    return err


def _table_tag(mode, C):
    """The logit table's GEMM: on the 16-bit MFMA where D = 9 C is a multiple of 8 (C = 64; not D = 1620) and the mode is no x3 one."""
    return 'head_logit_table' if (mode in X3 or (9 * C) % 8) else 'head_logit_table_' + _half_of(mode)


def _default_tags(mode, C):
    """(ran, not_ran) of the default route of a 16-bit mode."""
    prec = _half_of(mode)
    if mode in X3:
        return (f'head_kv_fused_{prec}x3', f'head_decode_fused_{prec}x3', 'head_logit_table'), ('head_kv_chain*', 'head_decode_chain*')
    sfx = CHAIN_SUFFIX[mode]
    if C == 64:
        return ('head_kv_chain' + sfx, 'head_decode_chain' + sfx, _table_tag(mode, C)), ('head_decode_fused*',)
    return ('head_kv_chain' + sfx, 'head_decode_fused_' + prec, _table_tag(mode, C)), ('head_decode_chain*',)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_every_16bit_mode_on_the_default_route(dev, name, mode):
    """All seven modes, both regimes, both tail families, C = 64 (chained kv + chained decode) and C = 180 (chained kv + 128-row decode;
    the x3 modes: the wide kernels), on the whole grid with the traversal hint and small-integer LR pixels under the bilinear residual."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd._lib import HEAD_TABLE_GEMM
    g, fx = _setup(dev, name)
    ran, not_ran = _default_tags(mode, fx.C)
    if mode in X3 and fx.C == 64:
        _run(g, fx, dev, hip_ops.Options(mode, head_route=HEAD_TABLE_GEMM), 'ints', hinted=True, ran=ran, not_ran=not_ran + ('head_logit_table_w*',), label=name)
        if fx.regime == 'onehot':
            _run(g, fx, dev, hip_ops.Options(mode), 'ints', hinted=True, ran=ran[:2] + ('head_logit_table_w4',), not_ran=not_ran, label=name)
    else:
        _run(g, fx, dev, hip_ops.Options(mode), 'ints', hinted=True, ran=ran, not_ran=not_ran, label=name)


def _route_cases():
    from ciaosr_amd._lib import HEAD_NO_CHAIN, HEAD_NO_DECODE_CHAIN, HEAD_NO_LOGIT_TABLE, HEAD_WIDE_WG
    return {'no_decode_chain': HEAD_NO_DECODE_CHAIN, 'no_chain': HEAD_NO_CHAIN, 'no_table': HEAD_NO_LOGIT_TABLE,
            'no_decode_chain+no_table': HEAD_NO_DECODE_CHAIN | HEAD_NO_LOGIT_TABLE, 'no_chain+no_table': HEAD_NO_CHAIN | HEAD_NO_LOGIT_TABLE,
            'wide': HEAD_WIDE_WG, 'wide+no_table': HEAD_WIDE_WG | HEAD_NO_LOGIT_TABLE}


@pytest.mark.parametrize('route', ['no_decode_chain', 'no_chain', 'no_table', 'no_decode_chain+no_table', 'no_chain+no_table', 'wide', 'wide+no_table'])
@pytest.mark.parametrize('name', list(FIXTURES))
def test_route_bits(dev, name, route):
    """HEAD_NO_DECODE_CHAIN (chained kv, 128-row decode), HEAD_NO_CHAIN (the 128-row kernels), HEAD_NO_LOGIT_TABLE (imnet_k's output
    layer on the MFMA per row; no table, hence no chained kernel) alone and combined, in every mode; HEAD_WIDE_WG (the 256-row cut) for
    'f16' and 'f16-pairs', alone and without the table.  No LR image (no residual): the comparison is exact but for fp32 conversions."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd._lib import HEAD_TABLE_GEMM
    bits = _route_cases()[route]
    wide, table = route.startswith('wide'), 'no_table' not in route
    for mode in (('f16', 'f16-pairs') if wide else MODES):
        g, fx = _setup(dev, name)
        prec = _half_of(mode)
        b = bits | (HEAD_TABLE_GEMM if (mode in X3 and fx.C == 64) else 0)
        opt = hip_ops.Options(mode, head_route=b)
        if mode in X3:
            ran, not_ran = (f'head_kv_fused_{prec}x3', f'head_decode_fused_{prec}x3'), ('head_kv_chain*', 'head_decode_chain*')
        elif wide or route.startswith('no_chain') or not table:
            ran, not_ran = (f'head_kv_fused_{prec}', f'head_decode_fused_{prec}'), ('head_kv_chain*', 'head_decode_chain*')
        else:                                           # no_decode_chain
            ran, not_ran = ('head_kv_chain' + CHAIN_SUFFIX[mode], f'head_decode_fused_{prec}'), ('head_decode_chain*',)
        ran += (_table_tag(mode, fx.C),) if table else ()
        not_ran += () if table else ('head_logit_table*',)
        kernel = (g._head.route_code(fx.hw[0], fx.hw[1], fx.Q, opt) >> 6) & 3
        assert kernel == (2 if (wide or mode in X3) else 1), (route, mode, kernel)      # HeadKernel: 1 = the 128-row cut, 2 = the wide cut
        _run(g, fx, dev, opt, None, hinted=True, ran=ran, not_ran=not_ran, label=f'{name} {route}')


@pytest.mark.parametrize('name', ['c64-dyadic-onehot', 'c64-ragged-onehot', 'c180-dyadic-onehot', 'c180-ragged-onehot', 'c64-dyadic-uniform'])
def test_traversal_and_chunking(dev, name):
    """The same grid as the caller's own tensors (index order: the chained kernel without its traversal hint, or -- where a row tile
    leaves its key window -- its flagged fallback to the 128-row kernel: either tag, the same answer), a prefix of the grid with Q not a
    multiple of 64, and eval_bsize = 1000 < Q (a chunk boundary inside a grid row).  LR pixels all zero under the residual."""
    from ciaosr_amd import hip_ops
    for mode in ('bf16', 'bf16-single', 'f16', 'f16-pairs'):
        g, fx = _setup(dev, name)
        kv = 'head_kv_chain' + CHAIN_SUFFIX[mode]
        _run(g, fx, dev, hip_ops.Options(mode), 'zeros', hinted=False, ran=(kv,), label=f'{name} own tensors')
        _run(g, fx, dev, hip_ops.Options(mode), 'zeros', hinted=True, chunk=1000, ran=(kv,), label=f'{name} eval_bsize 1000')
        _run(g, fx, dev, hip_ops.Options(mode), 'zeros', hinted=False, chunk=1000, ran=(kv,), label=f'{name} own tensors, eval_bsize 1000')
    if name == eh.PREFIX[0]:
        for mode in MODES:
            g, fx = _setup(dev, name, Q=PREFIX_Q)
            assert fx.Q == PREFIX_Q and fx.Q % 64
            _run(g, fx, dev, hip_ops.Options(mode), 'zeros', hinted=False, label=f'{name} prefix of {fx.Q}')


@pytest.mark.parametrize('name', list(FIXTURES))
def test_fp32_control(dev, name):
    """The fp32 kernels on the same fixtures to the same bound: the 576-deep table GEMM, no table, and the staged route."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd._lib import HEAD_TABLE_GEMM, HEAD_NO_LOGIT_TABLE, HEAD_STAGED
    g, fx = _setup(dev, name)
    _run(g, fx, dev, hip_ops.Options(head_route=HEAD_TABLE_GEMM), 'ints', ran=('head_kv_fused', 'head_decode_fused', 'head_logit_table'),
         not_ran=('head_logit_table_w*', 'head_qk_maps'), label=f'{name} fp32 table gemm')
    _run(g, fx, dev, hip_ops.Options(head_route=HEAD_NO_LOGIT_TABLE), 'ints', ran=('head_kv_fused', 'head_decode_fused'), not_ran=('head_logit_table*',),
         label=f'{name} fp32 no table')
    _run(g, fx, dev, hip_ops.Options(head_route=HEAD_STAGED), 'ints', ran=('head_rows', 'local_attention'), not_ran=('head_kv_fused*',), label=f'{name} fp32 staged')


def test_the_bound_has_teeth(dev):
    """The comparison itself, on the GPU: a head whose decode input layer lacks its last 8 columns (Dv = 1800: the ragged last MFMA step)
    and one whose imnet_v lacks the layer-0 tail term, run through the default f16 / bf16 kernels and held against the UNMUTATED
    expectation, miss the bound by three orders of magnitude -- what a kernel that dropped those terms would do."""
    from ciaosr_amd import hip_ops
    from tests.test_hip_parity import _my_generator
    fx = eh.case('c180-dyadic-onehot')
    for label, key, cols in (('last 8 input columns of imnet_q layer 0', 'imnet_q.layers.0.weight', 8), ('tail term of imnet_v layer 0', 'imnet_v.layers.0.weight', 4)):
        P = {k: v.clone() for k, v in fx.params.items()}
        P[key][:, -cols:] = 0
        g = _my_generator(fx.C, eh.HIDDEN, P, dev, eval_bsize=30000)
        for mode in ('f16', 'bf16'):
            got = g._predict([fx.feat.to(dev)], fx.coord.to(dev), fx.cell.to(dev), 30000, None, hip_ops.Options(mode)).cpu()
            err, where = eh.worst_query(got, fx.want)
            print(f'{label} zeroed, {mode}: max|hip - float64 of the intact head| = {err:.3f} = {err / (BOUND * fx.scale):.2e} x the bound (worst at {where})')
            assert err >= 1e3 * BOUND * fx.scale, (label, mode, err)
