"""The fp32 fused head kernels in both workgroup shapes (kv_rows, decode_rows in {32, 64}) on the exact-arithmetic fixtures.

The automatic rules take the 64-row forms only from 32 768 (kv) and 131 009 (decode) queries on, which no other test reaches: here the
options ask for them on small inputs.  On the fixtures of tests/exact_head.py every fp32 sum is exact, so a misplaced table row, a
register read before its load arrived or a wrong chunk of Z shows at full size; the bound is that of test_head_exact_gpu.py,

    max |got - want| <= GPU_BOUND * max(1, max |want|)        (what is not exact is the final fp32 add of the bilinear residual).

Routes: HEAD_TABLE_GEMM (the logits from the logit table's rows) and HEAD_NO_LOGIT_TABLE (imnet_k's output layer on the MFMA).  Sizes: the whole ragged grids (4897 = 64 * 76 + 33 queries,
4897 % 16 = 1; 2120 at C = 180, where Dv = 1800 = 7 * 256 + 8 leaves decode a last chunk of 8 columns and n_out = 1620 a part-filled
last v-out unit) and prefixes of 1, 17, 63 and 65 queries: a last workgroup of one query, or one query past a full workgroup.  The
head builds a logit table only when 4 Q > 9 H W (head.hip, head_route), so under HEAD_TABLE_GEMM those short prefixes still take the MFMA
logits and the expected tags say so; the prefixes of 1425 (C = 64) and 449 (C = 180) queries are the short ones that do read the table:
1425 % 16 = 449 % 16 = 1.  Each (rows, route) runs with small-integer LR pixels -- the bilinear residual decode adds -- and without an
LR image.

On random weights nothing is exact, but a row's arithmetic does not depend on the workgroup's shape: the four (kv_rows, decode_rows)
pairs must agree bit for bit."""
import itertools

import pytest
import torch

from tests import exact_head as eh

pytestmark = pytest.mark.gpu

ROWS = list(itertools.product((32, 64), (32, 64)))          # (kv_rows, decode_rows)
SIZES = [('c64-ragged-onehot', None), ('c64-ragged-onehot', 1), ('c64-ragged-onehot', 17), ('c64-ragged-onehot', 63),
         ('c64-ragged-onehot', 65), ('c64-dyadic-uniform', 17), ('c64-dyadic-uniform', 65),
         ('c180-ragged-onehot', None), ('c180-ragged-onehot', 65), ('c180-dyadic-uniform', 65),
         ('c64-ragged-onehot', 1425), ('c180-ragged-onehot', 449)]
WITH_TABLE = {('c64-ragged-onehot', None), ('c180-ragged-onehot', None), ('c64-ragged-onehot', 1425), ('c180-ragged-onehot', 449)}
STAGED_TAGS = ('head_rows', 'local_attention', 'mlp_*', 'decode_residual')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _routes():
    from ciaosr_amd._lib import HEAD_TABLE_GEMM, HEAD_NO_LOGIT_TABLE
    return [('table gemm', HEAD_TABLE_GEMM, ('head_logit_table',), ('head_logit_table_w*', 'head_qk_maps')),
            ('no table', HEAD_NO_LOGIT_TABLE, (), ('head_logit_table*',))]


@pytest.mark.parametrize('name,Q', SIZES, ids=[f'{n}-{q or "whole"}' for n, q in SIZES])
def test_row_settings_on_exact_fixtures(dev, name, Q):
    from ciaosr_amd import hip_ops
    from tests.test_head_exact_gpu import _run, _setup
    g, fx = _setup(dev, name, Q)
    assert fx.Q == (Q or {'c64-ragged-onehot': 4897, 'c180-ragged-onehot': 2120}[name])
    table = 4 * fx.Q > 9 * fx.hw[0] * fx.hw[1]
    assert table == ((name, Q) in WITH_TABLE)
    for (kv, dec), (label, bits, ran, not_ran) in itertools.product(ROWS, _routes()):
        if not table:
            ran, not_ran = (), ('head_logit_table*',)
        opt = hip_ops.Options(head_route=bits, kv_rows=kv, decode_rows=dec)
        for x_kind in ('ints', None):
            _run(g, fx, dev, opt, x_kind, ran=('head_kv_fused', 'head_decode_fused') + ran, not_ran=STAGED_TAGS + not_ran,
                 label=f'{name} Q={fx.Q} {label} LR={x_kind}')


def test_workgroup_shapes_agree_bit_for_bit_on_random_weights(dev):
    from ciaosr_amd import hip_ops
    from ciaosr_amd._lib import HEAD_NO_LOGIT_TABLE
    from ciaosr_amd.coords import make_coord, make_cell
    from tests.helpers import randn, seeded_head
    from tests.test_hip_parity import _my_generator
    g = _my_generator(64, (256,) * 4, seeded_head(64, 3, head_gain=2.0), dev, eval_bsize=30000)
    feat = randn((1, 64, 21, 30), 11).to(dev)
    coord, cell = make_coord((59, 83)).unsqueeze(0).to(dev), make_cell((59, 83)).unsqueeze(0).to(dev)
    x = (randn((1, 3, 21, 30), 12) * 0.3).to(dev)
    for bits in (0, HEAD_NO_LOGIT_TABLE):                  # the default route (Winograd logit table) and the MFMA logits
        outs = {}
        for kv, dec in ROWS:
            with hip_ops.profile():
                outs[kv, dec] = g._predict([feat], coord, cell, 30000, x, hip_ops.Options(head_route=bits, kv_rows=kv, decode_rows=dec)).cpu()
            prof = hip_ops.profile.results()
            assert 'head_kv_fused' in prof and 'head_decode_fused' in prof, sorted(prof)
        ref = outs[32, 32]
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        for k, v in outs.items():
            assert torch.equal(v, ref), f'head_route={bits} rows {k}: differs from (32, 32) by {(v - ref).abs().max().item():.3e}'
