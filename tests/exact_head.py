"""Head fixtures on which 16-bit arithmetic is exact, and their float64 answer (CPU only; shares no code with the HIP kernels).

The argument.  The fused head (imnet_k / imnet_v -> 4-way attention -> imnet_q) rounds to bf16 / IEEE half at a known set of tensors: the
unfold rows U, the (q * key) rows of the logit-table GEMM, every post-ReLU hidden activation, Z, and the weights.  `exact_head` builds
heads and feature maps for which every one of those tensors already IS a bf16 (and so a half) number, and every fp32 sum is a sum of
multiples of one power of two whose absolute terms add up to less than 2^24 of that unit -- so no order of summation, no hi + lo split,
no error-feedback rounding, no calibrated bias (dW = 0) and no choice between a table and an MFMA output layer can change a bit.  One
float64 evaluation of oracle.ciaosr_oracle.query_rgb is then the answer of every precision mode, every kernel cut and every route, and a
dropped or misplaced term is wrong by a whole weight unit.  What is NOT exact is the final fp32 add of the bilinear residual, hence the
bound of test_head_exact_gpu.py:   max |got - want| <= 1e-5 * max(1, max |want|).

How the fixtures get there.
  features   channel 0 is a position code px (y % py) + (x % px) - 1 (CODE below), channel 1 is all ones, the rest are sparse draws of
             {-1, 1, 2}.
  weights    sparse and ternary (every input column of every layer is read by at least one row), times a power of two where needed,
             small integer biases: bf16(w) == w, every `lo` fragment is zero.
  'onehot'   imnet_k's output layer is scaled by LOGIT_UNIT = 1024.  (The issue's 64 leaves exp(-64) = 1.6e-28, which is not 0 in fp32;
             exp(-1024) underflows in fp32 AND in float64, so the runner-up's probability IS 0 and the winner's IS 1 on the GPU and in
             the reference alike.)  A logit is 1024 * (mul * s + code + 1): s comes from the general sparse layers (a handful of live
             output rows, so that it stays within a few units), code + 1 in 0 .. mul - 1 travels through one dedicated unit per layer
             from the key pixel's channel 0 to the output row of (channel 1, centre tap), where q * key = 1.  The key pixels of a query
             carry different codes, so logits of different key pixels always differ, and whenever s ties between the two best the
             runner-up is often exactly one unit away -- for 34 .. 56 % of the queries (asserted: >= 20 %), so a logit that is wrong by one
             unit changes the answer.  (At the map's border the clamp makes two samples read the same pixel: they then have the same
             logit AND the same value row, so their (1/2, 1/2) is as exact as (1, 0).)
  'uniform'  imnet_k's output layer is zero: attention exactly 1/4, Z the mean of four val * wv rows (multiples of 1/4).
  'dyadic'   LR map and target grid are powers of two, so coord, cell, rel * H, cell * H are exact in fp32; the four tail columns of
             layer 0 carry +-(target / map) so that tail terms are integers.
  'zero'     tail columns zero: ragged maps and arbitrary grids, the coordinates only select keys.
  cs_attn    every weight zero and `down.bias` = 6 * beta_c: scores 0, a uniform softmax over zero values, so the non-local map is
             beta_c (small integers, constant over the map) after the reference's division by 6 -- exactly, in fp32 and float64
             (checked here on the CPU).  The Dv = 9 C + Cn layout, imnet_v's Cn output rows and imnet_q's Cn input columns (the ragged
             last 8-column chunk at C = 180) are therefore live.

What these fixtures deliberately do not cover: the spatial variation of the non-local columns (a per-channel constant here; cs_attn's
own values are held by test_csattn_oracle_gpu.py and the PSNR tests), the Winograd logit table of the fp32 default route (it multiplies
by sixths and is not exact), and rounding behaviour on real-valued data, which stays with the PSNR-bounded tests of test_hip_parity.py.

`exact_head` checks its own output with a hooked float64 evaluation (oracle.mlp and oracle._nearest replaced by recording
restatements): round_to(half)(t) == t for U, q * key, every hidden activation and Z; every pre-activation, logit and table entry a
multiple of its unit with sum |terms| < 2^24 units.  A fixture that fails is a builder bug (other seed, other sparsity), never a tolerance.

Measured on an MI355X over the 465 runs of test_head_exact_gpu.py (output scale 16.5 .. 88.5, bound 1e-5 x scale), worst |got - want|:
  bf16, bf16-single, bf16x3, f16, f16-pairs, f16x3, f16x3-fast, fp32 control -- every mode alike:
    0.0 (bitwise the float64 answer) on every run without an LR image, with an all-zero one, and on every dyadic grid;
    1.155e-05 (C = 64, 21 x 30 -> 59 x 83) and 5.0e-06 (C = 180, 12 x 16 -> 40 x 53) on the ragged grids with integer LR pixels: the
    fp32 bilinear residual alone, the same figure in every mode, cut and route; at most 6.4e-7 x scale = 1/15 of the bound.
No kernel defect was found; test_the_bound_has_teeth shows on the GPU what a dropped term does to the same comparison.
"""
import contextlib
from collections import namedtuple

import torch

from oracle import ciaosr_oracle as orc
from tests.helpers import head_shapes

LOGIT_UNIT = 1024.0
HIDDEN = (256,) * 4
CODE_COL = 0 * 9 + 4        # reference unfold order c * 9 + tap: channel 0 (position code), centre tap
ONES_COL = 1 * 9 + 4        # channel 1 (all ones), centre tap
TWO24 = float(1 << 24)
# per MLP: entries per row beyond the column cover in layer 0 / in the hidden layers / in the output layer, number of output rows that are
# not zero (0: all), range of the hidden biases
KNOBS = {'k': (1, 1, 1, 6, -1, 0), 'v': (1, 1, 1, 0, 0, 1), 'q': (0, 1, 24, 0, 0, 1)}
# the position code of channel 0: period (py, px), code = px * (y % py) + (x % px) < mul; a logit is LOGIT_UNIT * (mul * s + code).
# Period 2 tells the four pixels of a 2 x 2 block apart, which is what the keys of a query form on a dyadic grid; on a ragged grid a query
# near a pixel centre has keys TWO pixels apart (the shift is a little more than half a pixel each way), which takes period 3
CODE = {'dyadic': (2, 2, 4.0), 'zero': (3, 3, 16.0)}

# the cases of test_head_exact_gpu.py: name -> (C, LR map, target grid, regime, tail)
CASES = {
    'c64-dyadic-onehot': (64, (16, 32), (64, 128), 'onehot', 'dyadic'),
    'c64-dyadic-uniform': (64, (16, 32), (64, 128), 'uniform', 'dyadic'),
    'c64-ragged-onehot': (64, (21, 30), (59, 83), 'onehot', 'zero'),
    'c64-ragged-uniform': (64, (21, 30), (59, 83), 'uniform', 'zero'),
    'c180-dyadic-onehot': (180, (8, 16), (32, 64), 'onehot', 'dyadic'),
    'c180-dyadic-uniform': (180, (8, 16), (32, 64), 'uniform', 'dyadic'),
    'c180-ragged-onehot': (180, (12, 16), (40, 53), 'onehot', 'zero'),
    'c180-ragged-uniform': (180, (12, 16), (40, 53), 'uniform', 'zero'),
}
PREFIX = ('c64-dyadic-onehot', 5000)     # the first 5000 queries of that grid: 5000 % 64 = 8, and the prefix ends inside a grid row
GPU_BOUND = 1e-5                         # test_head_exact_gpu.py: max |got - want| <= GPU_BOUND * max(1, max |want|)

Fixture = namedtuple('Fixture', 'C hw target Q regime tail params feat coord cell want scale figures rec')


def round_to(half):
    """x -> x rounded to bf16 / IEEE half, kept in x's dtype (via fp32: every value checked here is an fp32 number)."""
    t = torch.bfloat16 if half == 'bf16' else torch.float16
    return lambda v: v.float().to(t).to(v.dtype)


# ------------------------------------------------------------------------------------------------
# the builder
# ------------------------------------------------------------------------------------------------
def _ternary(g, rows, cols, per_row, cover=True):
    """[rows][cols] of {-1, 0, 1}: `per_row` random entries per row and, with `cover`, one more per column in a random row."""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    sign = lambda n: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    if cover:
        w[torch.randint(0, rows, (cols,), generator=g), torch.arange(cols)] = sign(cols)
    for _ in range(per_row):
        w[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = sign(rows)
    return w


def _features(g, C, hw, p_nz, code):
    H, W = hw
    u = torch.rand(C, H, W, generator=g)
    f = torch.zeros(C, H, W, dtype=torch.float64)
    f[u < p_nz] = 1.0
    f[u < 0.55 * p_nz] = -1.0
    f[u < 0.20 * p_nz] = 2.0
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    f[0] = (code[1] * (yy % code[0]) + (xx % code[1]) - 1).double()
    f[1] = 1.0
    return f.unsqueeze(0)


def _mlp_params(g, prefix, in_dim, out_dim, n_tail, tail_unit, first_per_row, hid_per_row, out_per_row, out_rows, bias_lo, bias_hi):
    """Sparse ternary MLPRefiner parameters (reference names).  The last `n_tail` input columns of layer 0 are the tail (rel_y, rel_x,
    scale_y, scale_x): +-tail_unit in one of them for half of the rows, or zero."""
    P = {}
    body = in_dim - n_tail
    w0 = torch.zeros(256, in_dim, dtype=torch.float64)
    w0[:, :body] = _ternary(g, 256, body, first_per_row)
    if n_tail and tail_unit:
        rows = torch.nonzero(torch.rand(256, generator=g) < 0.5)[:, 0]
        cols = body + torch.randint(0, n_tail, (rows.numel(),), generator=g)
        w0[rows, cols] = (torch.randint(0, 2, (rows.numel(),), generator=g) * 2 - 1).double() * tail_unit
    P[f'{prefix}.layers.0.weight'] = w0
    P[f'{prefix}.layers.0.bias'] = torch.randint(bias_lo, bias_hi + 1, (256,), generator=g).double()
    for n in range(1, len(HIDDEN)):
        P[f'{prefix}.layers.{2 * n}.weight'] = _ternary(g, 256, 256, hid_per_row)
        P[f'{prefix}.layers.{2 * n}.bias'] = torch.randint(bias_lo, bias_hi + 1, (256,), generator=g).double()
    wl = _ternary(g, out_dim, 256, out_per_row, cover=False)
    if out_rows:
        wl[torch.randperm(out_dim, generator=g)[out_rows:]] = 0.0
    P[f'{prefix}.layers.{2 * len(HIDDEN)}.weight'] = wl
    bl = torch.randint(-1, 2, (out_dim,), generator=g).double()
    bl[wl.abs().sum(1) == 0] = 0.0
    P[f'{prefix}.layers.{2 * len(HIDDEN)}.bias'] = bl
    return P


def _params(g, C, regime, tail_unit, code_mul):
    D, Cn = 9 * C, C
    Dv = D + Cn
    P = {}
    # imnet_k: few active output rows and small hidden values keep s = sum_d (q key)_d wk_d within a few units
    P.update(_mlp_params(g, 'imnet_k', D + 4, D, 4, tail_unit, *KNOBS['k']))
    P.update(_mlp_params(g, 'imnet_v', Dv + 4, Dv, 4, tail_unit, *KNOBS['v']))
    P.update(_mlp_params(g, 'imnet_q', Dv, 3, 0, 0.0, *KNOBS['q']))
    last = 2 * len(HIDDEN)
    if regime == 'uniform':
        P[f'imnet_k.layers.{last}.weight'].zero_()
        P[f'imnet_k.layers.{last}.bias'].zero_()
    else:
        # the dedicated unit 0 of every layer carries code + 1 from the key's channel 0 to the output row of (channel 1, centre tap)
        for n in range(len(HIDDEN)):
            w, b = P[f'imnet_k.layers.{2 * n}.weight'], P[f'imnet_k.layers.{2 * n}.bias']
            w[0] = 0.0
            w[0, CODE_COL if n == 0 else 0] = 1.0
            b[0] = 1.0 if n == 0 else 0.0
        w5, b5 = P[f'imnet_k.layers.{last}.weight'], P[f'imnet_k.layers.{last}.bias']
        w5 *= code_mul
        b5 *= code_mul
        w5[ONES_COL] = 0.0
        w5[ONES_COL, 0] = 1.0
        b5[ONES_COL] = 0.0
        w5 *= LOGIT_UNIT
        b5 *= LOGIT_UNIT
    # cs_attn: all zero but down.bias = 6 beta_c, beta_c in {-1, 1, 2}: the non-local map is exactly beta_c
    for k, shape in head_shapes(C, HIDDEN, True).items():
        if k.startswith('cs_attn.'):
            P[k] = torch.zeros(shape, dtype=torch.float64)
    P['cs_attn.escape_NaN'] = torch.tensor([1e-4]).double()
    beta = torch.tensor([-1.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    P['cs_attn.down.bias'] = 6.0 * beta
    assert set(P) == set(head_shapes(C, HIDDEN, True)), sorted(set(P) ^ set(head_shapes(C, HIDDEN, True)))
    return P


def queries_of(target, Q=None):
    """(coord, cell) [1, Q, 2] float32 of the target grid, or of its first Q queries in index order."""
    coord, cell = orc.make_coord(target).unsqueeze(0), orc.make_cell(target).unsqueeze(0)
    return (coord, cell) if Q is None else (coord[:, :Q].contiguous(), cell[:, :Q].contiguous())


# ------------------------------------------------------------------------------------------------
# the hooked float64 evaluation
# ------------------------------------------------------------------------------------------------
class Record:
    """What the hooked oracle saw: per MLP prefix the list of calls (input, pre-activations, output), and per sample the key index."""

    def __init__(self):
        self.mlp = {'imnet_k': [], 'imnet_v': [], 'imnet_q': []}
        self.key_idx = []
        self.rows = []          # the first _nearest call's rows: the query's unfold rows


@contextlib.contextmanager
def _hooked(rec):
    keep_mlp, keep_nearest = orc.mlp, orc._nearest

    def mlp(x, params, prefix, act=None):
        assert act is None
        ids = orc.mlp_layer_ids(params, prefix)
        h = x.reshape(-1, x.shape[-1])
        pre = []
        for n, i in enumerate(ids):
            w, b = params[f'{prefix}.layers.{i}.weight'], params[f'{prefix}.layers.{i}.bias']
            mag = h.abs() @ w.abs().t() + b.abs()           # sum of |terms|: bounds every partial sum in every order
            h = h @ w.t() + b
            pre.append((h, mag.max().item()))
            if n + 1 < len(ids):
                h = torch.relu(h)
        rec.mlp[prefix].append((x.reshape(-1, x.shape[-1]), pre, h))
        return h.reshape(*x.shape[:-1], -1)

    def nearest(fmap, coord):
        out = keep_nearest(fmap, coord)
        if not rec.rows:
            rec.rows.append(out)
        if fmap.shape[1] == 2:                             # the key-coordinate lookup: same coordinates on an index map
            H, W = fmap.shape[-2:]
            idx = torch.arange(H * W, dtype=fmap.dtype).view(1, 1, H, W).expand(fmap.shape[0], 1, H, W)
            rec.key_idx.append(keep_nearest(idx, coord)[..., 0].long())
        return out

    orc.mlp, orc._nearest = mlp, nearest
    try:
        yield
    finally:
        orc.mlp, orc._nearest = keep_mlp, keep_nearest


def reference64(params, feat, coord, cell, rec=None):
    """oracle.query_rgb on float64 copies -> (out [1, Q, 3], intermediates); `rec`: a Record to fill."""
    P = {k: v.double() for k, v in params.items()}
    with torch.no_grad(), _hooked(rec) if rec is not None else contextlib.nullcontext():
        return orc.query_rgb(feat.double(), coord.double(), cell.double(), P, return_intermediates=True)


def finish(rec, params, key=None, wk=None, val=None, wv=None, queries=None, samples=None):
    """The head behind the two MLPs, restated from a Record: logits, softmax, Z, imnet_q.  `key` replaces the recorded key rows in the
    logit's product; `samples` [n] reads the key, wk, val and wv rows of those queries instead of the queries' own; `queries` [n]
    restricts the evaluation to those queries (the mutations of the sharpness tests).  Returns (out [n, 3], logit [n, 4], attn [n, 4],
    z [n, Dv])."""
    q = rec.rows[0][0]                                                               # [Q, D]
    Q, D = q.shape
    queries = torch.arange(Q) if queries is None else queries
    samples = queries if samples is None else samples
    q = q[queries]
    key = torch.stack([c[0][samples, :D] for c in rec.mlp['imnet_k']], 1) if key is None else key[samples]      # [n, 4, D]
    val = torch.stack([c[0][samples, :-4] for c in rec.mlp['imnet_v']], 1)                                      # [n, 4, Dv]
    wk = torch.stack([c[2][samples] for c in rec.mlp['imnet_k']], 1)
    wv = torch.stack([c[2][samples] for c in rec.mlp['imnet_v']], 1)
    logit = (q.unsqueeze(1) * key * wk).sum(-1)
    attn = logit.softmax(-1)
    z = (attn.unsqueeze(-1) * (val * wv)).sum(1)
    P = {k: v.double() for k, v in params.items() if k.startswith('imnet_q')}
    return orc.mlp(z, P, 'imnet_q'), logit, attn, z


def _is_multiple(t, unit):
    return bool((torch.round(t / unit) * unit == t).all())


def check_exact(fx, half):
    """The exactness assertions on a fixture, for the 16-bit type `half` ('both': bf16 and f16).  Returns a dict of figures (one-unit
    share, maxima)."""
    halves = ('bf16', 'f16') if half == 'both' else (half,)
    rec, P = fx.rec, fx.params
    C, (H, W) = fx.C, fx.hw
    D, Dv = 9 * C, 10 * C

    def same(name, t):
        for h in halves:
            r = round_to(h)(t)
            assert torch.equal(r, t), f'{name} is not exact in {h}: worst |round(t) - t| = {(r - t).abs().max().item():.3e}'

    for k, v in P.items():
        if k.startswith('imnet'):
            same(k, v)
    feat64 = fx.feat.double()
    U = torch.nn.functional.unfold(feat64, 3, padding=1)[0].t()                      # [HW, D], reference column order
    same('U', U)
    nl = orc.cross_scale_attention(feat64, {k: v.double() for k, v in P.items()})
    beta = (P['cs_attn.down.bias'].double() / 6.0).view(1, C, 1, 1).expand_as(nl)
    assert torch.equal(nl, beta), 'non-local map is not the constant beta_c in float64'
    nl32 = orc.cross_scale_attention(fx.feat.float(), {k: v.float() for k, v in P.items()})
    assert torch.equal(nl32.double(), beta), 'non-local map is not the constant beta_c in float32'
    same('non-local map', nl)
    unit = LOGIT_UNIT if fx.regime == 'onehot' else 1.0
    fig = {}
    for prefix in ('imnet_k', 'imnet_v', 'imnet_q'):
        for x, pre, out in rec.mlp[prefix]:
            nt = 4 if (prefix != 'imnet_q' and fx.tail == 'zero') else 0          # zero-weighted tail columns: rel of a ragged grid is not exact
            same(prefix + ' input', x[:, :x.shape[1] - nt])
            for n, (h, mag) in enumerate(pre):
                u = 0.25 if prefix == 'imnet_q' else (unit if (prefix == 'imnet_k' and n == len(pre) - 1) else 1.0)
                assert _is_multiple(h, u), f'{prefix} layer {n}: pre-activation is not a multiple of {u}'
                assert mag / u < TWO24, f'{prefix} layer {n}: sum |terms| = {mag / u:.3e} units'
                if n + 1 < len(pre):
                    fig[f'{prefix}.h{n}.max'] = max(fig.get(f'{prefix}.h{n}.max', 0.0), h.max().item())
                    fig[f'{prefix}.h{n}.alive'] = (h > 0).double().mean().item()
                    same(f'{prefix} hidden {n}', torch.relu(h))
    out, logit, attn, z = finish(rec, P)
    assert torch.equal(out, fx.want[0]), 'the restated tail of the head differs from oracle.query_rgb'
    q = rec.rows[0][0]
    key = torch.stack([c[0][:, :D] for c in rec.mlp['imnet_k']], 1)
    wk = torch.stack([c[2] for c in rec.mlp['imnet_k']], 1)
    wv = torch.stack([c[2] for c in rec.mlp['imnet_v']], 1)
    val = torch.stack([c[0][:, :-4] for c in rec.mlp['imnet_v']], 1)
    same('q * key (sampled)', q.unsqueeze(1) * key)
    same('wv', wv)
    same('val * wv', val * wv)
    same('Z', z)
    assert _is_multiple(logit, unit) and ((q.unsqueeze(1) * key * wk).abs().sum(-1).max().item() / unit) < TWO24
    # the whole logit table: one row per (LR pixel, 3 x 3 key offset), G = (q * key) . W5 and the bias term (q * key) . b5
    last = 2 * len(HIDDEN)
    w5, b5 = P[f'imnet_k.layers.{last}.weight'].double(), P[f'imnet_k.layers.{last}.bias'].double()
    Um = U.view(H, W, D)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            a = Um[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
            b = Um[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)]
            qk = (a * b).reshape(-1, D)
            same('q * key (table operand)', qk)
            G = qk @ w5
            assert _is_multiple(G, unit) and _is_multiple(qk @ b5, unit)
            assert (qk.abs() @ w5.abs()).max().item() / unit < TWO24
            fig['table.max'] = max(fig.get('table.max', 0.0), G.abs().max().item() / unit)
    fig['logit.max'] = logit.abs().max().item() / unit
    fig['z.max'] = z.abs().max().item()
    kidx = torch.stack([k[0] for k in rec.key_idx], 1)                               # [Q, 4]
    if fx.regime == 'uniform':
        assert torch.equal(logit, torch.zeros_like(logit)) and torch.equal(attn, torch.full_like(attn, 0.25))
    else:
        # equal logits only where two samples read the same key pixel; the runner-up among the distinct ones
        eq_logit = logit.unsqueeze(1) == logit.unsqueeze(2)
        eq_key = kidx.unsqueeze(1) == kidx.unsqueeze(2)
        assert torch.equal(eq_logit, eq_key), 'two different key pixels of one query have the same logit'
        top = logit.max(1, keepdim=True).values
        second = torch.where(logit < top, logit, torch.full_like(logit, -float('inf'))).max(1).values
        gap = (top[:, 0] - second) / unit
        assert (gap >= 1).all()
        fig['one_unit_share'] = (gap == 1).double().mean().item()
        fig['distinct_keys_share'] = (eq_key.sum((1, 2)) == 4).double().mean().item()
        fig['winner_hist'] = [int(v) for v in torch.bincount(logit.argmax(1), minlength=4)]
    return fig


_cache = {}


def case(name, half='both', Q=None, keep_record=False):
    """exact_head of a CASES entry (Q: its first Q queries)."""
    C, hw, target, regime, tail = CASES[name]
    return exact_head(C, hw, target + ((Q,) if Q else ()), half, regime, tail, keep_record=keep_record)


def exact_head(C, hw, queries, half='both', regime='onehot', tail='dyadic', seed=0, keep_record=False):
    """The fixture: head parameters (reference state_dict names, float32, hidden (256,) * 4, cs_attn included), feature map [1, C, H, W],
    coord / cell [1, Q, 2] (float32) and the float64 expectation `want` [1, Q, 3] (no residual), with `scale` = max(1, max |want|).
    `queries` = (ht, wt) for the whole target grid or (ht, wt, Q) for its first Q queries.  The result has passed check_exact for
    `half` (its figures -- the one-unit share among them -- are in `figures`); fixtures are cached per argument set and must not be
    modified.  `keep_record`: return (uncached) the fixture with `rec`, the Record of the hooked evaluation, several hundred MB."""
    key = (C, tuple(hw), tuple(queries), half, regime, tail, seed)
    if key in _cache and not keep_record:
        return _cache[key]
    H, W = hw
    target, Q = tuple(queries[:2]), (queries[2] if len(queries) > 2 else None)
    if tail == 'dyadic':
        pow2 = lambda n: n & (n - 1) == 0
        assert all(pow2(v) for v in (H, W) + target) and target[0] >= H and target[1] >= W, 'dyadic: map and grid must be powers of two'
        tail_unit = float(max(target[0] // H, target[1] // W))
    else:
        assert tail == 'zero'
        tail_unit = 0.0
    g = torch.Generator().manual_seed(1000 * seed + C)
    feat = _features(g, C, hw, 0.25, CODE[tail])
    P64 = _params(g, C, regime, tail_unit, CODE[tail][2])
    coord, cell = queries_of(target, Q)
    rec = Record()
    want, _ = reference64(P64, feat, coord, cell, rec)
    fx = Fixture(C, (H, W), target, coord.shape[1], regime, tail, {k: v.float() for k, v in P64.items()}, feat.float(), coord, cell, want,
                 max(1.0, want.abs().max().item()), None, rec)
    for k, v in P64.items():
        assert torch.equal(fx.params[k].double(), v), k
    fx = fx._replace(figures=check_exact(fx, half))
    _cache[key] = fx._replace(rec=None)
    return fx if keep_record else _cache[key]


def residual64(x_lr, coord):
    """The bilinear residual of the generator's forward in float64: [1, Q, 3]."""
    return orc.bilinear_residual(x_lr.double(), coord.double())


def worst_query(got, want):
    """(max |got - want|, 'query q channel k') for [1, Q, 3] tensors."""
    d = (got.double() - want.double()).abs()[0]
    i = int(d.argmax())
    return d.max().item(), f'query {i // d.shape[1]} channel {i % d.shape[1]}'
