"""Encoder-trunk fixtures on which fp32 arithmetic is exact, and their float64 answer (CPU only; shares no code with the HIP kernels).

The argument.  Every fp32 trunk route -- the F(4x4, 3x3) and F(2x2, 3x3) Winograd dense layers, the halo-resident direct kernel, the two
scatter forms, the generic split-K convolution, the small-map 3x3 kernel, the 1x1 kernels, the EDSR resident kernel -- forms sums of
products of activations and (for Winograd: transformed) weights.  `check_exact` asserts, on a float64 re-evaluation of the fixture, that
every sum ANY of those routes can form has addends that are multiples of one power of two q and  sum |addends| < 2^22 q : every partial
sum in every order (split-K partials, K-sliced waves, the scatter accumulator, fused bias / residual / alpha epilogues, the two 1-D stages
of the Winograd transforms) is then an fp32 number with two bits to spare, no operation rounds, and ONE float64 evaluation is the answer
of every route: test_trunk_exact_gpu.py asserts torch.equal.  A dropped, misplaced or doubled term is wrong by a whole unit.

Why Winograd can be exact.  B^T and A^T are integer matrices; G g G^T is applied once at pack time in fp64 and rounded to fp32
(csrc/pack_ops.hip).  A weight 9 * 2^-j * {-1, 0, 1} with at most one non-zero tap per (output, input) channel pair makes
U = G g G^T dyadic (G4 = Gi4 / 24 with Gi4 integer: 9 / 576 = 1 / 64), and the fp64 pack with its rounded sixths rounds to exactly that
rational U (emulated and asserted here).  The matrices below are restated from the kernels' header comments.

How the fixtures get there.
  image      [B, 3, H, W] in {-1, 0, 1}; channel ch is non-zero only on the lattice (y % 3, x % 3) == psi_ch, there with probability P_NZ.
  stem       sfe1 / conv_first: one +-1 tap per row (all 27 columns read).  sfe2: nine +-1 taps per row, one per lattice phase (all 576
             columns read), so at every pixel at most ONE term is non-zero: the block input is in {-1, 0, 1}, P_NZ of it non-zero, away
             from the border; sfe1's bias (+-1 on BIASED = 4 channels) is compensated in sfe2's, so only border pixels (where the padding
             removes a bias term) leave that range, up to 3.
  feeders    dense layers below the probe: one tap of +-9/16 on group 0 (a permutation of its channels), bias -8/16 (a quarter of the
             rows: -7/16): the ReLU leaves {0, 1/16, 2/16} (10/16 .. at the few border pixels of magnitude 2): a spatially varying map one
             to two bits wide in units of 1/16.
  probe      dense layer l: TAPS = 16 taps per output row, at least one in each of its l + 1 input groups, never two on one (output, input)
             pair, every input channel read by some row; +-9/16 on the feeder groups, whose values are multiples of 1/16, and (for l > 0)
             +-9/256 on group 0, whose values are integers, so that all addends share the unit 9/256 -- with 9/16 on integers too the
             group-0 terms alone cost four bits and F(4x4) misses the condition; bias a small integer times the layer's unit.
  lff, gff   sparse ternary 1x1 / 3x3, every input column read, small integer biases.
  NB = 2     two blocks of two layers, 4 taps per probe row, sfe1's bias zero (block 1 must read integers of magnitude <= 5 everywhere).
             Block 0's probe has one tap per group and the bias -17/256: its ReLU leaves {0, 1/256}; block 0's lff scales the columns of
             each group back to integers (1, 16, 256), so block 1 reads a small-integer map again.
  mid 32     C = G = 32, two blocks of three layers on the generic route (no Winograd): the same shapes with weights +-1.
  EDSR       conv_first as sfe1; body and conv_after_body nine +-1 taps per row (every column read), times a power of two per layer;
             res_scale 0.25.

Reference mutations (`MUTATIONS`, for test_trunk_exact_host.py): what a kernel defect of each kind does to the float64 answer.

Host figures, worst log2(sum |addends| / q) over every fixture and map test_trunk_exact_gpu.py runs (asserted: < 22, of 24 available):
  probes (l = 0 .. 7, every map, B = 1 and 3)   direct 9 cin sum 8.3;  F(2x2): B^T d B 5.7, sum_c U V 9.7, A^T M A + bias 11.5;
                                                 F(4x4): 10.0, 17.7, 20.2;  lff + residual 11.1;  gff.1 + residual 13.3
  NB = 2                                         direct 8.7;  F(2x2) 6.7, 11.0, 12.3;  F(4x4) 10.6, 18.8, 21.2;  lff 11.6;  gff 13.6
  mid 32                                         direct 4.4;  lff 4.9;  gff 6.4
  EDSR                                           convolutions 11.5, with res + 0.25 (sum + bias) 12.0
The fp64 pack emulation rounds to the rational U on every dense layer; F(2x2) and F(4x4) evaluated in float64 equal the direct sum.

Measured on an MI355X (profiles/trunk_exact.txt), worst |got - want| over the runs of test_trunk_exact_gpu.py:
  F(4x4) forced (19 runs), F(2x2) forced (19), direct gather forced (19), scatter one-launch kernel (7), scatter step of conv_f32.hip (7),
  generic route at mid 32 (1), the (131, 253) map on the default route (1), EDSR per image (8), EDSR resident (8):   0.0 on every run --
  bitwise the float64 answer; no route needed a non-zero bound and no kernel or packing defect was found.  test_the_bound_has_teeth: one
  probe tap zeroed in the model moves every dense route 9 output units (1.3e-3 of the output scale) away from the unchanged answer.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

TWO22 = float(1 << 22)
W9 = 9.0 / 16.0                 # the Winograd-exact dense-layer weight
TAPS = 16                       # taps per output row of a probe layer
P_NZ = 0.4                      # share of an image channel's lattice sites that are non-zero
BIASED = 4                      # channels of the first convolution with a non-zero bias

# ---- the standard transform matrices, restated from the header comments of dense_wino_f32.hip / dense_wino4_f32.hip ----------------------
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
GI2 = torch.tensor([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], dtype=torch.float64)                    # G2 = GI2 / 2
G2 = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)
GI4 = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64)   # G4 = GI4 / 24
G4 = torch.tensor([[1.0 / 4, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6], [1.0 / 24, 1.0 / 12, 1.0 / 6],
                   [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1.0]], dtype=torch.float64)          # the double constants of the pack kernel
WINO = {2: (BT2, AT2, GI2, G2), 4: (BT4, AT4, GI4, G4)}

Fixture = namedtuple('Fixture', 'kind name hw B params x want scale unit res_scale')


# ------------------------------------------------------------------------------------------------
# units
# ------------------------------------------------------------------------------------------------
def unit_of(t):
    """The largest power of two that divides every element of t (inf for an all-zero tensor)."""
    t = t[t != 0].double()
    if t.numel() == 0:
        return math.inf
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return 2.0 ** int((e.to(torch.int64) - 53 + torch.log2(low).round().to(torch.int64)).min())


def _bits(mag, q):
    return -math.inf if mag == 0 else math.log2(mag / q)


class Figures(dict):
    """stage -> worst log2(sum |addends| / q) seen; `note` asserts the condition and records the figure."""

    def note(self, stage, mag, q, where=''):
        mag = float(mag)
        if mag == 0.0:
            return
        assert q > 0 and math.isfinite(q), (stage, where, q)
        assert mag < TWO22 * q, f'{stage} {where}: sum |addends| = 2^{_bits(mag, q):.2f} units of {q}: not below 2^22'
        self[stage] = max(self.get(stage, -math.inf), _bits(mag, q))


def _multiple(t, q):
    return q == math.inf and not t.any() or bool((torch.round(t / q) * q == t).all())


# ------------------------------------------------------------------------------------------------
# sparse float64 evaluation of a convolution, with the sum of |terms|
# ------------------------------------------------------------------------------------------------
def conv_terms(x, w, b, skip=None):
    """x [N, ci, H, W], w [co, ci, k, k], b [co] (float64) -> (y, sum of |terms| incl. |bias|), tap by tap over the non-zero weights.
    `skip` = (co, ci, a, b, col): that tap's product is left out at column `col` (a reference mutation)."""
    N, _, H, W_ = x.shape
    co, k = w.shape[0], w.shape[-1]
    p = k // 2
    xp = F.pad(x, (p, p, p, p))
    xa = xp.abs()
    y = b.view(1, co, 1, 1).expand(N, co, H, W_).clone()
    ya = y.abs()
    for o, c, a, bb in w.nonzero().tolist():
        v = float(w[o, c, a, bb])
        t = v * xp[:, c, a:a + H, bb:bb + W_]
        if skip is not None and (o, c, a, bb) == tuple(skip[:4]):
            t = t.clone()
            t[:, :, skip[4]] = 0.0
        y[:, o] += t
        ya[:, o] += abs(v) * xa[:, c, a:a + H, bb:bb + W_]
    return y, ya


def _check_direct(fig, stage, x, w, b, y_abs, group, res=None, alpha=1.0, where=''):
    """The direct sum of a convolution (any order, any split) and its fused epilogue  res + alpha * (sum + bias)."""
    q = math.inf
    for g0 in range(0, w.shape[1], group):
        qw, qx = unit_of(w[:, g0:g0 + group]), unit_of(x[:, g0:g0 + group])
        if math.isfinite(qw) and math.isfinite(qx):
            q = min(q, qw * qx)
    assert _multiple(b, q), f'{stage} {where}: the bias is not a multiple of the unit {q}'
    fig.note(stage, y_abs.max(), q, where)
    if res is not None:
        q2 = min(q * alpha, unit_of(res))
        fig.note(stage + '+res', (res.abs() + alpha * y_abs).max(), q2, where)


def _check_wino(fig, m, x, w, b, y_direct, where=''):
    """The dense layer in F(m x m, 3 x 3) form: the pack emulation, B^T d B as two 1-D stages, sum_c U V per transformed position,
    A^T M A + bias.  Asserts that the result is the direct one."""
    BT, AT, GI, Gd = WINO[m]
    n = m + 2
    N, cin, H, W_ = x.shape
    co = w.shape[0]
    assert (w != 0).sum((2, 3)).max() <= 1, f'{where}: more than one tap on an (output, input) channel pair'
    # the exact rational U = G g G^T: integer GI, weights 9 * 2^-j (F(4x4): (w / 9) * GI GI / 64) or any dyadic (F(2x2): w * GI GI / 4)
    if m == 4:
        w9 = w / 9.0
        assert torch.equal(w9 * 9.0, w) and _multiple(w9, unit_of(w9)), f'{where}: weights are not 9 * 2^-j'
        U = torch.einsum('ia,jb,ocab->ocij', GI, GI, w9) / 64.0
    else:
        U = torch.einsum('ia,jb,ocab->ocij', GI, GI, w) / 4.0
    # the pack: G from the double constants (1.0 / 6 ..), combined in fp64, rounded to fp32
    gg = Gd[:, None, :, None] * Gd[None, :, None, :]                                    # [n][n][3][3], each product rounded to fp64
    packed = torch.einsum('ijab,ocab->ocij', gg, w).float().double()
    assert torch.equal(packed, U), f'{where}: the fp64 pack of F({m}x{m}) does not round to the rational U'
    Ty, Tx = -(-H // m), -(-W_ // m)
    xp = F.pad(x, (1, Tx * m - W_ + 1, 1, Ty * m - H + 1))                              # zeros outside the map, as the kernels read them
    M = torch.zeros(N, co, Ty, Tx, n, n, dtype=torch.float64)
    Ma = torch.zeros_like(M)
    qM = math.inf
    for c0 in range(0, cin, 64):
        used = [c for c in range(c0, min(cin, c0 + 64)) if w[:, c].any()]
        if not used:
            continue
        d = xp[:, used].unfold(2, n, m).unfold(3, n, m)                                  # [N][c][Ty][Tx][n][n]
        qd = unit_of(d)
        if not math.isfinite(qd):
            continue
        t = torch.matmul(BT, d)
        fig.note(f'f{m}.in', torch.matmul(BT.abs(), d.abs()).max(), qd, where)
        V = torch.matmul(t, BT.t())
        fig.note(f'f{m}.in', torch.matmul(t.abs(), BT.abs().t()).max(), qd, where)
        Uc = U[:, used]
        qM = min(qM, unit_of(Uc) * qd)
        M += torch.einsum('ocij,nctsij->notsij', Uc, V)
        Ma += torch.einsum('ocij,nctsij->notsij', Uc.abs(), V.abs())
    fig.note(f'f{m}.sum', Ma.max(), qM, where)
    assert _multiple(b, qM), f'{where}: the bias is not a multiple of the unit {qM}'
    Y = torch.matmul(torch.matmul(AT, M), AT.t()) + b.view(1, co, 1, 1, 1, 1)
    Ya = torch.matmul(torch.matmul(AT.abs(), M.abs()), AT.abs().t()) + b.abs().view(1, co, 1, 1, 1, 1)
    fig.note(f'f{m}.out', Ya.max(), qM, where)
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, co, Ty * m, Tx * m)[:, :, :H, :W_]
    assert torch.equal(Y, y_direct), f'{where}: F({m}x{m}) in float64 differs from the direct sum'


# ------------------------------------------------------------------------------------------------
# the float64 trunks
# ------------------------------------------------------------------------------------------------
def _conv(P, name):
    return P[name + '.weight'].double(), P[name + '.bias'].double()


def rdn_eval(P, x, fig=None, wino=True, mutate=None):
    """The RDN trunk of ciaosr_oracle.rdn_features in float64, convolution by convolution over the non-zero taps.  `fig`: a Figures to
    run check_exact's assertions into (`wino`: the dense layers in both Winograd forms too).  `mutate` = (kind, ...) applies one
    reference mutation to the LAST block's probe layer: ('seam', col) | ('swap', c1, c2) | ('lastrow',)."""
    x = x.double()
    C = P['sfe1.weight'].shape[0]
    nb = 1 + max(int(k.split('.')[1]) for k in P if k.startswith('rdbs.'))
    nl = 1 + max(int(k.split('.')[3]) for k in P if k.startswith('rdbs.0.layers.'))
    chk = fig is not None
    w, b = _conv(P, 'sfe1')
    s1, a = conv_terms(x, w, b)
    if chk:
        _check_direct(fig, 'stem', x, w, b, a, 3, where='sfe1')
    w, b = _conv(P, 'sfe2')
    h, a = conv_terms(s1, w, b)
    if chk:
        _check_direct(fig, 'stem', s1, w, b, a, C, where='sfe2')
    local = []
    for blk in range(nb):
        t = h
        for l in range(nl):
            w, b = _conv(P, f'rdbs.{blk}.layers.{l}.conv')
            tin, skip, probe = t, None, (blk == nb - 1 and l == nl - 1)
            if mutate is not None and probe:
                if mutate[0] == 'swap':
                    perm = list(range(t.shape[1]))
                    perm[mutate[1]], perm[mutate[2]] = mutate[2], mutate[1]
                    tin = t[:, perm]
                elif mutate[0] == 'seam':
                    o, c, ta, tb = w.nonzero()[0].tolist()
                    skip = (o, c, ta, tb, mutate[1])
            y, a = conv_terms(tin, w, b, skip)
            if mutate is not None and probe and mutate[0] == 'lastrow':
                y = y.clone()
                y[:, :, -1] = 0.0
            if chk:
                where = f'block {blk} layer {l}'
                _check_direct(fig, 'dense.direct', t, w, b, a, C, where=where)
                if wino:
                    _check_wino(fig, 2, t, w, b, y, where)
                    _check_wino(fig, 4, t, w, b, y, where)
                fig['dense.alive'] = min(fig.get('dense.alive', 1.0), (y > 0).double().mean().item())
            t = torch.cat([t, torch.relu(y)], 1)
        if chk:
            fig[f'block{blk}.in.max'] = max(fig.get(f'block{blk}.in.max', 0.0), h.abs().max().item())
        w, b = _conv(P, f'rdbs.{blk}.lff')
        y, a = conv_terms(t, w, b)
        if chk:
            _check_direct(fig, 'lff', t, w, b, a, C, res=h, where=f'block {blk}')
        h = h + y
        local.append(h)
    cat = torch.cat(local, 1)
    w, b = _conv(P, 'gff.0')
    g, a = conv_terms(cat, w, b)
    if chk:
        _check_direct(fig, 'gff', cat, w, b, a, C, where='gff.0')
    w, b = _conv(P, 'gff.1')
    y, a = conv_terms(g, w, b)
    if chk:
        _check_direct(fig, 'gff', g, w, b, a, C, res=s1, where='gff.1')
    return y + s1


def edsr_eval(P, x, res_scale, fig=None):
    """ciaosr_oracle.edsr_features in float64, the same way."""
    x = x.double()
    chk = fig is not None
    nb = 1 + max(int(k.split('.')[1]) for k in P if k.startswith('body.'))
    w, b = _conv(P, 'conv_first')
    f, a = conv_terms(x, w, b)
    if chk:
        _check_direct(fig, 'stem', x, w, b, a, 3, where='conv_first')
    h = f
    for blk in range(nb):
        w, b = _conv(P, f'body.{blk}.conv1')
        y, a = conv_terms(h, w, b)
        if chk:
            _check_direct(fig, 'edsr.conv', h, w, b, a, 64, where=f'body.{blk}.conv1')
        r = torch.relu(y)
        w, b = _conv(P, f'body.{blk}.conv2')
        y, a = conv_terms(r, w, b)
        if chk:
            _check_direct(fig, 'edsr.conv', r, w, b, a, 64, res=h, alpha=res_scale, where=f'body.{blk}.conv2')
        h = h + y * res_scale
    w, b = _conv(P, 'conv_after_body')
    y, a = conv_terms(h, w, b)
    if chk:
        _check_direct(fig, 'edsr.conv', h, w, b, a, 64, res=f, where='conv_after_body')
    return y + f


# ------------------------------------------------------------------------------------------------
# the builders
# ------------------------------------------------------------------------------------------------
def _sign(g, n=None):
    s = (torch.randint(0, 2, (n or 1,), generator=g) * 2 - 1).double()
    return s if n else float(s[0])


def _cover(g, co, ci, k, scale=1.0):
    """[co][ci][k][k] of scale * {-1, 0, 1}: the ci k k input columns dealt out to the rows in turn (every column read by exactly one
    row), and one random tap for every row that got none."""
    w = torch.zeros(co, ci * k * k, dtype=torch.float64)
    cols = torch.randperm(ci * k * k, generator=g)
    w[torch.arange(cols.numel()) % co, cols] = _sign(g, cols.numel())
    for r in range(cols.numel(), co):
        w[r, int(torch.randint(0, ci * k * k, (1,), generator=g))] = _sign(g)
    return w.view(co, ci, k, k) * scale


def _ints(g, n, lo, hi):
    return torch.randint(lo, hi + 1, (n,), generator=g).double()


def _stem(g, C, first, second, biased=BIASED):
    """sfe1 (one tap per row) and sfe2 (one tap per lattice phase and row) -> parameters and psi [3][2], the images' lattice phases."""
    P = {}
    psi = torch.randint(0, 3, (3, 2), generator=g)
    w1 = _cover(g, C, 3, 3)
    b1 = torch.zeros(C, dtype=torch.float64)
    b1[torch.randperm(C, generator=g)[:biased]] = _sign(g, biased)
    P[first + '.weight'], P[first + '.bias'] = w1, b1
    if second is None:
        return P, psi
    # channel c of sfe1's output is non-zero where (y, x) = psi[ch] - (a - 1, b - 1) mod 3
    tap = w1.view(C, -1).abs().argmax(1)
    ch, a, b = tap // 9, tap % 9 // 3, tap % 3
    ph1 = torch.stack([(psi[ch, 0] - (a - 1)) % 3, (psi[ch, 1] - (b - 1)) % 3], 1)                  # [C][2]
    w2 = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    for py in range(3):
        for px in range(3):
            src = torch.randperm(C, generator=g)                  # row r reads, for this phase, channel src[r] ...
            ta, tb = (ph1[src, 0] - py + 1) % 3, (ph1[src, 1] - px + 1) % 3      # ... at the one tap that is non-zero on this phase
            w2[torch.arange(C), src, ta, tb] = _sign(g, C)
    P[second + '.weight'] = w2
    P[second + '.bias'] = -(w2.sum((2, 3)) @ b1)                  # sfe1's bias, removed again wherever all nine taps are inside the map
    return P, psi


def _block(g, P, prefix, C, nl, w, narrow, taps=TAPS):
    """One dense block: nl - 1 feeders and the probe, then lff.  `narrow`: the probe is cut narrow and lff scales each group back to
    integers (a block whose output another block reads)."""
    wino = w != 1.0
    narrow = narrow and wino
    u = w / 9.0 if wino else 1.0                                    # the unit of a layer that reads integers
    for l in range(nl):
        cin = C * (l + 1)
        wt = torch.zeros(C, cin, 3, 3, dtype=torch.float64)
        if l < nl - 1:                                              # feeder: one tap on group 0
            src = torch.randperm(C, generator=g)
            wt[torch.arange(C), src, torch.randint(0, 3, (C,), generator=g), torch.randint(0, 3, (C,), generator=g)] = _sign(g, C) * w
            if wino:
                seven = (_ints(g, C, 0, 3) == 0).double() * (0.0 if narrow else 1.0)   # a quarter of the rows: -7 u instead of -8 u
                bias = -(8.0 - seven) * u
            else:
                bias = -_ints(g, C, 0, 1)
        else:                                                       # probe
            n_g = [1] * (l + 1)
            for _ in range(0 if narrow else max(0, taps - (l + 1))):
                n_g[int(torch.randint(0, l + 1, (1,), generator=g))] += 1
            first = [torch.randperm(C, generator=g) for _ in n_g]       # row o's first tap in group gi: every input channel is read
            for o in range(C):
                for gi, cnt in enumerate(n_g):
                    rest = [c for c in torch.randperm(C, generator=g).tolist() if c != int(first[gi][o])]
                    for c in [int(first[gi][o])] + rest[:cnt - 1]:
                        wg = w * u if (wino and gi == 0 and l > 0) else w      # group 0 holds integers, the feeders multiples of u
                        wt[o, gi * C + c, int(torch.randint(0, 3, (1,), generator=g)), int(torch.randint(0, 3, (1,), generator=g))] = _sign(g) * wg
            uo = u * (u if l > 0 else 1.0)                          # feeders' outputs are multiples of u
            bias = -(9.0 * (l + 1) - 1.0) * uo * torch.ones(C, dtype=torch.float64) if narrow else _ints(g, C, -4, 4) * uo
        P[f'{prefix}.layers.{l}.conv.weight'], P[f'{prefix}.layers.{l}.conv.bias'] = wt, bias
    wl = _cover(g, C, C * (nl + 1), 1)
    if narrow:
        for gi in range(1, nl + 1):
            wl[:, gi * C:(gi + 1) * C] *= (1.0 / u) ** (2 if (gi == nl and nl > 1) else 1)
    P[prefix + '.lff.weight'], P[prefix + '.lff.bias'] = wl, _ints(g, C, -1, 1) if narrow else _ints(g, C, -2, 2)


def rdn_params(nl, nb=1, C=64, seed=0):
    """Reference-named float64 RDN parameters: nb blocks of nl dense layers, the last layer of each the probe."""
    g = torch.Generator().manual_seed(7919 * seed + 100 * nl + 10 * nb + C)
    P, psi = _stem(g, C, 'sfe1', 'sfe2', BIASED if nb == 1 or C != 64 else 0)
    for b in range(nb):
        _block(g, P, f'rdbs.{b}', C, nl, W9 if C == 64 else 1.0, narrow=b < nb - 1, taps=TAPS if nb == 1 else 4)
    P['gff.0.weight'], P['gff.0.bias'] = _cover(g, C, C * nb, 1), _ints(g, C, -2, 2)
    P['gff.1.weight'], P['gff.1.bias'] = _cover(g, C, C, 3), _ints(g, C, -2, 2)
    return P, psi


EDSR_RES_SCALE = 0.25


def edsr_params(nb=2, seed=0):
    g = torch.Generator().manual_seed(104729 * seed + nb)
    P, psi = _stem(g, 64, 'conv_first', None)
    for b in range(nb):
        P[f'body.{b}.conv1.weight'], P[f'body.{b}.conv1.bias'] = _cover(g, 64, 64, 3, 0.5), _ints(g, 64, -2, 2) * 0.5
        P[f'body.{b}.conv2.weight'], P[f'body.{b}.conv2.bias'] = _cover(g, 64, 64, 3, 0.5), _ints(g, 64, -2, 2) * 0.25
    P['conv_after_body.weight'], P['conv_after_body.bias'] = _cover(g, 64, 64, 3, 0.25), _ints(g, 64, -2, 2) * 0.25
    return P, psi


def lr_images(psi, hw, B, seed=0):
    """[B, 3, H, W] float32 in {-1, 0, 1}: channel ch non-zero only where (y % 3, x % 3) == psi[ch], there with probability P_NZ."""
    H, W_ = hw
    g = torch.Generator().manual_seed(31 * seed + 1000 * H + W_)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W_), indexing='ij')
    x = torch.zeros(B, 3, H, W_)
    for ch in range(3):
        on = ((yy % 3 == psi[ch, 0]) & (xx % 3 == psi[ch, 1])).float()
        val = (torch.randint(0, 2, (B, H, W_), generator=g) * 2 - 1).float() * (torch.rand(B, H, W_, generator=g) < P_NZ).float()
        x[:, ch] = on * val
    return x


# ------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------
_params_cache, _cache = {}, {}


def _rdn_params32(key, nl, nb, C):
    if key not in _params_cache:
        P, psi = rdn_params(nl, nb, C)
        P32 = {k: v.float() for k, v in P.items()}
        for k, v in P.items():
            assert torch.equal(P32[k].double(), v), k
        _params_cache[key] = (P32, psi)
    return _params_cache[key]


def check_exact(fx):
    """Re-evaluates the fixture in float64 and asserts, for every sum a route can form, that all addends are multiples of one power of two
    q and sum |addends| < 2^22 q; returns the figures (stage -> worst log2(sum |addends| / q)).  A condition on the fixture."""
    fig = Figures()
    if fx.kind == 'edsr':
        want = edsr_eval(fx.params, fx.x, fx.res_scale, fig)
    else:
        want = rdn_eval(fx.params, fx.x, fig, wino=fx.params['sfe1.weight'].shape[0] == 64)
    assert torch.equal(want, fx.want)
    assert torch.equal(fx.x, fx.x.round()) and fx.x.abs().max() <= 1
    return fig


def _fixture(kind, name, params, psi, hw, B, res_scale=None):
    key = (name, tuple(hw), B)
    if key not in _cache:
        x = lr_images(psi, hw, B)
        want = edsr_eval(params, x, res_scale) if kind == 'edsr' else rdn_eval(params, x)
        fx = Fixture(kind, name, tuple(hw), B, params, x, want, max(1.0, want.abs().max().item()), unit_of(want), res_scale)
        _cache[key] = fx
    return _cache[key]


def probe(l, hw=(21, 37), B=1):
    """RDN, one block of l + 1 dense layers: l feeders and the probe layer l."""
    P, psi = _rdn_params32(('probe', l), l + 1, 1, 64)
    return _fixture('rdn', f'probe{l}', P, psi, hw, B)


def two_blocks(hw=(21, 37), B=1):
    """RDN, NB = 2 blocks of two layers: the X ping-pong and the global concat's column offset of block 1."""
    P, psi = _rdn_params32(('nb2',), 2, 2, 64)
    return _fixture('rdn', 'nb2', P, psi, hw, B)


def narrow32(hw=(19, 24), B=1):
    """RDN with mid_channels = channel_growth = 32, two blocks of three layers: the generic route."""
    P, psi = _rdn_params32(('mid32',), 3, 2, 32)
    return _fixture('rdn', 'mid32', P, psi, hw, B)


def edsr(hw, B=1):
    """EDSR, C = 64, two blocks, res_scale 0.25."""
    if 'edsr' not in _params_cache:
        P, psi = edsr_params(2)
        _params_cache['edsr'] = ({k: v.float() for k, v in P.items()}, psi)
        for k, v in P.items():
            assert torch.equal(_params_cache['edsr'][0][k].double(), v), k
    P, psi = _params_cache['edsr']
    return _fixture('edsr', 'edsr', P, psi, hw, B, EDSR_RES_SCALE)


# the cases of test_trunk_exact_gpu.py (test_trunk_exact_host.py runs check_exact on every one of them)
FORCED_MAPS = [(16, 32), (17, 33), (21, 37), (7, 30)]
BIG = (131, 253)
EDSR_MAPS = [(12, 12), (13, 25), (7, 30), (19, 70)]


def forced_cases():
    """(probe, map) of the forced halo-resident routes: all eight probes on (21, 37), probes 0, 1 and 7 on the other maps."""
    return [(l, hw) for hw in FORCED_MAPS for l in (range(8) if hw == (21, 37) else (0, 1, 7))]


def small_cases():
    return [(l, hw) for hw in ((21, 37), (17, 33)) for l in (0, 3, 7)]


def all_fixtures():
    """name -> thunk of every fixture the GPU file runs."""
    out = {}
    for l, hw in forced_cases() + small_cases():
        out[f'probe{l}-{hw[0]}x{hw[1]}'] = lambda l=l, hw=hw: probe(l, hw)
    out['probe7-17x33-b3'] = lambda: probe(7, (17, 33), 3)
    out['nb2-21x37'] = lambda: two_blocks((21, 37))
    out['mid32-19x24'] = lambda: narrow32((19, 24))
    out[f'probe7-{BIG[0]}x{BIG[1]}'] = lambda: probe(7, BIG)
    for hw in EDSR_MAPS:
        for B in (1, 3):
            out[f'edsr-{hw[0]}x{hw[1]}-b{B}'] = lambda hw=hw, B=B: edsr(hw, B)
    return out


# ------------------------------------------------------------------------------------------------
# helpers of the tests
# ------------------------------------------------------------------------------------------------
def worst_element(got, want):
    """(max |got - want|, 'image i channel c row y column x') for [B, C, H, W] tensors."""
    d = (got.double() - want.double()).abs()
    i = int(d.argmax())
    _, C, H, W_ = d.shape
    return d.max().item(), f'image {i // (C * H * W_)} channel {i // (H * W_) % C} row {i // W_ % H} column {i % W_}', \
        (i // (C * H * W_), i // (H * W_) % C, i // W_ % H, i % W_)


def swap_pair(fx):
    """Two input channels of the probe's last group in different 8-channel steps, the first of them read by the probe."""
    nl = 1 + max(int(k.split('.')[3]) for k in fx.params if k.startswith('rdbs.0.layers.'))
    w = fx.params[f'rdbs.0.layers.{nl - 1}.conv.weight']
    g0 = 64 * (nl - 1)
    c1 = g0 + int(w[:, g0:].abs().sum((0, 2, 3)).argmax())
    return c1, g0 + (c1 - g0 + 8) % 64


# reference mutations: name -> (map, mutate argument of rdn_eval as a function of the fixture)
MUTATIONS = {
    'tap dropped right of the 12-pixel seam (x = 12)': ((21, 37), lambda fx: ('seam', 12)),
    'tap dropped right of the 8x16 seam (x = 16)': ((21, 37), lambda fx: ('seam', 16)),
    'tap dropped right of the 16x32 seam (x = 32)': ((21, 37), lambda fx: ('seam', 32)),
    'two input channels of the last group swapped': ((21, 37), lambda fx: ('swap',) + swap_pair(fx)),
    'last row (one-row partial 4x4 tile, H = 16 + 5) dropped': ((21, 37), lambda fx: ('lastrow',)),
}
