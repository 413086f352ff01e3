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

The 16-bit RDN trunk modes ('bf16', 'bf16-single', 'f16', 'f16-pairs'; rounding points: see H16 below).  Every tensor those modes round
to bf16 / half is such a number on the probe and NB = 2 fixtures already -- block inputs, feeder outputs, the weights 9 * 2^-j, the ternary
lff weights and the probe's output under 'f16' -- so `check_exact_h16` asserts that and the same condition, and fx.want, the same object,
is the answer of every 16-bit route: test_trunk_h16_exact_gpu.py asserts torch.equal.  Such weights have no lo half; `split_probe`
multiplies the probe's weights by 1 + s 2^-8 (hi + lo == w in both types, lo != 0 on every tap, half subnormals among them), with the
condition asserted for the hi products, the lo products and both in one sum, and a second answer (`want_single`) for the mode that
multiplies by hi alone.  'f16' is left out of the split fixtures (its fusion rounds the probe's output, which needs more than 11 bits
there); 'bf16-single' meets the condition on them at the full 16 taps per row.  `H16_MUTATIONS`: what a dropped or misplaced lo
fragment and a skipped 16-bit write of the fusion epilogue do to the float64 answer.

Host figures of the 16-bit cases (test_trunk_h16_exact_host.py; worst log2(sum |addends| / q) over every case of h16_cases, < 22 asserted):
  probes, every mode            direct 9 cin sum 8.3 (no lo);  lff + residual 11.1;  gff.1 + residual 13.3
  NB = 2, every mode            direct 8.8;  lff + residual 11.8;  gff.1 + residual 13.8
  split probes, bf16            hi 12.3, lo 7.9, hi + lo 16.3;  lff + residual 19.1;  gff.1 + residual 21.4
  split probes, f16-pairs       hi 13.3, lo 5.1, hi + lo 16.3;  lff + residual 19.1;  gff.1 + residual 21.4
  split probes, bf16-single     hi 12.3;  lff + residual 15.1;  gff.1 + residual 17.4
Mutations of the reference (split probes 0, 3, 7 on (21, 37); one output unit 2^-12 / 2^-16 / 2^-16): one lo fragment's worth of one
output row dropped 14 / 7 / 7 units in bf16 and 2 / 1 / 1 in half; two lo taps swapped 42 / 14 / 14 and 6 / 2 / 2; the 16-bit write of
block 1's input skipped at one pixel column (NB = 2) 2348 units.

Measured on an MI355X (profiles/trunk_h16_exact.txt), |got - want| of test_trunk_h16_exact_gpu.py: 0.0 on all 154 runs -- dense_h16_kernel<LO>
(72 unsplit, 9 split), dense_h16_dma_kernel (10), dense_h16_wide_kernel<LO, 1> (37, 9), <LO, 2> (8, 9), in both element types, with
cast_group_h16_kernel and, under 'f16', the fusion on gemm_h16.hip in each: bitwise the float64 answer, no defect found.  A model whose
probe lo pack lacks one fragment's worth of one row is 7 (bf16) / 1 (half) output units off on each of the three cuts.
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
    cs = w.flatten(2).any(2).any(0).nonzero().flatten().tolist()              # the input channels some tap reads: the others are not copied
    at = {c: i for i, c in enumerate(cs)}
    xp = F.pad(x if len(cs) == x.shape[1] else x[:, cs], (p, p, p, p))
    xa = xp.abs()
    y = b.view(1, co, 1, 1).expand(N, co, H, W_).clone()
    ya = y.abs()
    for o, c, a, bb in w.nonzero().tolist():
        v = float(w[o, c, a, bb])
        if skip is not None and (o, c, a, bb) == tuple(skip[:4]):
            t = v * xp[:, at[c], a:a + H, bb:bb + W_]
            t[:, :, skip[4]] = 0.0
            y[:, o] += t
        else:
            y[:, o].add_(xp[:, at[c], a:a + H, bb:bb + W_], alpha=v)
        ya[:, o].add_(xa[:, at[c], a:a + H, bb:bb + W_], alpha=abs(v))
    return y, ya


def _check_direct(fig, stage, x, w, b, y_abs, group, res=None, alpha=1.0, where='', units=None):
    """The direct sum of a convolution (any order, any split) and its fused epilogue  res + alpha * (sum + bias).  `units`: unit_of of
    each input group where the caller has them already."""
    q = math.inf
    for g0 in range(0, w.shape[1], group):
        qw, qx = unit_of(w[:, g0:g0 + group]), units[g0 // group] if units else unit_of(x[:, g0:g0 + group])
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
# the 16-bit trunk modes
# ------------------------------------------------------------------------------------------------
# The rounding points of a 16-bit RDN trunk mode, restated from the header of independent_refs.rdn_trunk_16bit_emulation and from
# rdn_route / block_dense / block_fuse of csrc/encoder.hip (h = the mode's element type, bf16 or IEEE half):
#   every mode    each block's input (group 0 of the 16-bit rows Xb: cast_group) and every dense layer's output (the layer's own 16-bit
#                 write beside its fp32 one) are rounded to h before a dense layer reads them; the dense weights are packed as
#                 hi = h(w), lo = h(w - hi); products exact, accumulation, bias and ReLU in fp32; stem, gff and all residual sums fp32.
#   pairs         'bf16', 'f16-pairs': every dense product is taken with hi and with lo, as separate MFMAs into one fp32 sum.
#   single        'bf16-single', 'f16': hi alone; the lo pack is not read.
#   lff16         'f16' alone: the local fusion reads the SAME 16-bit rows -- the last layer's output included, which nothing else reads
#                 in 16 bits -- with weights h(w_lff), fp32 accumulation, bias and fp32 residual; its epilogue writes the block's output
#                 in fp32 and, rounded to h, as group 0 of the next block's 16-bit rows (no cast_group after block 0).  The other
#                 three modes fuse in fp32 on the fp32 layer outputs with the fp32 weights.
H16 = namedtuple('H16', 'mode half pairs lff16')
H16_MODES = {m: H16(m, 'bf16' if m.startswith('bf16') else 'f16', m in ('bf16', 'f16-pairs'), m == 'f16') for m in ('bf16', 'bf16-single', 'f16', 'f16-pairs')}


def round16(t, half):
    """t (fp32 numbers held in float64) rounded to bf16 / IEEE half, in float64."""
    return t.float().to(torch.bfloat16 if half == 'bf16' else torch.float16).double()


def split16(w, half):
    """hi = h(w), lo = h(w - hi): the weight pair of the fragment pack."""
    hi = round16(w, half)
    return hi, round16(w - hi, half)


def _is16(t, half, what):
    bad = round16(t, half) != t
    assert not bad.any(), f'{what}: {int(bad.sum())} of {t.numel()} values are not {half} numbers (e.g. {t[bad][0].item()!r})'


def _h16_weights(fig, t, w, b, h16, C, where, units):
    """The weights a dense layer of that mode multiplies by; with `fig`, condition (b) on the direct 9 cin sums for the hi and the lo
    products on their own (a kernel accumulates them as separate MFMAs, in any order and any K split) and for both in one sum."""
    hi, lo = split16(w, h16.half)
    if not h16.pairs:
        lo = torch.zeros_like(lo)
    if fig is not None:                   # (the input groups: rdn_eval asserts each as it is made)
        if h16.pairs:
            assert torch.equal(hi + lo, w), f'{where}: hi + lo is not the weight'
        if lo.any():                      # (no lo: hi is the weight, and the caller's 'dense.direct' is the hi sum)
            a_hi, a_lo = conv_terms(t, hi, b)[1], conv_terms(t, lo, torch.zeros_like(b))[1]
            _check_direct(fig, 'dense.hi', t, hi, b, a_hi, C, where=where, units=units)
            _check_direct(fig, 'dense.lo', t, lo, torch.zeros_like(b), a_lo, C, where=where, units=units)
            _check_direct(fig, 'dense.hi+lo', t, torch.cat([hi, lo], 0), b, a_hi + a_lo, C, where=where, units=units)
            fig['lo.taps'] = fig.get('lo.taps', 0) + int((lo != 0).sum())
    return hi + lo


# ------------------------------------------------------------------------------------------------
# the float64 trunks
# ------------------------------------------------------------------------------------------------
def _conv(P, name):
    return P[name + '.weight'].double(), P[name + '.bias'].double()


def rdn_eval(P, x, fig=None, wino=True, mutate=None, h16=None):
    """The RDN trunk of ciaosr_oracle.rdn_features in float64, convolution by convolution over the non-zero taps.  `fig`: a Figures to
    run check_exact's assertions into (`wino`: the dense layers in both Winograd forms too).  `mutate` = (kind, ...) applies one
    reference mutation to the LAST block's probe layer: ('seam', col) | ('swap', c1, c2) | ('lastrow',); or ('stale16', col): in every
    block after the first, the 16-bit rows keep the previous block's input at pixel column col (see H16_MUTATIONS).  `h16`: an H16 --
    the dense layers multiply by the weights that 16-bit mode multiplies by (hi + lo, or hi alone), and `fig` also takes
    check_exact_h16's assertions."""
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
    local, h_before = [], None
    for blk in range(nb):
        t = h
        if mutate is not None and mutate[0] == 'stale16' and blk > 0:
            t = h.clone()
            t[:, :, :, mutate[1]] = h_before[:, :, :, mutate[1]]
        h_before = h
        units = [unit_of(t)] if chk else None          # unit_of of each input group of the block's dense layers
        if chk and h16 is not None:        # group 0 of the 16-bit rows: cast_group, or (lff16, blk > 0) the previous block's epilogue
            _is16(h, h16.half, f'block {blk} input')
        for l in range(nl):
            w, b = _conv(P, f'rdbs.{blk}.layers.{l}.conv')
            if h16 is not None:
                w = _h16_weights(fig, t, w, b, h16, C, f'block {blk} layer {l}', units)
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
                _check_direct(fig, 'dense.direct', t, w, b, a, C, where=where, units=units)
                units.append(unit_of(torch.relu(y)))
                if wino:
                    _check_wino(fig, 2, t, w, b, y, where)
                    _check_wino(fig, 4, t, w, b, y, where)
                fig['dense.alive'] = min(fig.get('dense.alive', 1.0), (y > 0).double().mean().item())
                if h16 is not None and (l < nl - 1 or h16.lff16):       # the 16-bit copy of the output that a later layer or lff16 reads
                    _is16(torch.relu(y), h16.half, f'block {blk} layer {l} output')
            t = torch.cat([t, torch.relu(y)], 1)
        if chk:
            fig[f'block{blk}.in.max'] = max(fig.get(f'block{blk}.in.max', 0.0), h.abs().max().item())
        w, b = _conv(P, f'rdbs.{blk}.lff')
        if chk and h16 is not None and h16.lff16:                       # cast_weights: the local fusion multiplies by half(w)
            _is16(w, h16.half, f'block {blk} lff weights')
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


# ------------------------------------------------------------------------------------------------
# the 16-bit trunk modes: fixtures, the condition, mutations, cases
# ------------------------------------------------------------------------------------------------
SPLIT = 2.0 ** -8               # 2^-9: probe 7 misses the condition at gff.1 (22.09 bits); 2^-7: every half `lo` is zero
_single_cache, _h16_memo = {}, {}


def _probe_name(P):
    nb = 1 + max(int(k.split('.')[1]) for k in P if k.startswith('rdbs.'))
    nl = 1 + max(int(k.split('.')[3]) for k in P if k.startswith('rdbs.0.layers.'))
    return f'rdbs.{nb - 1}.layers.{nl - 1}.conv.weight'


def split_probe(l, hw=(21, 37), B=1):
    """probe(l, ...) with every weight of the probe layer multiplied by 1 + s * 2^-8, s = +-1 per tap from a seeded generator: neither a
    bf16 nor a half number, but hi + lo == w exactly in both types and lo != 0 on every tap (half: the lo of the 9/256 taps is the
    subnormal 2^-16).  `want` is the float64 evaluation with those weights -- the answer of the pair modes 'bf16' and 'f16-pairs';
    want_single(fx, half) is the answer of a mode that multiplies by hi alone ('bf16-single').  Mode 'f16' is left out of this fixture:
    its local fusion reads the probe's output rounded to half, and those values (multiples of 2^-16 up to a few units) need more than
    the 11 bits of a half significand."""
    key = ('split', l)
    if key not in _params_cache:
        P, psi = _rdn_params32(('probe', l), l + 1, 1, 64)
        g = torch.Generator().manual_seed(977 + l)
        name = _probe_name(P)
        w = P[name].double()
        ws = w * (1.0 + (torch.randint(0, 2, w.shape, generator=g) * 2 - 1).double() * SPLIT)
        assert torch.equal(ws.float().double(), ws)
        _params_cache[key] = (dict(P, **{name: ws.float()}), psi)
    P, psi = _params_cache[key]
    return _fixture('rdn', f'split{l}', P, psi, hw, B)


def want_single(fx, half):
    """The float64 evaluation of a split fixture with the probe weights rounded once to the element type: what a mode that ignores `lo`
    computes."""
    key = (fx.name, fx.hw, fx.B, half)
    if key not in _single_cache:
        name = _probe_name(fx.params)
        _single_cache[key] = rdn_eval(dict(fx.params, **{name: round16(fx.params[name].double(), half).float()}), fx.x)
    return _single_cache[key]


def h16_answer(fx, mode):
    """The float64 answer of a 16-bit trunk mode on a fixture: fx.want itself, but want_single where hi alone is not the weight."""
    h = H16_MODES[mode]
    return want_single(fx, h.half) if fx.name.startswith('split') and not h.pairs else fx.want


def check_exact_h16(fx, mode):
    """check_exact for a 16-bit trunk mode (rounding points: see H16).  Re-evaluates the fixture in float64 with the weights that mode
    multiplies by and asserts  (a) every tensor a route of the mode rounds to its element type is such a number already: each block's
    input (group 0 of the 16-bit rows, which under 'f16' the previous block's fusion epilogue writes), every dense-layer output a later
    layer or the 16-bit fusion reads, the dense weights as hi + lo (pairs) or hi alone, the fusion weights under 'f16';  (b) the condition
    (addends multiples of one power of two q, sum |addends| < 2^22 q) on the direct 9 cin sums with the hi weights, with the lo weights
    and with both in one sum;  (c) the same for stem, lff, gff and the residual epilogues as in check_exact.  Returns the figures."""
    h = H16_MODES[mode]
    split = fx.name.startswith('split')
    assert fx.kind == 'rdn' and fx.params['sfe1.weight'].shape[0] == 64 and not (split and h.lff16)
    # (an unsplit fixture has no lo: the two bf16 modes multiply by the same weights and round the same tensors -- one evaluation)
    key = (fx.name, fx.hw, fx.B, h.half, h.lff16, h.pairs and split)
    if not split and not h.lff16 and (key[:4] + (True, False)) in _h16_memo:
        key = key[:4] + (True, False)          # ... and what 'f16' asserts on it contains what 'f16-pairs' needs
    if key not in _h16_memo:
        fig = Figures()
        got = rdn_eval(fx.params, fx.x, fig, wino=False, h16=h)
        assert torch.equal(got, h16_answer(fx, mode))
        _h16_memo[key] = fig
    fig = Figures(_h16_memo[key])
    for k, w in fx.params.items():
        if '.layers.' in k and k.endswith('.weight') and not (split and k == _probe_name(fx.params)):
            _is16(w.double(), h.half, k)                              # hi alone is the weight
    assert torch.equal(fx.x, fx.x.round()) and fx.x.abs().max() <= 1
    return fig


def lo_mutated(fx, half, kind, row=5):
    """The parameters of a split fixture with the `lo` halves of output row `row` of the probe changed as a kernel defect would (K order
    of the fragment pack: k = (a * 3 + b) * cin + ci): 'drop' -- one fragment's worth, the 16 consecutive K indices around the row's
    first tap, zero;  'swap' -- the lo halves of the row's first two taps with opposite lo exchanged."""
    name = _probe_name(fx.params)
    w = fx.params[name].double()
    hi, lo = split16(w, half)
    assert torch.equal(hi + lo, w)
    co, cin = w.shape[:2]
    lo_k = lo.permute(0, 2, 3, 1).reshape(co, -1).clone()
    taps = lo_k[row].nonzero().flatten().tolist()
    if kind == 'drop':
        k0 = taps[0] // 16 * 16
        lo_k[row, k0:k0 + 16] = 0.0
    else:
        k1, k2 = next((a, b) for a in taps for b in taps if lo_k[row, b] == -lo_k[row, a])     # (same magnitude: input groups of one unit)
        lo_k[row, k1], lo_k[row, k2] = lo_k[row, k2].clone(), lo_k[row, k1].clone()
    wm = hi + lo_k.view(co, 3, 3, cin).permute(0, 3, 1, 2)
    assert torch.equal(wm.float().double(), wm) and not torch.equal(wm, w)
    return dict(fx.params, **{name: wm.float()})


STALE_COLUMN = 18
# reference mutations of the 16-bit routes: name -> function of (probe, element type) -> (fixture, mutated float64 answer)
H16_MUTATIONS = {
    "one lo fragment's worth of taps dropped (16 consecutive K indices of one output row)":
        lambda l, half: (split_probe(l), rdn_eval(lo_mutated(split_probe(l), half, 'drop'), split_probe(l).x)),
    'two lo taps of one output row swapped':
        lambda l, half: (split_probe(l), rdn_eval(lo_mutated(split_probe(l), half, 'swap'), split_probe(l).x)),
    f"the fusion epilogue's 16-bit write of block 1's input skipped at pixel column {STALE_COLUMN} (the rows keep block 0's input there)":
        lambda l, half: (two_blocks(), rdn_eval(two_blocks().params, two_blocks().x, mutate=('stale16', STALE_COLUMN))),
}

# the cases of test_trunk_h16_exact_gpu.py (test_trunk_h16_exact_host.py runs check_exact_h16 on every (fixture, mode) of them)
H16_ALL = tuple(H16_MODES)
H16_SINGLE = ('f16', 'bf16-single')                       # no lo pack: a batch takes dense_h16_dma_kernel on the 12 x 12 route
H16_SPLIT = ('bf16', 'f16-pairs', 'bf16-single')
H16_SMALL_MAPS = [(12, 12), (13, 25), (21, 37), (7, 30)]   # one 12 x 12 tile; one-pixel remainders; ragged; lower than a tile
H16_WIDE_MAPS = [(64, 256), (65, 225), (17, 1000)]         # 32 whole 16 x 32 tiles; one-row and one-column remainders; a strip
H16_WIDE2 = ((81, 257), 3)                                 # 162 tiles of 16 x 32 in the launch: the 16 x 32 tile shape (R = 2)
H16Case = namedtuple('H16Case', 'fixture l hw B direct modes kernel')


def h16_cases():
    """kernel: '12x12' = dense_h16_kernel, 'dma' = dense_h16_dma_kernel where the mode has no lo pack (dense_h16_kernel<true> else),
    'wide1' / 'wide2' = dense_h16_wide_kernel<LO, R>."""
    out = []
    for hw in H16_SMALL_MAPS:
        out += [H16Case('probe', l, hw, 1, 1, H16_ALL, '12x12') for l in (range(8) if hw == (21, 37) else (0, 1, 7))]
    out.append(H16Case('nb2', None, (21, 37), 1, 1, H16_ALL, '12x12'))
    out += [H16Case('probe', l, hw, 3, 1, H16_SINGLE, 'dma') for hw in ((21, 37), (13, 25)) for l in (0, 7)]
    out.append(H16Case('nb2', None, (21, 37), 3, 1, H16_SINGLE, 'dma'))
    out += [H16Case('probe', l, hw, 1, 0, H16_ALL, 'wide1') for hw in H16_WIDE_MAPS for l in (0, 3, 7)]
    out += [H16Case('probe', l, H16_WIDE2[0], H16_WIDE2[1], 0, H16_ALL, 'wide2') for l in (0, 7)]
    for hw, B, direct, kernel in (((21, 37), 1, 1, '12x12'), ((65, 225), 1, 0, 'wide1'), H16_WIDE2 + (0, 'wide2')):
        out += [H16Case('split', l, hw, B, direct, H16_SPLIT, kernel) for l in (0, 3, 7)]
    out.append(H16Case('nb2', None, (65, 225), 2, 0, ('f16',), 'wide1'))       # the fusion epilogue's 16-bit write feeds block 1
    return out


def h16_fixture(c):
    return two_blocks(c.hw, c.B) if c.fixture == 'nb2' else (split_probe if c.fixture == 'split' else probe)(c.l, c.hw, c.B)


def h16_id(c):
    return f"{c.fixture}{'' if c.l is None else c.l}-{c.hw[0]}x{c.hw[1]}-b{c.B}-{c.kernel}"


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
