"""References that share no code with the HIP kernels, for the GPU tests that hold cs_attn and the 16-bit wide dense kernel to them
(test_csattn_oracle_gpu.py, test_dense_wide_emulation_gpu.py), and the mutations that show on the CPU that those references are sharp
(test_reference_sharpness.py).  Nothing here needs a GPU.

cs_attn:  oracle.ciaosr_oracle.cross_scale_attention in float64 (2.6e-6 .. 4.0e-6 from the four committed `csattn_c64_*` reference
          outputs, test_oracle_pin.py::test_csattn_c64_float64).  Hooks on its softmax and its PReLU outputs give the mutated oracle (two
          probabilities swapped) and the emulation of the 16-bit modes (1x1-conv outputs and probabilities rounded to the type).
dense:    the torch-CPU RDN trunk with the 16-bit modes' rounding points (test_hip_parity._rdn_trunk_bf16_emulation), extended to
          'f16-pairs' and to a mutation that drops one halo column of one tap.
"""
import contextlib

import torch

from oracle import ciaosr_oracle as orc
from tests.helpers import randn

# ------------------------------------------------------------------------------------------------
# cs_attn
# ------------------------------------------------------------------------------------------------
# the sizes test_csattn_oracle_gpu.py runs (scale 2, C = 64); L = (Hp / 2) * (Wp / 2) keys per query
C64_SMALL = [(64, 70), (58, 54), (48, 40), (45, 51)]          # below 4096 padded pixels but (64, 70): the composed tail is forced
C64_SIZES = C64_SMALL + [
    (50, 150), (40, 200),
    (90, 102),      # L = 2295, L % 4 = 3: the masked tail of the register-resident softmax kernels
    (108, 76),      # L = 2052: just past the loop -> register switch (Lld / 4 > 512)
    (128, 64),      # L = 2048: just before it
    (194, 192),     # L = 9312: past the register kernels' limit (Lld / 4 <= 2304)
    (190, 187),     # L = 8930, reflect-padded: the largest row the register kernels take in the suite
]
C180_SIZES = [(64, 64), (66, 67), (96, 96)]
OTHER_SCALES = [((3,), (50, 47)), ((4,), (45, 54)), ((2, 3, 4), (30, 34))]
H16_SIZES = [(50, 150), (90, 102), (45, 51), (194, 192)]


def csattn_module(channel, scales=(2,), seed=3, gain=1.5, default_init=False):
    """The project's CrossScaleAttention (CPU) with the goldens' peaked recipe (tools/make_golden.py: seeded_init_(seed 3, gain 1.5)),
    or -- `default_init` -- torch's default initialisation under manual_seed(5), the broad-softmax regime of the route sweeps."""
    from ciaosr_amd.init_utils import seeded_init_
    from ciaosr_amd.nonlocal_attn import CrossScaleAttention
    if default_init:
        torch.manual_seed(5)
        return CrossScaleAttention(channel=channel, scale=list(scales)).eval()
    att = CrossScaleAttention(channel=channel, scale=list(scales)).eval()
    seeded_init_(att, seed=seed, gain=gain)
    return att


def csattn_input(channel, hw, seed=33, default_init=False):
    """Unscaled white noise (the goldens' input); randn(seed 91) * 0.5 with the default-init module."""
    return randn((1, channel) + tuple(hw), 91) * 0.5 if default_init else randn((1, channel) + tuple(hw), seed)


class _HookedF:
    """torch.nn.functional with the oracle's softmax and prelu results passed through hooks."""

    def __init__(self, prob_hook=None, act_hook=None):
        self._prob, self._act = prob_hook, act_hook

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def softmax(self, *a, **kw):
        p = torch.nn.functional.softmax(*a, **kw)
        return self._prob(p) if self._prob else p

    def prelu(self, *a, **kw):
        y = torch.nn.functional.prelu(*a, **kw)
        return self._act(y) if self._act else y


@contextlib.contextmanager
def _hooked_oracle(prob_hook, act_hook):
    keep = orc.F
    orc.F = _HookedF(prob_hook, act_hook)
    try:
        yield
    finally:
        orc.F = keep


def csattn_oracle64(att, x, prob_hook=None, act_hook=None):
    """float64 oracle of `att` (a CrossScaleAttention module, any device) on x [1,C,H,W]; returns float64 [1, ns*C, H, W] on the CPU.
    prob_hook(prob [1, L, Hp, Wp]) / act_hook(y) replace the softmax / the 1x1-conv + PReLU outputs."""
    P = {'cs_attn.' + k: v.detach().cpu().double() for k, v in att.state_dict().items()}
    with torch.no_grad(), _hooked_oracle(prob_hook, act_hook):
        return orc.cross_scale_attention(x.detach().cpu().double(), P, scales=tuple(att.scale), softmax_scale=float(att.softmax_scale))


def swap_two_keys(row):
    """The mutation of the sharpness check, as a softmax hook: for the queries of one row of the padded map, the probabilities of two
    vertically adjacent keys of the LAST key column change places -- what a kernel does that mis-indexes one key of a ragged last tile.
    `row` is the last row of the map, H - 1: the last padded row where H needs no padding, and the last one that reaches the cropped
    output where it does (at scale 4 the padded rows past H contribute to no output pixel).  Of the Hp/s - 1 adjacent pairs of that
    column, the one whose two probabilities differ most over those queries: with the peaked softmax of the goldens' recipe (3 to 4
    effective keys of thousands) most pairs hold two zeros, and swapping two zeros mutates nothing."""
    def hook(prob):
        _, L, Hp, Wp = prob.shape
        s = int(round((Hp * Wp / L) ** 0.5))
        hr, wr = Hp // s, Wp // s
        assert hr * wr == L and hr >= 2 and row < Hp
        last = prob[0].view(hr, wr, Hp, Wp)[:, wr - 1, row, :]                     # [hr][Wp]: last key column, the row's queries
        a = int((last[1:] - last[:-1]).abs().sum(1).argmax())
        k1 = a * wr + wr - 1
        k2 = k1 + wr
        out = prob.clone()
        out[0, k1, row, :] = prob[0, k2, row, :]
        out[0, k2, row, :] = prob[0, k1, row, :]
        return out
    return hook


def round_to(half):
    """x -> x rounded to bf16 / IEEE half, kept in x's dtype."""
    t = torch.bfloat16 if half == 'bf16' else torch.float16
    return lambda v: v.float().to(t).to(v.dtype)


def worst_element(got, want):
    """(max |got - want|, 'row r col c channel k') for [1, C, H, W] tensors."""
    d = (got.double() - want.double()).abs()[0]
    i = int(d.argmax())
    c, rem = divmod(i, d.shape[1] * d.shape[2])
    r, col = divmod(rem, d.shape[2])
    return d.max().item(), f'row {r} col {col} channel {c}'


# ------------------------------------------------------------------------------------------------
# 16-bit dense layers of the RDN trunk
# ------------------------------------------------------------------------------------------------
WIDE_SIZES = [(150, 170), (192, 192), (24, 1040), (129, 257)]
WIDE_MODES = ['f16', 'f16-pairs', 'bf16', 'bf16-single']


def wide_tiles(hw):
    """Tiles of 16 x 32 pixels; the wide kernel runs from 32 on (dense_h16_wide_ok, csrc/dense_h16.hip)."""
    return -(-hw[0] // 16) * -(-hw[1] // 32)


def rdn_trunk_16bit_emulation(x, P, nb, nl, mode, drop_halo=None):
    """torch-CPU RDN trunk with the rounding points of a 16-bit trunk mode (csrc/encoder.hip, rdn_forward):

      every mode   dense-layer inputs rounded to the element type; products exact in fp32, fp32 accumulation; sfe / gff convolutions fp32
      'bf16'       weights as the pair bf16(w) + bf16(w - bf16(w)); the 1x1 local feature fusion in fp32 on the fp32 layer outputs
      'bf16-single' weights bf16(w) alone; fp32 fusion
      'f16'        weights half(w); the fusion reads the same 16-bit rows with half(w) weights, fp32 residual sum
      'f16-pairs'  weights half(w) + half(w - half(w)) (frag16_lo, encoder_hip.py); fp32 fusion like 'bf16' (Mode::lff16 is false for pairs)

    drop_halo = (x0, (ky, kx)): the mutation of the sharpness check -- in layer 0 of block 0, outputs of column x0 - 1 lose the product
    of tap (ky, kx) with the input column x0 = the first halo column right of a tile boundary (needs kx = 2)."""
    F = torch.nn.functional
    assert mode in WIDE_MODES
    half = (lambda t: t.half().float()) if mode.startswith('f16') else (lambda t: t.bfloat16().float())
    pair = lambda t: half(t) + half(t - half(t))
    wq = pair if mode in ('bf16', 'f16-pairs') else half
    sfe1 = F.conv2d(x, P['sfe1.weight'], P['sfe1.bias'], padding=1)
    cur = F.conv2d(sfe1, P['sfe2.weight'], P['sfe2.bias'], padding=1)
    outs = []
    for b in range(nb):
        feats = [cur]
        for l in range(nl):
            inp = torch.cat([half(f) for f in feats], 1)
            w = wq(P[f'rdbs.{b}.layers.{l}.conv.weight'])
            pre = F.conv2d(inp, w, P[f'rdbs.{b}.layers.{l}.conv.bias'], padding=1)
            if drop_halo is not None and b == 0 and l == 0:
                x0, (ky, kx) = drop_halo
                assert kx == 2 and 0 < x0 < inp.shape[-1]
                col = F.pad(inp, (0, 0, 1, 1))[:, :, ky:ky + inp.shape[-2], x0]             # input rows y + ky - 1 of column x0
                pre[:, :, :, x0 - 1] -= torch.einsum('oc,bch->boh', w[:, :, ky, kx], col)
            feats.append(F.relu(pre))
        if mode == 'f16':
            cur = cur + F.conv2d(torch.cat([half(f) for f in feats], 1), half(P[f'rdbs.{b}.lff.weight']), P[f'rdbs.{b}.lff.bias'])
        else:
            cur = cur + F.conv2d(torch.cat(feats, 1), P[f'rdbs.{b}.lff.weight'], P[f'rdbs.{b}.lff.bias'])
        outs.append(cur)
    g = F.conv2d(torch.cat(outs, 1), P['gff.0.weight'], P['gff.0.bias'])
    return F.conv2d(g, P['gff.1.weight'], P['gff.1.bias'], padding=1) + sfe1
