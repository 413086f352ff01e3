"""Probe trunks, adversarial parameters, float64 references and mutations for the SwinIR trunks (csrc/swinir.hip, csrc/swin_window.h,
csrc/swinir_h16.hip, the packing of ciaosr_amd/swinir_hip.py).  CPU only; tests/test_swin_probe_host.py shows on the CPU that the bounds
derived here tell a wrong trunk from a right one, tests/test_swin_probe_gpu.py holds the kernels to them.

  build(kind)            a LocalImplicitSRSWINIR generator with one of the KINDS trunks (mlp_ratio 2, '1conv', patch norm), small heads
  adversarial_(gen, s)   seeded_init_(gain 1.3), then LayerNorm weights 1 + 0.5 u (u uniform in [-1, 1]), LayerNorm biases 0.3 randn, bias
                         tables 1.0 randn, every Linear / Conv bias of the trunk 0.1 randn -- no two channels, heads or table entries a
                         kernel could confuse hold the same value (seeded_init_ leaves every norm at (1, 0))
  ref64(gen, x)          tests.torch_trunks.swinir_features on a float64 copy (the checker test_host_logic.py pins to the reference project)
  e32(gen, x)            max |swinir_features(fp32, CPU) - ref64|: the fp32 checker's own error on that case
  emu16(gen, x)          the f16_linears emulation of tests/test_swinir_h16_host.py on the same weights
  MUTATIONS              name -> context manager that patches the float64 copy: each stands for one defect of a kernel or of the packing
  CASES                  (kind, map, batch); x = randn(seed of the case) * 0.3

Bounds (nothing the code under test computes enters them):
  fp32 route   MARGIN * e32                                    MARGIN = 8: same arithmetic width as the checker, other summation orders
  f16 route    MARGIN * e32 + 2 * max |emu16 - checker32|      (sequential MFMA chains over up to 576 terms, split-K slabs), device expf /
                                                                erff / sqrtf good to a few ulp

Refused kinds: none -- LocalImplicitSRSWINIR and PackedSwinIR.supported() accept every kind of the table, windows 4, 6 and 7 included."""
import contextlib
import copy
import functools
import zlib

import torch
import torch.nn as nn
import torch.nn.functional as F

MARGIN = 8            # bound of the fp32 route in units of the fp32 checker's own error
SEPARATION = 10       # a mutation must move the float64 answer by this many bounds
LKC = 192             # K staged per pass by swin_linear_f16_kernel (csrc/swinir_h16.hip)

# kind -> (embed_dim, heads, window); every trunk: mlp_ratio 2, resi_connection '1conv', patch norm, img_size 3 windows
KINDS = {
    'c180': (180, 6, 8),       # the shipped width: ld 192, d 30; one unshifted and one shifted block
    'c180x2': (180, 6, 8),     # two groups: RSTB residual and the two token buffers
    'c60': (60, 6, 8),         # ld 64, hidden 120 padded to 128
    'c64d32': (64, 2, 8),      # head dim = WMAXD: no zero padding in LDS
    'c8d2': (8, 4, 8),         # smallest head dim, C much smaller than ld
    'c240': (240, 8, 8),       # ld 256: the f16 LN staging in chunks 192 + 64
    'c288': (288, 9, 8),       # n4 = 72: second float4 on 8 lanes; hidden 576 = three K chunks in fc2
    'c512': (512, 16, 8),      # the C <= 512 edge: every lane holds two float4
    'c60w4': (60, 6, 4),       # N = 16, shift 2
    'c60w6': (60, 6, 6),       # N = 36, shift 3
    'c60w7': (60, 6, 7),       # N = 49, shift 3
    'faint': (60, 6, 8),       # c60 with conv_first.bias = 0 and an image scale that puts the token variance after conv_first at eps
}
DEPTHS = {'c180x2': [2, 2]}
LN_EPS = 1e-5
ROUTE_KINDS = ('c180', 'c60', 'c60w4', 'c60w6', 'c60w7')
BIG_MAPS = ((128, 128), (128, 136), (136, 136))      # 16 384 tokens: the last on gemm_small_f32; 17 408: linears on the 1x1 implicit GEMM;
#                                                      18 496: the 3x3 convolutions leave conv3x3_small too


def _cases():
    out = []
    for kind, (_, _, ws) in KINDS.items():
        if kind in ROUTE_KINDS:
            # own img_size (the blocks' attn_mask buffers), reflect padding on both axes, one window row, the smallest legal map
            maps = [(3 * ws, 3 * ws), (5 * ws + 5, 6 * ws + 3), (ws, 2 * ws + 4), (ws // 2 + 1, ws + 1)]
        elif kind == 'faint':
            maps = [(13, 19)]
        else:
            maps = [(16, 24), (13, 19)]
        out += [(kind, hw, 2) for hw in maps]
    out += [('c60', hw, 1) for hw in BIG_MAPS]
    return out


CASES = _cases()


def case_id(case):
    kind, hw, B = case
    return f'{kind}-{hw[0]}x{hw[1]}-B{B}'


def find_case(kind, hw):
    return next(c for c in CASES if c[0] == kind and c[1] == tuple(hw))


def _gen(seed, name):
    from ciaosr_amd.init_utils import _gen as g
    return g(seed, name)


def trunk_modules(gen):
    return (gen.conv_first, gen.patch_embed, gen.layers, gen.norm, gen.conv_after_body)


def blocks(gen):
    return [b for layer in gen.layers for b in layer.residual_group.blocks]


def layer_norms(gen):
    """(name, module) of every LayerNorm of the trunk, in state_dict order."""
    return [(n, m) for n, m in gen.named_modules() if isinstance(m, nn.LayerNorm)]


@torch.no_grad()
def adversarial_(gen, seed):
    from ciaosr_amd.init_utils import seeded_init_
    seeded_init_(gen, seed, gain=1.3)
    trunk = {id(m) for top in trunk_modules(gen) for m in top.modules()}
    for name, m in gen.named_modules():
        if id(m) not in trunk:
            continue
        if isinstance(m, nn.LayerNorm):
            m.weight.copy_(1 + 0.5 * (2 * torch.rand(m.weight.shape, generator=_gen(seed, 'adv.' + name + '.weight')) - 1))
            m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=_gen(seed, 'adv.' + name + '.bias')))
        elif isinstance(m, (nn.Linear, nn.Conv2d)):
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=_gen(seed, 'adv.' + name + '.bias')))
        if hasattr(m, 'relative_position_bias_table'):
            t = m.relative_position_bias_table
            t.copy_(torch.randn(t.shape, generator=_gen(seed, 'adv.' + name + '.relative_position_bias_table')))
    return gen


def build(kind, seed=9):
    """The generator of `kind` on the CPU with adversarial parameters, built the way tests/test_swinir_h16_gpu.py::_trunk builds one.
    `kind` may also be an (embed_dim, heads, window) triple outside the table: built without asking supported()."""
    from ciaosr_amd import CiaoSR, LocalImplicitSRSWINIR
    from ciaosr_amd.encoders import SwinIR
    C, heads, ws = KINDS[kind] if isinstance(kind, str) else kind
    depths = DEPTHS.get(kind, [2]) if isinstance(kind, str) else [2]
    enc = dict(type=SwinIR, upscale=4, in_chans=3, img_size=3 * ws, window_size=ws, img_range=1., depths=depths, embed_dim=C,
               num_heads=[heads] * len(depths), mlp_ratio=2, upsampler='pixelshuffle', resi_connection='1conv')
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[64, 64])
    gen = dict(type=LocalImplicitSRSWINIR, window_size=ws, encoder=enc, imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64),
               feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                   test_cfg=dict(scale=4)).eval()
    g = adversarial_(model.generator, seed).eval()
    assert not isinstance(kind, str) or g._encoder_hip.supported(), g._encoder_hip.why_unsupported()
    g.probe_image_scale = 1.0
    if kind == 'faint':
        with torch.no_grad():
            g.conv_first.bias.zero_()
            t = g.conv_first(_randn_image((2, 3, 13, 19), 0))
            var = t.var(dim=1, unbiased=False).mean().item()          # over the channels of a token
        g.probe_image_scale = (LN_EPS / var) ** 0.5
    return g


@functools.lru_cache(maxsize=None)
def trunk(kind):
    """build(kind), once per process; never moved or changed (the GPU tests build their own and move that)."""
    return build(kind)


def _randn_image(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(seed))) * 0.3


def case_input(case):
    kind, hw, B = case
    return _randn_image((B, 3) + tuple(hw), zlib.crc32(case_id(case).encode()) % 100000) * trunk(kind).probe_image_scale


class _Trunk(nn.Module):
    """Deep copies of the parameter containers swinir_features reads -- not of the generator, whose packed structs hold ctypes pointers."""

    def __init__(self, gen):
        super().__init__()
        self.window_size = gen.window_size
        self.conv_first, self.patch_embed, self.layers, self.norm, self.conv_after_body = (copy.deepcopy(m).cpu() for m in trunk_modules(gen))


def _copy64(gen):
    return _Trunk(gen).double()


def ref64(gen, x, mutation=None):
    """swinir_features in float64 on the CPU on a deep copy of the generator; under MUTATIONS[mutation] when one is named."""
    from tests.torch_trunks import swinir_features
    g = _copy64(gen)
    with torch.no_grad(), (MUTATIONS[mutation](g) if mutation else contextlib.nullcontext()):
        return swinir_features(g, x.detach().cpu().double())


def checker32(gen, x):
    from tests.torch_trunks import swinir_features
    g = _Trunk(gen).float()
    with torch.no_grad():
        return swinir_features(g, x.detach().cpu().float())


def e32(gen, x):
    return (checker32(gen, x).double() - ref64(gen, x)).abs().max().item()


def emu16(gen, x):
    from tests.test_swinir_h16_host import f16_linears
    from tests.torch_trunks import swinir_features
    g = _Trunk(gen).float()
    with torch.no_grad(), f16_linears(g):
        return swinir_features(g, x.detach().cpu().float())


class Reference:
    """Everything the tests of one case share: the input, the float64 answer [B,C,H,W], the fp32 checker's error and the two bounds."""

    def __init__(self, case):
        self.case, self.id = case, case_id(case)
        gen = trunk(case[0])
        self.x = case_input(case)
        self.want = ref64(gen, self.x)
        chk = checker32(gen, self.x)
        self.e32 = (chk.double() - self.want).abs().max().item()
        self.d16 = (emu16(gen, self.x) - chk).abs().max().item()
        self.scale = self.want.abs().max().item()
        self.bound32 = MARGIN * self.e32
        self.bound16 = MARGIN * self.e32 + 2 * self.d16

    def mutated(self, name):
        """max |ref64 under the mutation - ref64|."""
        return (ref64(trunk(self.case[0]), self.x, name) - self.want).abs().max().item()


@functools.lru_cache(maxsize=None)
def reference(case):
    return Reference(case)


# ---- mutations -----------------------------------------------------------------------------------------------------------------
class _Proxy:
    """A module whose named attributes are replaced (tests.torch_trunks looks `torch` and `F` up at call time)."""

    def __init__(self, base, **over):
        self._base = base
        self.__dict__.update(over)

    def __getattr__(self, k):
        return getattr(self._base, k)


@contextlib.contextmanager
def _patched(**attrs):
    """tests.torch_trunks with module attributes replaced, restored on exit."""
    from tests import torch_trunks as tt
    keep = {k: getattr(tt, k) for k in attrs}
    for k, v in attrs.items():
        setattr(tt, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(tt, k, v)


@contextlib.contextmanager
def _hooks(handles):
    try:
        yield
    finally:
        for h in handles:
            h.remove()


def _block_norms(g):
    return [m for b in blocks(g) for m in (b.norm1, b.norm2)]


def _all_norms(g):
    return [m for _, m in layer_norms(g)]


@contextlib.contextmanager
def m_gamma_roll(g):
    """g4[t] read one channel off: LayerNorm weight rolled by one channel."""
    for m in _all_norms(g):
        m.weight.data = m.weight.data.roll(1)
    yield


@contextlib.contextmanager
def m_beta_drop(g):
    """b4[t] never added: LayerNorm bias dropped."""
    for m in _all_norms(g):
        m.bias.data.zero_()
    yield


@contextlib.contextmanager
def m_norm1_for_norm2(g):
    """ln1_w / ln1_b packed (or passed) for the second norm of the block."""
    for b in blocks(g):
        b.norm2.weight.data, b.norm2.bias.data = b.norm1.weight.data.clone(), b.norm1.bias.data.clone()
    yield


@contextlib.contextmanager
def m_unbiased_var(g):
    """Variance divided by C - 1."""
    def make(m):
        def fwd(x):
            mean = x.mean(-1, keepdim=True)
            var = (x - mean).pow(2).sum(-1, keepdim=True) / (x.shape[-1] - 1)
            return (x - mean) / (var + m.eps).sqrt() * m.weight + m.bias
        return fwd
    for m in _all_norms(g):
        m.forward = make(m)
    yield


@contextlib.contextmanager
def m_eps_1e6(g):
    """eps 1e-6 instead of nn.LayerNorm's 1e-5 (the `faint` case)."""
    for m in _all_norms(g):
        m.eps = 1e-6
    yield


@contextlib.contextmanager
def m_bias_transposed(g):
    """Packed bias [heads][N][N] with i and j swapped."""
    for b in blocks(g):
        b.attn.relative_position_index = b.attn.relative_position_index.t().contiguous()
    yield


@contextlib.contextmanager
def m_head_swap(g):
    """Bias slice of head h + 1 used for head h."""
    for b in blocks(g):
        b.attn.relative_position_bias_table.data = b.attn.relative_position_bias_table.data.roll(-1, 1)
    yield


def _mask_patch(fn):
    from tests import torch_trunks as tt
    orig = tt._window_attention
    return _patched(_window_attention=lambda a, xw, mask: orig(a, xw, None if mask is None else fn(mask)))


def m_mask_neighbour(g):
    """Mask of window w + 1 used for window w."""
    return _mask_patch(lambda m: m.roll(-1, 0))


def m_mask_dropped(g):
    """No mask on shifted blocks."""
    return _mask_patch(lambda m: None)


def m_shift_sign(g):
    """Tokens of a shifted block gathered (and scattered back) with shift of the opposite sign; the mask unchanged."""
    return _patched(torch=_Proxy(torch, roll=lambda x, shifts, dims: torch.roll(x, tuple(-s for s in shifts), dims)))


@contextlib.contextmanager
def m_q_bias_unscaled(g):
    """qkv_b packed without attn.scale on its q part (the weights carry the scale)."""
    for b in blocks(g):
        C = b.attn.qkv.bias.shape[0] // 3
        b.attn.qkv.bias.data[:C] /= b.attn.scale
    yield


def m_gelu_tanh(g):
    """tanh approximation of GELU instead of erf."""
    return _patched(F=_Proxy(F, gelu=lambda x: F.gelu(x, approximate='tanh')))


def m_pad_replicate(g):
    """Replicate padding of the image instead of reflect."""
    return _patched(F=_Proxy(F, pad=lambda x, p, mode: F.pad(x, p, 'replicate')))


def _pad_symmetric(x, p, mode):
    left, right, top, bottom = p
    assert left == 0 and top == 0
    if right:
        x = torch.cat([x, x[..., -right:].flip(-1)], -1)
    if bottom:
        x = torch.cat([x, x[..., -bottom:, :].flip(-2)], -2)
    return x


def m_pad_symmetric(g):
    """Edge-inclusive (`symmetric`) padding instead of reflect: 2 (H - 1) - y + 1."""
    return _patched(F=_Proxy(F, pad=_pad_symmetric))


def m_rstb_residual_late(g):
    """RSTB residual taken from the blocks' output instead of the group input (the two token buffers confused)."""
    handles = []
    for layer in g.layers:
        seen = {}
        first = layer.residual_group.blocks[0].norm1
        handles.append(first.register_forward_pre_hook(lambda m, args, seen=seen: seen.__setitem__('t', args[0])))

        def after(m, args, out, seen=seen):
            r = args[0]
            t = seen['t'].transpose(1, 2).reshape(r.shape)
            return out + r - t                    # the caller adds t: conv(r) + r
        handles.append(layer.conv.register_forward_hook(after))
    return _hooks(handles)


def m_final_residual_dropped(g):
    """The final `+ conv_first(x)` dropped."""
    seen = {}
    return _hooks([g.conv_first.register_forward_hook(lambda m, a, out: seen.__setitem__('x', out)),
                   g.conv_after_body.register_forward_hook(lambda m, a, out: out - seen['x'])])


def _zero_cols(mods, lo):
    def hook(m, a, out):
        out = out.clone()
        out[..., lo:] = 0
        return out
    return _hooks([m.register_forward_hook(hook) for m in mods])


def m_ln_chunk2_zero(g):
    """LN output columns [192, ld) zero in front of qkv and fc1: the second K chunk of the f16 LN staging lost."""
    return _zero_cols(_block_norms(g), LKC)


def m_ln_float4_2_zero(g):
    """LN output columns [256, C) zero: the second float4 of a lane lost."""
    return _zero_cols(_all_norms(g), 256)


MUTATIONS = {
    'gamma_roll': m_gamma_roll, 'beta_drop': m_beta_drop, 'norm1_for_norm2': m_norm1_for_norm2, 'unbiased_var': m_unbiased_var,
    'eps_1e-6': m_eps_1e6, 'bias_transposed': m_bias_transposed, 'head_swap': m_head_swap, 'mask_neighbour': m_mask_neighbour,
    'mask_dropped': m_mask_dropped, 'shift_sign': m_shift_sign, 'q_bias_unscaled': m_q_bias_unscaled, 'gelu_tanh': m_gelu_tanh,
    'pad_replicate': m_pad_replicate, 'pad_symmetric': m_pad_symmetric, 'rstb_residual_late': m_rstb_residual_late,
    'final_residual_dropped': m_final_residual_dropped, 'ln_chunk2_zero': m_ln_chunk2_zero, 'ln_float4_2_zero': m_ln_float4_2_zero,
}

_ODD = [('c180', (45, 51)), ('c60', (45, 51))]
_WINDOWS = [('c60w4', (25, 27)), ('c60w6', (35, 39)), ('c60w7', (40, 45))]
# mutation -> the (kind, map) cases it is aimed at; every one of them must separate from the fp32 bound of its case
TARGETS = {
    'gamma_roll': _ODD + [('c8d2', (13, 19)), ('c512', (13, 19))], 'beta_drop': _ODD, 'norm1_for_norm2': _ODD, 'unbiased_var': _ODD,
    'eps_1e-6': [('faint', (13, 19))],
    'bias_transposed': _ODD + _WINDOWS, 'head_swap': _ODD + _WINDOWS + [('c64d32', (13, 19))], 'mask_neighbour': _ODD + _WINDOWS,
    'mask_dropped': _ODD + _WINDOWS, 'shift_sign': _ODD + _WINDOWS, 'q_bias_unscaled': _ODD + [('c8d2', (13, 19)), ('c64d32', (13, 19))],
    'gelu_tanh': [('c8d2', (16, 24)), ('c8d2', (13, 19))] + [('c60', hw) for hw in BIG_MAPS], 'pad_replicate': _ODD + _WINDOWS, 'pad_symmetric': _ODD + _WINDOWS,
    'rstb_residual_late': [('c180x2', (16, 24)), ('c180x2', (13, 19))],
    'final_residual_dropped': _ODD,
    'ln_chunk2_zero': [('c240', (13, 19)), ('c288', (13, 19))], 'ln_float4_2_zero': [('c288', (13, 19)), ('c512', (13, 19))],
}
# the mutations that must also separate from the f16 bound on at least one of their cases
F16_MUST = ('gamma_roll', 'beta_drop', 'norm1_for_norm2', 'bias_transposed', 'head_swap', 'mask_neighbour', 'mask_dropped', 'shift_sign',
            'q_bias_unscaled', 'pad_replicate', 'pad_symmetric', 'ln_chunk2_zero', 'ln_float4_2_zero')


# ---- failure message -----------------------------------------------------------------------------------------------------------
def describe_worst(got, want, ws):
    """(max |got - want|, text) for [B,C,H,W] tensors: the worst element (image, channel, row, column) with the got / want values there,
    the quarter of the channel range it falls in (a LayerNorm lane defect stays in one) and its window (a window defect stays in one)."""
    d = (got.double() - want.double()).abs()
    i = int(d.argmax())
    _, C, H, W = d.shape
    b, c, y, x = i // (C * H * W), i // (H * W) % C, i // W % H, i % W
    text = (f'image {b} channel {c} row {y} column {x}: got {got[b, c, y, x].item()!r}, want {want[b, c, y, x].item()!r}; channel quarter '
            f'{min(4 * c // C, 3)} of 4 (C = {C}), window ({y // ws}, {x // ws}) of the unshifted grid, token ({y % ws}, {x % ws}) in it')
    return d.max().item(), text
