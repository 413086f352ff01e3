"""The opt-in SwinIR trunk with f16 linears (Options.swin_h16, csrc/swinir_h16.hip), everything that needs no GPU: the two exports and
the grown structs, the option's way through hip_ops.Options, the argument checks of the forward entry (all of them run before any
launch, so they can be called with pointers that are never dereferenced), and the CPU EMULATION of what the kernels round -- the operands
of qkv / proj / fc1 / fc2 to IEEE half, products accumulated in fp64 -- held to the 0.01 dB gate through the oracle head.  The emulation
is also the reference error level of tests/test_swinir_h16_gpu.py."""
import contextlib
import ctypes as C
import math

import pytest
import torch

from ciaosr_amd import _lib, hip_ops

ERR_BAD_ARG, ERR_WORKSPACE = -1, -4
GT30_SEED = 30      # as tests/test_hip_parity.py: white noise that places GT' 30 dB from the reference output


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
def swin_linears(gen):
    """The four Linear modules of every Swin block of a LocalImplicitSRSWINIR generator."""
    return [m for layer in gen.layers for b in layer.residual_group.blocks for m in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]


@contextlib.contextmanager
def f16_linears(gen, dtype=torch.float16):
    """Inside the block, qkv / proj / fc1 / fc2 of every Swin block compute round16(x) . round16(W)^T + b with the products accumulated
    in fp64 (rounded to fp32 once at the end): the operand rounding of the f16 MFMA without any summation error of its own.  Everything
    else tests/torch_trunks.swinir_features evaluates -- LayerNorm, attention, GELU, the residual stream, the convolutions -- stays fp32."""
    mods = swin_linears(gen)

    def make(m):
        w = m.weight.detach().to(dtype).double()
        b = m.bias.detach().double()
        return lambda x: (x.to(dtype).double() @ w.t() + b).to(x.dtype)

    for m in mods:
        m.forward = make(m)
    try:
        yield
    finally:
        for m in mods:
            del m.forward


def emulated_features(gen, x):
    """(fp32 checker features, features with f16-rounded linear operands) of x [B,3,H,W], both on x's device."""
    from tests.torch_trunks import swinir_features
    with torch.no_grad():
        want = swinir_features(gen, x)
        with f16_linears(gen):
            emu = swinir_features(gen, x)
    return want, emu


# ---- exports, structs, the option ------------------------------------------------------------------------------------------------
def test_exports_version_and_struct_sizes():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 240
    res, args = _lib.SIGNATURES['ciaosr_swinir_workspace_bytes_batch_f16']
    assert res is C.c_size_t and args == [C.c_int, C.c_int, C.c_int, C.POINTER(_lib.SwinirWeightsT)]
    res, args = _lib.SIGNATURES['ciaosr_swinir_forward_batch_f16']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_lib.SwinirWeightsT), C.c_void_p,
                                       C.POINTER(_lib.OptionsT), C.c_void_p, C.c_size_t, C.c_void_p]
    assert hasattr(lib, 'ciaosr_swinir_workspace_bytes_batch_f16') and hasattr(lib, 'ciaosr_swinir_forward_batch_f16')
    assert C.sizeof(_lib.OptionsT) == lib.ciaosr_sizeof(b'ciaosr_options_t') > 0
    assert C.sizeof(_lib.SwinBlockT) == lib.ciaosr_sizeof(b'ciaosr_swin_block_t') > 0
    # csa_block_mb stays the last field (tests/test_csattn_blocks_host.py pins it): swin_h16 sits in front of it
    assert [f[0] for f in _lib.OptionsT._fields_[-2:]] == ['swin_h16', 'csa_block_mb']
    assert [f[0] for f in _lib.SwinBlockT._fields_[-4:]] == ['qkv_w16', 'proj_w16', 'fc1_w16', 'fc2_w16']


def test_header_declares_both_exports():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ciaosr_hip.h')).read()
    assert 'size_t ciaosr_swinir_workspace_bytes_batch_f16(int B, int H, int W, const ciaosr_swinir_weights_t* w);' in hdr
    assert 'int ciaosr_swinir_forward_batch_f16(const float* x_bchw, int B, int H, int W, const ciaosr_swinir_weights_t* w, float* feat_bhwc,' in hdr
    assert 'int swin_h16;' in hdr


def test_option_round_trips_and_acts_only_where_the_trunk_is_f16():
    from ciaosr_amd.swinir_hip import PackedSwinIR
    o = hip_ops.Options('f16', swin_h16=1)
    assert o.swin_h16 == 1 and o._c.swin_h16 == 1 and 'swin_h16=1' in repr(o)
    assert o.replace(precision='fp32').swin_h16 == 1 and o.replace(swin_h16=0).swin_h16 == 0
    assert o.replace(query_grid_w=5).swin_h16 == 1
    assert hip_ops.as_options(dict(precision='f16', swin_h16=1)).swin_h16 == 1
    assert hip_ops.Options().swin_h16 == 0 and 'swin_h16' not in repr(hip_ops.Options('f16'))
    acts = {m: PackedSwinIR.uses_h16(hip_ops.Options(m, swin_h16=1)) for m in hip_ops.PRECISIONS}
    assert acts == {'fp32': False, 'bf16': False, 'bf16-single': False, 'bf16x3': False, 'f16': True, 'f16-pairs': True, 'f16x3': False,
                    'f16x3-fast': True}
    assert not any(PackedSwinIR.uses_h16(hip_ops.Options(m)) for m in hip_ops.PRECISIONS)
    # out of range: refused by every entry point that takes options (options_ok), before any pointer is touched
    lib = _lib.load()
    assert lib.ciaosr_head_workspace_bytes_opt(8, 8, None, 4, hip_ops.Options(swin_h16=2).c_arg()) == 0


def test_restorer_follows_the_option():
    """The tile loops batch SwinIR tiles only when the option acts on what the generator really runs; 'bf16' runs as 'bf16x3' here."""
    from ciaosr_amd.restorer import SWIN_TILE_BATCH, trunk_batches
    from tests.test_host_logic import _swinir_ciaosr
    m = _swinir_ciaosr(dict(scale=4, tile=192, tile_overlap=32, precision='f16', hip_options=dict(swin_h16=1)))
    assert m.options().swin_h16 == 1 and trunk_batches(m.generator, m.options())
    assert m.tile_batch() == SWIN_TILE_BATCH and SWIN_TILE_BATCH in (1, 2, 4, 7, 8)
    m.test_cfg['tile_batch'] = 3
    assert m.tile_batch() == 3
    for prec in ('fp32', 'f16x3', 'bf16', 'bf16x3'):
        m.test_cfg['precision'] = prec
        assert not trunk_batches(m.generator, m.options()), prec
    m.test_cfg['precision'] = 'f16'
    m.test_cfg.pop('hip_options')
    assert not trunk_batches(m.generator, m.options())
    assert m.generator._encoder_hip.trunk_half(m.options()) is None


# ---- argument checks of the entry points -------------------------------------------------------------------------------------------
class _Fake:
    """A weights struct whose device pointers are never dereferenced: every check under test runs on the host before any launch."""

    def __init__(self, C_=180, heads=6, hidden=360, groups=1, depth=2, w16=True):
        ld = (C_ + 63) // 64 * 64
        P = 0x10000                                        # 16-byte aligned, never read
        st = _lib.SwinirWeightsT()
        st.embed_dim, st.num_heads, st.window_size, st.hidden, st.num_groups, st.depth = C_, heads, 8, hidden, groups, depth
        for cv, cin in ((st.conv_first, 3), (st.conv_after_body, ld)):
            cv.weight, cv.bias, cv.cin, cv.cout, cv.ksize = P, P, cin, C_, 3
        st.pe_norm_w = st.pe_norm_b = st.norm_w = st.norm_b = P
        self.blocks = (_lib.SwinBlockT * (groups * depth))()
        for sb in self.blocks:
            for name, _ in _lib.SwinBlockT._fields_:
                if name not in ('shift', 'mask') and (w16 or not name.endswith('16')):
                    setattr(sb, name, P)
        self.gconv = (_lib.ConvT * groups)()
        for cv in self.gconv:
            cv.weight, cv.bias, cv.cin, cv.cout, cv.ksize = P, P, ld, C_, 3
        st.blocks, st.group_conv = self.blocks, self.gconv
        self.st = st

    def bytes(self, B, H, W):
        return _lib.load().ciaosr_swinir_workspace_bytes_batch_f16(B, H, W, C.byref(self.st))

    def forward(self, B, H, W, ws_bytes=None, opt=None):
        P = 0x10000
        n = self.bytes(max(B, 1), H, W) if ws_bytes is None else ws_bytes
        return _lib.load().ciaosr_swinir_forward_batch_f16(P, B, H, W, C.byref(self.st), P, opt, P, n, None)


def test_workspace_bytes_zero_for_bad_arguments_and_increasing_in_b():
    f = _Fake()
    lib = _lib.load()
    assert lib.ciaosr_swinir_workspace_bytes_batch_f16(1, 48, 48, None) == 0
    assert f.bytes(0, 48, 48) == 0 and f.bytes(-1, 48, 48) == 0 and f.bytes(1, 0, 48) == 0 and f.bytes(1, 48, -3) == 0
    bad = _Fake()
    bad.st.window_size = 0
    assert bad.bytes(1, 48, 48) == 0
    for hw in ((48, 48), (45, 51), (192, 192)):
        sizes = [f.bytes(B, *hw) for B in range(1, 10)]
        assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    # the fp32 entry's byte count is untouched by the new one
    assert lib.ciaosr_swinir_workspace_bytes(48, 48, C.byref(f.st)) > 0


def test_forward_refuses_bad_arguments_before_any_launch():
    assert _Fake().forward(0, 48, 48) == ERR_BAD_ARG                               # B = 0
    assert _Fake().forward(-2, 48, 48) == ERR_BAD_ARG
    assert _Fake(C_=90, heads=3, hidden=180).forward(1, 48, 48) == ERR_BAD_ARG     # C not a multiple of 4
    assert _Fake(C_=180, heads=12).forward(1, 48, 48) == ERR_BAD_ARG               # head dimension 15: odd
    assert _Fake(C_=180, heads=5).forward(1, 48, 48) == ERR_BAD_ARG                # head dimension 36 > 32
    assert _Fake(w16=False).forward(1, 48, 48) == ERR_BAD_ARG                      # no f16 weight pointers (the fp32 struct)
    one = _Fake()
    one.blocks[1].fc2_w16 = None
    assert one.forward(2, 48, 48) == ERR_BAD_ARG                                   # one of them missing
    assert _Fake().forward(1, 4, 48) == ERR_BAD_ARG                                # reflect padding needs pad < size
    assert _Fake().forward(1, 48, 48, opt=hip_ops.Options(swin_h16=2).c_arg()) == ERR_BAD_ARG
    shifted = _Fake()
    shifted.blocks[1].shift = 4                                                    # a shifted block without its mask
    assert shifted.forward(1, 48, 48) == ERR_BAD_ARG
    f = _Fake()
    need = f.bytes(2, 45, 51)
    assert f.forward(2, 45, 51, ws_bytes=need - 1) == ERR_WORKSPACE                # a too-small workspace
    assert f.forward(2, 45, 51, ws_bytes=f.bytes(1, 45, 51)) == ERR_WORKSPACE
    assert f.forward(1, 48, 48, ws_bytes=0) == ERR_WORKSPACE


# ---- the emulation against the gate -----------------------------------------------------------------------------------------------
def test_f16_linears_emulation_meets_the_psnr_gate_on_the_c5_fixture():
    """swinir_c5 (LR 24 x 24, x3.3, the fixture's seeded weights): features of the fp32 checker and of the emulation through the oracle
    head; |PSNR(emulated, GT) - PSNR(fp32, GT)| <= 0.01 dB against the synthetic GT and against GT' = fp32 output + 30 dB noise."""
    from ciaosr_amd.coords import make_coord, make_cell
    from ciaosr_amd.init_utils import seeded_init_, synthetic_pair
    from ciaosr_amd.metrics import psnr_tensors
    from oracle import ciaosr_oracle as orc
    from tests.helpers import load_golden
    from tests.test_host_logic import _swinir_ciaosr
    fx = load_golden('swinir_c5')
    model = _swinir_ciaosr(dict(scale=3.3))
    assert seeded_init_(model, seed=int(fx['weight_seed']), gain=float(fx['gain']), head_gain=math.sqrt(6.0)) == str(fx['sha'])
    lq = torch.from_numpy(fx['lq'])
    ht, wt = [int(v) for v in fx['target']]
    coord, cell = make_coord((ht, wt)).unsqueeze(0), make_cell((ht, wt)).unsqueeze(0)
    mean = torch.tensor(model.rgb_mean).view(1, 3, 1, 1)
    x = lq - mean
    want, emu = emulated_features(model.generator, x)
    scale = want.abs().max().item()
    d = (emu - want).abs().max().item()
    params = {k[len('generator.'):]: v.detach() for k, v in model.state_dict().items()}

    def image(feat):
        pred = orc.generator_forward(x, coord, cell, params, feature=feat)
        return (pred + mean.view(1, 1, 3)).clamp(0, 1).view(1, ht, wt, 3).permute(0, 3, 1, 2).contiguous()

    ref, out = image(want), image(emu)
    assert (ref - torch.from_numpy(fx['out'])).abs().max().item() < 1e-3          # the checker + oracle head IS the fixture's image
    _, gt = synthetic_pair(24, 24, 3.3)
    d_psnr = abs(psnr_tensors(out, gt, crop_border=3) - psnr_tensors(ref, gt, crop_border=3))
    gt30 = ref.double() + torch.randn(ref.shape, generator=torch.Generator().manual_seed(GT30_SEED), dtype=torch.float64) * 10 ** (-30 / 20)
    psnr30 = lambda a: -10 * math.log10((a.double() - gt30).pow(2).mean().item())
    d_psnr30 = abs(psnr30(out) - psnr30(ref))
    print(f'f16 linears emulated, swinir_c5 24x24: features max|d| {d:.3e} (scale {scale:.3f}), image max|d| {(out - ref).abs().max().item():.3e}, '
          f'PSNR delta vs GT {d_psnr:.5f} dB, at 30 dB {d_psnr30:.5f} dB')
    assert 0 < d < 1e-3 * max(scale, 1.0)          # the emulation rounds something, and stays at the half-precision level
    assert d_psnr <= 0.01 and d_psnr30 <= 0.01, (d_psnr, d_psnr30)
    assert not any('forward' in m.__dict__ for m in swin_linears(model.generator))     # the patch is undone
