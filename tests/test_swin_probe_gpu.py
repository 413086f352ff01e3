"""The SwinIR trunks on the GPU against the float64 reference of tests/swin_probe.py, with adversarial norms, bias tables and biases, at
the widths, windows and map sizes where the kernels take another path (swin_probe.KINDS / CASES).

  fp32 trunk (ciaosr_swinir_forward_f32)            max |got - ref64| <= 8 * e32
  f16-linear trunk (ciaosr_swinir_forward_batch_f16) max |got - ref64| <= 8 * e32 + 2 * max |emu16 - checker32|

e32 is the fp32 PyTorch checker's own error against float64 on the same case, emu16 the CPU emulation of the half operands: nothing the
kernels compute enters a bound, and tests/test_swin_probe_host.py shows that every mutation of swin_probe.MUTATIONS exceeds them tenfold.
Every run asserts through hip_ops.profile that the intended kernels ran: the seven-launch block (2 LayerNorms per block + 2, one each of
qkv, attention, proj, fc1, fc2) and no *_f16 tag, or the five-launch block and at most two LayerNorm launches.  A failure names the worst
element, the quarter of the channel range and the window it falls in.

Measured on the MI355X (fp32: max |hip - float64| / e32, bound 8; f16: max |hip - float64| / the f16 bound, bound 1):

  case               fp32  f16      case               fp32  f16
  c180-24x24-B2      0.42  0.40     c512-16x24-B2      0.34  0.46
  c180-45x51-B2      0.40  0.52     c512-13x19-B2      0.31  0.44
  c180-8x20-B2       0.35  0.48     c60w4-12x12-B2     0.45  0.51
  c180-5x9-B2        0.50  0.48     c60w4-25x27-B2     0.45  0.45
  c180x2-16x24-B2    0.44  0.49     c60w4-4x12-B2      0.51  0.47
  c180x2-13x19-B2    0.43  0.51     c60w4-3x5-B2       0.53  0.50
  c60-24x24-B2       0.43  0.54     c60w6-18x18-B2     0.37  0.52
  c60-45x51-B2       0.37  0.50     c60w6-35x39-B2     0.45  0.44
  c60-8x20-B2        0.31  0.53     c60w6-6x16-B2      0.52  0.49
  c60-5x9-B2         0.38  0.45     c60w6-4x7-B2       0.44  0.48
  c64d32-16x24-B2    0.42  0.53     c60w7-21x21-B2     0.43  0.53
  c64d32-13x19-B2    0.38  0.53     c60w7-40x45-B2     0.38  0.48
  c8d2-16x24-B2      1.21  0.40     c60w7-7x18-B2      0.36  0.50
  c8d2-13x19-B2      1.09  0.45     c60w7-4x8-B2       0.67  0.45
  c240-16x24-B2      0.39  0.49     faint-13x19-B2     0.39  0.50
  c240-13x19-B2      0.37  0.49     c60-128x128-B1     0.86  0.47
  c288-16x24-B2      0.37  0.47     c60-128x136-B1     0.93  0.46
  c288-13x19-B2      0.34  0.45     c60-136x136-B1     1.18  0.52

The fp32 trunk is closer to float64 than the CPU checker on all but four cases (the 8- and 16-term sums of c8d2, where one rounding
decides, and the 18 496-token map): the margin of 8 was not needed, let alone raised.  The f16 trunk sits at the emulation's own error.

Checked once against three deliberately wrong kernels (wrong numbers only, every read in bounds; not kept): beta of a lane's second float4
read at the first one's index in layernorm_kernel, the same for gamma and beta in the LN staging of swin_linear_f16_kernel, and a bias row
pitch of 64 instead of N in window_attention_body.  Both routes of every c288, c512, c60w4, c60w6 and c60w7 case failed (32 tests, by hundreds to
tens of thousands of bounds) and nothing else did; the 26 SwinIR tests that existed before (test_swinir_h16_gpu.py, the swinir tests of test_hip_parity.py)
all passed on those kernels.
"""
import pytest
import torch

from tests import swin_probe as sp

pytestmark = pytest.mark.gpu

F32_TAGS = ('swin_qkv', 'swin_window_attention', 'swin_proj', 'swin_fc1', 'swin_fc2')
F16_TAGS = ('swin_qkv_f16', 'swin_window_attention', 'swin_proj_f16', 'swin_fc1_f16', 'swin_fc2_f16')

_gens = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _gen(dev, kind):
    """The generator of `kind` on the device, built once per module (swin_probe.trunk(kind), the references' source, stays on the CPU)."""
    if kind not in _gens:
        _gens[kind] = sp.build(kind).to(dev).eval()
        assert _gens[kind]._encoder_hip.supported()
    return _gens[kind]


def _launches():
    from ciaosr_amd import hip_ops
    return {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def _no_f16(tags):
    return not any(k.startswith('swin_') and k.endswith('_f16') for k in tags)


@pytest.mark.parametrize('case', sp.CASES, ids=sp.case_id)
def test_fp32_trunk_against_float64(dev, case):
    from ciaosr_amd import hip_ops
    kind, hw, B = case
    r = sp.reference(case)
    gen = _gen(dev, kind)
    n = len(sp.blocks(gen))
    x = r.x.to(dev)
    got = []
    for b in range(B):
        with hip_ops.profile():
            got.append(gen._encoder_hip.forward_hwc(x[b]))
        tags = _launches()
        assert tags.get('swin_layernorm') == 2 * n + 2 and all(tags.get(k) == n for k in F32_TAGS) and _no_f16(tags), (r.id, b, tags)
    got = torch.stack(got).permute(0, 3, 1, 2).cpu()
    assert got.shape == r.want.shape and torch.isfinite(got).all(), r.id
    err, where = sp.describe_worst(got, r.want, sp.KINDS[kind][2])
    print(f'swin probe fp32 {r.id}: max|hip - float64| = {err:.3e} = {err / r.e32:.2f} e32 (bound {sp.MARGIN} e32 = {r.bound32:.3e}, scale {r.scale:.3f})')
    assert err <= r.bound32, f'{r.id}: max|hip - float64| = {err:.3e} = {err / r.e32:.2f} e32 > {sp.MARGIN} e32 at {where}'


@pytest.mark.parametrize('case', sp.CASES, ids=sp.case_id)
def test_f16_linear_trunk_against_float64(dev, case):
    from ciaosr_amd import hip_ops
    kind, hw, B = case
    r = sp.reference(case)
    gen = _gen(dev, kind)
    enc = gen._encoder_hip
    n = len(sp.blocks(gen))
    opt = hip_ops.Options('f16', swin_h16=1)
    x = r.x.to(dev)
    with hip_ops.profile():
        got = enc.forward_hwc_batch(x, opt)
    tags = _launches()
    assert all(tags.get(k) == n for k in F16_TAGS) and tags.get('swin_layernorm', 0) <= 2, (r.id, tags)
    assert not any(k in tags for k in ('swin_qkv', 'swin_proj', 'swin_fc1', 'swin_fc2')), (r.id, tags)
    assert got.shape == (B,) + hw + (sp.KINDS[kind][0],)
    for b in range(B):
        single = enc.forward_hwc(x[b], opt)
        assert torch.equal(got[b], single), (r.id, b, (got[b] - single).abs().max().item())
    got = got.permute(0, 3, 1, 2).cpu()
    assert torch.isfinite(got).all(), r.id
    err, where = sp.describe_worst(got, r.want, sp.KINDS[kind][2])
    print(f'swin probe f16 {r.id}: max|hip - float64| = {err:.3e} = {err / r.bound16:.3f} of the bound {r.bound16:.3e} '
          f'({sp.MARGIN} e32 = {r.bound32:.3e} + 2 x emulation {r.d16:.3e})')
    assert err <= r.bound16, f'{r.id}: max|hip - float64| = {err:.3e} = {err / r.bound16:.3f} of the f16 bound at {where}'


def _kept(enc, ptr):
    """The tensor PackedSwinIR keeps alive behind a pointer of its struct."""
    return next(t for t in enc._keep if torch.is_tensor(t) and t.data_ptr() == ptr).cpu()


@pytest.mark.parametrize('kind', ['c180', 'c180x2', 'c8d2', 'c64d32', 'c60w4', 'c60w7'])
def test_packing(dev, kind):
    """What PackedSwinIR._build hands the kernels: qkv_b = bias * scale on its q part (the weights carry the scale too), the [heads][N][N]
    bias = the table gathered by the relative offsets of the two tokens (written out here, not read from relative_position_index), the four
    norms of the struct = the modules' parameters, the shift of every block.  Here and not in the host file: _build packs the convolutions
    through the device (encoder_hip._pack_conv), so it cannot run without one."""
    cpu = sp.trunk(kind)
    C, heads, ws = sp.KINDS[kind]
    N, d = ws * ws, C // heads
    enc = _gen(dev, kind)._encoder_hip
    st = enc.struct()
    assert (st.embed_dim, st.num_heads, st.window_size, st.hidden) == (C, heads, ws, 2 * C)
    assert torch.equal(_kept(enc, st.pe_norm_w), cpu.patch_embed.norm.weight.detach()) and torch.equal(_kept(enc, st.pe_norm_b), cpu.patch_embed.norm.bias.detach())
    assert torch.equal(_kept(enc, st.norm_w), cpu.norm.weight.detach()) and torch.equal(_kept(enc, st.norm_b), cpu.norm.bias.detach())
    ys, xs = torch.arange(N) // ws, torch.arange(N) % ws
    rel = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)         # [i][j]
    blocks = sp.blocks(cpu)
    assert st.num_groups * st.depth == len(blocks)
    for i, b in enumerate(blocks):
        sb = st.blocks[i]
        a = b.attn
        assert a.scale == d ** -0.5 and sb.shift == b.shift_size == (ws // 2 if i % 2 else 0)
        scale = torch.ones(3 * C)
        scale[:C] = a.scale
        bq = a.qkv.bias.detach()
        assert torch.equal(_kept(enc, sb.qkv_b), bq * scale) and not torch.equal(_kept(enc, sb.qkv_b), bq)
        wq = _kept(enc, sb.qkv_w)
        assert wq.shape == (3 * C, (C + 63) // 64 * 64) and torch.equal(wq[:, :C], a.qkv.weight.detach() * scale[:, None]) and not wq[:, C:].any()
        table = a.relative_position_bias_table.detach()
        want = torch.stack([table[rel, h] for h in range(heads)])
        got = _kept(enc, sb.bias)
        assert got.shape == (heads, N, N) and torch.equal(got, want), (kind, i)
        assert not torch.equal(got, want.transpose(1, 2)) and not torch.equal(got, want.roll(-1, 0))
        for ptr, p in ((sb.ln1_w, b.norm1.weight), (sb.ln1_b, b.norm1.bias), (sb.ln2_w, b.norm2.weight), (sb.ln2_b, b.norm2.bias),
                       (sb.proj_b, a.proj.bias), (sb.fc1_b, b.mlp.fc1.bias), (sb.fc2_b, b.mlp.fc2.bias)):
            assert torch.equal(_kept(enc, ptr), p.detach()), (kind, i)


@pytest.mark.parametrize('name', ['gamma_roll', 'beta_drop', 'norm1_for_norm2', 'head_swap', 'q_bias_unscaled'])
def test_the_bounds_have_teeth_on_the_device(dev, name):
    """The comparison itself, on the GPU: a trunk whose PARAMETERS carry one of the mutations that need no patched arithmetic, run through
    both routes and held against the UNCHANGED float64 answer, misses both bounds -- what a kernel or a packing with that defect would do.  At least 9 bounds: the mutated float64 answer is 10 or more away
    on this case (tests/test_swin_probe_host.py) and a right kernel at most one from it."""
    from ciaosr_amd import hip_ops
    r = sp.reference(sp.find_case('c60', (45, 51)))
    wrong = sp.build('c60')
    with torch.no_grad(), sp.MUTATIONS[name](wrong):
        pass
    enc = wrong.to(dev).eval()._encoder_hip
    x = r.x.to(dev)
    f32 = torch.stack([enc.forward_hwc(x[b]) for b in range(x.shape[0])]).permute(0, 3, 1, 2).cpu()
    f16 = enc.forward_hwc_batch(x, hip_ops.Options('f16', swin_h16=1)).permute(0, 3, 1, 2).cpu()
    e32, _ = sp.describe_worst(f32, r.want, 8)
    e16, _ = sp.describe_worst(f16, r.want, 8)
    print(f'swin probe teeth {name} on {r.id}: fp32 route {e32 / r.bound32:.0f} bounds, f16 route {e16 / r.bound16:.0f} bounds')
    assert e32 > (sp.SEPARATION - 1) * r.bound32 and e16 > (sp.SEPARATION - 1) * r.bound16, (name, e32, r.bound32, e16, r.bound16)
