"""The float64 reference and the bounds of tests/swin_probe.py tell a wrong SwinIR trunk from a right one -- shown on the CPU, before any kernel
is involved.  Bounds: fp32 route MARGIN * e32 (e32 = the fp32 checker's own error against float64 on that case, MARGIN = 8), f16 route
MARGIN * e32 + 2 * max |emu16 - checker32|.  Every mutation of swin_probe.MUTATIONS moves the float64 answer by at least 10 fp32 bounds
on every case it is aimed at (swin_probe.TARGETS); the F16_MUST subset by 10 f16 bounds on at least one of them.

Measured on the CPU (min over the mutation's cases of |ref64 mutated - ref64| / fp32 bound; max over them of the same / f16 bound):

  mutation                  fp32     f16      mutation                  fp32     f16
  gamma_roll               22 600   1 717     shift_sign                6 090     331
  beta_drop                21 960     883     q_bias_unscaled           2 000     133
  norm1_for_norm2          12 180     564     gelu_tanh                    18     0.2   fp32 route only
  unbiased_var                240     158     pad_replicate            50 840   2 043
  eps_1e-6 (faint)         28 170     452     pad_symmetric            49 950   2 007
  bias_transposed           6 610     373     rstb_residual_late       44 160   1 476
  head_swap                 6 610     391     final_residual_dropped   26 220   1 054
  mask_neighbour            4 810     331     ln_chunk2_zero           12 600     592
  mask_dropped              4 370     201     ln_float4_2_zero         22 600   2 038

fp32 route only: gelu_tanh (0.2 f16 bounds: |gelu_tanh - gelu_erf| <= 5e-4 lies under the rounding of the half operands).  It is aimed at the
cases whose fp32 bound is smallest -- c8d2 (sums of 8 and 16 terms) and the three big c60 maps -- because on the wide trunks it reaches
only 2.4 (c512) to 9 (c60) fp32 bounds; the GELU epilogues (gemm_small_f32, the 1x1 implicit GEMM, the f16 linear) do not depend on C."""
import pytest
import torch

from tests import swin_probe as sp


def _ref(kind, hw):
    return sp.reference(sp.find_case(kind, hw))


@pytest.mark.parametrize('case', sp.CASES, ids=sp.case_id)
def test_bounds_are_positive_and_tighter_than_the_old_one(case):
    """e32 and the emulation error are real numbers of the fp32 / half level, and MARGIN * e32 is below the bound the existing trunk tests
    use, 2e-4 * max(scale, 1)."""
    r = sp.reference(case)
    print(f'{r.id}: scale {r.scale:.3f}, e32 {r.e32:.3e}, fp32 bound {r.bound32:.3e}, |emu16 - checker32| {r.d16:.3e}, f16 bound {r.bound16:.3e}')
    assert torch.isfinite(r.want).all() and r.want.shape == (case[2], sp.KINDS[case[0]][0]) + case[1]
    assert 0 < r.e32 < 1e-5 * max(r.scale, 1.0)
    assert r.bound32 == sp.MARGIN * r.e32 and r.bound32 < 2e-4 * max(r.scale, 1.0)
    assert r.e32 < r.d16 < 1e-3 * max(r.scale, 1.0)
    assert r.bound16 == sp.MARGIN * r.e32 + 2 * r.d16
    assert sp.MARGIN <= 32


def test_every_mutation_has_cases_and_every_route_kind_its_four_maps():
    assert set(sp.TARGETS) == set(sp.MUTATIONS) and all(sp.TARGETS.values()) and set(sp.F16_MUST) <= set(sp.MUTATIONS)
    for kind in sp.ROUTE_KINDS:
        ws = sp.KINDS[kind][2]
        maps = [c[1] for c in sp.CASES if c[0] == kind]
        assert maps[0] == tuple(sp.trunk(kind).layers[0].residual_group.blocks[1].input_resolution)        # the blocks' own attn_mask
        assert maps[1][0] % ws and maps[1][1] % ws                                                          # reflect padding on both axes
        assert maps[2][0] == ws and maps[3] == (ws // 2 + 1, ws + 1)
        assert all(-h % ws < h and -w % ws < w for h, w in maps)                                            # legal: pad < size
        assert all(b.shift_size == (ws // 2 if i % 2 else 0) for i, b in enumerate(sp.blocks(sp.trunk(kind))))
    assert [c[1][0] * c[1][1] for c in sp.CASES[-3:]] == [16384, 17408, 18496]      # around gemm_small_ok (16 384) and conv3x3_small_ok (18 432)
    assert sp.find_case('c180x2', (16, 24)) and len(sp.trunk('c180x2').layers) == 2
    for kind in ('c240', 'c288'):
        assert sp.KINDS[kind][0] > sp.LKC
    assert sp.KINDS['c288'][0] > 256 and sp.KINDS['c512'][0] == 512


@pytest.mark.parametrize('name,kind,hw', [(n, k, hw) for n, t in sp.TARGETS.items() for k, hw in t])
def test_mutation_separates_from_the_fp32_bound(name, kind, hw):
    r = _ref(kind, hw)
    d = r.mutated(name)
    print(f'{name} on {r.id}: |ref64 mutated - ref64| = {d:.3e} = {d / r.bound32:.1f} fp32 bounds = {d / r.bound16:.2f} f16 bounds')
    assert d >= sp.SEPARATION * r.bound32, (name, r.id, d, r.bound32)


@pytest.mark.parametrize('name', sp.F16_MUST)
def test_mutation_separates_from_the_f16_bound(name):
    ratios = {}
    for kind, hw in sp.TARGETS[name]:
        r = _ref(kind, hw)
        ratios[r.id] = r.mutated(name) / r.bound16
    print(f'{name}: f16 bounds {ratios}')
    assert max(ratios.values()) >= sp.SEPARATION, (name, ratios)


def test_the_mutations_leave_no_patch_behind():
    """After a mutated evaluation tests.torch_trunks is what it was, and the shared trunk's parameters are untouched."""
    from tests import torch_trunks as tt
    r = _ref('c60', (5, 9))
    keep = (tt.torch, tt.F, tt._window_attention)
    sd = {k: v.clone() for k, v in sp.trunk('c60').state_dict().items()}
    for name in sp.MUTATIONS:
        r.mutated(name)
    assert (tt.torch, tt.F, tt._window_attention) == keep
    assert all(torch.equal(v, sd[k]) for k, v in sp.trunk('c60').state_dict().items())
    assert torch.equal(sp.ref64(sp.trunk('c60'), r.x), r.want)


@pytest.mark.parametrize('kind', list(sp.KINDS))
def test_adversarial_parameters_are_all_distinct(kind):
    """No LayerNorm weight or bias vector, bias-table slice or linear bias of any block is constant or equal to another's; the channels of a
    LayerNorm weight are all distinct and lie in [0.5, 1.5]."""
    g = sp.trunk(kind)
    vecs = {}
    for n, m in sp.layer_norms(g):
        w = m.weight.detach()
        assert w.unique().numel() == w.numel() and 0.5 <= w.min() and w.max() <= 1.5, n
        assert (w - 1).abs().max() > 0.25 and m.bias.detach().abs().max() > 0.15, n
        vecs[n + '.weight'], vecs[n + '.bias'] = w, m.bias.detach()
    for i, b in enumerate(sp.blocks(g)):
        table = b.attn.relative_position_bias_table.detach()
        assert table.std() > 0.5
        for h in range(table.shape[1]):
            vecs[f'block{i}.table.head{h}'] = table[:, h]
        for n, lin in (('qkv', b.attn.qkv), ('proj', b.attn.proj), ('fc1', b.mlp.fc1), ('fc2', b.mlp.fc2)):
            vecs[f'block{i}.{n}.bias'] = lin.bias.detach()
    for n, cv in [('conv_first', g.conv_first), ('conv_after_body', g.conv_after_body)] + [(f'layers.{i}.conv', l.conv) for i, l in enumerate(g.layers)]:
        vecs[n + '.bias'] = cv.bias.detach()
    if kind == 'faint':
        assert not vecs.pop('conv_first.bias').any()
    names = sorted(vecs)
    for n in names:
        assert vecs[n].std() > 0, f'{n} is constant'
    for i, a in enumerate(names):
        for b_ in names[i + 1:]:
            if vecs[a].shape == vecs[b_].shape:
                assert not torch.equal(vecs[a], vecs[b_]), (a, b_)


def test_gathered_bias_is_not_symmetric_and_differs_between_heads():
    """What makes the transposed table and the swapped head visible: the gathered [heads][N][N] bias is neither symmetric nor shared."""
    for kind in ('c60', 'c60w4', 'c60w6', 'c60w7'):
        a = sp.blocks(sp.trunk(kind))[0].attn
        N = sp.KINDS[kind][2] ** 2
        bias = a.relative_position_bias_table[a.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1)
        assert (bias - bias.transpose(1, 2)).abs().max() > 1 and (bias[0] - bias[1]).abs().max() > 1


def test_faint_case_puts_the_token_variance_at_eps():
    g = sp.trunk('faint')
    x = sp.case_input(sp.find_case('faint', (13, 19)))
    with torch.no_grad():
        t = g.conv_first(torch.nn.functional.pad(x, (0, 5, 0, 3), mode='reflect'))
    var = t.var(dim=1, unbiased=False)
    assert not g.conv_first.bias.any() and 0 < g.probe_image_scale < 0.1
    assert sp.LN_EPS / 3 < var.mean().item() < 3 * sp.LN_EPS, var.mean().item()


def test_every_kind_is_supported_and_a_516_wide_trunk_is_not():
    """Every kind of the table is accepted (none refused).  embed_dim 516 = 43 heads of 12 meets every other condition and is refused with
    the sentence that says why: both C entry points enforce C <= 512 (a token's values in one wavefront's registers)."""
    for kind in sp.KINDS:
        assert sp.trunk(kind)._encoder_hip.supported(), kind
    wide = sp.build((516, 43, 8))._encoder_hip
    assert not wide.supported()
    assert 'embed_dim <= 512' in wide.why_unsupported() and 'embed_dim=516' in wide.why_unsupported()
    assert 'embed_dim <= 512' in sp.trunk('c512')._encoder_hip.why_unsupported()
    assert sp.build((512, 16, 8))._encoder_hip.supported()


@pytest.mark.parametrize('name', ['gamma_roll', 'beta_drop', 'norm1_for_norm2', 'head_swap', 'q_bias_unscaled'])
def test_parameter_mutations_separate_on_the_case_the_device_test_uses(name):
    """tests/test_swin_probe_gpu.py runs these five (they change parameters only) through the kernels on c60 (45, 51): there they are 10 of
    either bound away."""
    r = _ref('c60', (45, 51))
    d = r.mutated(name)
    assert d >= sp.SEPARATION * r.bound32 and d >= sp.SEPARATION * r.bound16, (name, d, r.bound32, r.bound16)
