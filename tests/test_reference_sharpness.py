"""The two references of the GPU tests test_csattn_oracle_gpu.py and test_dense_wide_emulation_gpu.py are sharp: a mutation of the
REFERENCE (the kernels are left alone; no GPU) of the kind those tests exist to catch moves it by more than the bound they apply, at
every size they run.

cs_attn: for the queries of the last row, the probabilities of two adjacent keys of the last key column change places
         (independent_refs.swap_two_keys).  Measured distance to the unmutated float64 oracle, goldens' recipe:
           C = 64, scale 2   0.023 .. 0.21 (output scale 1.66 .. 2.06): 230 .. 2100 x the fp32 bound TOL = 1e-4; at the four sizes
                             the 16-bit modes run, 1.3 x (90, 102), 1.8 x (45, 51), 7 x (194, 192) and 13 x (50, 150) the bf16
                             bound 0.01 x scale (the f16 bound is ten times tighter)
           C = 180           0.030 .. 0.19
           C = 64, scale 3   0.021;  scale 4  7.3e-4 (only the first row of the last 4-row block is inside the crop);  [2, 3, 4]  0.45
dense:   layer 0 of block 0 loses, for the outputs left of a 32-pixel tile boundary, the product of tap (1, 2) with the first halo
         column (independent_refs.rdn_trunk_16bit_emulation(drop_halo=...)).  Measured at one block of one layer: 0.031 .. 0.042 x the
         feature scale, 310 .. 420 x the bound 1e-4 x scale (and above the deeper trunks' yardstick too: the 12 x 12 kernels sit within
         6e-3 x scale of the emulation at 16 blocks of 8 layers, test_rdn_trunk_bf16_dense_layers).
The asserts ask for the applied bound to be exceeded (cs_attn: 5 x TOL and the loosest bound applied at the size; dense: 10 x).
One more CPU figure belongs here: how much of the 16-bit cs_attn bounds the modes' own rounding uses up."""
import pytest
import torch

from tests import independent_refs as refs
from tests.helpers import randn

TOL = 1e-4      # test_hip_parity.TOL, the fp32 bound of test_csattn_oracle_gpu.py

_BIG = {(194, 192), (190, 187)}     # ~20 s each for the pair of float64 runs
CSA_CASES = ([pytest.param(64, (2,), hw, marks=[pytest.mark.slow] if hw in _BIG else []) for hw in refs.C64_SIZES] +
             [pytest.param(180, (2,), hw) for hw in refs.C180_SIZES] +
             [pytest.param(64, scales, hw) for scales, hw in refs.OTHER_SCALES])


@pytest.mark.parametrize('C,scales,hw', CSA_CASES)
def test_swapped_keys_move_the_csattn_oracle_past_the_bound(C, scales, hw):
    att = refs.csattn_module(C, scales)
    x = refs.csattn_input(C, hw)
    want = refs.csattn_oracle64(att, x)
    mutated = refs.csattn_oracle64(att, x, prob_hook=refs.swap_two_keys(hw[0] - 1))
    moved, where = refs.worst_element(mutated, want)
    scale = want.abs().max().item()
    bound = 0.01 * scale if (C == 64 and tuple(scales) == (2,) and hw in refs.H16_SIZES) else TOL     # the loosest bound applied at this size
    print(f'cs_attn C={C} scales {list(scales)} {hw}: two swapped probabilities move the oracle by {moved:.3e} at {where} '
          f'(output scale {scale:.3f}; loosest bound applied {bound:.3e})')
    assert moved > 5 * TOL and moved > bound, (moved, bound)


@pytest.mark.parametrize('half', ['bf16', 'f16'])
@pytest.mark.parametrize('hw', [hw for hw in refs.H16_SIZES if hw not in _BIG])
def test_16bit_bounds_leave_room_for_the_modes_own_rounding(hw, half):
    """The 16-bit bounds of test_csattn_oracle_gpu.py (0.01 / 0.001 x scale) against what the modes' arithmetic costs by itself: the
    float64 oracle with the 1x1-conv outputs and the probabilities rounded to the type.  Measured 5.6e-3 .. 7.9e-3 x scale (bf16) and
    7.5e-4 .. 8.7e-4 x scale (f16) here, 5.9e-3 / 9.5e-4 at (194, 192): the bounds hold for a correct kernel but with little room in
    f16, so a size that misses them by a uniformly spread excess is to be judged against 2 x this emulation, not against the build."""
    att = refs.csattn_module(64)
    x = refs.csattn_input(64, hw)
    want = refs.csattn_oracle64(att, x)
    emu = refs.csattn_oracle64(att, x, prob_hook=refs.round_to(half), act_hook=refs.round_to(half))
    rel = (emu - want).abs().max().item() / want.abs().max().item()
    bound = 0.01 if half == 'bf16' else 0.001
    print(f'cs_attn C=64 {hw} {half}: rounding emulation sits {rel:.2e} x scale from the float64 oracle (bound {bound:g} x scale)')
    assert 0.1 * bound < rel < bound


@pytest.mark.parametrize('mode', ['f16-pairs', 'bf16-single'])
@pytest.mark.parametrize('hw', refs.WIDE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_dropped_halo_column_moves_the_dense_emulation_past_the_bound(hw, mode):
    """Both weight forms, one of each element type; the boundary is the last whole tile's right edge (x0 = the last multiple of 32
    below W), which on the ragged sizes is the edge towards the partial tile."""
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_hip_parity import _restorer
    model = _restorer('rdn', 4, torch.device('cpu'), dict(scale=4), blocks=1, layers=1)
    seeded_init_(model, seed=23, gain=1.6)
    params = {k[len('generator.'):]: v.detach().clone() for k, v in model.state_dict().items()}
    x = randn((1, 3) + hw, 78) * 0.3
    x0 = (hw[1] - 1) // 32 * 32
    with torch.no_grad():
        want = refs.rdn_trunk_16bit_emulation(x, params, 1, 1, mode)
        mutated = refs.rdn_trunk_16bit_emulation(x, params, 1, 1, mode, drop_halo=(x0, (1, 2)))
    scale = want.abs().max().item()
    d = (mutated - want).abs()
    print(f'dense {mode} {hw}: a dropped halo column at x = {x0} moves the emulation by max {d.max().item():.3e} = '
          f'{d.max().item() / scale:.2e} x scale (bound 1e-4 x scale = {1e-4 * scale:.3e})')
    assert d.max().item() > 10 * 1e-4 * scale
    cols = d.amax((0, 1, 2)).nonzero().flatten().tolist()
    assert cols and min(cols) >= x0 - 3 and max(cols) <= x0 + 1, cols      # one input column of one layer, seen through gff's 3 x 3
