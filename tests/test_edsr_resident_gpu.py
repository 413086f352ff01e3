"""The opt-in EDSR trunk over tile batches (Options.edsr_resident -> ciaosr_edsr_forward_batch_f32: the body convolutions of a whole batch
on the halo-resident fp32 kernel of csrc/dense_f32.hip) on the GPU: the trunk against the CPU oracle at the bound the per-image trunk is
held to, batch == singles bitwise, option off == the old entry bitwise and launch for launch, the restorer's tile loops sharing the trunk
launches (counted), and the RDN instantiation of the generalised kernel against bits recorded from the commit before it."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, SQRT6, randn

pytestmark = pytest.mark.gpu

ON = dict(edsr_resident=1, dense_min_tiles=1)
LR = (40, 52)                   # tile 24, overlap 8: rows 0, 16 and columns 0, 16, 28 -> 6 tiles
TILED = dict(scale=2, tile=24, tile_overlap=8, hip_options=dict(ON))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _edsr(dev, blocks=2, test_cfg=None, res_scale=None, seed=21, gain=1.25, head_gain=None):
    """EDSR restorer with small heads; -> (model on dev, the generator's parameters on the CPU for the oracle)."""
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_hip_parity import _restorer
    model = _restorer('edsr', 2, dev, dict(scale=2) if test_cfg is None else test_cfg, blocks=blocks, hidden=(64, 64))
    if head_gain is None:
        seeded_init_(model, seed=seed, gain=gain)
    else:
        seeded_init_(model, seed=seed, gain=gain, head_gain=head_gain)
    if res_scale is not None:
        for blk in model.generator.body:
            blk.res_scale = res_scale
    params = {k[len('generator.'):]: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(dev), params


def _tags():
    from ciaosr_amd import hip_ops
    return {k: v['launches'] for k, v in hip_ops.profile.results().items()}


_trunks = {}


def _trunk(dev, blocks):
    if blocks not in _trunks:
        _trunks[blocks] = _edsr(dev, blocks)
    return _trunks[blocks]


# ---- 4. against the CPU oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks,hw', [(2, (12, 12)), (2, (13, 25)), (2, (7, 30)), (2, (19, 70)), (16, (24, 24))])
def test_trunk_vs_oracle(dev, blocks, hw):
    """(12, 12) one exact tile, (13, 25) one-pixel remainder tiles on both axes, (7, 30) lower than a tile, (19, 70) 2 x 6 ragged tiles;
    (24, 24) at the config's 16 blocks.  The bound of tests/test_hip_parity.py::test_encoder_features_vs_oracle, on its inputs."""
    from ciaosr_amd import hip_ops
    from oracle import ciaosr_oracle as orc
    model, params = _trunk(dev, blocks)
    x = randn((1, 3) + hw, 77) * 0.3
    want = orc.edsr_features(x, params)
    with hip_ops.profile():
        got = model.generator.gen_feature(x.to(dev), hip_ops.Options(**ON))[0].cpu()
    tags = _tags()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'edsr_resident {blocks} blocks {hw}: max|d| {err:.3e} (feature scale {scale:.3f}), tags {tags}')
    assert tags.get('enc_edsr_resident') == 2 * blocks + 1, tags
    # the stem runs per image under its own tags (image_to_hwc4, enc_patch_first, enc_conv_first): no enc_conv3x3 launch is left
    assert 'enc_conv3x3' not in tags and tags.get('enc_conv_first') == 1 and tags.get('enc_patch_first') == 1, tags
    assert got.shape == want.shape
    assert err < 2e-4 * max(scale, 1.0), (err, scale)


def test_res_scale_is_applied_where_the_definition_says(dev):
    from ciaosr_amd import hip_ops
    from oracle import ciaosr_oracle as orc
    model, params = _edsr(dev, 2, res_scale=0.1)
    x = randn((1, 3, 13, 25), 77) * 0.3
    want = orc.edsr_features(x, params, res_scale=0.1)
    with hip_ops.profile():
        got = model.generator.gen_feature(x.to(dev), hip_ops.Options(**ON))[0].cpu()
    assert _tags().get('enc_edsr_resident') == 5
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    far = (orc.edsr_features(x, params, res_scale=1.0) - want).abs().max().item()
    print(f'edsr_resident res_scale 0.1 (13, 25): max|d| {err:.3e} (feature scale {scale:.3f}; res_scale 1 would be {far:.3e} away)')
    assert far > 100 * 2e-4 * max(scale, 1.0)            # the case tells the two apart
    assert err < 2e-4 * max(scale, 1.0), (err, scale)


# ---- 5. batch == singles ----------------------------------------------------------------------------------------------------------------
def test_batch_is_bitwise_the_singles(dev):
    from ciaosr_amd import hip_ops
    model, _ = _trunk(dev, 2)
    enc = model.generator._encoder_hip
    opt = hip_ops.Options(**ON)
    big = (randn((3, 25, 80), 78) * 0.3).to(dev)
    crops = torch.stack([big[:, i0:i0 + 19, j0:j0 + 70] for i0, j0 in ((0, 0), (3, 5), (6, 10))]).contiguous()
    with hip_ops.profile():
        batch = enc.forward_hwc_batch(crops, opt)
    assert _tags().get('enc_edsr_resident') == 5              # three images, the launches of one
    singles = [enc.forward_hwc(crops[i], opt) for i in range(3)]
    assert batch.shape == (3, 19, 70, 64)
    for i in range(3):
        assert torch.equal(batch[i], singles[i]), i
    assert not torch.equal(singles[0], singles[1])
    assert torch.equal(enc.forward_hwc_batch(crops[1:2], opt)[0], singles[1])


# ---- 6. option off == the old entry ---------------------------------------------------------------------------------------------------
def _old_entry(enc, x_chw):
    from ciaosr_amd import _lib, hip_ops
    st = enc.struct(None)
    _, H, W = x_chw.shape
    ws = torch.empty(_lib.load().ciaosr_edsr_workspace_bytes(H, W, C.byref(st)), dtype=torch.uint8, device=x_chw.device)
    out = torch.empty(H, W, st.mid_channels, dtype=torch.float32, device=x_chw.device)
    _lib.call('ciaosr_edsr_forward_f32', hip_ops.ptr(x_chw), H, W, C.byref(st), hip_ops.ptr(out), hip_ops.ptr(ws), ws.numel(), hip_ops.stream_ptr())
    return out


def test_option_off_is_the_old_entry(dev):
    from ciaosr_amd import _lib, hip_ops
    model, _ = _trunk(dev, 2)
    enc = model.generator._encoder_hip
    x = (randn((2, 3, 19, 24), 79) * 0.3).to(dev).contiguous()
    with hip_ops.profile():
        want = [_old_entry(enc, x[i]) for i in range(2)]
    old_tags = _tags()
    st = enc.struct(None)
    lib = _lib.load()
    n = lib.ciaosr_edsr_workspace_bytes_batch(2, 19, 24, C.byref(st), None)
    assert n == lib.ciaosr_edsr_workspace_bytes(19, 24, C.byref(st))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    got = torch.empty(2, 19, 24, 64, dtype=torch.float32, device=dev)
    with hip_ops.profile():
        _lib.call('ciaosr_edsr_forward_batch_f32', hip_ops.ptr(x), 2, 19, 24, C.byref(st), hip_ops.ptr(got), None, hip_ops.ptr(ws), n, hip_ops.stream_ptr())
    new_tags = _tags()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert 'enc_edsr_resident' not in new_tags and new_tags == old_tags, (new_tags, old_tags)
    # the same with an options struct whose field is 0
    off = hip_ops.Options(dense_min_tiles=1)
    _lib.call('ciaosr_edsr_forward_batch_f32', hip_ops.ptr(x), 2, 19, 24, C.byref(st), hip_ops.ptr(got.zero_()), off.c_arg(), hip_ops.ptr(ws), n,
              hip_ops.stream_ptr())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the Python layers with default options: the old entry, launch for launch
    with hip_ops.profile():
        one = _old_entry(enc, x[0])
    direct = _tags()
    with hip_ops.profile():
        feat = model.generator.gen_feature(x[:1])[0]
    through = _tags()
    through.pop('hwc_to_nchw', None)                           # gen_feature's own layout change, not a trunk launch
    direct.pop('hwc_to_nchw', None)
    assert through == direct and 'enc_edsr_resident' not in through, (through, direct)
    assert torch.equal(feat[0].permute(1, 2, 0), one)
    assert torch.equal(enc.forward_hwc_batch(x)[1], want[1])


# ---- 7. through the restorer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiled(dev):
    """The restorer of test 7, its LR image, and restore at tile_batch = 1 (with its launch counts): computed once, left unchanged."""
    from ciaosr_amd import hip_ops
    model, params = _edsr(dev, 2, test_cfg=dict(TILED), seed=23, gain=1.25, head_gain=SQRT6)
    lq = (randn((1, 3) + LR, 5) * 0.2 + 0.45).clamp(0, 1)
    model.test_cfg['tile_batch'] = 1
    model.test_cfg['encoder_ahead'] = False
    with hip_ops.profile():
        out1 = model.restore(lq.to(dev))
    tags1 = _tags()
    return model, params, lq, out1, tags1


def _cfg(model, **kw):
    model.test_cfg.clear()
    model.test_cfg.update(dict(TILED), **kw)


def test_restore_tile_batches_share_the_trunk_launches(dev, tiled):
    from ciaosr_amd import hip_ops
    model, _, lq, out1, tags1 = tiled
    assert out1.shape == (1, 3, 80, 104)
    assert tags1.get('enc_edsr_resident') == 6 * 5 and tags1.get('enc_conv_first') == 6 and 'enc_conv3x3' not in tags1, tags1
    _cfg(model, tile_batch=4, encoder_ahead=False)
    with hip_ops.profile():
        out4 = model.restore(lq.to(dev))
    tags4 = _tags()
    assert torch.equal(out4, out1)
    # 6 tiles in groups of 4 + 2: 2 groups x (2 blocks x 2 + 1) launches, against 6 x 5 tile by tile
    assert tags4.get('enc_edsr_resident') == 2 * 5 and tags4.get('enc_conv_first') == 6 and 'enc_conv3x3' not in tags4, tags4
    _cfg(model, tile_batch=4, encoder_ahead=True)
    assert torch.equal(model.restore(lq.to(dev)), out1)
    _cfg(model, tile_batch=1, encoder_ahead=True)
    assert torch.equal(model.restore(lq.to(dev)), out1)
    _cfg(model)                                                # the default: EDSR_TILE_BATCH, one group
    assert model.tile_batch() == 8
    with hip_ops.profile():
        out8 = model.restore(lq.to(dev))
    assert torch.equal(out8, out1) and _tags().get('enc_edsr_resident') == 5


def test_restore_vs_oracle(dev, tiled):
    from oracle import ciaosr_oracle as orc
    from tests.test_hip_parity import NORTH_STAR_TOL
    model, params, lq, out1, _ = tiled
    want = orc.forward_test(lq, None, None, params, scale=2, tile=24, tile_overlap=8)
    err = (out1.cpu() - want).abs().max().item()
    print(f'edsr_resident restore x2, LR {LR}, 6 tiles: max|d| vs the oracle {err:.3e}')
    assert want.shape == out1.shape and err < NORTH_STAR_TOL, err


def test_render_and_render_many_are_restore_bitwise(dev, tiled):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.scene import Grid
    model, _, lq, out1, _ = tiled
    x = lq.to(dev)
    _cfg(model, tile_batch=4)
    assert torch.equal(model.render(model.encode(x), scale=2), out1)
    # a non-integer scale needs the any-scale tile plan (tile_plan.py); under it the x2 grid is planned that way too, which is not
    # bitwise the reference's integer-scale clip_test -- with or without this option -- so the many-target walk is held to the single calls
    _cfg(model, tile_batch=4, tile_any_scale=True)
    one2 = model.render(model.encode(x, max_scale=2), scale=2)
    one15 = model.render(model.encode(x, max_scale=2), scale=1.5)
    with hip_ops.profile():
        many = model.render_many(model.encode(x, max_scale=2), [Grid(scale=2), Grid(scale=1.5)])
    tags = _tags()
    assert many[0].shape == out1.shape and torch.equal(many[0], one2)
    assert many[1].shape == (1, 3, 60, 78) and torch.equal(many[1], one15)
    assert (one2 - out1).abs().max().item() < 1e-5
    assert tags.get('enc_edsr_resident') == 2 * 5, tags       # one walk: the 6 tiles' trunks in groups of 4 + 2, once for both targets


# ---- 8. the RDN bits ---------------------------------------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize('B', [1, 3])
def test_rdn_direct_kernel_bits_are_the_parents(dev, B):
    """tests/golden/rdn_direct_29x40.npz (tools/make_rdn_direct_fixture.py, run on the library of the commit before the kernel was
    generalised): features of image 0, SHA-256 of the features of images 1 and 2."""
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_hip_parity import _restorer
    fx = np.load(os.path.join(GOLDEN, 'rdn_direct_29x40.npz'))
    h, w = [int(v) for v in fx['shape']]
    assert (h, w) == (29, 40) and int(fx['blocks']) == 2 and int(fx['layers']) == 3
    model = _restorer('rdn', 4, dev, dict(scale=4), blocks=int(fx['blocks']), layers=int(fx['layers']), hidden=(64, 64))
    assert seeded_init_(model, seed=int(fx['weight_seed']), gain=float(fx['gain'])) == str(fx['sha'])
    x = (randn((3, 3, h, w), int(fx['input_seed'])) * 0.3).to(dev)
    enc = model.to(dev).generator._encoder_hip
    with hip_ops.profile():
        got = enc.forward_hwc_batch(x[:B].contiguous(), hip_ops.Options(dense_direct=1, dense_min_tiles=1))
    tags = _tags()
    assert tags.get('enc_dense_gather') == 2 * 3 and 'enc_edsr_resident' not in tags, tags
    assert torch.equal(got[0].cpu(), torch.from_numpy(fx['feat0']))
    for i in range(1, B):
        assert _sha(got[i]) == str(fx[f'sha_feat{i}']), i
