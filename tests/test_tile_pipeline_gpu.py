"""The one batched tile loop of CiaoSR.clip_test on CiaoSR.trunk_ahead, at the smallest shape with ragged groups: LR 40 x 56 in 2 x 3 tiles
of 24 (overlap 8).  Every `tile_batch` x `encoder_ahead` is bitwise the one-tile-at-a-time image, the trunk is called once per group
with the group's size, whatever `encoder_ahead` is, and when a group's trunk is launched the feature maps of at most one earlier group
are still alive -- the group whose heads run beside it under `encoder_ahead`, none without."""
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = (40, 56)
TILED = dict(scale=2, tile=24, tile_overlap=8)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _model(kind, dev):
    """'rdn': the small RDN restorer of the scene tests.  'wide': the small EDSR restorer of tests/test_pyramid_gpu.py."""
    if kind == 'rdn':
        from tests.test_render_many_gpu import _model as scene_model
        return scene_model('rdn', dev)
    from tests.test_pyramid_gpu import _model as pyramid_model
    return pyramid_model(dict(), dev, 'wide')


@pytest.mark.parametrize('kind,precision', [('rdn', 'fp32'), ('wide', 'f16')])
def test_batched_tile_loop_is_bitwise_the_one_tile_loop(dev, monkeypatch, kind, precision):
    from ciaosr_amd.restorer import tile_grid
    from tests.test_render_many_gpu import _lq
    assert tile_grid(*LR, 24, 8) == (24, [(0, 0), (0, 16), (0, 32), (16, 0), (16, 16), (16, 32)])
    model = _model(kind, dev)
    lq = _lq(*LR, dev)
    model.test_cfg = dict(TILED, precision=precision, tile_batch=1)
    want = model.restore(lq)
    assert want.shape == (1, 3, 80, 112) and want.std().item() > 1e-3
    trunk = model.generator._encoder_hip
    inner = trunk.forward_hwc_batch
    calls, alive, refs = [], [], []

    def counted(x, *args, **kw):
        calls.append(x.shape[0])
        alive.append(sum(ref() is not None for ref in refs))          # earlier groups' feature maps at this launch
        feats = inner(x, *args, **kw)
        refs.append(weakref.ref(feats))
        return feats

    monkeypatch.setattr(trunk, 'forward_hwc_batch', counted)
    for n_batch, sizes in ((2, [2, 2, 2]), (4, [4, 2]), (6, [6])):
        for ahead in (True, False):
            model.test_cfg = dict(TILED, precision=precision, tile_batch=n_batch, encoder_ahead=ahead)
            for _ in range(2):
                del calls[:], alive[:], refs[:]
                got = model.restore(lq)
                assert calls == sizes, (n_batch, ahead, calls)
                assert alive == [int(ahead and g > 0) for g in range(len(sizes))], (n_batch, ahead, alive)
                assert torch.equal(got, want), (n_batch, ahead, (got - want).abs().max().item())
