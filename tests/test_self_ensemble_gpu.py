"""Self-ensemble on the device: the two kernels against torch's flip / transpose, `restore(..., self_ensemble=...)` against the torch
restatement of its definition (eight plain `restore` calls, mapped back, added in member order, divided once) -- bitwise --, the
equivariance of the full ensemble, the scene path and `forward_test`.

The oracle's division: `tensor / python_number` on the device multiplies by the reciprocal, which is not the correctly rounded quotient the
definition asks for (it is for n = 8, not for n = 3).  The fp64 quotient of two fp32 numbers, rounded to fp32, IS the correctly rounded
fp32 quotient (53 >= 2 * 24 + 2 bits: the double rounding is innocuous), so `_div` divides tensor by tensor in fp64 on the host."""
import ctypes

import pytest
import torch

from tests.test_scene_restorer_gpu import _crop, _device_grid, _grid, _lq, _model

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (63, 65), (64, 64), (65, 130), (1, 200), (200, 1)]     # below, on and across the 64 x 64 LDS tile in each axis
BAD_ARG = -1


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _t(x, k):
    if k & 1:
        x = x.flip(-1)
    if k & 2:
        x = x.flip(-2)
    if k & 4:
        x = x.transpose(-1, -2)
    return x.contiguous()


def _u(x, k):
    if k & 4:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-2)
    if k & 1:
        x = x.flip(-1)
    return x.contiguous()


def _div(acc, n):
    num = acc.double().cpu()
    return (num / torch.full_like(num, float(n))).float().to(acc.device)


def _mean(parts):
    """`parts`: the U_k(out_k) in member order."""
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return _div(acc, len(parts))


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 6])
@pytest.mark.parametrize('shape', SHAPES)
def test_kernels_against_torch(dev, planes, shape):
    from ciaosr_amd import hip_ops
    h, w = shape
    g = torch.Generator().manual_seed(1000 * h + w + planes)
    x = torch.randn(planes, h, w, generator=g).to(dev)
    members = []
    for k in range(8):
        got = hip_ops.dihedral(x, k)
        want = _t(x, k)
        assert got.shape == want.shape == ((planes, w, h) if k & 4 else (planes, h, w))
        assert torch.equal(got, want), k
        members.append(torch.randn(want.shape, generator=g).to(dev))
        # `first` on a buffer full of NaN: acc is not read
        acc = torch.full((planes, h, w), float('nan'), device=dev)
        assert hip_ops.dihedral_accum(acc, members[k], k, True) is acc
        assert torch.equal(acc, _u(members[k], k)), k
        # a second member on top, then the division, in one call and on its own
        other = torch.randn(planes, h, w, generator=g).to(dev)
        acc2 = other.clone()
        hip_ops.dihedral_accum(acc2, members[k], k, False)
        assert torch.equal(acc2, other + _u(members[k], k)), k
        acc3 = other.clone()
        hip_ops.dihedral_accum(acc3, members[k], k, False, divisor=3.0)
        assert torch.equal(acc3, _div(other + _u(members[k], k), 3)), k
    for ids, n in ((range(8), 8), ((3, 4, 0), 3)):
        ids = list(ids)
        acc = torch.full((planes, h, w), float('nan'), device=dev)
        for i, k in enumerate(ids):
            hip_ops.dihedral_accum(acc, members[k], k, i == 0, divisor=float(n) if i == n - 1 else 0.0)
        assert torch.equal(acc, _mean([_u(members[k], k) for k in ids])), ids
    # batch axes in front are planes
    x4 = x.reshape(1, planes, h, w)
    assert torch.equal(hip_ops.dihedral(x4, 5), _t(x4, 5))
    with pytest.raises(ValueError):
        hip_ops.dihedral_accum(torch.empty(planes, h, w + 1, device=dev), x, 4, True)


def test_bad_arguments_are_refused_and_leave_the_output_untouched(dev):
    from ciaosr_amd import _lib, hip_ops
    lib = _lib.load()
    src = torch.randn(2, 5, 7).to(dev)
    dst = torch.full((2, 5, 7), 7.5, device=dev)
    p, s, null = hip_ops.ptr, hip_ops.stream_ptr(), ctypes.c_void_p(0)
    bad = [(p(src), p(dst), 2, 5, 7, 8), (p(src), p(dst), 2, 5, 7, -1), (p(src), p(dst), 0, 5, 7, 1), (p(src), p(dst), 2, 0, 7, 1),
           (p(src), p(dst), 2, 5, -7, 1), (null, p(dst), 2, 5, 7, 1), (p(src), null, 2, 5, 7, 1), (p(dst), p(dst), 2, 5, 7, 1)]
    for args in bad:
        assert lib.ciaosr_dihedral_f32(*args, s) == BAD_ARG, args[2:]
    bad = [(p(dst), p(src), 2, 5, 7, 8, 0, 0.0), (p(dst), p(src), 2, 5, 7, -1, 0, 0.0), (p(dst), p(src), 0, 5, 7, 1, 0, 0.0),
           (p(dst), p(src), 2, 5, 0, 1, 0, 0.0), (null, p(src), 2, 5, 7, 1, 0, 0.0), (p(dst), null, 2, 5, 7, 1, 0, 0.0),
           (p(dst), p(dst), 2, 5, 7, 1, 0, 0.0), (p(dst), p(src), 2, 5, 7, 1, 0, -1.0), (p(dst), p(src), 2, 5, 7, 1, 0, float('nan')),
           (p(dst), p(src), 2, 5, 7, 1, 1, float('inf'))]
    for args in bad:
        assert lib.ciaosr_dihedral_accum_f32(*args, s) == BAD_ARG, args[2:]
    torch.cuda.synchronize()
    assert torch.equal(dst, torch.full_like(dst, 7.5))
    with pytest.raises(_lib.CiaoSRHipError):
        hip_ops.dihedral(src, 8)


# ---- restore against the definition ---------------------------------------------------------------------------------------------------
_cache = {}


def _grids(ht, wt, dev, device_grid):
    """The caller's tensors for k < 4 and the definition's `hip_ops.make_coord_cell(Wt, Ht)` for k & 4."""
    return (_device_grid if device_grid else _grid)(ht, wt, dev), _device_grid(wt, ht, dev)


def _parts(model, lq, ht, wt, dev, device_grid=False):
    """U_k of the eight plain restores, k = 0 .. 7, and the plain restore itself (member 0)."""
    return [_u(model.restore(_t(lq, k), *_grids(ht, wt, dev, device_grid)[1 if k & 4 else 0], self_ensemble=False), k) for k in range(8)]


def _rdn_case(dev, precision, s):
    """RDN on the non-square 20 x 28 image: (model config, lq, caller's grid, parts, the ensemble result), computed once per module."""
    key = (precision, s)
    if key not in _cache:
        model = _model('rdn', dev)
        model.test_cfg = dict(scale=4, precision=precision)
        lq = _lq(20, 28, dev, seed=9)
        ht, wt = round(20 * s), round(28 * s)
        f16 = precision != 'fp32'
        parts = _parts(model, lq, ht, wt, dev, device_grid=f16)
        got = model.restore(lq, *_grids(ht, wt, dev, f16)[0], self_ensemble=True)
        _cache[key] = (dict(model.test_cfg), lq, (ht, wt), parts, got)
    return _cache[key]


@pytest.mark.parametrize('precision,s', [('fp32', 4), ('f16', 4), ('fp32', 2.7)])
def test_restore_is_the_definition(dev, precision, s):
    cfg, lq, (ht, wt), parts, got = _rdn_case(dev, precision, s)
    assert got.shape == (1, 3, ht, wt) and got.dtype == torch.float32
    assert torch.equal(got, _mean(parts)), (got - _mean(parts)).abs().max().item()
    assert not torch.equal(got, parts[0])                                      # the members differ: the mean is not the plain restore
    model = _model('rdn', dev)
    model.test_cfg = cfg
    f16 = precision != 'fp32'
    sub = model.restore(lq, *_grids(ht, wt, dev, f16)[0], self_ensemble=(3, 4, 0))
    assert torch.equal(sub, _mean([parts[3], parts[4], parts[0]]))
    one = model.restore(lq, *_grids(ht, wt, dev, f16)[0], self_ensemble=[6])
    assert torch.equal(one, parts[6])
    model.test_cfg = dict(cfg, self_ensemble=True)                             # the config key is the default of the argument
    assert torch.equal(model.restore(lq, *_grids(ht, wt, dev, f16)[0]), got)
    assert torch.equal(model.restore(lq, *_grids(ht, wt, dev, f16)[0], self_ensemble=False), parts[0])
    with pytest.raises(ValueError):
        model.graphed_restore(lq, *_grids(ht, wt, dev, f16)[0])


@pytest.mark.parametrize('kind', ['edsr', 'swinir'])
def test_restore_other_trunks(dev, kind):
    model = _model(kind, dev)
    model.test_cfg = dict(scale=3.3)
    lq = _lq(24, 24, dev)
    ht = wt = round(24 * 3.3)
    got = model.restore(lq, *_grid(ht, wt, dev), self_ensemble=True)
    assert torch.equal(got, _mean(_parts(model, lq, ht, wt, dev)))


@pytest.mark.parametrize('any_scale,size', [(False, (80, 112)), (True, (108, 151))])
def test_tiled_restore_is_the_definition(dev, any_scale, size):
    model = _model('rdn', dev)
    cfg = dict(scale=2, tile=32, tile_overlap=8)
    if any_scale:
        cfg['tile_any_scale'] = True
    model.test_cfg = cfg
    lq = _lq(40, 56, dev)
    got = model.restore(lq, *_grid(*size, dev), self_ensemble=True)
    parts = _parts(model, lq, *size, dev)
    assert got.shape == (1, 3, *size) and torch.equal(got, _mean(parts))
    assert not torch.equal(got, parts[0])


def test_full_ensemble_is_equivariant(dev):
    """T_j of the ensemble of lq against the ensemble of T_j(lq): the same eight fp32 images per pixel, added in another order.  Bound
    (derived, not measured): the values lie in [0, 1], so every partial sum is at most 8 and each of the seven adds errs by at most half
    an ulp of 8, 2^-21; the division by 8 is exact.  Per side 7 * 2^-21 / 8 < 4.2e-7, so the two sides differ by less than 1e-6."""
    cfg, lq, (ht, wt), parts, got = _rdn_case(dev, 'fp32', 4)
    model = _model('rdn', dev)
    model.test_cfg = cfg
    for j in (1, 2, 4, 7):
        size = (wt, ht) if j & 4 else (ht, wt)
        turned = model.restore(_t(lq, j), *_device_grid(*size, dev), self_ensemble=True)
        want = _t(got, j)
        assert turned.shape == want.shape
        err = (turned - want).abs().max().item()
        assert err <= 1e-6, (j, err)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def test_scene_renders_are_the_ensemble_restore(dev):
    from ciaosr_amd import metrics_hip, scene
    cfg, lq, _, _, _ = _rdn_case(dev, 'fp32', 4)
    model = _model('rdn', dev)
    model.test_cfg = dict(cfg, scene_cache_mb=800)
    enc = model.encode(lq, self_ensemble=True)
    assert isinstance(enc, scene.EnsembleEncoded) and enc.ids == tuple(range(8)) and enc.shape == (20, 28)
    assert [m.shape for m in enc.members] == [(28, 20) if k & 4 else (20, 28) for k in range(8)]
    assert all(m.cache.budget == (800 << 20) // 8 for m in enc.members)
    assert enc.scene_bytes == sum(m.scene_bytes for m in enc.members) > 0
    for s in (4, 2.7):
        want = _rdn_case(dev, 'fp32', s)[4]
        ht, wt = want.shape[-2:]
        got = model.render(enc, scale=s)
        assert torch.equal(got, want), (s, (got - want).abs().max().item())
        windows = [(ht // 3, wt // 4, 17, 23), (ht - 9, 0, 9, 13), (5, 0, 1, wt)]          # interior, a corner, one full-width row
        for window in windows:
            assert torch.equal(model.render(enc, size=(ht, wt), window=window), _crop(want, window)), (s, window)
        u8 = model.render(enc, scale=s, as_u8=True)
        assert u8.dtype == torch.uint8 and torch.equal(u8, metrics_hip.tensor2img_u8(want))
        targets = [scene.Grid(scale=s), scene.Grid(size=(ht, wt), window=windows[0])]
        many = model.render_many(enc, targets)
        assert len(many) == 2 and torch.equal(many[0], want) and torch.equal(many[1], _crop(want, windows[0]))
    sub = model.encode(lq, self_ensemble=(3, 4, 0))
    assert sub.ids == (3, 4, 0) and len(sub.members) == 3
    assert torch.equal(model.render(sub, scale=4), model.restore(lq, *_grid(80, 112, dev), self_ensemble=(3, 4, 0)))
    # what an ensemble record does not serve, refused before any device work
    m = scene.view_matrix((10, 14), 2.0, 30.0, (16, 16))
    for call in (lambda: model.render_view(enc, m, (16, 16)), lambda: model.render_many(enc, [scene.Grid(scale=4), scene.View(m, (16, 16))]),
                 lambda: model.render_pyramid(enc, scale=4), lambda: model.prefetch(enc, [scene.Grid(scale=4)]),
                 lambda: model.encode_rgba(torch.rand(1, 4, 20, 28, device=dev), self_ensemble=True)):
        with pytest.raises(ValueError):
            call()
    plain = model.encode(lq)                                                               # the plain path is what it was
    assert isinstance(plain, scene.EncodedImage) and torch.equal(model.render(plain, scale=4), _rdn_case(dev, 'fp32', 4)[3][0])


def test_tiled_scene_render_is_the_ensemble_restore(dev):
    model = _model('rdn', dev)
    model.test_cfg = dict(scale=2, tile=32, tile_overlap=8, tile_any_scale=True)
    lq = _lq(40, 56, dev)
    want = model.restore(lq, *_grid(108, 151, dev), self_ensemble=(0, 5, 2))
    enc = model.encode(lq, max_scale=2.7, self_ensemble=(0, 5, 2))
    window = (9, 41, 61, 35)                                                               # crosses both seams of the 2 x 2 tiles
    assert torch.equal(model.render(enc, size=(108, 151), window=window), _crop(want, window))
    assert torch.equal(model.render(enc, size=(108, 151)), want)


# ---- forward_test ----------------------------------------------------------------------------------------------------------------------
def test_forward_test_scores_the_ensembled_image(dev):
    cfg, lq, (ht, wt), parts, got = _rdn_case(dev, 'fp32', 4)
    model = _model('rdn', dev)
    model.test_cfg = dict(cfg, self_ensemble=True, metrics=['PSNR'], crop_border=2)
    gt = (_lq(ht, wt, dev, seed=21)[0].permute(1, 2, 0).reshape(1, ht * wt, 3)).contiguous()
    coord, cell = _grid(ht, wt, dev)
    res = model(lq=lq, gt=gt, test_mode=True, coord=coord, cell=cell)['eval_result']
    gt_img = gt.view(1, ht, wt, 3).permute(0, 3, 1, 2).contiguous()
    want = model.evaluate(_mean(parts), gt_img)
    assert list(res) == ['PSNR'] and res['PSNR'] == want['PSNR']
    model.test_cfg = dict(cfg, metrics=['PSNR'], crop_border=2)
    assert model(lq=lq, gt=gt, test_mode=True, coord=coord, cell=cell)['eval_result']['PSNR'] == model.evaluate(parts[0], gt_img)['PSNR']
