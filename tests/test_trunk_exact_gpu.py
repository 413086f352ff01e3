"""Every fp32 trunk route against the float64 answer of fixtures on which fp32 arithmetic is exact (tests/exact_trunk.py).

On these fixtures every sum any route can form -- the direct 9 cin sums in any order and split, the Winograd input transforms, the
transformed-domain sums over channels, the output transforms, bias, residual and alpha epilogues -- consists of multiples of one power of
two whose absolute values add up to less than 2^22 of it (check_exact; test_trunk_exact_host.py runs it on every case below), so no fp32
operation rounds and ONE float64 evaluation is the answer of every route.  The bound is therefore ZERO:

    torch.equal(got.double(), want)

A failure here is a defect of a kernel or of its packing, not noise; the message names the worst element (image, channel, row, column)
with the got / want values there.  Every run asserts through hip_ops.profile that the intended kernel ran and the excluded ones did not."""
import pytest
import torch

from tests import exact_trunk as et

pytestmark = pytest.mark.gpu

DENSE_TAGS = ('enc_dense_wino4', 'enc_dense_wino', 'enc_dense_gather', 'enc_dense_scatter')
# route -> (options, the dense tag that must run)
FORCED = {'wino4': (dict(dense_min_tiles=1), 'enc_dense_wino4'), 'wino2': (dict(dense_min_tiles=1, dense_direct=2), 'enc_dense_wino'),
          'direct': (dict(dense_min_tiles=1, dense_direct=1), 'enc_dense_gather')}
SMALL = {'scatter': (dict(), 'enc_dense_scatter'), 'scatter_step': (dict(scatter_small_max=-1), 'enc_dense_scatter')}
ROUTES = dict(FORCED, **SMALL)

_models = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _build(params, dev, res_scale=None):
    """A generator on the device whose trunk holds `params` (reference names) -> its PackedEncoder."""
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR, LocalImplicitSRRDN
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[32, 32])
    heads = dict(imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=None)
    if 'sfe1.weight' in params:
        mid = params['sfe1.weight'].shape[0]
        nb = 1 + max(int(k.split('.')[1]) for k in params if k.startswith('rdbs.'))
        nl = 1 + max(int(k.split('.')[3]) for k in params if k.startswith('rdbs.0.layers.'))
        gen = dict(type=LocalImplicitSRRDN, encoder=dict(type='RDN', in_channels=3, out_channels=3, mid_channels=mid, num_blocks=nb, upscale_factor=4,
                                                          num_layers=nl, channel_growth=mid), **heads)
    else:
        nb = 1 + max(int(k.split('.')[1]) for k in params if k.startswith('body.'))
        gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=64, num_blocks=nb), **heads)
    g = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=2)).eval().generator
    sd = g.state_dict()
    assert set(params) <= set(sd) and all(sd[k].shape == v.shape for k, v in params.items())
    trunk = [k for k in sd if not k.startswith(('imnet', 'cs_attn', 'non_local'))]
    assert set(trunk) == set(params), sorted(set(trunk) ^ set(params))
    g.load_state_dict(params, strict=False)
    if res_scale is not None:
        for blk in g.body:
            blk.res_scale = res_scale
    g = g.to(dev)
    assert g._encoder_hip.supported()
    return g._encoder_hip


def _encoder(fx, dev):
    """One packed trunk per fixture family (the parameters do not depend on the map), shared by every test."""
    if fx.name not in _models:
        _models[fx.name] = _build(fx.params, dev, fx.res_scale)
    return _models[fx.name]


def _run(enc, fx, dev, opts, ran=(), not_ran=(), counts=None, label=''):
    """One trunk call against the float64 answer -> (worst |got - want|, where, (got, want) there, the output).  `ran` / `not_ran`: profiler
    tags (exact names); `counts`: launches per tag."""
    from ciaosr_amd import hip_ops
    opt = hip_ops.Options(**opts)
    with hip_ops.profile():
        got = enc.forward_hwc_batch(fx.x.to(dev).contiguous(), opt)
    tags = {k: v['launches'] for k, v in hip_ops.profile.results().items()}
    got = got.permute(0, 3, 1, 2).cpu()
    missing, extra = [t for t in ran if t not in tags], [t for t in not_ran if t in tags]
    assert not missing and not extra, f'{label} {opt}: expected tags missing {missing}, unexpected tags present {extra}; ran {tags}'
    for t, n in (counts or {}).items():
        assert tags.get(t) == n, f'{label} {opt}: {t} ran {tags.get(t)} times, expected {n}; {tags}'
    want = fx.want
    assert got.shape == want.shape and torch.isfinite(got).all(), f'{label} {opt}: shape {tuple(got.shape)} or non-finite output'
    err, where, (i, c, y, x) = et.worst_element(got, want)
    print(f'{label} {opt}: max|hip - float64| = {err:.3e} (bound 0; output scale {fx.scale:.3f}, unit {fx.unit}); tags {tags}')
    return err, where, (got[i, c, y, x].item(), want[i, c, y, x].item()), got


def _exact(enc, fx, dev, opts, **kw):
    err, where, (g, w), got = _run(enc, fx, dev, opts, **kw)
    assert torch.equal(got.double(), fx.want), f"{kw.get('label', '')} {opts}: max|hip - float64| = {err:.3e} = {err / fx.unit:.1f} output units at {where}: got {g!r}, want {w!r}; " \
                                              f'{int((got.double() != fx.want).sum())} of {got.numel()} elements differ'


def _rdn_tags(dense, route=None):
    """(ran, not_ran) of an RDN call.  The two scatter forms share their tag: the step of conv_f32.hip is told from the one-launch kernel by
    its split-K reduction (these maps are far too small to fill the device without one), which nothing else on a small-map route launches."""
    ran, not_ran = ('enc_conv_first', 'enc_conv3x3', 'enc_conv1x1', dense), tuple(t for t in DENSE_TAGS if t != dense) + ('enc_edsr_resident',)
    if route == 'scatter_step':
        ran += ('conv_splitk_reduce',)
    elif route is not None:
        not_ran += ('conv_splitk_reduce',)
    return ran, not_ran


@pytest.mark.parametrize('route', list(FORCED))
@pytest.mark.parametrize('l,hw', et.forced_cases())
def test_forced_halo_resident_routes(dev, l, hw, route):
    """F(4x4), F(2x2) and the direct gather kernel forced onto small maps: (16, 32) exactly one 16x32 tile, (17, 33) a one-pixel remainder in
    all three tilings, (21, 37) partial 4x4 tiles with one valid row and column, (7, 30) lower than any tile; all eight probes on (21, 37)."""
    fx = et.probe(l, hw)
    opts, dense = FORCED[route]
    ran, not_ran = _rdn_tags(dense, route)
    _exact(_encoder(fx, dev), fx, dev, opts, ran=ran, not_ran=not_ran, counts={dense: l + 1}, label=f'probe {l} {hw} {route}')


@pytest.mark.parametrize('route', list(SMALL))
@pytest.mark.parametrize('l,hw', et.small_cases())
def test_small_map_scatter_routes(dev, l, hw, route):
    """Unforced: the scatter form on its one-launch kernel, and (scatter_small_max = -1) the scatter step of conv_f32.hip."""
    fx = et.probe(l, hw)
    opts, dense = SMALL[route]
    ran, not_ran = _rdn_tags(dense, route)
    _exact(_encoder(fx, dev), fx, dev, opts, ran=ran, not_ran=not_ran, label=f'probe {l} {hw} {route}')


def test_mid32_on_the_generic_route(dev):
    fx = et.narrow32((19, 24))
    _exact(_encoder(fx, dev), fx, dev, {}, ran=('enc_conv_first', 'enc_conv3x3', 'enc_conv1x1'), not_ran=DENSE_TAGS + ('enc_edsr_resident',), label='mid 32 (19, 24) generic')


@pytest.mark.parametrize('route', ['wino4', 'wino2', 'direct', 'scatter', 'scatter_step'])
def test_two_blocks(dev, route):
    """NB = 2: the X ping-pong and the global concat's column offset of block 1."""
    fx = et.two_blocks((21, 37))
    opts, dense = ROUTES[route]
    ran, not_ran = _rdn_tags(dense, route)
    _exact(_encoder(fx, dev), fx, dev, opts, ran=ran, not_ran=not_ran, counts={dense: 4} if route in FORCED else None, label=f'NB = 2 (21, 37) {route}')


@pytest.mark.parametrize('route', list(FORCED))
def test_batch_of_three_images(dev, route):
    """B = 3 different images in one call on the halo-resident routes (the batch shares the dense launches): each equals its own answer."""
    fx = et.probe(7, (17, 33), 3)
    opts, dense = FORCED[route]
    ran, not_ran = _rdn_tags(dense, route)
    _exact(_encoder(fx, dev), fx, dev, opts, ran=ran, not_ran=not_ran, counts={dense: 8}, label=f'probe 7 (17, 33) B = 3 {route}')


def test_big_map_on_the_default_route(dev):
    """(131, 253) = 33 143 pixels at default options: F(4x4) unforced, the local fusion on conv1x1_resident_f32 (from 32 768 pixels, K = 576),
    stem and gff.1 past the 18 432-pixel limit of conv3x3_small on the split-K generic convolution."""
    fx = et.probe(7, et.BIG)
    assert 32768 <= fx.hw[0] * fx.hw[1] < 34000
    ran, not_ran = _rdn_tags('enc_dense_wino4')
    _exact(_encoder(fx, dev), fx, dev, {}, ran=ran, not_ran=not_ran, counts={'enc_dense_wino4': 8}, label=f'probe 7 {et.BIG} default')


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('hw', et.EDSR_MAPS)
@pytest.mark.parametrize('route', ['per_image', 'resident'])
def test_edsr(dev, route, hw, B):
    """EDSR, two blocks, res_scale 0.25: the per-image entry and the opt-in resident kernel over the batch."""
    fx = et.edsr(hw, B)
    enc = _encoder(fx, dev)
    assert enc.struct(None).res_scale == et.EDSR_RES_SCALE
    if route == 'resident':
        _exact(enc, fx, dev, dict(edsr_resident=1, dense_min_tiles=1), ran=('enc_conv_first', 'enc_edsr_resident'), not_ran=('enc_conv3x3',) + DENSE_TAGS,
               counts={'enc_edsr_resident': 5, 'enc_conv_first': B}, label=f'edsr {hw} B = {B} resident')
    else:
        _exact(enc, fx, dev, {}, ran=('enc_conv_first', 'enc_conv3x3'), not_ran=('enc_edsr_resident',) + DENSE_TAGS, counts={'enc_conv_first': B},
               label=f'edsr {hw} B = {B} per image')


@pytest.mark.parametrize('route', list(ROUTES))
def test_the_bound_has_teeth(dev, route):
    """The comparison itself, on the GPU: a model whose probe layer lacks ONE tap (one weight changed by one unit, 9/16 -> 0), run through
    each dense route and held against the UNCHANGED answer, is off by at least one output unit -- what a kernel that dropped that one
    product would do."""
    fx = et.probe(3, (21, 37))
    if 'teeth' not in _models:
        P = {k: v.clone() for k, v in fx.params.items()}
        w = P['rdbs.0.layers.3.conv.weight']
        o, c, a, b = [int(v) for v in (w[:, 64:] != 0).nonzero()[0]]
        assert abs(w[o, 64 + c, a, b].item()) == et.W9
        w[o, 64 + c, a, b] = 0.0
        _models['teeth'] = _build(P, dev)
    opts, dense = ROUTES[route]
    ran, not_ran = _rdn_tags(dense, route)
    err, where, (g, w_), got = _run(_models['teeth'], fx, dev, opts, ran=ran, not_ran=not_ran, label=f'one probe tap zeroed, {route}')
    print(f'one probe tap zeroed, {route}: {err / fx.unit:.0f} output units = {err / fx.scale:.2e} x the output scale at {where} (got {g!r}, want {w_!r})')
    assert not torch.equal(got.double(), fx.want) and err >= fx.unit, (route, err)
