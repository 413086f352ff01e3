"""Grey images on the GPU: the quantisers against the numpy restatement (tests/grey_ref.py), the one-byte-per-pixel PNG filter and files
against the restatement, Pillow's decoder and the match contract (tests/png_match_ref.py), the one-component JPEG files against
Pillow's mode-L files byte for byte, the renders of `CiaoSR.encode_grey` against convert('L') of the colour renders they are defined
by, the pyramid and NIQE.  Never the device against itself.
Run on the GPU box:  python -m pytest tests/test_grey_gpu.py -m gpu -q
"""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from tests import grey_ref as ref
from tests import png_match_ref as mref
from tests import view_reference as vr
from tests.test_grey_host import CONTENTS, JPEG_CONTENTS, make_grey, pil_grey, pil_jpeg_grey

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT_SIZES = [(1, 1), (5, 7), (33, 17), (64, 1025), (16, 256)]     # the last one: W % 4 == 0, the float4 loads and word stores
PNG_SIZES = [(1, 1), (1, 7), (5, 1), (7, 5), (33, 17), (96, 128), (256, 384), (3, 1025)]
JPEG_SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (33, 65), (96, 128), (250, 253)]
QUALITIES = [1, 35, 75, 90, 100]
FINAL = b'\x01\x00\x00\xff\xff'                            # an empty stored block with BFINAL: ends a segment that is not the last
PLAIN_LAUNCHES = dict(jpeg_coef=1, jpeg_count=1, jpeg_scan=1, jpeg_zero=1, jpeg_pack=1, jpeg_ffcount=1, jpeg_scan2=1, jpeg_stuff=1)
OPT_LAUNCHES = dict(PLAIN_LAUNCHES, jpeg_hist=1, jpeg_tables=1)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _dev(grey, dev):
    return torch.from_numpy(np.ascontiguousarray(grey)).to(dev)


def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


# -- the quantisers ---------------------------------------------------------------------------------------------------------------------
def _render_like(h, w, seed):
    """[3, h, w] fp32 with values below 0, above 1, every (k + 0.5) / 255 tie, inf and NaN among uniform noise."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(3, h, w, generator=g) * 1.5 - 0.25
    flat = t.view(-1)
    n = flat.numel()
    if n >= 600:
        halves = (torch.arange(255, dtype=torch.float32) + 0.5) / 255
        flat[0:255] = halves
        flat[n // 2:n // 2 + 255] = halves
        flat[300] = float('nan')
        flat[n - 7] = float('nan')
        flat[301], flat[302], flat[303] = -3.0, 7.0, float('inf')
    elif n >= 100:
        flat[3], flat[4], flat[5], flat[6], flat[7] = float('nan'), -3.0, 7.0, 0.5 / 255, 254.5 / 255
    return t


@pytest.mark.parametrize('h,w', QUANT_SIZES)
def test_tensor2img_grey_is_the_grey_of_tensor2img(dev, h, w):
    from ciaosr_amd import metrics_hip
    t = _render_like(h, w, seed=100 * h + w).to(dev)
    if h == 1:
        t[1] = float('nan')                                 # NaN -> 0 in that byte
    want = ref.grey_of_bgr(metrics_hip.tensor2img_u8(t).cpu().numpy())
    got = metrics_hip.tensor2img_grey_u8(t)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(metrics_hip.tensor2img_grey_u8(t.unsqueeze(0)).cpu().numpy(), want)
    # a pitched buffer at an odd byte offset, a word-aligned one, and a word-aligned start with an odd pitch: nothing beyond a row
    for pitch, start in ((w + 6, 1), (w + 3, 3), ((w + 7) // 4 * 4, 0), (w + (w + 1) % 2, 4)):
        buf = torch.full((h * pitch + 16,), 0xAB, dtype=torch.uint8, device=dev)
        view = torch.as_strided(buf, (h, w), (pitch, 1), start)
        assert metrics_hip.tensor2img_grey_u8(t, out=view) is view
        raw = buf.cpu().numpy()
        rows = raw[start:start + h * pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :w], want), (pitch, start)
        assert (rows[:, w:] == 0xAB).all() and (raw[:start] == 0xAB).all() and (raw[start + h * pitch:] == 0xAB).all(), (pitch, start)
    # a neutral render gives its own bytes
    neutral = t[:1].expand(3, -1, -1).contiguous()
    assert np.array_equal(metrics_hip.tensor2img_grey_u8(neutral).cpu().numpy(), metrics_hip.tensor2img_u8(neutral).cpu().numpy()[:, :, 1])


@pytest.mark.parametrize('h,w', QUANT_SIZES)
def test_grey_from_bgr(dev, h, w):
    from ciaosr_amd import metrics_hip
    rng = np.random.RandomState(7 * h + w)
    big = rng.randint(0, 256, (h + 3, w + 5, 3), dtype=np.uint8)
    if h * w >= 2000:                                       # some of the triples on which the alpha formula would be off by one
        odd = ref.disagreement_set()[::40][:h * w // 2].astype(np.uint8)
        crop = big[1:1 + h, 2:2 + w].reshape(-1, 3).copy()
        crop[:len(odd)] = odd
        big[1:1 + h, 2:2 + w] = crop.reshape(h, w, 3)
        assert (ref.grey_of_bgr(big[1:1 + h, 2:2 + w]) != ref.alpha_of_bgr(big[1:1 + h, 2:2 + w])).sum() >= len(odd)
    for view, pixels in ((_dev(big, dev)[1:1 + h, 2:2 + w], big[1:1 + h, 2:2 + w]), (_dev(big[:h, :w], dev), big[:h, :w])):
        assert np.array_equal(metrics_hip.grey_from_bgr_u8(view).cpu().numpy(), ref.grey_of_bgr(pixels))
        assert np.array_equal(metrics_hip.grey_from_bgr_u8(view, order='rgb').cpu().numpy(), ref.grey_of_bgr(pixels[:, :, ::-1]))


# -- PNG: the filter and the files --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _png_reference(h, w, content):
    img = make_grey(h, w, content)
    return img, ref.filter_rows(img)[0]


@pytest.mark.parametrize('h,w', PNG_SIZES)
def test_png_filter_and_files(dev, h, w):
    from ciaosr_amd import png_hip
    for content in CONTENTS:
        img, stream = _png_reference(h, w, content)
        t = _dev(img, dev)
        for rows in (0, 1, 5):
            r = ref.rows_per_band(w, rows)
            hist_want, adler_want = ref.band_tables(stream, h, w, r)
            got, hist, adler = png_hip.filter_u8(t, rows_per_band=rows)
            assert np.array_equal(got.cpu().numpy(), stream), (content, rows)
            assert np.array_equal(hist.cpu().numpy()[:, :257].astype(np.int64), hist_want[:, :257]), (content, rows)
            assert np.array_equal(adler.cpu().numpy().astype(np.int64), adler_want), (content, rows)
            png = png_hip.encode_png(t, rows_per_band=rows)
            assert png[25] == 0 and np.array_equal(pil_grey(png), img), (content, rows)
            assert zlib.decompress(b''.join(d for tag, d in _chunks(png) if tag == b'IDAT')) == bytes(stream), (content, rows)
            assert png_hip.encode_png(t, 'grey', rows) == png, (content, rows)                  # two calls give equal bytes


def _chunks(png):
    from tests.rgba_ref import chunks
    return chunks(png)


def test_png_every_filter_wins_on_the_device(dev):
    from ciaosr_amd import png_hip
    seen = set()
    for content in CONTENTS:
        got = png_hip.filter_u8(_dev(make_grey(33, 17, content), dev))[0].cpu().numpy().reshape(33, 18)
        seen |= set(got[:, 0].tolist())
    assert seen == {0, 1, 2, 3, 4}, seen


def test_png_pitched_crop(dev):
    from ciaosr_amd import png_hip
    big = make_grey(40, 31, 'noise', seed=3)
    big[10:30, 8:20] = make_grey(20, 12, 'ramp')
    t = _dev(big, dev)
    for y0, x0 in ((3, 5), (3, 6)):                         # an even and an odd first byte
        view = t[y0:y0 + 33, x0:x0 + 17]
        assert not view.is_contiguous() and view.stride(0) == 31 and (view.data_ptr() - t.data_ptr()) % 2 == (y0 * 31 + x0) % 2
        for lz in (False, True):
            png = png_hip.encode_png(view, matches=lz)
            assert png == png_hip.encode_png(view.contiguous(), matches=lz)
            assert np.array_equal(pil_grey(png), big[y0:y0 + 33, x0:x0 + 17])


@pytest.mark.parametrize('rows', [0, 3])
def test_png_tiles_are_the_single_encoder(dev, rows):
    from ciaosr_amd import png_hip
    img = make_grey(70, 91, 'noise', seed=2)
    img[20:50, 11:60] = make_grey(30, 49, 'ramp')
    img[55:, 70:] = 9
    t = _dev(img, dev)
    rects = [(0, 0, 70, 91), (69, 90, 1, 1), (41, 51, 29, 40), (0, 0, 1, 1), (11, 5, 33, 65), (13, 7, 33, 65), (3, 89, 60, 2), (55, 71, 15, 19)]
    for lz in (False, True):
        files, launches = _profile_of(lambda: png_hip.encode_png_tiles(t, rects, rows_per_band=rows, matches=lz))
        want = dict(png_grey_filter_tiles_u8=1, deflate_plan=1, png_tiles_scan=1, deflate_pack=1)
        if lz:
            want.update(deflate_lz_match=1, deflate_lz_plan=1, deflate_lz_pack=1)
        assert launches == want
        assert len(files) == len(rects)
        for (y0, x0, h, w), png in zip(rects, files):
            assert png == png_hip.encode_png(t[y0:y0 + h, x0:x0 + w], rows_per_band=rows, matches=lz), (y0, x0, h, w, lz)
            assert np.array_equal(pil_grey(png), img[y0:y0 + h, x0:x0 + w])
    _, single = _profile_of(lambda: png_hip.encode_png(t))
    assert single == dict(png_grey_filter_u8=1, deflate_plan=1, deflate_scan=1, deflate_pack=1)


def _match_images():
    half = make_grey(256, 256, 'noise', seed=4)
    half[:, 128:] = 200
    columns = lambda h, w: np.ascontiguousarray(np.broadcast_to(make_grey(1, w, 'noise', seed=6), (h, w)))   # Up leaves rows of zeros
    return {'flat': make_grey(64, 64, 'flat'), 'half': half, 'w1': make_grey(3000, 1, 'flat'), 'w1_noise': make_grey(300, 1, 'noise'),
            'w2': columns(900, 2), 'w3': make_grey(900, 3, 'flat0'), 'w16': columns(300, 16), 'w16_flat': make_grey(300, 16, 'flat255')}


@pytest.mark.parametrize('name', sorted(_match_images()))
def test_png_matches(dev, name):
    from ciaosr_amd import _lib, png_hip
    img = _match_images()[name]
    h, w = img.shape
    t = _dev(img, dev)
    line = w + 1
    z_lz, z_lit = png_hip.encode_zlib(t, matches=True), png_hip.encode_zlib(t)
    png_lz, png_lit = png_hip.encode_png(t, matches=True), png_hip.encode_png(t)
    assert len(png_lz) <= len(png_lit) and len(z_lz) <= len(z_lit)                       # never larger than the literal file
    assert np.array_equal(pil_grey(png_lz), img) and np.array_equal(pil_grey(png_lit), img)
    stream, _, adler = png_hip.filter_u8(t)
    raw = stream.cpu().numpy().tobytes()
    assert raw == bytes(ref.filter_rows(img)[0]) == zlib.decompress(z_lz)
    offs = ref.band_offsets(h, w, _lib.load().ciaosr_png_grey_rows_per_band(w, 0))
    lz = png_hip.deflate_huff(stream, offs, matches=True, line=line, bpp=1)
    lit = png_hip.deflate_huff(stream, offs)
    partials = [(int(a), int(b), offs[i + 1] - offs[i]) for i, (a, b) in enumerate(adler.cpu().tolist())]
    assert png_hip.zlib_stream(lz, partials) == z_lz and png_hip.zlib_stream(lit, partials) == z_lit     # the one call is the stages
    in_match_mode = 0
    for i, (seg, plain) in enumerate(zip(lz, lit)):
        band = raw[offs[i]:offs[i + 1]]
        assert len(seg) <= len(plain), i
        if seg == plain:
            continue
        blocks, data, _ = mref.inflate_tokens(seg if i == len(lz) - 1 else seg + FINAL)
        assert data == band, i
        assert blocks[0]['type'] == 2 and blocks[0]['tokens'] == mref.parse(band, line, 1), i
        in_match_mode += 1
    print(f'{name}: {in_match_mode} of {len(lz)} bands in match mode, {len(z_lz)} B against {len(z_lit)} B')
    if name != 'w1_noise':
        assert in_match_mode >= 1 and len(z_lz) < len(z_lit)


# -- JPEG: Pillow's mode-L files, byte for byte -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('content', JPEG_CONTENTS)
def test_jpeg_files_are_pillows(dev, content):
    from ciaosr_amd.jpeg_hip import encode_jpeg
    for h, w in JPEG_SIZES:
        img = make_grey(h, w, content)
        t = _dev(img, dev)
        for q in QUALITIES:
            for optimize in (False, True):
                want = pil_jpeg_grey(img, q, optimize)
                for mcus in (0, 1, 3):
                    got = encode_jpeg(t, quality=q, mcus_per_chunk=mcus, optimize=optimize)
                    assert got == want, (h, w, content, q, optimize, mcus, len(got), len(want))
    assert np.array_equal(pil_grey(got).shape, (h, w))


def test_jpeg_pitched_crop_and_tiles(dev):
    from ciaosr_amd import jpeg_hip
    img = make_grey(72, 137, 'noise', seed=5)
    img[10:60, 21:120] = make_grey(50, 99, 'ramp')
    img[:, 125:] = make_grey(72, 12, 'checker')
    t = _dev(img, dev)
    rects = [(0, 0, 72, 137), (71, 136, 1, 1), (3, 5, 33, 65), (5, 3, 33, 65), (9, 11, 8, 8), (0, 121, 72, 16), (17, 1, 9, 17), (40, 100, 32, 37)]
    for optimize in (False, True):
        want = [pil_jpeg_grey(img[y0:y0 + h, x0:x0 + w], 90, optimize) for y0, x0, h, w in rects]
        files, launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, rects, optimize=optimize))
        assert launches == (OPT_LAUNCHES if optimize else PLAIN_LAUNCHES)
        _, few = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, rects[:2], optimize=optimize))
        assert few == launches                              # whatever the number of crops
        assert files == want
        for mcus in (1, 3):
            assert jpeg_hip.encode_jpeg_tiles(t, rects, mcus_per_chunk=mcus, optimize=optimize) == want, (optimize, mcus)
        for (y0, x0, h, w), data in zip(rects, want):
            view = t[y0:y0 + h, x0:x0 + w]
            single, one = _profile_of(lambda: jpeg_hip.encode_jpeg(view, optimize=optimize))
            assert single == data and one == launches, (y0, x0, h, w, optimize)


def test_jpeg_length_limiting(dev):
    """An image whose AC tree is more than 16 levels deep before limiting (chosen on the CPU by the rule of tests/jpeg_opt_ref.py on
    the one component, and asserted here): the device's limiting step runs on a one-component scan."""
    from ciaosr_amd.jpeg_hip import encode_jpeg
    from tests.test_jpeg_opt_host import craft
    img = np.ascontiguousarray(craft(512, 512, seed=1, p=0.4)[:, :, 0])
    depths = ref.jpeg_table_depths(img, 100)
    assert max(depths) > 16, depths
    want = pil_jpeg_grey(img, 100, optimize=True)
    t = _dev(img, dev)
    assert encode_jpeg(t, quality=100, optimize=True) == want
    assert encode_jpeg(t, quality=100, optimize=True, mcus_per_chunk=5) == want
    assert encode_jpeg(t, quality=100) == pil_jpeg_grey(img, 100)


def test_jpeg_refusals_launch_nothing(dev):
    from ciaosr_amd import hip_ops, jpeg_hip
    t = _dev(make_grey(16, 16, 'noise'), dev)
    with hip_ops.profile():
        for kw in (dict(progressive=True), dict(subsampling='420'), dict(order='rgb')):
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg(t, **kw)
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg_tiles(t, [(0, 0, 8, 8)], **kw)
    assert hip_ops.profile.results() == {}


# -- renders ----------------------------------------------------------------------------------------------------------------------------
LR = (24, 20)
TILED = dict(tile=16, tile_overlap=4, tile_any_scale=True)


def _model(dev, cfg):
    """fp32: the tiny EDSR generator of tests/test_png_gpu.py (16 channels, 2 blocks, seeded weights).  f16: the library's 16-bit head
    runs fused kernels only and refuses that generator's head outright (`ciaosr_head_prepare_f16`: unsupported configuration, with or
    without this feature), so the f16 cases run the tiny seeded RDN restorer that the scene, view and RGBA tests use for f16."""
    if cfg.get('precision', 'fp32') == 'fp32':
        from tests.test_png_gpu import _restorer
        return _restorer(dict(cfg)).to(dev)
    from tests.test_view_gpu import _model as view_model
    model = view_model('rdn', dev, 3)
    model.test_cfg = dict(cfg)
    return model


def _grey_input(dev, h=LR[0], w=LR[1]):
    g = torch.Generator().manual_seed(11)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    smooth = 0.5 + 0.35 * torch.sin(y / 3.0) * torch.cos(x / 4.0)
    img = (smooth + 0.08 * torch.randn(h, w, generator=g)).clamp(0, 1)
    return (img * 255).round().div(255)[None, None].to(dev)


def _l(colour_u8):
    """convert('L') of a uint8 [H, W, 3] BGR device image, on the host."""
    from PIL import Image
    bgr = colour_u8.cpu().numpy()
    pil = np.asarray(Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).convert('L'))
    assert np.array_equal(pil, ref.grey_of_bgr(bgr))
    return pil


@pytest.mark.parametrize('tiled', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_renders_are_the_grey_of_the_colour_renders(dev, precision, tiled):
    from ciaosr_amd import scene
    model = _model(dev, dict(precision=precision, **(TILED if tiled else {})))
    x1 = _grey_input(dev)
    x3 = x1.expand(-1, 3, -1, -1).contiguous()
    enc, plain = model.encode_grey(x1, max_scale=2.7), model.encode(x3, max_scale=2.7)
    assert enc.grey and not plain.grey and not enc.alpha and tuple(enc.x.shape) == (1, 3) + LR
    size = (round(24 * 2.7), round(20 * 2.7))
    colour_differs = False
    for window in (None, (5, 7, 30, 41)):
        got = model.render(enc, scale=2.7, window=window, as_u8=True)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (size if window is None else window[2:])
        colour = model.render(plain, scale=2.7, window=window, as_u8=True)
        assert np.array_equal(got.cpu().numpy(), _l(colour)), window
        colour_differs |= bool((colour[:, :, 0] != colour[:, :, 2]).any())
        fp = model.render(enc, scale=2.7, window=window)                        # as_u8=False: the plain encode's fp32, bit for bit
        assert fp.dtype == torch.float32 and torch.equal(fp, model.render(plain, scale=2.7, window=window))
    assert colour_differs                                   # the colour render of a grey input is NOT grey: what the feature is for
    # a 30-degree view with fill 0.25: outside the image the byte of (fill, fill, fill)
    vsize = (48, 44)
    m = scene.view_matrix((6.0, 8.0), 2.0, 30, vsize)
    inside = vr.members(*vr.lr_points(m, *vsize), (0, 0) + LR).reshape(vsize)
    assert (~inside).sum() > 300 and inside.sum() > 300
    view = model.render_view(enc, m, vsize, fill=0.25, as_u8=True)
    assert np.array_equal(view.cpu().numpy(), _l(model.render_view(plain, m, vsize, fill=0.25, as_u8=True)))
    assert (view.cpu().numpy()[~inside] == 64).all()
    assert torch.equal(model.render_view(enc, m, vsize, fill=0.25), model.render_view(plain, m, vsize, fill=0.25))
    # a list in one walk
    targets = lambda: [scene.Grid(scale=2.7), scene.View(m, vsize, 0.25), scene.Grid(scale=1.5, window=(2, 3, 20, 17))]
    many = model.render_many(model.encode_grey(x1, max_scale=2.7), targets(), as_u8=True)
    want = model.render_many(model.encode(x3, max_scale=2.7), targets(), as_u8=True)
    assert [tuple(g.shape) for g in many] == [size, vsize, (20, 17)]
    for g, c in zip(many, want):
        assert g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), _l(c))
    assert torch.equal(many[0], model.render(enc, scale=2.7, as_u8=True)) and torch.equal(many[1], view)
    # a self-ensemble record may be grey: quantised once, after the mean
    ens, ens3 = model.encode_grey(x1, max_scale=2.7, self_ensemble=(0, 5)), model.encode(x3, max_scale=2.7, self_ensemble=(0, 5))
    assert ens.grey and ens.ids == (0, 5)
    for window in (None, (5, 7, 30, 41)):
        got = model.render(ens, scale=2.7, window=window, as_u8=True)
        assert got.dim() == 2 and np.array_equal(got.cpu().numpy(), _l(model.render(ens3, scale=2.7, window=window, as_u8=True)))
        assert torch.equal(model.render(ens, scale=2.7, window=window), model.render(ens3, scale=2.7, window=window))
    got = model.render_many(ens, [scene.Grid(scale=2.7), scene.Grid(scale=2)], as_u8=True)
    want = model.render_many(ens3, [scene.Grid(scale=2.7), scene.Grid(scale=2)], as_u8=True)
    assert all(np.array_equal(g.cpu().numpy(), _l(c)) for g, c in zip(got, want))
    with pytest.raises(ValueError):
        model.render_view(ens, m, vsize, as_u8=True)
    with pytest.raises(ValueError):
        model.encode_grey(x3)
    with pytest.raises(ValueError):
        model.encode_rgba(torch.cat([x1, x1], 1))           # grey + alpha


def test_pyramid(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import scene
    from ciaosr_amd.pyramid import dzi_plan, level_sizes, write_dzi
    model = _model(dev, dict())
    x1 = _grey_input(dev)
    x3 = x1.expand(-1, 3, -1, -1).contiguous()
    sizes = [(1, 1), (2, 2), (3, 3), (6, 5), (12, 10), (24, 20), (48, 40)]
    assert level_sizes(48, 40) == sizes
    imgs = model.render_pyramid(model.encode_grey(x1, max_scale=2), scale=2)
    assert [tuple(im.shape) for im in imgs] == sizes and all(im.dtype == torch.uint8 and im.is_cuda for im in imgs)
    colour = model.render_many(model.encode(x3, max_scale=2), [scene.Grid(size=s) for s in sizes[5:]], as_u8=True)
    for k, c in zip((5, 6), colour):
        assert np.array_equal(imgs[k].cpu().numpy(), _l(c)), k
    base = Image.fromarray(imgs[5].cpu().numpy(), 'L')      # the grey smallest model level, 24 x 20
    for k in range(5):
        want = np.asarray(base.resize((sizes[k][1], sizes[k][0]), Image.BICUBIC))
        assert np.array_equal(imgs[k].cpu().numpy(), want), k
    levels = [im.cpu().numpy() for im in imgs]
    plan = dzi_plan(48, 40, 16, 2)
    colour_run = write_dzi(model, model.encode(x3, max_scale=2), str(tmp_path / 'rgb'), 'img', scale=2, tile_size=16, overlap=2)
    manifest = open(str(tmp_path / 'rgb' / 'img.dzi'), 'rb').read()
    sizes_of = {}
    for name, kw in (('png', {}), ('lz', dict(matches=True)), ('jpg', dict(fmt='jpg', quality=85, optimize=True))):
        res = write_dzi(model, model.encode_grey(x1, max_scale=2), str(tmp_path / name), 'img', scale=2, tile_size=16, overlap=2, **kw)
        assert res['levels'] == sizes and res['model_levels'] == [5, 6] and res['files'] == colour_run['files']
        ext = 'jpg' if name == 'jpg' else 'png'
        assert open(str(tmp_path / name / 'img.dzi'), 'rb').read() == manifest.replace(b'Format="png"', f'Format="{ext}"'.encode())
        sizes_of[name] = 0
        for lv, level in zip(plan, levels):
            for col, row, y0, x0, h, w in lv['tiles']:
                data = open(str(tmp_path / name / 'img_files' / str(lv['level']) / f'{col}_{row}.{ext}'), 'rb').read()
                sizes_of[name] += len(data)
                crop = level[y0:y0 + h, x0:x0 + w]
                if ext == 'png':
                    assert data[25] == 0 and np.array_equal(pil_grey(data), crop), (name, lv['level'], col, row)
                else:
                    assert data == pil_jpeg_grey(crop, 85, optimize=True), (lv['level'], col, row)
                    assert pil_grey(data).shape == crop.shape
    assert sizes_of['lz'] <= sizes_of['png']
    for kw in (dict(progressive=True), dict(subsampling='420')):
        with pytest.raises(ValueError):
            write_dzi(model, model.encode_grey(x1, max_scale=2), str(tmp_path / 'bad'), 'img', scale=2, fmt='jpg', **kw)
    assert not (tmp_path / 'bad').exists()


def test_niqe_of_a_grey_image_is_that_of_its_replicated_image(dev):
    from ciaosr_amd import niqe_hip
    params = niqe_hip.load_params(os.path.join(REPO, 'tests', 'golden', 'niqe_pris_params.npz'))
    rng = np.random.RandomState(9)
    y, x = np.mgrid[0:192, 0:288]
    img = np.clip(128 + 60 * np.sin(y / 7.0) * np.cos(x / 9.0) + rng.normal(0, 12, (192, 288)), 0, 255).astype(np.uint8)
    g = _dev(img, dev)
    wide = _dev(np.stack([img, img, img], axis=-1), dev)
    assert torch.equal(niqe_hip.moments_u8(g, params), niqe_hip.moments_u8(wide, params))
    score = niqe_hip.niqe_u8(g, params)
    assert score == niqe_hip.niqe_u8(wide, params) and np.isfinite(score)
    assert torch.equal(niqe_hip.moments_u8(g[3:, 5:], params), niqe_hip.moments_u8(wide[3:, 5:], params))     # a pitched view
    with pytest.raises(ValueError):
        niqe_hip.niqe_u8(g[:50], params)                    # too small for two blocks: a ValueError as for colour


# -- tools/render.py --grey -------------------------------------------------------------------------------------------------------------
def test_render_cli_grey(dev, tmp_path, capsys):
    import json
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, scene
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_grey01
    from ciaosr_amd.init_utils import seeded_init_
    from ciaosr_amd.pyramid import dzi_plan
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, grey_png, colour_png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png'), str(tmp_path / 'colour.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    g = (_grey_input('cpu', 24, 30)[0, 0].numpy() * 255).round().astype(np.uint8)
    Image.fromarray(g, 'L').save(grey_png)
    Image.fromarray(np.stack([g, 255 - g, g], axis=-1), 'RGB').save(colour_png)
    view, size = (11.0, 14.5, 2.2, 20.0), (37, 45)
    flags = ['--scale', '2.5', '--view', *[str(v) for v in view], '--size', str(size[0]), str(size[1]), '--dzi', '2', '--dzi-tile', '32']
    niqe = os.path.join(REPO, 'tests', 'golden', 'niqe_pris_params.npz')
    with hip_ops.profile():
        paths = render.main([config, ckpt, grey_png, *flags, '--grey', '--png-matches', '--niqe', niqe, '--out', str(tmp_path / 'a')])
    prof = hip_ops.profile.results()
    assert 'not a grey image' not in capsys.readouterr().out
    assert [os.path.basename(p) for p in paths] == ['img_x2p5.png', 'img_view0.png']
    assert prof['png_grey_filter_u8']['launches'] == 2 and prof['tensor2img_grey_u8']['launches'] >= 2
    assert 'png_filter_u8' not in prof and 'tensor2img_u8' not in prof and prof['deflate_lz_match']['launches'] >= 2
    assert json.load(open(str(tmp_path / 'a' / 'niqe.json'))) == {'img_x2p5.png': None, 'img_view0.png': None}      # too small for two blocks
    # the files decode to the device images of the same encode
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                 # what the tool sets
    lq1, was_grey = imread_grey01(grey_png)
    assert was_grey
    enc = model.encode_grey(lq1.unsqueeze(0).to(dev), max_scale=2.5)
    m = scene.view_matrix(view[:2], view[2], view[3], size)
    want = model.render_many(enc, [scene.Grid(scale=2.5), scene.View(m, size)], as_u8=True)
    for path, img in zip(paths, want):
        data = open(path, 'rb').read()
        assert data[25] == 0 and np.array_equal(pil_grey(data), img.cpu().numpy())
    levels = [im.cpu().numpy() for im in model.render_pyramid(enc, scale=2)]
    plan = dzi_plan(48, 60, 32, 1)
    for lv, level in zip(plan, levels):
        for col, row, y0, x0, h, w in lv['tiles']:
            data = open(str(tmp_path / 'a' / 'img_files' / str(lv['level']) / f'{col}_{row}.png'), 'rb').read()
            assert np.array_equal(pil_grey(data), level[y0:y0 + h, x0:x0 + w]), (lv['level'], col, row)
    # JPEG, optimised: Pillow's mode-L files of the same device images; a file that was not grey is reported
    paths = render.main([config, ckpt, grey_png, *flags, '--grey', '--jpeg', '85', '--jpeg-optimize', '--out', str(tmp_path / 'b')])
    assert [os.path.basename(p) for p in paths] == ['img_x2p5.jpg', 'img_view0.jpg']
    for path, img in zip(paths, want):
        assert open(path, 'rb').read() == pil_jpeg_grey(img.cpu().numpy(), 85, optimize=True)
    for lv, level in zip(plan, levels):
        for col, row, y0, x0, h, w in lv['tiles']:
            data = open(str(tmp_path / 'b' / 'img_files' / str(lv['level']) / f'{col}_{row}.jpg'), 'rb').read()
            assert data == pil_jpeg_grey(level[y0:y0 + h, x0:x0 + w], 85, optimize=True), (lv['level'], col, row)
    assert b'Format="jpg"' in open(str(tmp_path / 'b' / 'img.dzi'), 'rb').read()
    capsys.readouterr()
    paths = render.main([config, ckpt, colour_png, '--scale', '2', '--grey', '--self-ensemble', '--out', str(tmp_path / 'c')])
    assert 'not a grey image' in capsys.readouterr().out
    lq1, was_grey = imread_grey01(colour_png)
    assert not was_grey
    ens = model.encode_grey(lq1.unsqueeze(0).to(dev), max_scale=2, self_ensemble=True)
    assert np.array_equal(pil_grey(open(paths[0], 'rb').read()), model.render(ens, scale=2, as_u8=True).cpu().numpy())
