"""16-bit samples on the GPU: the uint16 quantisers against torch's own arithmetic on the host and the numpy grey formula, the depth-16
PNG filter, files, crops, tiles and matches against the restatement of tests/png16_ref.py, Pillow's decoder (grey) and the match
contract (tests/png_match_ref.py), the `as_u16` renders against the quantiser's definition applied to the fp32 renders, and
tools/render.py --depth16 end to end.  Never the device against itself.
Run on the GPU box:  python -m pytest tests/test_depth16_gpu.py -m gpu -q
"""
import functools
import io
import os
import zlib

import numpy as np
import pytest
import torch

from tests import png16_ref as ref
from tests import view_reference as vr
from tests.test_depth16_host import FILTER_SIZES

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINAL = b'\x01\x00\x00\xff\xff'                            # an empty stored block with BFINAL: ends a segment that is not the last
QUANT_SIZES = [(7, 1), (5, 3), (3, 4), (7, 5), (6, 259), (4, 1027)]
KINDS = [(1, 'grey'), (3, 'bgr'), (3, 'rgb')]
PREFIX = {1: 'png16_grey_', 3: 'png16_'}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _dev(img, order, dev):
    """The device tensor of the image `img` (uint16 [H, W], or [H, W, 3] in R G B order) that `order` names."""
    arr = img[:, :, ::-1] if order == 'bgr' else img
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def _host(t):
    return t.cpu().numpy()


def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def _pil16(png):
    from PIL import Image
    with Image.open(io.BytesIO(png)) as f:
        assert f.mode.startswith('I;16'), f.mode
        return np.asarray(f).astype(np.uint16)


def _decode(png, c):
    """The samples of a file: Pillow's for grey, the reference decoder's for RGB (Pillow has no 16-bit RGB)."""
    if c == 1:
        got = _pil16(png)
        assert np.array_equal(got, ref.decode_png16(png))
        return got
    return ref.decode_png16(png)


# -- the quantisers ---------------------------------------------------------------------------------------------------------------------
def _render_like(h, w, seed):
    """[3, h, w] fp32: uniform noise from -0.25 to 1.25, and -- where they fit -- the ties (k + 0.5) / 65535 with both fp32 neighbours,
    exact k / 255, values far outside, the ends 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(3, h, w, generator=g) * 1.5 - 0.25
    flat = t.view(-1)
    k = torch.cat([torch.arange(0, 40), torch.arange(32700, 32840), torch.arange(65490, 65535)]).double()
    ties = ((k + 0.5) / 65535).float()
    special = torch.cat([ties, torch.nextafter(ties, torch.tensor(2.0)), torch.nextafter(ties, torch.tensor(-1.0)),
                         (torch.arange(256).double() / 255).float(), torch.tensor([-3.0, 7.0, 0.0, 1.0, -0.0, float('inf'), -float('inf')])])
    n = min(len(special), flat.numel())
    pick = torch.randperm(len(special), generator=g)[:n]
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = special[pick]
    return t


def _torch_q16(t):
    """The oracle: torch on the same tensor, on the host -> uint16 numpy with t's shape."""
    return (t.cpu().clamp(0, 1) * 65535).round().numpy().astype(np.uint16)


@pytest.mark.parametrize('h,w', QUANT_SIZES)
def test_tensor2img_u16_is_torchs_rounding(dev, h, w):
    from ciaosr_amd import metrics_hip
    t = _render_like(h, w, seed=100 * h + w)
    want = _torch_q16(t)[::-1].transpose(1, 2, 0)            # B G R, HWC
    assert np.array_equal(want, ref.image_of(t))
    got = metrics_hip.tensor2img_u16(t.to(dev))
    assert got.dtype == torch.uint16 and tuple(got.shape) == (h, w, 3) and got.is_cuda and got.is_contiguous()
    assert np.array_equal(_host(got), want)
    assert np.array_equal(_host(metrics_hip.tensor2img_u16(t.to(dev).unsqueeze(0))), want)
    # not the 8-bit image: k / 255 gives 257 k, and in general the high byte is not tensor2img_u8's byte
    levels = (torch.arange(256).double() / 255).float().reshape(1, 1, 256).expand(3, 1, 256).contiguous().to(dev)
    assert np.array_equal(_host(metrics_hip.tensor2img_u16(levels))[0, :, 0], 257 * np.arange(256))
    if h * w >= 1000:
        u8 = _host(metrics_hip.tensor2img_u8(t.to(dev)))
        assert ((want >> 8) != u8).any() and (want != 257 * u8.astype(np.uint16)).any()
    with pytest.raises(ValueError):
        metrics_hip.tensor2img_u16(t[:2].to(dev))


def _grey_triples():
    """uint16 B G R triples: the ends, neutral values, and triples on which L16 is not the plain mean."""
    rng = np.random.RandomState(5)
    fixed = np.array([[65535, 65535, 65535], [0, 0, 0], [65535, 0, 0], [0, 65535, 0], [0, 0, 65535], [1, 1, 1], [32768, 32768, 32768],
                      [65535, 65535, 0], [0, 65535, 65535], [12345, 54321, 777]], dtype=np.uint16)
    return np.concatenate([fixed, rng.randint(0, 65536, (90, 3)).astype(np.uint16)])


@pytest.mark.parametrize('h,w', QUANT_SIZES)
def test_tensor2img_grey_u16_and_grey_from_bgr_u16(dev, h, w):
    from ciaosr_amd import metrics_hip
    t = _render_like(h, w, seed=7 * h + w)
    tri = _grey_triples()[:h * w]                             # exact samples v / 65535 quantise back to v
    flat = t.view(3, -1)
    flat[:, :len(tri)] = torch.from_numpy((tri[:, ::-1].astype(np.float64) / 65535).astype(np.float32).T.copy())
    bgr = ref.image_of(t)
    assert np.array_equal(bgr.reshape(-1, 3)[:len(tri)], tri)
    want = ref.grey16(bgr)
    assert want.reshape(-1)[0] == 65535
    mean = bgr.astype(np.int64).sum(axis=2) // 3
    assert h * w < 10 or (want != mean).any()
    got = metrics_hip.tensor2img_grey_u16(t.to(dev))
    assert got.dtype == torch.uint16 and tuple(got.shape) == (h, w) and got.is_cuda
    assert np.array_equal(_host(got), want)
    assert np.array_equal(_host(metrics_hip.tensor2img_grey_u16(t.to(dev).unsqueeze(0))), want)
    neutral = t[:1].expand(3, -1, -1).contiguous()
    assert np.array_equal(_host(metrics_hip.tensor2img_grey_u16(neutral.to(dev))), _torch_q16(neutral)[0])
    # pitched outputs: a start at an odd sample (byte offset 2 mod 4) and at an even one, pitches odd and even; nothing beyond a row
    for pitch, start in ((w + 3, 1), (w + 2, 3), (w + 4, 0), (w + 1, 2)):
        buf = torch.from_numpy(np.full(h * pitch + 8, 0xABCD, dtype=np.uint16)).to(dev)
        view = torch.as_strided(buf, (h, w), (pitch, 1), start)
        assert metrics_hip.tensor2img_grey_u16(t.to(dev), out=view) is view
        raw = _host(buf)
        rows = raw[start:start + h * pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :w], want), (pitch, start)
        assert (rows[:, w:] == 0xABCD).all() and (raw[:start] == 0xABCD).all() and (raw[start + h * pitch:] == 0xABCD).all(), (pitch, start)
    with pytest.raises(ValueError):
        metrics_hip.tensor2img_grey_u16(t.to(dev), out=torch.empty((h, w), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        metrics_hip.tensor2img_grey_u16(t.to(dev), out=torch.empty((h, w + 1), dtype=torch.uint16, device=dev))
    # the same reduction from a 16-bit image, contiguous and as a crop at an odd pixel of a larger one, in both orders
    rng = np.random.RandomState(h + w)
    big = rng.randint(0, 65536, (h + 3, w + 5, 3)).astype(np.uint16)
    crop = big[1:1 + h, 3:3 + w].copy()
    crop.reshape(-1, 3)[:len(tri)] = tri
    big[1:1 + h, 3:3 + w] = crop
    for view, pixels in ((torch.from_numpy(big).to(dev)[1:1 + h, 3:3 + w], crop), (torch.from_numpy(crop).to(dev), crop)):
        assert np.array_equal(_host(metrics_hip.grey_from_bgr_u16(view)), ref.grey16(pixels))
        assert np.array_equal(_host(metrics_hip.grey_from_bgr_u16(view, order='rgb')), ref.grey16(pixels[:, :, ::-1]))
    with pytest.raises(ValueError):
        metrics_hip.grey_from_bgr_u16(torch.from_numpy(crop).to(dev), order='grey')


# -- PNG: the filter and the files --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(h, w, c, content):
    img = ref.make16(h, w, c, content)
    stream, kinds, _ = ref.filter_rows(img)
    return img, stream, kinds


@functools.lru_cache(maxsize=None)
def _tables(h, w, c, content, r):
    return ref.band_tables(_reference(h, w, c, content)[1], h, 1 + 2 * c * w, r)


@pytest.mark.parametrize('c,order', KINDS)
@pytest.mark.parametrize('h,w', FILTER_SIZES)
def test_png16_filter_and_files(dev, h, w, c, order):
    from ciaosr_amd import _lib, png_hip
    bpp, line = 2 * c, 1 + 2 * c * w
    for content in ref.CONTENTS:
        img, stream, _ = _reference(h, w, c, content)
        t = _dev(img, order, dev)
        for rows in (0, 1, 5):
            r = ref.rows_per_band(w, rows, bpp)
            assert getattr(_lib.load(), 'ciaosr_' + PREFIX[c] + 'rows_per_band')(w, rows) == r
            hist_want, adler_want = _tables(h, w, c, content, r)
            got, hist, adler = png_hip.filter_u8(t, order, rows_per_band=rows)
            assert got.dtype == torch.uint8 and got.numel() == h * line
            assert np.array_equal(_host(got), stream), (content, rows)
            assert np.array_equal(_host(hist)[:, :257].astype(np.int64), hist_want), (content, rows)
            assert np.array_equal(_host(adler).astype(np.int64), adler_want), (content, rows)
            png = png_hip.encode_png(t, order, rows_per_band=rows)
            assert ref.ihdr(png) == (w, h, 16, 0 if c == 1 else 2, 0, 0, 0), (content, rows)
            assert [tag for tag, _ in ref.chunks(png)] == [b'IHDR', b'IDAT', b'IEND']
            assert zlib.decompress(ref.idat(png)) == bytes(stream), (content, rows)
            assert png_hip.encode_png(t, order, rows) == png, (content, rows)                   # two calls give equal bytes
        assert np.array_equal(_decode(png, c), img), content


@pytest.mark.parametrize('c,order', KINDS)
def test_png16_every_filter_wins_on_the_device(dev, c, order):
    from ciaosr_amd import png_hip
    seen = set()
    for h, w in FILTER_SIZES:
        for content in ref.CONTENTS:
            got = _host(png_hip.filter_u8(_dev(ref.make16(h, w, c, content), order, dev), order)[0]).reshape(h, 1 + 2 * c * w)
            seen |= set(got[:, 0].tolist())
    assert seen == {0, 1, 2, 3, 4}, seen


def test_png16_byte_order_cannot_be_wrong_unnoticed(dev, tmp_path):
    """Every sample 0xHHLL with HH != LL and HH != 255 - LL: the stream holds HH first, and both decoders give the samples back."""
    from ciaosr_amd import png_hip
    from ciaosr_amd.imageio import read_png16
    for c, order in KINDS:
        img = ref.make16(9, 300, c, 'bytes')
        assert ((img >> 8) != (img & 255)).all() and ((img >> 8) != 255 - (img & 255)).all()
        t = _dev(img, order, dev)
        stream = _host(png_hip.filter_u8(t, order)[0]).reshape(9, -1)
        assert np.array_equal(ref.unfilter(stream.reshape(-1), 9, stream.shape[1], 2 * c), ref.byte_rows(img))
        png = png_hip.encode_png(t, order)
        assert np.array_equal(_decode(png, c), img)
        path = str(tmp_path / f'{c}{order}.png')
        png_hip.imwrite_gpu(t, path, order)
        assert open(path, 'rb').read() == png and np.array_equal(read_png16(path), img)       # the project's own reader closes the loop


def test_png16_refusals(dev):
    from ciaosr_amd import hip_ops, png_hip
    from ciaosr_amd._lib import CiaoSRHipError
    with hip_ops.profile():
        with pytest.raises(CiaoSRHipError, match='16-bit alpha'):
            png_hip.encode_png(torch.empty((4, 5, 4), dtype=torch.uint16, device=dev))
        with pytest.raises(ValueError):
            png_hip.encode_png(torch.empty((4, 5, 3), dtype=torch.uint16, device=dev), order='bgra')
        with pytest.raises(ValueError):
            png_hip.encode_png(torch.empty((4, 5), dtype=torch.uint16, device=dev), order='rgb')
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(torch.empty((4, 5, 2), dtype=torch.uint16, device=dev))
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(torch.empty((4, 5, 3), dtype=torch.uint16))                      # a host tensor
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(torch.empty((4, 5, 3), dtype=torch.int16, device=dev))
    assert hip_ops.profile.results() == {}
    from ciaosr_amd import jpeg_hip
    with pytest.raises((CiaoSRHipError, ValueError)):
        jpeg_hip.encode_jpeg(torch.empty((16, 16, 3), dtype=torch.uint16, device=dev))          # JPEG stays 8-bit


@pytest.mark.parametrize('c,order', KINDS)
def test_png16_pitched_crop(dev, c, order):
    from ciaosr_amd import png_hip
    big = ref.make16(40, 31, c, 'noise', seed=3)
    big[10:30, 8:20] = ref.make16(20, 12, c, 'wrap_ramp')
    t = _dev(big, order, dev)
    for y0, x0 in ((3, 5), (4, 5), (3, 6)):                 # odd first pixels on an odd pitch, and an even one
        view = t[y0:y0 + 33, x0:x0 + 17]
        off = view.data_ptr() - t.data_ptr()
        assert not view.is_contiguous() and off == 2 * c * (y0 * 31 + x0)
        if c == 1 and (y0, x0) == (3, 6):
            assert off % 4 == 2 and (2 * view.stride(0)) % 4 == 2          # grey16: two bytes past a word, on a pitch that is no word multiple
        for lz in (False, True):
            png = png_hip.encode_png(view, order, matches=lz)
            assert png == png_hip.encode_png(_dev(big[y0:y0 + 33, x0:x0 + 17], order, dev), order, matches=lz), (y0, x0, lz)
            assert np.array_equal(_decode(png, c), big[y0:y0 + 33, x0:x0 + 17])


@pytest.mark.parametrize('c,order', KINDS)
@pytest.mark.parametrize('rows', [0, 3])
def test_png16_tiles_are_the_single_encoder(dev, rows, c, order):
    from ciaosr_amd import png_hip
    img = ref.make16(70, 91, c, 'noise', seed=2)
    img[20:50, 11:60] = ref.make16(30, 49, c, 'wrap_ramp')
    img[55:, 70:] = 9
    t = _dev(img, order, dev)
    rects = [(0, 0, 70, 91), (69, 90, 1, 1), (41, 51, 29, 40), (0, 0, 1, 1), (11, 5, 33, 65), (13, 7, 33, 65), (3, 89, 60, 2), (55, 71, 15, 19)]
    name = PREFIX[c] + 'filter'
    for lz in (False, True):
        files, launches = _profile_of(lambda: png_hip.encode_png_tiles(t, rects, order, rows_per_band=rows, matches=lz))
        want = {name + '_tiles_u16': 1, 'deflate_plan': 1, 'png_tiles_scan': 1, 'deflate_pack': 1}
        if lz:
            want.update(deflate_lz_match=1, deflate_lz_plan=1, deflate_lz_pack=1)
        assert launches == want and len(launches) == (7 if lz else 4)
        assert len(files) == len(rects)
        for (y0, x0, h, w), png in zip(rects, files):
            assert png == png_hip.encode_png(t[y0:y0 + h, x0:x0 + w], order, rows_per_band=rows, matches=lz), (y0, x0, h, w, lz)
            assert ref.ihdr(png)[:4] == (w, h, 16, 0 if c == 1 else 2)
            if h * w <= 33 * 65:
                assert np.array_equal(_decode(png, c), img[y0:y0 + h, x0:x0 + w])
    _, single = _profile_of(lambda: png_hip.encode_png(t, order))
    assert single == {name + '_u16': 1, 'deflate_plan': 1, 'deflate_scan': 1, 'deflate_pack': 1}
    streams, offs = png_hip.encode_tiles_device(t, rects, order, rows_per_band=rows)
    o = offs.cpu().tolist()
    zs = png_hip.encode_zlib_tiles(t, rects, order, rows_per_band=rows)
    raw = _host(streams).tobytes()
    assert o[0] == 0 and [raw[o[k]:o[k + 1]] for k in range(len(rects))] == zs
    assert zs[4] == png_hip.encode_zlib(t[11:44, 5:70], order, rows_per_band=rows)


def _match_images(c):
    half = ref.make16(128 // c, 128, c, 'noise', seed=4)
    half[:, 64:] = 0xC8C8 if c == 1 else (0x1234, 0xC8C8, 0x00FF)
    columns = lambda h, w: np.ascontiguousarray(np.broadcast_to(ref.make16(1, w, c, 'noise', seed=6), (h, w, c)[:2 if c == 1 else 3]))
    return {'flat': ref.make16(64, 64, c, 'flat'), 'half': half, 'w1': ref.make16(3000 // c, 1, c, 'flat'),
            'w1_noise': ref.make16(300, 1, c, 'noise'), 'w2': columns(900 // c, 2), 'w2_flat': ref.make16(900 // c, 2, c, 'flat')}


@pytest.mark.parametrize('c,order', [(1, 'grey'), (3, 'bgr')])
@pytest.mark.parametrize('name', sorted(_match_images(1)))
def test_png16_matches(dev, name, c, order):
    from ciaosr_amd import _lib, png_hip
    img = _match_images(c)[name]
    h, w = img.shape[:2]
    bpp, line = 2 * c, 1 + 2 * c * w
    t = _dev(img, order, dev)
    z_lz, z_lit = png_hip.encode_zlib(t, order, matches=True), png_hip.encode_zlib(t, order)
    png_lz, png_lit = png_hip.encode_png(t, order, matches=True), png_hip.encode_png(t, order)
    assert len(png_lz) <= len(png_lit) and len(z_lz) <= len(z_lit)                       # never larger than the literal file
    assert ref.ihdr(png_lz) == ref.ihdr(png_lit) == (w, h, 16, 0 if c == 1 else 2, 0, 0, 0)
    stream, _, adler = png_hip.filter_u8(t, order)
    raw = _host(stream).tobytes()
    assert raw == bytes(ref.filter_rows(img)[0]) == zlib.decompress(z_lz) == zlib.decompress(z_lit)
    offs = ref.band_offsets(h, line, getattr(_lib.load(), 'ciaosr_' + PREFIX[c] + 'rows_per_band')(w, 0))
    lz = png_hip.deflate_huff(stream, offs, matches=True, line=line, bpp=bpp)
    lit = png_hip.deflate_huff(stream, offs)
    partials = [(int(a), int(b), offs[i + 1] - offs[i]) for i, (a, b) in enumerate(adler.cpu().tolist())]
    assert png_hip.zlib_stream(lz, partials) == z_lz and png_hip.zlib_stream(lit, partials) == z_lit     # the one call is the stages
    in_match_mode = 0
    for i, (seg, plain) in enumerate(zip(lz, lit)):
        band = raw[offs[i]:offs[i + 1]]
        assert len(seg) <= len(plain), i
        if seg == plain:
            continue
        blocks, data, _ = ref.inflate_tokens(seg if i == len(lz) - 1 else seg + FINAL)
        assert data == band, i
        assert blocks[0]['type'] == 2 and blocks[0]['tokens'] == ref.parse(band, line, bpp), i
        in_match_mode += 1
    print(f'{name} bpp {bpp}: {in_match_mode} of {len(lz)} bands in match mode, {len(z_lz)} B against {len(z_lit)} B')
    if name != 'w1_noise':
        assert in_match_mode >= 1 and len(z_lz) < len(z_lit)


# -- renders ----------------------------------------------------------------------------------------------------------------------------
def _render_model(dev, cfg):
    from tests.test_grey_gpu import _model
    return _model(dev, cfg)


def _want16(fp, grey=False):
    """The definition applied to an fp32 render [1, 3, H, W]: q16 per sample, B G R; for a grey record L16 of the three."""
    assert fp.dtype == torch.float32 and fp.dim() == 4 and fp.shape[0] == 1
    bgr = ref.image_of(fp)
    return ref.grey16(bgr) if grey else bgr


@pytest.mark.parametrize('tiled', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_as_u16_renders_are_the_quantised_fp32_renders(dev, precision, tiled):
    from ciaosr_amd import hip_ops, scene
    from tests.test_grey_gpu import LR, TILED, _grey_input
    model = _render_model(dev, dict(precision=precision, **(TILED if tiled else {})))
    x1 = _grey_input(dev)
    g = torch.Generator().manual_seed(3)
    x3 = (x1.cpu().expand(-1, 3, -1, -1) * 0.8 + 0.2 * torch.rand(1, 3, *LR, generator=g)).clamp(0, 1).contiguous().to(dev)
    size = (round(LR[0] * 2.7), round(LR[1] * 2.7))
    vsize = (48, 44)
    m = scene.view_matrix((6.0, 8.0), 2.0, 30, vsize)
    inside = vr.members(*vr.lr_points(m, *vsize), (0, 0) + LR).reshape(vsize)
    assert (~inside).sum() > 300 and inside.sum() > 300
    for grey, enc in ((False, model.encode(x3, max_scale=2.7)), (True, model.encode_grey(x1, max_scale=2.7))):
        shape = lambda hw: tuple(hw) if grey else tuple(hw) + (3,)
        for window in (None, (5, 7, 30, 41)):
            got = model.render(enc, scale=2.7, window=window, as_u16=True)
            assert got.dtype == torch.uint16 and got.is_cuda and tuple(got.shape) == shape(size if window is None else window[2:])
            assert np.array_equal(_host(got), _want16(model.render(enc, scale=2.7, window=window), grey)), (grey, window)
        u8 = _host(model.render(enc, scale=2.7, as_u8=True))
        full = _host(model.render(enc, scale=2.7, as_u16=True))
        assert ((full >> 8) != u8).any()                    # the high byte is not the as_u8 byte
        for fill in (0.0, 0.25):
            view = model.render_view(enc, m, vsize, fill=fill, as_u16=True)
            assert tuple(view.shape) == shape(vsize)
            assert np.array_equal(_host(view), _want16(model.render_view(enc, m, vsize, fill=fill), grey)), (grey, fill)
            assert (_host(view)[~inside] == (0 if fill == 0.0 else 16384)).all()               # rint(0.25 * 65535) = 16384, L16 of a neutral too
        targets = lambda: [scene.Grid(scale=2.7), scene.View(m, vsize, 0.25), scene.Grid(scale=1.5, window=(2, 3, 20, 17))]
        many = model.render_many(enc, targets(), as_u16=True)
        fps = model.render_many(enc, targets())
        assert [tuple(o.shape) for o in many] == [shape(size), shape(vsize), shape((20, 17))]
        for o, fp in zip(many, fps):
            assert o.dtype == torch.uint16 and np.array_equal(_host(o), _want16(fp, grey))
        assert np.array_equal(_host(many[0]), full)
    # self-ensemble records, colour and grey: quantised once, after the mean
    for grey, ens in ((False, model.encode(x3, max_scale=2.7, self_ensemble=(0, 5))), (True, model.encode_grey(x1, max_scale=2.7, self_ensemble=(0, 5)))):
        for window in (None, (5, 7, 30, 41)):
            got = model.render(ens, scale=2.7, window=window, as_u16=True)
            assert got.dtype == torch.uint16 and np.array_equal(_host(got), _want16(model.render(ens, scale=2.7, window=window), grey))
        got = model.render_many(ens, [scene.Grid(scale=2.7), scene.Grid(scale=2)], as_u16=True)
        fps = model.render_many(ens, [scene.Grid(scale=2.7), scene.Grid(scale=2)])
        assert all(np.array_equal(_host(o), _want16(fp, grey)) for o, fp in zip(got, fps))
    # the refusals: before any launch
    enc = model.encode(x3, max_scale=2.7)
    rgba = model.encode_rgba(torch.cat([x3, x1], 1), max_scale=2.7)
    torch.cuda.synchronize()
    with hip_ops.profile():
        for record in (enc, rgba):
            both = dict(as_u8=True, as_u16=True) if record is enc else dict(as_u16=True)
            with pytest.raises(ValueError):
                model.render(record, scale=2.7, **both)
            with pytest.raises(ValueError):
                model.render_view(record, m, vsize, **both)
            with pytest.raises(ValueError):
                model.render_many(record, [scene.Grid(scale=2.7)], **both)
        with pytest.raises(ValueError):
            model.render(ens, scale=2.7, as_u8=True, as_u16=True)
    assert hip_ops.profile.results() == {}
    assert model.render(rgba, scale=2.7, as_u8=True).shape[2] == 4                             # the 8-bit RGBA render is as before


# -- tools/render.py --depth16 ----------------------------------------------------------------------------------------------------------
def test_render_cli_depth16(dev, tmp_path, capsys):
    from ciaosr_amd import build_model, hip_ops, scene
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread16_grey01, imread16_rgb01, imread_rgb01
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_grey_gpu import _grey_input
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, grey_png, rgb_png = str(tmp_path / 'w.pth'), str(tmp_path / 'g16.png'), str(tmp_path / 'rgb16.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    g = _grey_input('cpu', 24, 30)[0, 0].double()
    rng = np.random.RandomState(8)
    g16 = (np.clip(g.numpy(), 0, 1) * 65535).round().astype(np.uint16) ^ rng.randint(0, 256, (24, 30)).astype(np.uint16)   # busy low bytes
    rgb16 = np.stack([g16, 65535 - g16, np.roll(g16, 3, axis=1)], axis=-1)
    for path, img in ((grey_png, g16), (rgb_png, rgb16)):
        with open(path, 'wb') as f:
            f.write(ref.write_png16(img))
    view, size = (11.0, 14.5, 2.2, 20.0), (37, 45)
    flags = ['--scale', '2.5', '--view', *[str(v) for v in view], '--size', str(size[0]), str(size[1])]
    m = scene.view_matrix(view[:2], view[2], view[3], size)
    dev_model = model.to(dev).eval()
    dev_model.test_cfg['tile_any_scale'] = True             # what the tool sets
    # grey
    with hip_ops.profile():
        paths = render.main([config, ckpt, grey_png, *flags, '--depth16', '--grey', '--png-matches', '--out', str(tmp_path / 'a')])
    prof = hip_ops.profile.results()
    out = capsys.readouterr().out
    assert '16 bits per sample' in out and 'not a grey image' not in out
    assert [os.path.basename(p) for p in paths] == ['g16_x2p5.png', 'g16_view0.png']
    assert prof['png16_grey_filter_u16']['launches'] == 2 and prof['tensor2img_grey_u16']['launches'] == 2 and prof['deflate_lz_match']['launches'] == 2
    assert not {'tensor2img_u8', 'tensor2img_grey_u8', 'png_filter_u8', 'png_grey_filter_u8'} & set(prof)
    lq1, was_grey, bits = imread16_grey01(grey_png)
    assert was_grey and bits == 16 and np.array_equal((lq1[0].double() * 65535).round().numpy().astype(np.uint16), g16)
    enc = dev_model.encode_grey(lq1.unsqueeze(0).to(dev), max_scale=2.5)
    want = dev_model.render_many(enc, [scene.Grid(scale=2.5), scene.View(m, size)], as_u16=True)
    for path, img in zip(paths, want):
        data = open(path, 'rb').read()
        assert ref.ihdr(data)[2:4] == (16, 0) and np.array_equal(_pil16(data), _host(img))
    # colour, with a self-ensemble --scale output
    paths = render.main([config, ckpt, rgb_png, *flags, '--depth16', '--out', str(tmp_path / 'b')])
    assert 'rgb16.png: 16 bits per sample' in capsys.readouterr().out
    lq, bits = imread16_rgb01(rgb_png)
    assert bits == 16
    truncated = imread_rgb01(rgb_png)                       # Pillow's 8-bit reading of the same file
    assert not torch.equal(lq, truncated) and (lq - truncated).abs().max() < 1 / 255          # another fp32 tensor goes into the model
    enc = dev_model.encode(lq.unsqueeze(0).to(dev), max_scale=2.5)
    want = dev_model.render_many(enc, [scene.Grid(scale=2.5), scene.View(m, size)], as_u16=True)
    for path, img in zip(paths, want):
        data = open(path, 'rb').read()
        assert ref.ihdr(data)[2:4] == (16, 2) and np.array_equal(ref.decode_png16(data), _host(img)[:, :, ::-1])
    enc8 = dev_model.encode(truncated.unsqueeze(0).to(dev), max_scale=2.5)
    assert not np.array_equal(_host(dev_model.render(enc8, scale=2.5, as_u16=True)), _host(want[0]))
    # an 8-bit input is allowed, here with --self-ensemble: the file keeps the model's precision, quantised once after the mean
    from PIL import Image
    eight = str(tmp_path / 'eight.png')
    Image.fromarray((rgb16 >> 8).astype(np.uint8), 'RGB').save(eight)
    paths = render.main([config, ckpt, eight, '--scale', '2', '--depth16', '--self-ensemble', '--out', str(tmp_path / 'c')])
    assert 'eight.png: 8 bits per sample' in capsys.readouterr().out
    ens = dev_model.encode(imread_rgb01(eight).unsqueeze(0).to(dev), max_scale=2, self_ensemble=True)
    data = open(paths[0], 'rb').read()
    got = ref.decode_png16(data)
    assert ref.ihdr(data)[2:4] == (16, 2) and np.array_equal(got, _host(dev_model.render(ens, scale=2, as_u16=True))[:, :, ::-1])
    assert (got != 257 * _host(dev_model.render(ens, scale=2, as_u8=True))[:, :, ::-1].astype(np.uint16)).any()
