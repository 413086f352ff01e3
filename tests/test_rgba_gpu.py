"""RGBA on the GPU: the four-byte-per-pixel PNG filter and files against the numpy restatement (tests/rgba_ref.py) and Pillow's decoder,
the three-channel coder against the bytes of the commit before (tests/golden/png_rgb_parent.npz), the quantise-and-pack kernels, the
renders of `CiaoSR.encode_rgba` against the two-item batch they are defined by, the pyramid and tools/render.py --alpha.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import rgba_ref as ref
from tests import view_reference as vr
from tests.test_rgba_host import CASES, make_rgba, pil_rgba

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 65), (70, 300)]
ORDERS = ['bgra', 'rgba']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _dev_img(rgba, order, dev):
    """The device image whose pixels are `rgba` (uint8 [H, W, 4] R G B A) in byte order `order`."""
    arr = rgba if order == 'rgba' else rgba[:, :, [2, 1, 0, 3]]
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def _crop_case(h, w, dev, order):
    """A pitched crop view of a larger noise image, and its pixels."""
    big = make_rgba(h + 5, w + 9, 'noise', seed=3)
    t = _dev_img(big, order, dev)[2:2 + h, 3:3 + w]
    assert h == 1 or t.stride(0) == 4 * big.shape[1] > 4 * w           # (a single row has no pitch to speak of)
    return t, big[2:2 + h, 3:3 + w]


_refs = {}


def _reference(key, rgba):
    """(stream, {rows: (hist, adler)}) of the restatement, computed once per image."""
    if key not in _refs:
        _refs[key] = (ref.filter_rows(rgba)[0], {})
    return _refs[key]


def _check_filter(t, rgba, key, order, rows):
    from ciaosr_amd import png_hip
    h, w = rgba.shape[:2]
    stream, tables = _reference(key, rgba)
    r = ref.rows_per_band(w, rows)
    if r not in tables:
        tables[r] = ref.band_tables(stream, h, w, r)
    got, hist, adler = png_hip.filter_u8(t, order, rows)
    assert np.array_equal(got.cpu().numpy(), stream), (key, order, rows)
    assert np.array_equal(hist.cpu().numpy()[:, :257].astype(np.int64), tables[r][0][:, :257]), (key, order, rows)
    assert np.array_equal(adler.cpu().numpy().astype(np.int64), tables[r][1]), (key, order, rows)


# -- the filter -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
def test_filter_is_the_restatement(dev, h, w):
    for case in CASES:
        rgba = make_rgba(h, w, case)
        for order in ORDERS:
            t = _dev_img(rgba, order, dev)
            for rows in (0, 1, 3):
                _check_filter(t, rgba, (h, w, case), order, rows)
    for order in ORDERS:
        t, rgba = _crop_case(h, w, dev, order)
        for rows in (0, 1, 3):
            _check_filter(t, rgba, (h, w, 'crop'), order, rows)


def test_the_tie_goes_to_the_lower_filter(dev):
    """The device's choice on the rows where Sub and Paeth leave the same bytes (tests/test_rgba_host.py asserts that they do)."""
    from ciaosr_amd import png_hip
    got = png_hip.filter_u8(_dev_img(make_rgba(5, 3, 'tie'), 'bgra', dev), 'bgra')[0].cpu().numpy().reshape(5, 13)
    assert got[:, 0].tolist() == [0, 1, 0, 1, 0]


# -- the files --------------------------------------------------------------------------------------------------------------------------
def _check_file(png, rgba):
    assert np.array_equal(pil_rgba(png), rgba)
    assert np.array_equal(ref.decode_rgba_png(png), rgba)


@pytest.mark.parametrize('h,w', SIZES)
def test_files_decode_to_the_pixels(dev, h, w):
    from ciaosr_amd import png_hip
    for k, case in enumerate(CASES):
        rgba = make_rgba(h, w, case)
        order = ORDERS[k % 2]
        _check_file(png_hip.encode_png(_dev_img(rgba, order, dev), order), rgba)
        _check_file(png_hip.encode_png(_dev_img(rgba, ORDERS[1 - k % 2], dev), ORDERS[1 - k % 2], 3), rgba)
    t, rgba = _crop_case(h, w, dev, 'bgra')
    _check_file(png_hip.encode_png(t, 'bgra'), rgba)


@pytest.mark.parametrize('case', ['noise', 'alpha0', 'ramp'])
def test_many_bands(dev, case):
    from ciaosr_amd import png_hip
    rgba = make_rgba(300, 257, case)
    png = png_hip.encode_png(_dev_img(rgba, 'bgra', dev), 'bgra', rows_per_band=2)
    _check_file(png, rgba)
    # the stream under the container is the restatement's: 150 bands of two rows
    raw = zlib.decompress(b''.join(d for t, d in ref.chunks(png) if t == b'IDAT'))
    assert raw == bytes(ref.filter_rows(rgba)[0])


def test_imwrite_gpu_rgba(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import png_hip
    rgba = make_rgba(33, 65, 'noise')
    path = str(tmp_path / 'sub' / 'x.png')
    png_hip.imwrite_gpu(_dev_img(rgba, 'bgra', dev), path, order='bgra')
    im = Image.open(path)
    assert im.mode == 'RGBA' and np.array_equal(np.asarray(im), rgba)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('rows', [0, 3])
def test_tiles_are_bitwise_the_single_encoder(dev, order, rows):
    from ciaosr_amd import hip_ops, png_hip
    rgba = make_rgba(70, 90, 'noise', seed=2)
    rgba[20:50, 10:60] = make_rgba(30, 50, 'alpha255')
    t = _dev_img(rgba, order, dev)
    rects = [(0, 0, 70, 90), (69, 89, 1, 1), (40, 50, 30, 40), (0, 0, 1, 1), (10, 5, 33, 65), (12, 7, 33, 65), (3, 88, 60, 2)]
    with hip_ops.profile():
        files = png_hip.encode_png_tiles(t, rects, order, rows)
    prof = hip_ops.profile.results()
    assert prof['png_rgba_filter_tiles_u8']['launches'] == 1 and prof['deflate_pack']['launches'] == 1
    assert prof['deflate_plan']['launches'] == 1 and prof['png_tiles_scan']['launches'] == 1 and 'png_filter_tiles_u8' not in prof
    assert len(files) == len(rects)
    for (y0, x0, h, w), png in zip(rects, files):
        assert png == png_hip.encode_png(t[y0:y0 + h, x0:x0 + w], order, rows), (y0, x0, h, w)
        _check_file(png, rgba[y0:y0 + h, x0:x0 + w])


def test_the_library_refuses_a_misaligned_source(dev):
    """Four bytes per pixel are read as 32-bit words: a view that starts off a word, or whose pitch is no multiple of 4, is refused by
    the tensor-level check and by the library itself, before any launch."""
    import ctypes as C
    from ciaosr_amd import _lib, hip_ops, png_hip
    from ciaosr_amd._lib import CiaoSRHipError
    buf = torch.zeros(4 * 7 * 5 + 64, dtype=torch.uint8, device=dev)
    off = torch.as_strided(buf, (5, 7, 4), (28, 4, 1), 1)
    odd = torch.as_strided(buf, (5, 7, 4), (30, 4, 1), 0)
    for bad in (off, odd):
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(bad, 'bgra')
    lib = _lib.load()
    out = torch.zeros(4096, dtype=torch.uint8, device=dev)
    hist = torch.zeros(5 * 260, dtype=torch.int32, device=dev)
    for ptr, pitch in ((buf.data_ptr() + 1, 28), (buf.data_ptr(), 30)):
        rc = lib.ciaosr_png_rgba_filter_u8(C.c_void_p(ptr), C.c_size_t(pitch), 5, 7, 1, 1, hip_ops.ptr(out), hip_ops.ptr(hist), hip_ops.ptr(hist),
                                           hip_ops.stream_ptr(dev))
        assert rc != 0 and b'argument' in lib.ciaosr_error_string(rc).lower()
    # the three-byte call takes any pitch and any start, as before
    rgb = torch.as_strided(buf, (5, 7, 3), (23, 3, 1), 1)
    assert len(png_hip.encode_png(rgb, 'bgr')) > 0


# -- three channels: the bytes of the commit before -------------------------------------------------------------------------------------
def test_three_channel_files_are_the_parents(dev):
    from ciaosr_amd import png_hip
    from tools.make_png_parent_golden import RECTS, SMALL, WIDE, image
    gold = np.load(os.path.join(REPO, 'tests', 'golden', 'png_rgb_parent.npz'))
    assert gold['rects'].tolist() == [list(r) for r in RECTS]
    small, wide = torch.from_numpy(image(*SMALL)).to(dev), torch.from_numpy(image(*WIDE)).to(dev)
    for order in ('bgr', 'rgb'):
        assert png_hip.encode_png(small, order) == gold[f'small_{order}'].tobytes(), order
        assert png_hip.encode_png(small, order, 3) == gold[f'small_{order}_rows3'].tobytes(), order
        files = png_hip.encode_png_tiles(wide, RECTS, order, 7)
        for k, data in enumerate(files):
            assert data == gold[f'wide_{order}_tile{k}'].tobytes(), (order, k)


# -- the pack kernels -------------------------------------------------------------------------------------------------------------------
def _two_items(h, w, seed):
    """[2, 3, h, w] fp32 with values below 0, above 1, every (k + 0.5) / 255 and NaN among uniform noise."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(2, 3, h, w, generator=g) * 1.5 - 0.25
    flat = t.view(-1)
    n = flat.numel()
    if n >= 600:
        halves = (torch.arange(255, dtype=torch.float32) + 0.5) / 255
        flat[0:255] = halves
        flat[n // 2:n // 2 + 255] = halves
        flat[300] = float('nan')
        flat[n - 7] = float('nan')
        flat[301], flat[302], flat[303] = -3.0, 7.0, float('inf')
    return t


@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (37, 53)])
def test_tensor2img_bgra_is_tensor2img_of_each_item_plus_the_alpha(dev, h, w):
    import ctypes as C
    from ciaosr_amd import _lib, hip_ops, metrics, metrics_hip
    t = _two_items(h, w, seed=h * 100 + w).to(dev)
    if h == 1:
        t[1] = float('nan')                                            # NaN -> 0 in every byte, so A = 0
    got = metrics_hip.tensor2img_bgra_u8(t)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 4) and got.is_cuda
    colour, grey = metrics_hip.tensor2img_u8(t[0]).cpu().numpy(), metrics_hip.tensor2img_u8(t[1]).cpu().numpy()
    want = ref.pack_bgra(colour, grey)
    assert np.array_equal(got.cpu().numpy(), want)
    if h > 1:                                                          # the host's tensor2img agrees where no NaN is (it has no NaN rule)
        clean = torch.nan_to_num(t.cpu(), nan=0.0, posinf=1.0)
        assert np.array_equal(colour.reshape(h, w, 3), metrics.tensor2img(clean[0]).reshape(h, w, 3))
    # a grey alpha image gives its own bytes
    t2 = t.clone()
    t2[1] = t[1, :1].expand(3, -1, -1)
    grey = metrics_hip.tensor2img_u8(t2[1]).cpu().numpy()
    assert np.array_equal(metrics_hip.tensor2img_bgra_u8(t2).cpu().numpy()[:, :, 3], grey[:, :, 0])
    # pitched destinations through the ABI: a word-aligned pitch, and one that is not (written in single bytes)
    for pitch, start in ((4 * w + 8, 0), (4 * w + 3, 0), (4 * w, 1)):
        buf = torch.full((h * pitch + 8,), 0xAB, dtype=torch.uint8, device=dev)
        _lib.call('ciaosr_tensor2img_bgra_u8', hip_ops.ptr(t[0]), hip_ops.ptr(t[1]), h, w, C.c_void_p(buf.data_ptr() + start), C.c_size_t(pitch),
                  hip_ops.stream_ptr(dev))
        rows = buf.cpu().numpy()[start:start + h * pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :4 * w].reshape(h, w, 4), want), (pitch, start)
        assert (rows[:, 4 * w:] == 0xAB).all() and (buf.cpu().numpy()[start + h * pitch:] == 0xAB).all()      # nothing beyond a row


@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (37, 53)])
def test_pack_bgra(dev, h, w):
    import ctypes as C
    from ciaosr_amd import _lib, hip_ops, metrics_hip
    rng = np.random.RandomState(h * 7 + w)
    big_a, big_b = rng.randint(0, 256, (h + 2, w + 3, 3), dtype=np.uint8), rng.randint(0, 256, (h + 4, w + 1, 3), dtype=np.uint8)
    a, b = torch.from_numpy(big_a).to(dev)[1:1 + h, 2:2 + w], torch.from_numpy(big_b).to(dev)[3:3 + h, 0:w]      # pitched sources
    want = ref.pack_bgra(big_a[1:1 + h, 2:2 + w], big_b[3:3 + h, 0:w])
    got = metrics_hip.pack_bgra_u8(a, b)
    assert tuple(got.shape) == (h, w, 4) and np.array_equal(got.cpu().numpy(), want)
    grey = a[:, :, 1:2].expand(-1, -1, 3).contiguous()
    assert torch.equal(metrics_hip.pack_bgra_u8(a, grey)[:, :, 3], a[:, :, 1])
    for pitch, start in ((4 * w + 4, 0), (4 * w + 1, 0), (4 * w, 3)):
        buf = torch.full((h * pitch + 8,), 0xCD, dtype=torch.uint8, device=dev)
        _lib.call('ciaosr_pack_bgra_u8', hip_ops.ptr(a), C.c_size_t(a.stride(0)), hip_ops.ptr(b), C.c_size_t(b.stride(0)), h, w,
                  C.c_void_p(buf.data_ptr() + start), C.c_size_t(pitch), hip_ops.stream_ptr(dev))
        rows = buf.cpu().numpy()[start:start + h * pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :4 * w].reshape(h, w, 4), want), (pitch, start)
        assert (rows[:, 4 * w:] == 0xCD).all() and (buf.cpu().numpy()[start + h * pitch:] == 0xCD).all()


# -- renders ----------------------------------------------------------------------------------------------------------------------------
LR = (24, 40)


def _model(dev, cfg):
    from tests.test_view_gpu import _model as view_model               # the tiny seeded RDN restorer of the scene and view tests
    model = view_model('rdn', dev, 3)
    model.test_cfg = dict(cfg)
    return model


def _rgba_input(dev, h=LR[0], w=LR[1]):
    """[1, 4, h, w]: seeded colour under a soft-edged alpha disc (0 outside, 1 inside, a ramp three pixels wide between)."""
    from tests.test_view_gpu import _lq
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing='ij')
    d = ((y - h / 2) ** 2 + (x - w / 2) ** 2).sqrt()
    alpha = ((0.4 * h + 1.5 - d) / 3.0).clamp(0, 1)
    assert (alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()
    return torch.cat([_lq(h, w, 'cpu'), alpha[None, None]], 1).to(dev)


def _batch2(x4):
    return torch.cat([x4[:, :3], x4[:, 3:4].expand(-1, 3, -1, -1)], 0)


def _pack(two):
    """The definition: tensor2img_u8 of each item, alpha by the restatement's formula, on the host."""
    from ciaosr_amd import metrics_hip
    return ref.pack_bgra(metrics_hip.tensor2img_u8(two[0]).cpu().numpy(), metrics_hip.tensor2img_u8(two[1]).cpu().numpy())


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_render_is_the_packed_two_item_render(dev, precision):
    from ciaosr_amd import scene
    model = _model(dev, dict(precision=precision))
    x4 = _rgba_input(dev)
    with pytest.raises(ValueError):
        model.encode_rgba(x4[:, :3])
    with pytest.raises(ValueError):
        model.encode_rgba(x4[0])
    for window in (None, (5, 7, 30, 41)):
        enc = model.encode_rgba(x4, max_scale=2.5)
        assert enc.alpha and tuple(enc.x.shape) == (2, 3) + LR
        got = model.render(enc, scale=2.5, window=window, as_u8=True)
        size = (60, 100) if window is None else window[2:]
        assert got.dtype == torch.uint8 and tuple(got.shape) == size + (4,) and got.is_cuda
        two = model.render(model.encode(_batch2(x4), max_scale=2.5), scale=2.5, window=window)
        assert tuple(two.shape) == (2, 3) + size
        assert np.array_equal(got.cpu().numpy(), _pack(two)), window
        alone = model.render(model.encode(x4[:, :3], max_scale=2.5), scale=2.5, window=window, as_u8=True)
        assert torch.equal(got[:, :, :3], alone), window
        assert torch.equal(model.render(enc, scale=2.5, window=window), two)      # as_u8=False: the fp32 batch (colour, alpha as grey)
    assert got[:, :, 3].min() != got[:, :, 3].max()                               # an alpha plane, not a constant
    plain = model.encode(x4[:, :3])
    assert not plain.alpha and tuple(model.render(plain, scale=2, as_u8=True).shape) == (48, 80, 3)


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_tiled_render_many(dev, precision):
    from ciaosr_amd import scene
    model = _model(dev, dict(precision=precision, tile=16, tile_overlap=4, tile_any_scale=True))
    x4 = _rgba_input(dev)
    size = (37, 45)
    fill = (0.75, 0.125, 0.5)
    targets = lambda: [scene.Grid(scale=2.5), scene.View(scene.view_matrix((5.0, 31.5), 2.2, 20, size), size, fill)]
    got = model.render_many(model.encode_rgba(x4, max_scale=2.5), targets(), as_u8=True)
    two = model.render_many(model.encode(_batch2(x4), max_scale=2.5), targets())
    alone = model.render_many(model.encode(x4[:, :3], max_scale=2.5), targets(), as_u8=True)
    assert [tuple(g.shape) for g in got] == [(60, 100, 4), size + (4,)]
    # the grid: both items are as in the plain batch
    assert np.array_equal(got[0].cpu().numpy(), _pack(two[0]))
    assert torch.equal(got[0][:, :, :3], alone[0]) and torch.equal(got[1][:, :, :3], alone[1])
    # the view: the colour item as in the plain batch; the alpha item as in the plain batch where the view is inside the image (there
    # the plain batch holds the caller's fill in item 1, the RGBA render 0)
    m = targets()[1].matrix
    y, x = vr.lr_points(m, *size)
    inside = vr.members(y, x, (0, 0) + LR).reshape(size)
    assert (~inside).sum() == 427 and inside.sum() == 1238
    want = _pack(two[1])
    view = got[1].cpu().numpy()
    assert np.array_equal(view[inside], want[inside]) and np.array_equal(view[:, :, :3], want[:, :, :3])
    assert (view[~inside][:, 3] == 0).all()
    # the single calls give the same images
    enc = model.encode_rgba(x4, max_scale=2.5)
    assert torch.equal(model.render(enc, scale=2.5, as_u8=True), got[0])
    assert torch.equal(model.render_view(enc, m, size, fill=fill, as_u8=True), got[1])


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_view_outside_is_transparent(dev, precision):
    from ciaosr_amd import scene
    model = _model(dev, dict(precision=precision))
    x4 = _rgba_input(dev)
    size = (48, 48)
    fill = (0.75, 0.125, 0.5)
    m = scene.view_matrix((6.0, 8.0), 2.0, 30, size)
    y, x = vr.lr_points(m, *size)
    inside = vr.members(y, x, (0, 0) + LR).reshape(size)
    assert (~inside).sum() == 789 and inside.sum() == 1515
    enc = model.encode_rgba(x4, max_scale=2.0)
    got = model.render_view(enc, m, size, fill=fill, as_u8=True).cpu().numpy()
    assert got.shape == size + (4,)
    fill_bgr = np.rint(np.float32(fill[::-1]) * np.float32(255)).astype(np.uint8)
    assert fill_bgr.tolist() == [128, 32, 191]
    assert (got[~inside][:, 3] == 0).all() and (got[~inside][:, :3] == fill_bgr).all()
    two = model.render_view(model.encode(_batch2(x4), max_scale=2.0), m, size, fill=fill)
    assert np.array_equal(got[inside], _pack(two)[inside])
    fp = model.render_view(enc, m, size, fill=fill)                    # fp32: item 0 the caller's fill, item 1 zeros outside
    out = torch.from_numpy(~inside).to(dev)
    assert torch.equal(fp[1][:, out], torch.zeros(3, int(out.sum()), device=dev))
    assert torch.equal(fp[0][:, out], torch.tensor(fill, device=dev)[:, None].expand(3, int(out.sum())))


# -- the pyramid ------------------------------------------------------------------------------------------------------------------------
def test_pyramid(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import scene
    from ciaosr_amd.pyramid import dzi_plan, level_sizes, write_dzi
    model = _model(dev, dict())
    x4 = _rgba_input(dev, 12, 10)
    sizes = [(1, 1), (2, 2), (3, 3), (6, 5), (12, 10), (24, 20)]
    assert level_sizes(24, 20) == sizes
    imgs = model.render_pyramid(model.encode_rgba(x4, max_scale=2), scale=2)
    assert [tuple(im.shape) for im in imgs] == [s + (4,) for s in sizes] and all(im.dtype == torch.uint8 and im.is_cuda for im in imgs)
    many = model.render_many(model.encode(_batch2(x4), max_scale=2), [scene.Grid(size=s) for s in sizes[4:]])
    for k, two in zip((4, 5), many):
        assert np.array_equal(imgs[k].cpu().numpy(), _pack(two)), k
    base = imgs[4].cpu().numpy()                                       # the smallest model level, 12 x 10
    rgb, a = Image.fromarray(np.ascontiguousarray(base[:, :, 2::-1])), Image.fromarray(np.ascontiguousarray(base[:, :, 3]))
    for k in range(4):
        wh = (sizes[k][1], sizes[k][0])
        got = imgs[k].cpu().numpy()
        assert np.array_equal(got[:, :, 2::-1], np.asarray(rgb.resize(wh, Image.BICUBIC))), k
        assert np.array_equal(got[:, :, 3], np.asarray(a.resize(wh, Image.BICUBIC))), k
    # the written tree: RGBA tiles that decode to the crops of their levels, under the manifest of the RGB run
    res = write_dzi(model, model.encode_rgba(x4, max_scale=2), str(tmp_path / 'rgba'), 'img', scale=2, tile_size=16, overlap=2)
    plain = write_dzi(model, model.encode(x4[:, :3], max_scale=2), str(tmp_path / 'rgb'), 'img', scale=2, tile_size=16, overlap=2)
    assert res['levels'] == plain['levels'] == sizes and res['model_levels'] == plain['model_levels'] == [4, 5]
    assert res['files'] == plain['files'] == 1 + 5 + 4
    assert open(str(tmp_path / 'rgba' / 'img.dzi'), 'rb').read() == open(str(tmp_path / 'rgb' / 'img.dzi'), 'rb').read()
    for lv, im in zip(dzi_plan(24, 20, 16, 2), imgs):
        level = im.cpu().numpy()[:, :, [2, 1, 0, 3]]
        for col, row, y0, x0, h, w in lv['tiles']:
            png = open(str(tmp_path / 'rgba' / 'img_files' / str(lv['level']) / f'{col}_{row}.png'), 'rb').read()
            _check_file(png, level[y0:y0 + h, x0:x0 + w])
    with pytest.raises(ValueError, match='alpha'):
        write_dzi(model, model.encode_rgba(x4, max_scale=2), str(tmp_path / 'jpg'), 'img', scale=2, fmt='jpg')
    assert not (tmp_path / 'jpg').exists()


# -- tools/render.py --alpha ------------------------------------------------------------------------------------------------------------
def test_render_cli_alpha(dev, tmp_path, capsys):
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops, scene
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_rgba01
    from ciaosr_amd.init_utils import seeded_init_
    from ciaosr_amd.pyramid import dzi_plan
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png, opaque = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png'), str(tmp_path / 'opaque.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    x4 = _rgba_input('cpu', 24, 30)
    rgba = (x4[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
    Image.fromarray(rgba, 'RGBA').save(png)
    full = rgba.copy()
    full[:, :, 3] = 255
    Image.fromarray(full, 'RGBA').save(opaque)
    view, size = (11.0, 14.5, 2.2, 20.0), (37, 45)
    flags = ['--scale', '2.5', '--view', *[str(v) for v in view], '--size', str(size[0]), str(size[1]), '--dzi', '2', '--dzi-tile', '32']
    with hip_ops.profile():
        paths = render.main([config, ckpt, png, *flags, '--alpha', '--out', str(tmp_path / 'a')])
    prof = hip_ops.profile.results()
    assert [os.path.basename(p) for p in paths] == ['img_x2p5.png', 'img_view0.png']
    assert prof['png_rgba_filter_u8']['launches'] == 2 and prof['tensor2img_bgra_u8']['launches'] >= 2 and 'png_filter_u8' not in prof
    # the files decode to the device images of the same encode
    model = model.to(dev).eval()
    model.test_cfg['tile_any_scale'] = True                            # what the tool sets
    lq4, is_opaque = imread_rgba01(png)
    assert not is_opaque
    enc = model.encode_rgba(lq4.unsqueeze(0).to(dev), max_scale=2.5)           # the tool's: the largest --scale
    m = scene.view_matrix(view[:2], view[2], view[3], size)
    want = model.render_many(enc, [scene.Grid(scale=2.5), scene.View(m, size)], as_u8=True)
    for path, img in zip(paths, want):
        _check_file(open(path, 'rb').read(), img.cpu().numpy()[:, :, [2, 1, 0, 3]])
    levels = model.render_pyramid(enc, scale=2)
    for lv, im in zip(dzi_plan(48, 60, 32, 1), levels):
        level = im.cpu().numpy()[:, :, [2, 1, 0, 3]]
        for col, row, y0, x0, h, w in lv['tiles']:
            data = open(str(tmp_path / 'a' / 'img_files' / str(lv['level']) / f'{col}_{row}.png'), 'rb').read()
            assert np.array_equal(pil_rgba(data), level[y0:y0 + h, x0:x0 + w]), (lv['level'], col, row)
    # an opaque input: one line, and the files of the run without the flag, byte for byte
    capsys.readouterr()
    with_flag = render.main([config, ckpt, opaque, *flags, '--alpha', '--out', str(tmp_path / 'b')])
    assert 'no transparent pixel' in capsys.readouterr().out
    without = render.main([config, ckpt, opaque, *flags, '--out', str(tmp_path / 'c')])
    seen = 0
    for root, _, names in os.walk(str(tmp_path / 'c')):
        for n in names:
            other = os.path.join(str(tmp_path / 'b'), os.path.relpath(os.path.join(root, n), str(tmp_path / 'c')))
            assert open(os.path.join(root, n), 'rb').read() == open(other, 'rb').read(), n
            seen += 1
    assert seen == 2 + 1 + sum(len(lv['tiles']) for lv in dzi_plan(48, 60, 32, 1))
    assert sum(len(f) for _, _, f in os.walk(str(tmp_path / 'b'))) == seen
    assert [os.path.basename(p) for p in with_flag] == [os.path.basename(p) for p in without]
