"""Pyramidal tiled TIFF on the GPU (ciaosr_amd/tiff_hip.py, csrc/tiff_tiles.h): every tile's zlib stream inflated (zlib checks the
Adler-32) and held to the predicted bytes of tests/tiff_ref.py; the match coder; whole files opened by Pillow and the reference
reader; the box halving; render_pyramid(as_u16=True), pyramid.write_tiff and tools/render.py --tiff end to end; launches and copies.
The device is never held against itself.  Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import functools
import io
import os
import zlib

import numpy as np
import pytest
import torch

from tests import tiff_ref as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = [(1, 1), (16, 16), (17, 33), (37, 53), (6, 259)]      # 6 x 259: a row wider than one pass of the workgroup
TILES = [16, 32, 64]                                            # 64: tiles that are mostly padding
ROWS = [0, 5, 16]                                               # several bands per tile and a short last one
PILLOW_MODES = {'rgb8': 'RGB', 'grey8': 'L', 'grey16': 'I;16', 'rgba8': 'RGBA'}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _host(t):
    return t.cpu().numpy()


def _swapped(img):
    """R G B (A) <-> B G R (A) of a numpy image; a grey one is returned as it is"""
    if img.ndim == 2:
        return img
    return np.ascontiguousarray(img[:, :, [2, 1, 0] + ([3] if img.shape[2] == 4 else [])])


def _orders(kind):
    """[(the `order` argument, whether the device image holds B G R)]"""
    if kind.startswith('grey'):
        return [('bgr', False), ('grey', False)]
    return [('bgra', True), ('rgba', False)] if kind == 'rgba8' else [('bgr', True), ('rgb', False)]


def _dev_image(img, bgr, dev):
    return torch.from_numpy(_swapped(img) if bgr else np.array(img, order='C')).to(dev)  # (a copy: the shared reference is read-only)


@functools.lru_cache(maxsize=None)
def _reference(kind, h, w, tile):
    """(the image in stream order, the predicted bytes of every tile): computed once, shared, never written to"""
    img = ref.make_image(h, w, kind, seed=3)
    img.setflags(write=False)
    return img, tuple(ref.tiles_bytes(img, tile))


def _inflate_all(streams):
    out = []
    for z in streams:
        d = zlib.decompressobj()
        raw = d.decompress(z)
        assert d.eof and d.unused_data == b'' and z[:2] == b'\x78\x01'
        out.append(raw)
    return out


# -- tiles against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('kind', ref.KINDS)
def test_tiles_are_the_reference_bytes(dev, kind, which):
    from ciaosr_amd import tiff_hip
    order, bgr = _orders(kind)[which]
    for h, w in IMAGES:
        for tile in TILES:
            img, want = _reference(kind, h, w, tile)
            t = _dev_image(img, bgr, dev)
            for rows in ROWS:
                got = tiff_hip.encode_tiff_tiles(t, tile, order, rows)
                assert len(got) == len(want) == -(-h // tile) * -(-w // tile)
                raw = _inflate_all(got)
                for k, (a, b) in enumerate(zip(raw, want)):
                    assert a == b, (kind, order, h, w, tile, rows, k)
    # bitwise repeatable, also over other bytes in freed memory
    img, _ = _reference(kind, 37, 53, 16)
    t = _dev_image(img, bgr, dev)
    first = tiff_hip.encode_tiff_tiles(t, 16, order, 5)
    torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(0xA5)
    assert tiff_hip.encode_tiff_tiles(t, 16, order, 5) == first
    out, offs = tiff_hip.encode_tiff_tiles_device(t, 16, order, 5)
    o = offs.cpu().tolist()
    assert o[0] == 0 and all(b > a for a, b in zip(o, o[1:])) and [bytes(_host(out[o[k]:o[k + 1]])) for k in range(len(first))] == first


@pytest.mark.parametrize('kind', ref.KINDS)
def test_pitched_crop_never_reads_past_the_crop(dev, kind):
    """A crop of a larger image whose surroundings hold other samples: a source index that is not clamped to the crop's last row and
    column shows as other bytes.  16-bit kinds start at an odd pixel (2-byte alignment only)."""
    from ciaosr_amd import tiff_hip
    h, w, y0, x0 = 37, 53, 3, 5
    order, bgr = _orders(kind)[0]
    for tile in (16, 64):
        img, want = _reference(kind, h, w, tile)
        c, dtype = ref.kind_shape(kind)
        big = np.full((h + 7, w + 12) + ((c,) if c > 1 else ()), np.iinfo(dtype).max // 3 * 2 + 1, dtype=dtype)
        big[y0:y0 + h, x0:x0 + w] = _swapped(img) if bgr else img
        view = torch.from_numpy(big).to(dev)[y0:y0 + h, x0:x0 + w]
        assert not view.is_contiguous()
        for rows in (0, 5):
            assert tuple(_inflate_all(tiff_hip.encode_tiff_tiles(view, tile, order, rows))) == want, (kind, tile, rows)
    # the crop that ends with the buffer's last row and column: padding must repeat them, there is nothing behind
    img, want = _reference(kind, 17, 33, 32)
    arr = _swapped(img) if bgr else img
    big = np.zeros((20, 40) + arr.shape[2:], dtype=arr.dtype)
    big[3:, 7:] = arr
    view = torch.from_numpy(big).to(dev)[3:, 7:]
    assert tuple(_inflate_all(tiff_hip.encode_tiff_tiles(view, 32, order))) == want


@pytest.mark.parametrize('kind', ['grey16', 'rgb16'])
def test_predictor_borrows_across_the_bytes_of_a_sample(dev, kind):
    """Neighbouring samples 0 and 65535: a predictor that worked on bytes would write other bytes (tests/test_tiff_host.py shows the
    reference itself differs from the byte-wise rule)."""
    from ciaosr_amd import tiff_hip
    c = ref.kind_shape(kind)[0]
    y, x, k = np.meshgrid(np.arange(17), np.arange(33), np.arange(c), indexing='ij')
    img = np.where((x + y + k) % 2 == 0, 0, 65535).astype(np.uint16)
    img[5:9] = np.where((x[5:9] % 3) == 0, 0x00FF, 0x0100)                       # 0x0100 - 0x00FF = 1: the low byte borrows
    img = img[:, :, 0].copy() if c == 1 else img
    bytewise = np.frombuffer(ref.padded_tile(img, 0, 0, 16).astype('<u2').tobytes(), dtype=np.uint8).reshape(16, -1).astype(int)
    d = bytewise.copy()
    d[:, 2 * c:] = (bytewise[:, 2 * c:] - bytewise[:, :-2 * c]) % 256
    want = ref.tiles_bytes(img, 16)
    assert bytes(d.astype(np.uint8).reshape(-1)) != want[0]
    order, bgr = _orders(kind)[0]
    assert _inflate_all(tiff_hip.encode_tiff_tiles(_dev_image(img, bgr, dev), 16, order, 5)) == want


# -- the match coder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ref.KINDS)
def test_matches_decode_to_the_same_bytes_and_are_never_longer(dev, kind):
    from ciaosr_amd import tiff_hip
    order, bgr = _orders(kind)[0]
    shorter = 0
    for h, w in IMAGES:
        for tile in TILES:
            img, want = _reference(kind, h, w, tile)
            t = _dev_image(img, bgr, dev)
            for rows in (0, 5):
                lit = tiff_hip.encode_tiff_tiles(t, tile, order, rows)
                lz = tiff_hip.encode_tiff_tiles(t, tile, order, rows, matches=True)
                assert tuple(_inflate_all(lz)) == want, (kind, h, w, tile, rows)
                assert all(len(a) <= len(b) for a, b in zip(lz, lit)), (kind, h, w, tile, rows)
                shorter += sum(len(a) < len(b) for a, b in zip(lz, lit))
    assert shorter > 0
    # 17 x 17 at T = 64: 47 of 64 rows and columns are padding -- zeros after the predictor and repeats of the row above.  The
    # literal coder cannot go below one bit per byte of it; matches can.
    img = ref.make_image(17, 17, kind, seed=9)
    t = _dev_image(img, bgr, dev)
    (lit,), (lz,) = tiff_hip.encode_tiff_tiles(t, 64, order), tiff_hip.encode_tiff_tiles(t, 64, order, matches=True)
    assert _inflate_all([lz]) == _inflate_all([lit]) == ref.tiles_bytes(img, 64)
    padding = 64 * 64 * img.dtype.itemsize * (1 if img.ndim == 2 else img.shape[2]) - 17 * 17 * img.dtype.itemsize * (1 if img.ndim == 2 else img.shape[2])
    print(f'{kind}: 17 x 17 at T = 64: literal {len(lit)} B, matches {len(lz)} B, {padding} B of padding')
    assert len(lit) >= padding // 8 and len(lz) < len(lit)
    assert tiff_hip.encode_tiff_tiles(t, 64, order, matches=True) == [lz]         # repeatable


# -- whole files -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('matches', [False, True])
@pytest.mark.parametrize('kind', ref.KINDS)
def test_files_are_read_by_pillow_and_the_reference_reader(dev, tmp_path, kind, matches):
    from PIL import Image
    from ciaosr_amd import tiff_hip
    order, bgr = _orders(kind)[0]
    for (h, w), tile in (((77, 131), 32), ((17, 33), 16), ((16, 16), 16)):
        levels = ref.pyramid_of(ref.make_image(h, w, kind, seed=5), tile)
        assert [lv.shape[:2] for lv in levels] == tiff_hip.tiff_level_sizes(h, w, tile)
        on_dev = [_dev_image(lv, bgr, dev) for lv in levels]
        data = tiff_hip.encode_tiff(on_dev, tile, order, matches=matches)
        path = str(tmp_path / f'{kind}_{h}.tif')
        res = tiff_hip.imwrite_gpu_tiff(on_dev, path, tile, order, matches=matches)
        assert open(path, 'rb').read() == data and res == dict(levels=len(levels), bytes=len(data), tiles=sum(
            -(-lv.shape[0] // tile) * -(-lv.shape[1] // tile) for lv in levels))
        ifds = ref.read_ifds(data)
        assert [sorted(tags) for _, tags in ifds] == [[t for t in tiff_hip.TAGS if t != 338 or kind == 'rgba8']] * len(levels)
        assert all(off % 2 == 0 and all(o % 2 == 0 for o in tags[324][1]) for off, tags in ifds)
        got = ref.read_tiff(data)
        assert len(got) == len(levels)
        for a, b in zip(got, levels):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        pages = ref.pillow_pages(data)
        assert len(pages) == len(levels)
        if kind in PILLOW_MODES:
            assert Image.open(io.BytesIO(data)).mode == PILLOW_MODES[kind]
            for a, b in zip(pages, levels):
                assert a.dtype == b.dtype and np.array_equal(a, b)
    # a single image is a one-level file, whatever its size
    img = ref.make_image(37, 53, kind, seed=6)
    one = tiff_hip.encode_tiff(_dev_image(img, bgr, dev), 16, order, matches=matches)
    (page,) = ref.read_tiff(one)
    assert np.array_equal(page, img)


# -- the box halving ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
def test_halve_box_u16_is_the_numpy_rule(dev, c):
    from ciaosr_amd import tiff_hip
    rng = np.random.RandomState(11 + c)
    for h, w in ((1, 1), (1, 7), (7, 1), (1, 2), (2, 1), (2, 2), (5, 8), (8, 5), (33, 17), (6, 259), (3, 600)):
        a = rng.randint(0, 65536, (h, w, c)).astype(np.uint16)
        a[rng.rand(h, w, c) < 0.3] = 65535                                       # sums that need more than 16 bits
        a = a[:, :, 0].copy() if c == 1 else a
        got = tiff_hip.halve_box_u16(torch.from_numpy(a).to(dev))
        assert got.dtype == torch.uint16 and np.array_equal(_host(got), ref.halve_box(a)), (h, w)
    big = rng.randint(0, 65536, (40, 50, c)).astype(np.uint16)
    big = big[:, :, 0].copy() if c == 1 else big
    view = torch.from_numpy(big).to(dev)[3:36, 5:22]                              # pitched, odd pixel origin
    assert np.array_equal(_host(tiff_hip.halve_box_u16(view)), ref.halve_box(big[3:36, 5:22]))


# -- render_pyramid(as_u16=True) -----------------------------------------------------------------------------------------------------------
def _tiny(test_cfg, dev):
    from tests.test_png_gpu import _restorer
    return _restorer(test_cfg).to(dev)


def _lq(c, h, w, dev, seed=5):
    return torch.rand(1, c, h, w, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.mark.parametrize('tiled', [False, True])
def test_render_pyramid_as_u16(dev, tiled):
    from PIL import Image
    from ciaosr_amd.pyramid import level_sizes
    from ciaosr_amd import hip_ops
    model = _tiny(dict(tile=12, tile_overlap=4, tile_any_scale=True) if tiled else {}, dev)
    h, w = 20, 18
    sizes = level_sizes(40, 36)
    first = min(k for k, s in enumerate(sizes) if s[0] >= h and s[1] >= w)
    assert sizes[first:] == [(20, 18), (40, 36)] and first == 5
    for grey in (False, True):
        lq = _lq(1 if grey else 3, h, w, dev)
        encode = model.encode_grey if grey else model.encode
        levels = model.render_pyramid(encode(lq, max_scale=2), scale=2, as_u16=True)
        assert [tuple(im.shape[:2]) for im in levels] == sizes and all(im.dtype == torch.uint16 and im.is_cuda for im in levels)
        assert all(im.dim() == (2 if grey else 3) for im in levels)
        fresh = encode(lq, max_scale=2)
        for k in range(first, len(sizes)):
            assert torch.equal(levels[k], model.render(fresh, size=sizes[k], as_u16=True)), (grey, k)
        for k in range(first - 1, -1, -1):                                       # every lower level: the halving of the one ABOVE it
            assert np.array_equal(_host(levels[k]), ref.halve_box(_host(levels[k + 1]))), (grey, k)
        # without the keyword: what render_pyramid is documented to give -- the as_u8 renders and Pillow's BICUBIC of the smallest
        plain = model.render_pyramid(encode(lq, max_scale=2), scale=2)
        assert all(im.dtype == torch.uint8 for im in plain) and [tuple(im.shape[:2]) for im in plain] == sizes
        for k in range(first, len(sizes)):
            assert torch.equal(plain[k], model.render(fresh, size=sizes[k], as_u8=True)), (grey, k)
        base = Image.fromarray(_host(plain[first]))
        for k in range(first):
            assert np.array_equal(_host(plain[k]), np.asarray(base.resize((sizes[k][1], sizes[k][0]), Image.BICUBIC))), (grey, k)
    rgba = model.encode_rgba(_lq(4, h, w, dev), max_scale=2)
    torch.cuda.synchronize()
    with hip_ops.profile():
        with pytest.raises(ValueError, match='alpha'):
            model.render_pyramid(rgba, scale=2, as_u16=True)
    assert hip_ops.profile.results() == {}


# -- write_tiff and tools/render.py --tiff -------------------------------------------------------------------------------------------------
def _pages_in_device_order(data, kind):
    """The file's levels as the device holds them (B G R [A] or grey), the top first; RGB 16 through the reference reader"""
    pages = ref.read_tiff(data)
    if kind in PILLOW_MODES:
        for a, b in zip(ref.pillow_pages(data), pages):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    return [_swapped(p) for p in pages]


def test_write_tiff_pages_are_render_pyramids_levels(dev, tmp_path):
    from ciaosr_amd.pyramid import write_tiff
    model = _tiny({}, dev)
    h, w, tile = 36, 28, 16
    sizes = [(72, 56), (36, 28), (18, 14), (9, 7)]
    cases = (('rgb8', 3, 8, False), ('rgb16', 3, 16, True), ('grey16', 1, 16, False), ('grey8', 1, 8, True), ('rgba8', 4, 8, True))
    for kind, c, depth, matches in cases:
        lq = _lq(c, h, w, dev)
        encode = {1: model.encode_grey, 3: model.encode, 4: model.encode_rgba}[c]
        path = str(tmp_path / f'{kind}.tif')
        res = write_tiff(model, encode(lq, max_scale=2), path, scale=2, tile=tile, depth=depth, matches=matches)
        data = open(path, 'rb').read()
        assert res['levels'] == sizes and res['model_levels'] == [0, 1] and res['bytes'] == len(data) and res['tiles'] == 20 + 6 + 2 + 1
        assert {'render_s', 'encode_s', 'write_s'} <= set(res)
        want = model.render_pyramid(encode(lq, max_scale=2), scale=2, **(dict(as_u16=True) if depth == 16 else {}))[::-1][:4]
        got = _pages_in_device_order(data, kind)
        assert len(got) == 4
        for a, b in zip(got, want):
            assert a.dtype == _host(b).dtype and np.array_equal(a, _host(b)), kind


def test_render_cli_tiff(dev, tmp_path, capsys):
    from PIL import Image
    from ciaosr_amd import build_model
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread16_grey01, imread16_rgb01, imread_rgb01
    from ciaosr_amd.init_utils import seeded_init_
    from tests import png16_ref
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt = str(tmp_path / 'w.pth')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    rgb16 = ref.make_image(20, 18, 'rgb16', seed=2)
    grey16 = ref.make_image(20, 18, 'grey16', seed=2)
    files = dict(rgb8=str(tmp_path / 'c8.png'), rgb16=str(tmp_path / 'c16.png'), grey16=str(tmp_path / 'g16.png'))
    Image.fromarray((rgb16 >> 8).astype(np.uint8), 'RGB').save(files['rgb8'])
    for kind, img in (('rgb16', rgb16), ('grey16', grey16)):
        with open(files[kind], 'wb') as f:
            f.write(png16_ref.write_png16(img))
    dev_model = model.to(dev).eval()
    dev_model.test_cfg['tile_any_scale'] = True             # what the tool sets
    sizes = [(40, 36), (20, 18), (10, 9)]
    for kind, flags in (('rgb8', []), ('rgb16', ['--depth16', '--png-matches']), ('grey16', ['--depth16', '--grey'])):
        out = str(tmp_path / kind)
        paths = render.main([config, ckpt, files[kind], '--scale', '2', '--tiff', '--tiff-tile', '16', *flags, '--out', out])
        name = os.path.splitext(os.path.basename(files[kind]))[0]
        assert [os.path.basename(p) for p in paths] == [f'{name}_x2.tif'] and sorted(os.listdir(out)) == [f'{name}_x2.tif']
        assert '3 levels (2 from the model)' in capsys.readouterr().out
        if kind == 'rgb8':
            enc = dev_model.encode(imread_rgb01(files[kind]).unsqueeze(0).to(dev), max_scale=2)
        elif kind == 'rgb16':
            enc = dev_model.encode(imread16_rgb01(files[kind])[0].unsqueeze(0).to(dev), max_scale=2)
        else:
            enc = dev_model.encode_grey(imread16_grey01(files[kind])[0].unsqueeze(0).to(dev), max_scale=2)
        want = dev_model.render_pyramid(enc, scale=2, **(dict(as_u16=True) if kind != 'rgb8' else {}))[::-1][:3]
        got = _pages_in_device_order(open(paths[0], 'rb').read(), kind)
        assert [p.shape[:2] for p in got] == sizes
        for a, b in zip(got, want):
            assert a.dtype == _host(b).dtype and np.array_equal(a, _host(b)), kind


# -- launches and copies -----------------------------------------------------------------------------------------------------------------
def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def test_launches_and_copies_do_not_grow_with_the_tiles(dev, monkeypatch):
    from ciaosr_amd import tiff_hip
    literal = dict(tiff_predict_tiles=1, deflate_plan=1, png_tiles_scan=1, deflate_pack=1)
    match = dict(literal, deflate_lz_match=1, deflate_lz_plan=1, deflate_lz_pack=1)
    img = ref.make_image(77, 131, 'rgb8', seed=1)
    levels = [_dev_image(lv, True, dev) for lv in ref.pyramid_of(img, 16)]
    assert len(levels) == 5
    tiff_hip.encode_tiff(levels, 16)                                             # workspaces grown
    for t in (levels[0], levels[-1]):                                            # 5 x 9 tiles, and one
        assert _profile_of(lambda: tiff_hip.encode_tiff_tiles(t, 16, 'bgr', 5))[1] == literal
        assert _profile_of(lambda: tiff_hip.encode_tiff_tiles(t, 16, 'bgr', 5, matches=True))[1] == match
    copies = []

    def counted(name):
        inner = getattr(torch.Tensor, name)

        def fn(self, *a, **k):
            if self.is_cuda and (name != 'to' or 'cpu' in [str(v) for v in a] + [str(v) for v in k.values()]):
                copies.append((name, tuple(self.shape)))
            return inner(self, *a, **k)
        return fn

    for name in ('cpu', 'item', 'tolist', 'numpy', 'to', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    _, launches = _profile_of(lambda: tiff_hip.encode_tiff(levels, 16, matches=True))
    monkeypatch.undo()
    assert launches == {k: 5 * v for k, v in match.items()}                      # per level, whatever its number of tiles
    tiles = [-(-lv.shape[0] // 16) * -(-lv.shape[1] // 16) for lv in levels]
    assert [c[0] for c in copies] == ['cpu', 'cpu'] * 5, copies                  # per level: the offsets, then the streams
    assert [c[1] for c in copies[0::2]] == [(n + 1,) for n in tiles]
