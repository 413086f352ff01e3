"""GPU tests of the device JPEG encoder (csrc/jpeg_u8.hip, ciaosr_amd/jpeg_hip.py): every file is held byte for byte to the numpy
restatement of the contract (tests/jpeg_ref.py) AND to Pillow's own file; the chunk seams, the tile lists, the launch and copy counts,
the capacity rule and the tools end to end.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as ref
from tests.test_jpeg_host import CONTENTS, SIZES, SUBSAMPLINGS, first_difference, make_image, pil_jpeg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = [10, 90, 100]
TILES_H, TILES_W = 200, 264


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _dev_img(rgb, order, dev):
    arr = rgb[:, :, ::-1] if order == 'bgr' else rgb
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def _want(rgb, quality, subsampling):
    """The file both judges agree on: the reference's, which must be Pillow's."""
    want = ref.encode(rgb, quality, subsampling)
    assert want == pil_jpeg(rgb, quality, subsampling)
    return want


@functools.lru_cache(maxsize=None)
def _tiles_image():
    return make_image(TILES_H, TILES_W, 'noise', seed=3)


@functools.lru_cache(maxsize=None)
def _tile_rects():
    from ciaosr_amd.pyramid import dzi_plan
    rects = [t[2:] for t in dzi_plan(TILES_H, TILES_W, 62, 1)[-1]['tiles']]                 # 4 x 5 tiles with their overlaps
    assert len(rects) == 20
    rects += [(0, 0, TILES_H, TILES_W), (199, 263, 1, 1), (0, 0, 1, 1), (57, 101, 1, 1),    # the whole image; single pixels
              (3, 5, 64, 64), (3, 5, 64, 64), (20, 30, 64, 64), (35, 37, 50, 90),           # the same rect twice; overlapping ones
              (1, 1, 17, 33), (7, 9, 9, 40), (11, 13, 40, 9), (101, 77, 24, 24),            # odd origins, the sizes of the host grid
              (0, 0, 16, 16), (5, 8, 15, 17), (150, 200, 50, 64), (199, 0, 1, 264),         # one MCU; one past; the corner; one row
              (0, 263, 200, 1), (64, 64, 72, 136), (9, 3, 33, 31), (120, 40, 8, 8), (33, 65, 47, 49)]
    assert len(rects) >= 40
    return rects


@functools.lru_cache(maxsize=None)
def _tile_wants(subsampling):
    img = _tiles_image()
    return [_want(img[y0:y0 + h, x0:x0 + w], 90, subsampling) for y0, x0, h, w in _tile_rects()]


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('content', CONTENTS)
def test_files_are_the_references_and_pillows(dev, content, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg
    for h, w in SIZES:
        rgb = make_image(h, w, content)
        imgs = {order: _dev_img(rgb, order, dev) for order in ('bgr', 'rgb')}
        for q in QUALITIES:
            want = _want(rgb, q, subsampling)
            for order, t in imgs.items():
                got = encode_jpeg(t, quality=q, subsampling=subsampling, order=order)
                assert got == want, (h, w, content, q, subsampling, order, first_difference(got, want), len(got), len(want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_a_pitched_crop_view(dev, subsampling):
    """A crop view whose origin is not aligned to 8 (nor its pitch to the crop): the view's own pixels and edges, nothing around them."""
    from ciaosr_amd.jpeg_hip import encode_jpeg
    big = make_image(90, 111, 'noise', seed=2)
    t = _dev_img(big, 'bgr', dev)
    for y0, x0, h, w in [(3, 5, 64, 75), (13, 21, 41, 37), (89, 110, 1, 1)]:
        view = t[y0:y0 + h, x0:x0 + w]
        assert not view.is_contiguous() or h == 1
        got = encode_jpeg(view, quality=90, subsampling=subsampling)
        assert got == _want(big[y0:y0 + h, x0:x0 + w], 90, subsampling), (y0, x0, h, w)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_chunk_seams(dev, subsampling):
    """72 x 136: 9 x 17 blocks; in 4:2:0 5 x 9 MCUs with a dummy row and a dummy column.  Noise at quality 100 puts 0xFF bytes into the
    stream, chunks of 1, 2 and 5 MCUs put seams everywhere: offsets, the words two chunks share and the DC predictors."""
    from ciaosr_amd.jpeg_hip import encode_jpeg, encode_scan
    rgb = make_image(72, 136, 'noise')
    t = _dev_img(rgb, 'bgr', dev)
    plain = ref.unstuffed(ref.scan_blocks(rgb, 100, subsampling))
    assert plain.count(b'\xff') >= 1                                                        # the stuffing path runs
    want = _want(rgb, 100, subsampling)
    for mcus in (1, 2, 5, 0):
        got = encode_jpeg(t, quality=100, subsampling=subsampling, mcus_per_chunk=mcus)
        assert got == want, (mcus, first_difference(got, want), len(got), len(want))
        assert encode_scan(t, quality=100, subsampling=subsampling, mcus_per_chunk=mcus) == ref.stuff(plain)
    # flat blocks of 6 (luma) and 4 (chroma) bits: five blocks share a word, and a one-MCU chunk ends inside its first byte's word
    flat = make_image(72, 136, 'flat')
    for mcus in (1, 5, 0):
        assert encode_jpeg(_dev_img(flat, 'bgr', dev), quality=90, subsampling=subsampling, mcus_per_chunk=mcus) == _want(flat, 90, subsampling)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_tiles_are_the_single_files(dev, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg, encode_jpeg_tiles
    rgb, rects = _tiles_image(), _tile_rects()
    t = _dev_img(rgb, 'bgr', dev)
    files = encode_jpeg_tiles(t, rects, quality=90, subsampling=subsampling)
    assert len(files) == len(rects)
    for k, ((y0, x0, h, w), got, want) in enumerate(zip(rects, files, _tile_wants(subsampling))):
        assert got == want, (k, (y0, x0, h, w), first_difference(got, want))
        assert got == encode_jpeg(t[y0:y0 + h, x0:x0 + w], quality=90, subsampling=subsampling), (k, (y0, x0, h, w))
    # in another order, with other neighbours in the list, and with small chunks
    pick = [7, 0, 39, 21, 20]
    again = encode_jpeg_tiles(t, [rects[k] for k in pick], quality=90, subsampling=subsampling, mcus_per_chunk=3)
    assert again == [files[k] for k in pick]


def test_a_wrong_edge_rule_would_show():
    """Host only.  A model that pads a crop from the image around it -- and not by repeating the crop's own last column and row -- codes
    other bytes: for the (5, 8, 15, 17) crop of the noise image at quality 90, 4:4:4, 482 of the 571 scan bytes differ (counted position
    by position; the two scans are 571 and 722 bytes long)."""
    rgb = _tiles_image()
    y0, x0, h, w = 5, 8, 15, 17
    right = ref.scan(rgb[y0:y0 + h, x0:x0 + w], 90, '444')
    wrong = ref.scan(rgb[y0:y0 + 16, x0:x0 + 24], 90, '444')                                # the same 2 x 3 blocks, the image's pixels
    differ = sum(a != b for a, b in zip(right, wrong)) + abs(len(right) - len(wrong))
    assert (len(right), len(wrong), differ) == WRONG_EDGE_FIGURES


# (bytes of the right scan, bytes of the wrong one, bytes that differ) of test_a_wrong_edge_rule_would_show
WRONG_EDGE_FIGURES = (571, 722, 482)


def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def test_launches_copies_and_repeatability(dev, monkeypatch):
    from ciaosr_amd import jpeg_hip
    rgb, rects = _tiles_image(), _tile_rects()
    t = _dev_img(rgb, 'bgr', dev)
    many = (rects * 2)[:60]
    first = jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420')                          # the workspace exists
    _, few_launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, rects[:3], subsampling='420'))
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
    second, many_launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420'))
    monkeypatch.undo()
    assert [c[0] for c in copies] == ['cpu', 'cpu'] and copies[0][1] == (61,), copies         # the offsets, then the scans
    assert few_launches == many_launches == dict(jpeg_coef=1, jpeg_count=1, jpeg_scan=1, jpeg_zero=1, jpeg_pack=1, jpeg_ffcount=1,
                                                 jpeg_scan2=1, jpeg_stuff=1)
    assert second == first
    copies.clear()
    for name in ('cpu', 'item', 'tolist', 'numpy', 'to', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    single, single_launches = _profile_of(lambda: jpeg_hip.encode_jpeg(t, subsampling='420'))
    monkeypatch.undo()
    assert [c[0] for c in copies] == ['item', 'cpu'] and single_launches == many_launches, copies   # the size, then the scan
    assert single == first[20]                                                                # rects[20] is the whole image
    torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(0xA5)                          # other bytes in freed memory
    assert jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420') == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev) == side
        assert jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420') == first
        assert jpeg_hip.encode_jpeg(t, subsampling='420') == single
    torch.cuda.current_stream(dev).wait_stream(side)


def test_capacity_is_never_exceeded(dev):
    from ciaosr_amd import _lib, hip_ops, jpeg_hip
    from ciaosr_amd._lib import CiaoSRHipError
    lib = _lib.load()
    rgb = make_image(72, 136, 'noise')
    t = _dev_img(rgb, 'bgr', dev)
    rects = [(0, 0, 72, 136), (3, 5, 20, 20)]
    host_rects = (C.c_int * 8)(*[v for r in rects for v in r])
    cap = lib.ciaosr_jpeg_tiles_capacity_bytes(host_rects, 2, 0)
    assert cap == 416 * 3 * (9 * 17 + 3 * 3)
    # a declared capacity below the need: refused before any launch, and nothing at all is written
    out = torch.full((cap + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    with hip_ops.profile():
        for declared in (cap - 1, cap // 2, 0):
            with pytest.raises(CiaoSRHipError, match='workspace'):
                jpeg_hip.encode_scans_device(t, rects, quality=100, out=out, capacity=declared)
    assert hip_ops.profile.results() == {}
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # the exact capacity: the scans are written, and not a byte at or beyond their end
    got, offs = jpeg_hip.encode_scans_device(t, rects, quality=100, out=out, capacity=cap)
    offs = offs.cpu().tolist()
    assert got is out and offs[0] == 0 and offs[2] <= cap
    raw = out.cpu().numpy()
    assert bool((raw[offs[2]:] == 0xA5).all())
    wants = [ref.scan(rgb[y0:y0 + h, x0:x0 + w], 100, '444') for y0, x0, h, w in rects]
    assert [raw[offs[k]:offs[k + 1]].tobytes() for k in range(2)] == wants
    # a short workspace is refused the same way
    nbytes = lib.ciaosr_jpeg_tiles_workspace_bytes(host_rects, 2, 0, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    o2 = torch.empty(3, dtype=torch.int64, device=dev)

    def run(ws_bytes=nbytes, quality=90, sub=0, mcus=0, arr=host_rects, n=2, h=72, w=136):
        return lib.ciaosr_jpeg_encode_tiles_u8(hip_ops.ptr(t), C.c_size_t(t.stride(0)), h, w, 1, arr, n, quality, sub, mcus, hip_ops.ptr(out),
                                               C.c_size_t(cap), hip_ops.ptr(o2), hip_ops.ptr(ws), C.c_size_t(ws_bytes), hip_ops.stream_ptr(dev))

    bad_arg, short = -1, -4
    with hip_ops.profile():
        assert run(ws_bytes=nbytes - 1) == short
        assert run(quality=0) == bad_arg and run(quality=101) == bad_arg and run(sub=1) == bad_arg and run(sub=3) == bad_arg
        assert run(mcus=-1) == bad_arg and run(n=0) == bad_arg and run(h=71) == bad_arg and run(w=135) == bad_arg
        for r in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (70, 0, 3, 5), (0, 130, 5, 7)):
            assert run(arr=(C.c_int * 8)(*r, 0, 0, 1, 1)) == bad_arg, r
    assert hip_ops.profile.results() == {}
    assert run() == 0
    torch.cuda.synchronize()


def test_refused_arguments_launch_nothing(dev):
    from ciaosr_amd import hip_ops, jpeg_hip
    from ciaosr_amd._lib import CiaoSRHipError
    rgb = make_image(37, 53, 'noise')
    t = _dev_img(rgb, 'bgr', dev)
    with hip_ops.profile():
        for bad in ([(0, 0, 38, 5)], [(0, 50, 5, 4)], [(0, 0, 0, 5)], [(3, 3, 5, 0)], [(-1, 0, 5, 5)], [(0, 0, 5, 5), (36, 52, 2, 1)], []):
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg_tiles(t, bad)
        for kw in (dict(quality=0), dict(quality=101), dict(quality=75.5), dict(subsampling='422'), dict(subsampling=2), dict(order='gbr'),
                   dict(mcus_per_chunk=-2)):
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg(t, **kw)
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg_tiles(t, [(0, 0, 5, 5)], **kw)
        with pytest.raises(CiaoSRHipError):
            jpeg_hip.encode_jpeg(rgb)
        with pytest.raises(CiaoSRHipError):
            jpeg_hip.encode_jpeg_tiles(torch.from_numpy(rgb), [(0, 0, 5, 5)])
    assert hip_ops.profile.results() == {}


def _rgb(u8_bgr):
    return np.ascontiguousarray(u8_bgr.cpu().numpy()[:, :, ::-1])


def _check_jpeg_tree(out_dir, name, levels_rgb, tile_size, overlap, quality, subsampling):
    """Every tile of the written tree opens in Pillow with the planned size and is byte for byte Pillow's file of the level's crop."""
    import xml.etree.ElementTree as ET
    from PIL import Image
    from ciaosr_amd.pyramid import dzi_plan
    root = ET.parse(os.path.join(out_dir, name + '.dzi')).getroot()
    assert root.get('Format') == 'jpg' and (int(root.get('TileSize')), int(root.get('Overlap'))) == (tile_size, overlap)
    top = levels_rgb[-1]
    plan = dzi_plan(top.shape[0], top.shape[1], tile_size, overlap)
    assert sorted(os.listdir(os.path.join(out_dir, name + '_files')), key=int) == [str(lv['level']) for lv in plan]
    files = 1
    for lv, img in zip(plan, levels_rgb):
        folder = os.path.join(out_dir, name + '_files', str(lv['level']))
        assert sorted(os.listdir(folder)) == sorted(f'{t[0]}_{t[1]}.jpg' for t in lv['tiles'])
        for col, row, y0, x0, h, w in lv['tiles']:
            path = os.path.join(folder, f'{col}_{row}.jpg')
            im = Image.open(path)
            assert im.format == 'JPEG' and im.mode == 'RGB' and im.size == (w, h)
            im.load()
            assert open(path, 'rb').read() == pil_jpeg(img[y0:y0 + h, x0:x0 + w], quality, subsampling), (lv['level'], col, row)
            files += 1
    return files


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_write_dzi_jpg(dev, tmp_path, subsampling):
    from tests.test_png_gpu import _restorer
    from tests.test_pyramid_gpu import _read_tree
    from ciaosr_amd.pyramid import write_dzi
    model = _restorer({}).to(dev)
    lq = torch.rand(1, 3, 12, 10, generator=torch.Generator().manual_seed(5)).to(dev)
    res = write_dzi(model, model.encode(lq, max_scale=4), str(tmp_path / 'jpg'), 'img', scale=4, tile_size=16, overlap=1, fmt='jpg', quality=85,
                    subsampling=subsampling)
    levels = [_rgb(im) for im in model.render_pyramid(model.encode(lq, max_scale=4), scale=4)]
    assert _check_jpeg_tree(str(tmp_path / 'jpg'), 'img', levels, 16, 1, 85, subsampling) == res['files'] == 1 + 5 + 4 + 9
    # the PNG pyramid of the same call without the new arguments: the same tree of .png files, the same pixels
    png = write_dzi(model, model.encode(lq, max_scale=4), str(tmp_path / 'png'), 'img', scale=4, tile_size=16, overlap=1)
    top, png_levels, files, nbytes = _read_tree(str(tmp_path / 'png'), 'img', 16, 1)
    assert (png['files'], png['bytes']) == (files, nbytes) and files == res['files']
    assert all(np.array_equal(a, b) for a, b in zip(png_levels, levels))


def test_render_cli_jpeg(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_u8
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_png_host import make_image as png_image
    from tests.test_pyramid_gpu import _read_tree
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray(png_image(12, 10, 'smooth')).save(png)
    argv = [config, ckpt, png, '--scale', '2', '--view', '5.0', '4.5', '2.2', '20', '--size', '21', '19', '--dzi', '2', '--dzi-tile', '16']
    plain = render.main(argv + ['--gpu-png', '--out', str(tmp_path / 'png')])
    jpg = render.main(argv + ['--jpeg', '90', '--jpeg-subsampling', '420', '--out', str(tmp_path / 'jpg')])
    assert [os.path.basename(p) for p in plain] == ['img_x2.png', 'img_view0.png']
    assert [os.path.basename(p) for p in jpg] == ['img_x2.jpg', 'img_view0.jpg']
    assert sorted(os.listdir(tmp_path / 'jpg')) == ['img.dzi', 'img_files', 'img_view0.jpg', 'img_x2.jpg']
    for a, b in zip(plain, jpg):                                                            # the PNG files hold the pixels that were coded
        rgb = imread_u8(a)
        assert open(b, 'rb').read() == pil_jpeg(rgb, 90, '420'), b
        assert Image.open(b).size == (rgb.shape[1], rgb.shape[0])
    top, levels, files, _ = _read_tree(str(tmp_path / 'png'), 'img', 16, 1)                 # without the flag: Format="png", .png tiles
    assert top == (24, 20)
    assert _check_jpeg_tree(str(tmp_path / 'jpg'), 'img', levels, 16, 1, 90, '420') == files
