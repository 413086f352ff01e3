"""GPU tests of progressive JPEG files (csrc/jpeg_prog_u8.hip, ciaosr_amd/jpeg_hip.py `progressive=True`): every file is held byte for
byte to the plain Python restatement of the contract (tests/jpeg_prog_ref.py) AND to Pillow's own `progressive=True` file; the scans
and tables one by one, EOB runs cut by their correction bits and by the 32767-block limit across chunk seams, the raster
re-addressing of 4:2:0 luma, the tile lists, the launch and copy counts, the capacity rule and the tools end to end.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_opt_ref as opt
from tests import jpeg_prog_ref as prog
from tests import jpeg_ref as ref
from tests.test_jpeg_gpu import QUALITIES, REPO, _dev_img, _rgb, _tile_rects, _tiles_image
from tests.test_jpeg_host import CONTENTS, SIZES, SUBSAMPLINGS, first_difference, make_image
from tests.test_jpeg_opt_gpu import OPT_LAUNCHES, PLAIN_LAUNCHES
from tests.test_jpeg_prog_host import CORR_SIZES, FLAT_SIDE, capacity_need, corr_image, corr_want, flat_want, parse, pil_jpeg_prog

pytestmark = pytest.mark.gpu
PROG_LAUNCHES = dict(jpeg_coef=1, prog_summary=1, prog_runs=1, prog_hist=1, prog_tables=1, prog_count=1, jpeg_scan=1, jpeg_zero=1,
                     prog_pack=1, prog_corr=1, jpeg_ffcount=1, jpeg_scan2=1, jpeg_stuff=1)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _want(rgb, quality, subsampling):
    """The file both judges agree on: the reference's, which must be Pillow's."""
    want = prog.encode(rgb, quality, subsampling)
    assert want == pil_jpeg_prog(rgb, quality, subsampling)
    return want


def _explain(got, want):
    """Where two files part: the first differing offset, the lengths, and the first scan whose data differs."""
    out = [first_difference(got, want), len(got), len(want)]
    try:
        a, b = parse(got)[1], parse(want)[1]
        out.append(('scan', next((s + 1 for s in range(min(len(a), len(b))) if a[s] != b[s]), None)))
    except (AssertionError, IndexError):
        out.append('unparsable')
    return out


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
                got = encode_jpeg(t, quality=q, subsampling=subsampling, order=order, progressive=True)
                assert got == want, (h, w, content, q, subsampling, order, _explain(got, want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_scans_and_tables_one_by_one(dev, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg, encode_scan
    for (h, w), content, q in (((100, 75), 'noise', 100), ((64, 64), 'ramp_noise', 90), ((17, 33), 'saturated', 10)):
        rgb = make_image(h, w, content)
        t = _dev_img(rgb, 'bgr', dev)
        scans, tables, _ = prog.code(rgb, q, subsampling)
        got_scans, got_tables = encode_scan(t, quality=q, subsampling=subsampling, progressive=True)
        assert len(got_scans) == 10 and len(got_tables) == 10
        for k in range(10):
            assert (list(got_tables[k][0]), list(got_tables[k][1])) == (list(tables[k][0]), list(tables[k][1])), ('table', k, h, w, q)
        for s in range(10):
            assert got_scans[s] == scans[s], ('scan', s + 1, h, w, q, first_difference(got_scans[s], scans[s]), len(got_scans[s]), len(scans[s]))
        # optimize does not matter
        assert encode_jpeg(t, quality=q, subsampling=subsampling, optimize=True, progressive=True) == \
            encode_jpeg(t, quality=q, subsampling=subsampling, progressive=True) == _want(rgb, q, subsampling)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('size', CORR_SIZES)
def test_correction_bits_cut_runs_across_chunk_seams(dev, size, subsampling):
    """Runs that libjpeg cuts above 937 buffered correction bits (the reference counts them), their bits packed by lanes of other
    chunks than the flush's."""
    from ciaosr_amd.jpeg_hip import encode_jpeg
    want, _, _, stats = corr_want(*size, subsampling)
    assert stats['corr_flushes'] >= 1, stats
    t = _dev_img(corr_image(*size), 'bgr', dev)
    for mcus in (0, 1, 2, 3, 7):
        got = encode_jpeg(t, quality=100, subsampling=subsampling, mcus_per_chunk=mcus, progressive=True)
        assert got == want, (size, mcus, _explain(got, want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_runs_of_32767_blocks(dev, subsampling):
    """A flat image of 33 124 blocks per component: every AC scan is one run, cut once at 0x7FFF, across every chunk seam."""
    from ciaosr_amd.jpeg_hip import encode_jpeg
    want, stats = flat_want(subsampling)
    assert stats['longest_run'] == 32767 and stats['full_flushes'] >= 2, stats
    t = torch.full((FLAT_SIDE, FLAT_SIDE, 3), 77, dtype=torch.uint8, device=dev)
    for mcus in (0, 5):
        got = encode_jpeg(t, quality=90, subsampling=subsampling, mcus_per_chunk=mcus, progressive=True)
        assert got == want, (mcus, _explain(got, want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_flat_small_images_and_dummy_blocks(dev, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg
    for h, w in ((17, 33), (1, 1)):                          # every AC scan has a single kind of symbol
        rgb = make_image(h, w, 'flat')
        for mcus in (0, 1):
            got = encode_jpeg(_dev_img(rgb, 'bgr', dev), quality=90, subsampling=subsampling, mcus_per_chunk=mcus, progressive=True)
            assert got == _want(rgb, 90, subsampling), (h, w, mcus)
    # 4:2:0: dummy luma blocks on the right, on the bottom and on both -- the AC scans skip them and walk the real ones in raster order
    for h, w in ((9, 40), (40, 9), (17, 33), (72, 136)):
        rgb = make_image(h, w, 'noise', seed=4)
        want = _want(rgb, 90, subsampling)
        for mcus in (0, 1, 3):
            got = encode_jpeg(_dev_img(rgb, 'bgr', dev), quality=90, subsampling=subsampling, mcus_per_chunk=mcus, progressive=True)
            assert got == want, (h, w, mcus, _explain(got, want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_a_pitched_crop_view(dev, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg
    big = make_image(90, 111, 'noise', seed=2)
    t = _dev_img(big, 'bgr', dev)
    for y0, x0, h, w in [(3, 5, 64, 75), (13, 21, 41, 37), (89, 110, 1, 1)]:
        view = t[y0:y0 + h, x0:x0 + w]
        assert not view.is_contiguous() or h == 1
        got = encode_jpeg(view, quality=90, subsampling=subsampling, progressive=True)
        assert got == _want(big[y0:y0 + h, x0:x0 + w], 90, subsampling), (y0, x0, h, w)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_tiles_are_the_single_files(dev, subsampling):
    from ciaosr_amd.jpeg_hip import encode_jpeg, encode_jpeg_tiles
    rgb, rects = _tiles_image(), _tile_rects()
    t = _dev_img(rgb, 'bgr', dev)
    files = encode_jpeg_tiles(t, rects, quality=90, subsampling=subsampling, progressive=True)
    assert len(files) == len(rects)
    for k, ((y0, x0, h, w), got, want) in enumerate(zip(rects, files, _tile_wants(subsampling))):
        assert got == want, (k, (y0, x0, h, w), _explain(got, want))
        assert got == encode_jpeg(t[y0:y0 + h, x0:x0 + w], quality=90, subsampling=subsampling, progressive=True), (k, (y0, x0, h, w))
    # in another order, with other neighbours in the list, and with small chunks
    pick = [7, 0, 39, 21, 20]
    again = encode_jpeg_tiles(t, [rects[k] for k in pick], quality=90, subsampling=subsampling, mcus_per_chunk=3, progressive=True)
    assert again == [files[k] for k in pick]


def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def test_launches_copies_and_repeatability(dev, monkeypatch):
    from ciaosr_amd import hip_ops, jpeg_hip
    rgb, rects = _tiles_image(), _tile_rects()
    t = _dev_img(rgb, 'bgr', dev)
    many = (rects * 2)[:60]
    first = jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420', progressive=True)          # the workspace exists
    assert first[:41] == _tile_wants('420')[:41] and first[41:] == first[:19]
    _, few_launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, rects[:3], subsampling='420', progressive=True))
    copies = []

    def counted(name):
        inner = getattr(torch.Tensor, name)

        def fn(self, *a, **k):
            if self.is_cuda and (name != 'to' or 'cpu' in [str(v) for v in a] + [str(v) for v in k.values()]):
                copies.append((name, tuple(self.shape)))
            return inner(self, *a, **k)
        return fn

    def count_copies():
        copies.clear()
        for name in ('cpu', 'item', 'tolist', 'numpy', 'to', '__array__'):
            monkeypatch.setattr(torch.Tensor, name, counted(name))

    count_copies()
    second, many_launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420', progressive=True))
    monkeypatch.undo()
    # the offsets with the tables (601 offsets and 60 x 10 records of 272 bytes in one int64 buffer), then the scans
    assert [c[0] for c in copies] == ['cpu', 'cpu'] and copies[0][1] == (10 * 60 + 1 + 10 * 60 * 272 // 8,), copies
    assert few_launches == many_launches == PROG_LAUNCHES
    assert second == first
    count_copies()
    single, single_launches = _profile_of(lambda: jpeg_hip.encode_jpeg(t, subsampling='420', progressive=True))
    monkeypatch.undo()
    assert [c[0] for c in copies] == ['cpu', 'cpu'] and copies[0][1] == (11 + 10 * 272 // 8,), copies
    assert single_launches == PROG_LAUNCHES and single == first[20]                           # rects[20] is the whole image
    torch.empty(1 << 22, dtype=torch.uint8, device=dev).fill_(0xA5)                          # other bytes in freed memory
    hip_ops.workspace(1, dev, slot='jpeg').view(torch.uint8).fill_(0xA5)                     # and in the workspace: stale marks and counts
    assert jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420', progressive=True) == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev) == side
        assert jpeg_hip.encode_jpeg_tiles(t, many, subsampling='420', progressive=True) == first
        assert jpeg_hip.encode_jpeg(t, subsampling='420', progressive=True) == single
    torch.cuda.current_stream(dev).wait_stream(side)
    # without the flag, in the same process: the launches and the files of the other two kinds
    opt_file, opt_launches = _profile_of(lambda: jpeg_hip.encode_jpeg(t, subsampling='420', optimize=True))
    assert opt_launches == OPT_LAUNCHES and opt_file == opt.encode(rgb, 90, '420')
    plain, plain_launches = _profile_of(lambda: jpeg_hip.encode_jpeg(t, subsampling='420'))
    assert plain_launches == PLAIN_LAUNCHES and plain == ref.encode(rgb, 90, '420')
    tiles, tiles_launches = _profile_of(lambda: jpeg_hip.encode_jpeg_tiles(t, rects[:3], subsampling='420'))
    assert tiles_launches == PLAIN_LAUNCHES
    assert tiles == [ref.encode(rgb[y0:y0 + h, x0:x0 + w], 90, '420') for y0, x0, h, w in rects[:3]]


def test_capacity_is_never_exceeded(dev):
    from ciaosr_amd import _lib, hip_ops, jpeg_hip
    from ciaosr_amd._lib import CiaoSRHipError
    lib = _lib.load()
    rgb = make_image(72, 136, 'noise')
    t = _dev_img(rgb, 'bgr', dev)
    rects = [(0, 0, 72, 136), (3, 5, 20, 20)]
    host_rects = (C.c_int * 8)(*[v for r in rects for v in r])
    cap = lib.ciaosr_jpeg_prog_tiles_capacity_bytes(host_rects, 2, 0)
    assert cap == capacity_need(72, 136, '444') + capacity_need(20, 20, '444')
    opt_cap = lib.ciaosr_jpeg_opt_tiles_capacity_bytes(host_rects, 2, 0)
    assert 0 < opt_cap < cap
    # a declared capacity below the need: refused before any launch, and nothing at all is written
    out = torch.full((cap + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    with hip_ops.profile():
        for declared in (cap - 1, opt_cap, 0):
            with pytest.raises(CiaoSRHipError, match='workspace'):
                jpeg_hip.encode_scans_device(t, rects, quality=100, out=out, capacity=declared, progressive=True)
    assert hip_ops.profile.results() == {}
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # the exact capacity: the scans are written, and not a byte at or beyond their end
    got, result = jpeg_hip.encode_scans_device(t, rects, quality=100, out=out, capacity=cap, progressive=True)
    offs, tables = jpeg_hip.split_progressive_result(result.cpu(), 2)
    assert got is out and offs[0] == 0 and offs[20] <= cap and offs == sorted(offs)
    raw = out.cpu().numpy()
    assert bool((raw[offs[20]:] == 0xA5).all())
    wants = [prog.code(rgb[y0:y0 + h, x0:x0 + w], 100, '444') for y0, x0, h, w in rects]
    assert [[raw[offs[10 * k + s]:offs[10 * k + s + 1]].tobytes() for s in range(10)] for k in range(2)] == [w[0] for w in wants]
    assert [[(list(c), list(v)) for c, v in tb] for tb in tables] == [[(list(c), list(v)) for c, v in w[1]] for w in wants]
    # a short workspace is refused the same way
    nbytes = lib.ciaosr_jpeg_prog_tiles_workspace_bytes(host_rects, 2, 0, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    words = lib.ciaosr_jpeg_prog_result_bytes(2) // 8
    res = torch.full((words + 16,), -1, dtype=torch.int64, device=dev)

    def run(ws_bytes=nbytes, quality=90, sub=0, mcus=0, arr=host_rects, n=2, h=72, w=136, capacity=cap):
        return lib.ciaosr_jpeg_prog_encode_tiles_u8(hip_ops.ptr(t), C.c_size_t(t.stride(0)), h, w, 1, arr, n, quality, sub, mcus,
                                                    hip_ops.ptr(out), C.c_size_t(capacity), hip_ops.ptr(res), hip_ops.ptr(ws),
                                                    C.c_size_t(ws_bytes), hip_ops.stream_ptr(dev))

    bad_arg, short = -1, -4
    with hip_ops.profile():
        assert run(ws_bytes=nbytes - 1) == short and run(capacity=cap - 1) == short
        assert run(ws_bytes=lib.ciaosr_jpeg_opt_tiles_workspace_bytes(host_rects, 2, 0, 0)) == short
        assert run(quality=0) == bad_arg and run(quality=101) == bad_arg and run(sub=1) == bad_arg and run(sub=3) == bad_arg
        assert run(mcus=-1) == bad_arg and run(n=0) == bad_arg and run(h=71) == bad_arg and run(w=135) == bad_arg
        for r in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (70, 0, 3, 5), (0, 130, 5, 7)):
            assert run(arr=(C.c_int * 8)(*r, 0, 0, 1, 1)) == bad_arg, r
    assert hip_ops.profile.results() == {}
    torch.cuda.synchronize()
    assert bool((res == -1).all())
    assert run() == 0
    torch.cuda.synchronize()
    back = res.cpu()
    assert bool((back[words:] == -1).all())                                                  # the result buffer's own end is respected
    wants90 = [prog.code(rgb[y0:y0 + h, x0:x0 + w], 90, '444')[1] for y0, x0, h, w in rects]
    assert jpeg_hip.split_progressive_result(back, 2)[1] == [[(tuple(c), tuple(v)) for c, v in tb] for tb in wants90]


def test_refused_arguments_launch_nothing(dev):
    from ciaosr_amd import hip_ops, jpeg_hip
    rgb = make_image(37, 53, 'noise')
    t = _dev_img(rgb, 'bgr', dev)
    with hip_ops.profile():
        for bad in ('yes', 1, None):
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg(t, progressive=bad)
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg_tiles(t, [(0, 0, 5, 5)], progressive=bad)
        for kw in (dict(quality=0), dict(subsampling='422'), dict(order='gbr'), dict(mcus_per_chunk=-2), dict(optimize=1)):
            with pytest.raises(ValueError):
                jpeg_hip.encode_jpeg(t, progressive=True, **kw)
        with pytest.raises(ValueError):
            jpeg_hip.encode_jpeg_tiles(t, [(0, 0, 38, 5)], progressive=True)
    assert hip_ops.profile.results() == {}


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_decoding_gives_the_baseline_files_pixels(dev, subsampling):
    """The coefficients are the same, so a decoder sees the same image."""
    from PIL import Image
    from ciaosr_amd.jpeg_hip import encode_jpeg
    for content in ('noise', 'ramp_noise'):
        t = _dev_img(make_image(100, 75, content), 'bgr', dev)
        for q in (10, 90):
            a = np.asarray(Image.open(io.BytesIO(encode_jpeg(t, quality=q, subsampling=subsampling, progressive=True))).convert('RGB'))
            b = np.asarray(Image.open(io.BytesIO(encode_jpeg(t, quality=q, subsampling=subsampling))).convert('RGB'))
            assert a.shape == (100, 75, 3) and np.array_equal(a, b), (content, q)


def _check_prog_tree(out_dir, name, levels_rgb, tile_size, overlap, quality, subsampling):
    """Every tile of the written tree is byte for byte Pillow's progressive file of the level's crop; the manifest is the plain one."""
    from ciaosr_amd.pyramid import dzi_manifest, dzi_plan
    top = levels_rgb[-1]
    assert open(os.path.join(out_dir, name + '.dzi')).read() == dzi_manifest(top.shape[0], top.shape[1], tile_size, overlap, 'jpg')
    plan = dzi_plan(top.shape[0], top.shape[1], tile_size, overlap)
    assert sorted(os.listdir(os.path.join(out_dir, name + '_files')), key=int) == [str(lv['level']) for lv in plan]
    files = 1
    for lv, img in zip(plan, levels_rgb):
        folder = os.path.join(out_dir, name + '_files', str(lv['level']))
        assert sorted(os.listdir(folder)) == sorted(f'{t[0]}_{t[1]}.jpg' for t in lv['tiles'])
        for col, row, y0, x0, h, w in lv['tiles']:
            data = open(os.path.join(folder, f'{col}_{row}.jpg'), 'rb').read()
            assert data == pil_jpeg_prog(img[y0:y0 + h, x0:x0 + w], quality, subsampling), (lv['level'], col, row)
            files += 1
    return files


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_write_dzi_jpg_progressive(dev, tmp_path, subsampling):
    from tests.test_png_gpu import _restorer
    from ciaosr_amd.pyramid import write_dzi
    model = _restorer({}).to(dev)
    lq = torch.rand(1, 3, 12, 10, generator=torch.Generator().manual_seed(5)).to(dev)
    res = write_dzi(model, model.encode(lq, max_scale=4), str(tmp_path / 'jpg'), 'img', scale=4, tile_size=16, overlap=1, fmt='jpg', quality=85,
                    subsampling=subsampling, progressive=True)
    levels = [_rgb(im) for im in model.render_pyramid(model.encode(lq, max_scale=4), scale=4)]
    assert _check_prog_tree(str(tmp_path / 'jpg'), 'img', levels, 16, 1, 85, subsampling) == res['files'] == 1 + 5 + 4 + 9
    plain = write_dzi(model, model.encode(lq, max_scale=4), str(tmp_path / 'plain'), 'img', scale=4, tile_size=16, overlap=1, fmt='jpg', quality=85,
                      subsampling=subsampling)
    assert plain['files'] == res['files']
    assert open(tmp_path / 'jpg' / 'img.dzi', 'rb').read() == open(tmp_path / 'plain' / 'img.dzi', 'rb').read()


def test_render_cli_jpeg_progressive(dev, tmp_path):
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
    with pytest.raises(SystemExit):
        render.main(argv + ['--jpeg-progressive', '--out', str(tmp_path / 'never')])
    assert not os.path.exists(tmp_path / 'never')
    plain = render.main(argv + ['--gpu-png', '--out', str(tmp_path / 'png')])
    jpg = render.main(argv + ['--jpeg', '90', '--jpeg-progressive', '--jpeg-subsampling', '420', '--out', str(tmp_path / 'jpg')])
    assert [os.path.basename(p) for p in jpg] == ['img_x2.jpg', 'img_view0.jpg']
    assert sorted(os.listdir(tmp_path / 'jpg')) == ['img.dzi', 'img_files', 'img_view0.jpg', 'img_x2.jpg']
    for a, b in zip(plain, jpg):                                                            # the PNG files hold the pixels that were coded
        rgb = imread_u8(a)
        assert open(b, 'rb').read() == pil_jpeg_prog(rgb, 90, '420'), b
    top, levels, files, _ = _read_tree(str(tmp_path / 'png'), 'img', 16, 1)
    assert top == (24, 20)
    assert _check_prog_tree(str(tmp_path / 'jpg'), 'img', levels, 16, 1, 90, '420') == files


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_padding_when_the_last_chunk_adds_no_byte(dev, subsampling):
    """A scan's last byte is padded with 1-bits by the chunk that owns it, which need not be the last chunk: with one MCU per chunk a
    progressive scan's chunks hold a few bits or none, and so do an optimised flat file's (1-bit codes: 6 bits per 4:4:4 MCU).  Every
    width from 1 to 24 blocks, so that the last chunk ends at every place of a byte."""
    from tests.test_jpeg_opt_host import pil_jpeg_opt
    from ciaosr_amd.jpeg_hip import encode_jpeg
    for blocks in range(1, 25):
        rgb = make_image(8, 8 * blocks, 'flat')
        t = _dev_img(rgb, 'bgr', dev)
        got = encode_jpeg(t, quality=90, subsampling=subsampling, mcus_per_chunk=1, progressive=True)
        assert got == pil_jpeg_prog(rgb, 90, subsampling), ('progressive', blocks, _explain(got, pil_jpeg_prog(rgb, 90, subsampling)))
        got = encode_jpeg(t, quality=90, subsampling=subsampling, mcus_per_chunk=1, optimize=True)
        want = pil_jpeg_opt(rgb, 90, subsampling)
        assert got == want, ('optimised', blocks, first_difference(got, want))
