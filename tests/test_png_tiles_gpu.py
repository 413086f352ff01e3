"""GPU tests of the tile-batched PNG encoder (ciaosr_png_encode_tiles_u8, png_hip.encode_png_tiles).  The judge of the bytes is the
single-image encoder on the pitched crop -- the contract is byte equality with it -- and the judge of the pixels is Pillow's decoder.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import numpy as np
import pytest
import torch

from tests import png_reference as ref
from tests.test_png_host import CONTENTS, five_filter_image, make_image, pil_pixels

pytestmark = pytest.mark.gpu
H, W = 37, 53
# y0 > 0 and x0 > 0; 1 x 1 at the bottom-right pixel; full width; the bottom-right corner; two that overlap; the whole image
RECTS = [(2, 3, 30, 40), (36, 52, 1, 1), (5, 0, 7, 53), (20, 30, 17, 23), (4, 5, 10, 10), (8, 9, 12, 14), (0, 0, 37, 53)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _five(h, w):
    """h x w from five_filter_image blocks (10 rows each: five pairs of an unrelated row and one that a single predictor explains)."""
    return np.concatenate([five_filter_image(w, seed=5 + k) for k in range(-(-h // 10))])[:h]


def _image(content):
    return _five(H, W) if content == 'five' else make_image(H, W, content)


def _dev_img(rgb, order, dev):
    arr = rgb[:, :, ::-1] if order == 'bgr' else rgb
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def _check_tiles(t, rgb, rects, files, order='bgr', rows=0):
    """Each file is the single call's on the pitched crop, byte for byte, and decodes to the crop's pixels."""
    from ciaosr_amd.png_hip import encode_png
    assert len(files) == len(rects)
    for k, ((y0, x0, h, w), png) in enumerate(zip(rects, files)):
        crop = t[y0:y0 + h, x0:x0 + w]
        assert png == encode_png(crop, order=order, rows_per_band=rows), (k, (y0, x0, h, w), rows)
        assert np.array_equal(pil_pixels(png), rgb[y0:y0 + h, x0:x0 + w]), (k, (y0, x0, h, w), rows)


@pytest.mark.parametrize('rows', [1, 3, 0])
@pytest.mark.parametrize('content', CONTENTS + ['five'])
def test_tiles_are_bitwise_the_single_encoder(dev, content, rows):
    from ciaosr_amd.png_hip import encode_png_tiles
    rgb = _image(content)
    if content == 'five':                                      # all five filters win a row of the y0 > 0, x0 > 0 crop
        y0, x0, h, w = RECTS[0]
        _, best = ref.filter_stream(np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w]))
        assert set(best.tolist()) == {0, 1, 2, 3, 4}
    for order in ('bgr', 'rgb'):
        t = _dev_img(rgb, order, dev)
        _check_tiles(t, rgb, RECTS, encode_png_tiles(t, RECTS, order=order, rows_per_band=rows), order, rows)


def test_a_wrong_predecessor_would_show(dev):
    """The crop's left column and top row are coded against zeros, not against the image's pixels there: the filtered stream of the
    tile is the reference filter's on the crop alone, and differs from the same rows cut out of the whole image's stream."""
    import zlib
    from ciaosr_amd.png_hip import encode_png_tiles
    rgb = make_image(H, W, 'noisy')
    y0, x0, h, w = RECTS[0]
    png, = encode_png_tiles(_dev_img(rgb, 'bgr', dev), [RECTS[0]])
    _, _, z = ref.idat_payload(png)
    crop = np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w])
    want, _ = ref.filter_stream(crop)
    assert zlib.decompress(z) == want
    whole, _ = ref.filter_stream(rgb)
    line = 3 * W + 1
    inside = b''.join(whole[(y0 + r) * line + 1 + 3 * x0:(y0 + r) * line + 1 + 3 * (x0 + w)] for r in range(h))
    mine = b''.join(want[r * (3 * w + 1) + 1:(r + 1) * (3 * w + 1)] for r in range(h))
    assert inside != mine


@pytest.mark.parametrize('tile,rows', [(2, 0), (8, 1)])
def test_many_tiles_and_more_bands_than_tiles(dev, tile, rows):
    """400 tiles (more than the scan's 256 lanes), and 25 tiles of 8 one-row bands each."""
    from ciaosr_amd import png_hip
    from ciaosr_amd.pyramid import dzi_plan
    rgb = make_image(40, 40, 'noisy', seed=tile)
    t = _dev_img(rgb, 'bgr', dev)
    rects = [tl[2:] for tl in dzi_plan(40, 40, tile, 0)[-1]['tiles']]
    assert len(rects) == (40 // tile) ** 2
    files = png_hip.encode_png_tiles(t, rects, rows_per_band=rows)
    _check_tiles(t, rgb, rects, files, rows=rows)
    out, offs = png_hip.encode_tiles_device(t, rects, rows_per_band=rows)
    offs = offs.cpu().tolist()
    streams = [ref.idat_payload(f)[2] for f in files]
    assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])) and offs[-1] == sum(len(z) for z in streams) <= out.numel()
    assert [b - a for a, b in zip(offs, offs[1:])] == [len(z) for z in streams]
    assert out[:offs[-1]].cpu().numpy().tobytes() == b''.join(streams)                     # back to back: no gaps, no padding


def test_stored_fallback_beside_huffman(dev):
    import zlib
    from ciaosr_amd.png_hip import encode_png_tiles
    rgb = make_image(48, 64, 'smooth').copy()
    rgb[8:40, 24:56] = np.random.RandomState(9).randint(0, 256, (32, 32, 3), dtype=np.uint8)
    rects = [(8, 24, 32, 32), (0, 0, 48, 20), (4, 20, 40, 40)]            # noise alone; smooth alone; both (it overlaps the other two)
    t = _dev_img(rgb, 'bgr', dev)
    files = encode_png_tiles(t, rects)
    _check_tiles(t, rgb, rects, files)
    first_block = [(ref.idat_payload(f)[2][2] >> 1) & 3 for f in files]                   # BTYPE of each stream's first block
    assert first_block[0] == 0 and first_block[1] == 2, first_block                        # stored beside dynamic Huffman
    for f, (y0, x0, h, w) in zip(files, rects):
        assert len(zlib.decompress(ref.idat_payload(f)[2])) == h * (3 * w + 1)
    # per band, too: one-row bands of the mixed tile choose for themselves
    files = encode_png_tiles(t, rects, rows_per_band=1)
    _check_tiles(t, rgb, rects, files, rows=1)


def test_repeatable_and_on_another_stream(dev):
    from ciaosr_amd.png_hip import encode_png_tiles
    rgb = make_image(H, W, 'noisy')
    t = _dev_img(rgb, 'bgr', dev)
    first = encode_png_tiles(t, RECTS, rows_per_band=3)
    torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(0xA5)                        # other bytes in freed memory
    assert encode_png_tiles(t, RECTS, rows_per_band=3) == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev) == side
        assert encode_png_tiles(t, RECTS, rows_per_band=3) == first
    torch.cuda.current_stream(dev).wait_stream(side)


def test_errors_launch_nothing(dev):
    from ciaosr_amd import hip_ops
    from ciaosr_amd._lib import CiaoSRHipError
    from ciaosr_amd.png_hip import encode_png_tiles
    rgb = make_image(H, W, 'random')
    t = _dev_img(rgb, 'bgr', dev)
    with hip_ops.profile():
        for bad in ([(0, 0, 38, 5)], [(0, 50, 5, 4)], [(0, 0, 0, 5)], [(3, 3, 5, 0)], [(-1, 0, 5, 5)], [(0, 0, 5, 5), (36, 52, 2, 1)], []):
            with pytest.raises(ValueError):
                encode_png_tiles(t, bad)
        with pytest.raises(ValueError):
            encode_png_tiles(t, RECTS, order='gbr')
        with pytest.raises(CiaoSRHipError):
            encode_png_tiles(rgb, RECTS)
        with pytest.raises(CiaoSRHipError):
            encode_png_tiles(torch.from_numpy(rgb), RECTS)
    assert hip_ops.profile.results() == {}


def test_the_library_checks_its_arguments(dev):
    """The C entry point refuses before any launch: rects that leave the image or are empty, no tiles, a short capacity or workspace."""
    import ctypes as C
    from ciaosr_amd import _lib, hip_ops
    lib = _lib.load()
    t = _dev_img(make_image(H, W, 'random'), 'bgr', dev)

    def run(rects, n=None, cap_cut=0, ws_cut=0, h=H, w=W):
        n = len(rects) if n is None else n
        arr = (C.c_int * (4 * max(len(rects), 1)))(*[v for r in rects for v in r])
        good = (C.c_int * 4)(0, 0, H, W)
        cap, nbytes = lib.ciaosr_png_tiles_capacity_bytes(good, 1, 0), lib.ciaosr_png_tiles_workspace_bytes(good, 1, 0)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        offs = torch.empty(len(rects) + 2, dtype=torch.int64, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return lib.ciaosr_png_encode_tiles_u8(hip_ops.ptr(t), C.c_size_t(t.stride(0)), h, w, 1, arr, n, 0, hip_ops.ptr(out),
                                              C.c_size_t(cap - cap_cut), hip_ops.ptr(offs), hip_ops.ptr(ws), C.c_size_t(nbytes - ws_cut),
                                              hip_ops.stream_ptr(dev))

    bad_arg, short = -1, -4
    assert lib.ciaosr_error_string(bad_arg).decode().startswith('bad argument') and lib.ciaosr_error_string(short).decode().startswith('workspace')
    with hip_ops.profile():
        assert run([(0, 0, H, W)], cap_cut=1) == short and run([(0, 0, H, W)], ws_cut=1) == short
        for rects in ([(0, 0, H + 1, W)], [(1, 0, H, W)], [(0, 1, H, W)], [(0, 0, 0, W)], [(0, 0, H, 0)], [(-1, 0, 2, 2)], [(0, -1, 2, 2)]):
            assert run(rects) == bad_arg, rects
        assert run([(0, 0, H, W)], n=0) == bad_arg and run([(0, 0, H, W)], n=-3) == bad_arg
    assert hip_ops.profile.results() == {}
    assert run([(0, 0, H, W)]) == 0
    torch.cuda.synchronize()


def test_two_synchronising_copies_whatever_the_number_of_tiles(dev, monkeypatch):
    from ciaosr_amd import hip_ops, png_hip
    from ciaosr_amd.pyramid import dzi_plan
    t = _dev_img(make_image(40, 40, 'noisy'), 'bgr', dev)
    rects = [tl[2:] for tl in dzi_plan(40, 40, 2, 0)[-1]['tiles']]
    assert len(rects) == 400
    png_hip.encode_png_tiles(t, rects)                                                     # the workspace exists
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
    with hip_ops.profile():
        files = png_hip.encode_png_tiles(t, rects)
    monkeypatch.undo()
    prof = hip_ops.profile.results()
    assert [c[0] for c in copies] == ['cpu', 'cpu'] and copies[0][1] == (401,), copies       # the offsets, then the streams
    assert len(files) == 400
    assert {k: v['launches'] for k, v in prof.items()} == dict(png_filter_tiles_u8=1, deflate_plan=1, png_tiles_scan=1, deflate_pack=1)
