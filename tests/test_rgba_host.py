"""Host-side tests of the RGBA feature (CiaoSR.encode_rgba, png_hip on [H, W, 4] images, tools/render.py --alpha): the container with
colour type 6 under Pillow's decoder, `imread_rgba01`, the ValueErrors that must come before the library is touched, the CLI's and
the pyramid writer's refusals of JPEG, the ABI surface, and the numpy restatement (tests/rgba_ref.py) against itself and Pillow.  Also
the image makers that tests/test_rgba_gpu.py shares."""
import io
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import rgba_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['ciaosr_tensor2img_bgra_u8', 'ciaosr_pack_bgra_u8', 'ciaosr_png_rgba_rows_per_band', 'ciaosr_png_rgba_filter_u8',
               'ciaosr_png_rgba_workspace_bytes', 'ciaosr_png_rgba_capacity_bytes', 'ciaosr_png_rgba_encode_u8',
               'ciaosr_png_rgba_tiles_workspace_bytes', 'ciaosr_png_rgba_tiles_capacity_bytes', 'ciaosr_png_rgba_encode_tiles_u8']
CASES = ['noise', 'flat', 'ramp', 'alpha0', 'alpha255', 'tie']


def make_rgba(h, w, case, seed=0):
    """uint8 [h, w, 4] R G B A.  'noise': seeded uniform bytes; 'flat': one colour; 'ramp': a horizontal ramp in every channel;
    'alpha0' / 'alpha255': smooth colour under a constant alpha; 'tie': rows of zeros alternate with rows of one colour, so on a coloured
    row Sub (1) and Paeth (4) leave the same bytes -- the first pixel, then zeros -- and beat the other three: the lower number must
    win, and it is not filter 0 (asserted in test_reference_against_itself)."""
    rng = np.random.RandomState(1000 * seed + 31 * h + w)
    if case == 'noise':
        return rng.randint(0, 256, (h, w, 4), dtype=np.uint8)
    if case == 'flat':
        return np.broadcast_to(np.array([200, 13, 77, 128], dtype=np.uint8), (h, w, 4)).copy()
    if case == 'ramp':
        x = np.arange(w)[None, :, None]
        return ((3 * x + np.array([0, 40, 80, 120])[None, None, :]) % 256 + np.zeros((h, 1, 1), dtype=np.int64)).astype(np.uint8)
    if case in ('alpha0', 'alpha255'):
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([(5 * x + y) % 256, (3 * y + 2 * x) % 256, (x * y) % 256, np.zeros_like(x)], axis=-1).astype(np.uint8)
        img[:, :, 3] = 0 if case == 'alpha0' else 255
        return img
    if case == 'tie':
        img = np.zeros((h, w, 4), dtype=np.uint8)
        img[1::2] = np.array([9, 250, 3, 128], dtype=np.uint8)
        return img
    raise KeyError(case)


def pil_rgba(png):
    from PIL import Image
    im = Image.open(io.BytesIO(png))
    assert im.mode == 'RGBA', im.mode
    return np.asarray(im)


def test_reference_against_itself():
    for h, w in ((1, 1), (1, 7), (7, 1), (5, 3), (33, 65)):
        for case in CASES:
            img = make_rgba(h, w, case)
            stream, kinds, costs = ref.filter_rows(img)
            assert len(stream) == h * (1 + 4 * w) and all(stream[y * (1 + 4 * w)] == k for y, k in enumerate(kinds))
            assert np.array_equal(ref.unfilter(stream, h, w), img), (h, w, case)
            for k, cost in zip(kinds, costs):
                assert cost[k] == min(cost) and k == cost.index(min(cost))
    # the tie case is one: on a coloured row Sub and Paeth cost the same, less than the other three, and Sub (1) is taken
    _, kinds, costs = ref.filter_rows(make_rgba(5, 3, 'tie'))
    for y in (1, 3):
        assert costs[y][1] == costs[y][4] < min(costs[y][0], costs[y][2], costs[y][3]) and kinds[y] == 1, (y, costs[y])
    assert kinds[0] == kinds[2] == 0 and costs[2][0] == costs[2][1] == 0        # a row of zeros: None and Sub tie at nothing
    # every filter type wins somewhere in the noise + ramp material, so the unfilter's five branches ran
    seen = set()
    for case in ('noise', 'ramp', 'alpha255', 'flat'):
        seen |= set(ref.filter_rows(make_rgba(33, 65, case))[1])
    seen |= set(ref.filter_rows(make_rgba(70, 300, 'noise'))[1])
    assert {0, 1, 2} <= seen, seen
    hist, adler = ref.band_tables(stream, 33, 65, 3)
    assert hist.shape == (11, 260) and hist[:, :256].sum() == len(stream) and (hist[:, 256] == 1).all()
    a = b = 0
    for i in range(11):                                                          # the partials combine to zlib's Adler-32
        n = int(hist[i, :256].sum())
        b = (b + int(adler[i, 1]) + n * a) % ref.ADLER
        a = (a + int(adler[i, 0])) % ref.ADLER
    assert ((len(stream) + b) % ref.ADLER) << 16 | (1 + a) % ref.ADLER == zlib.adler32(bytes(stream))
    assert ref.rows_per_band(300) == 131072 // 1201 and ref.rows_per_band(65535) == 1 and ref.rows_per_band(5, 3) == 3


def test_alpha_formula():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.alpha_of_bgr(np.stack([v, v, v], axis=-1)), v)      # the weights sum to 2^14: grey stays
    assert 4899 + 9617 + 1868 == 16384
    assert ref.alpha_of_bgr(np.array([[0, 0, 255]], dtype=np.uint8))[0] == (4899 * 255 + 8192) >> 14
    assert ref.alpha_of_bgr(np.array([[255, 0, 0]], dtype=np.uint8))[0] == (1868 * 255 + 8192) >> 14
    packed = ref.pack_bgra(np.array([[[1, 2, 3]]], dtype=np.uint8), np.array([[[7, 7, 7]]], dtype=np.uint8))
    assert packed.tolist() == [[[1, 2, 3, 7]]]


@pytest.mark.parametrize('case', CASES)
def test_container_colour_type_6(case):
    from ciaosr_amd import png_hip
    h, w = 33, 65
    img = make_rgba(h, w, case)
    z = zlib.compress(bytes(ref.filter_rows(img)[0]))
    for idat_max in (png_hip.IDAT_MAX, 100):
        png = png_hip.container(h, w, z, idat_max=idat_max, channels=4)
        assert np.array_equal(pil_rgba(png), img)
        assert np.array_equal(ref.decode_rgba_png(png), img)
    assert png_hip.container(h, w, z, channels=3) == png_hip.container(h, w, z)   # the default is the RGB container, unchanged
    assert png_hip.container(h, w, z)[25] == 2 and png_hip.container(h, w, z, channels=4)[25] == 6
    for bad in (5, 1, 0, None):
        with pytest.raises(ValueError):
            png_hip.container(h, w, z, channels=bad)


def test_imread_rgba01(tmp_path):
    from PIL import Image
    from ciaosr_amd.imageio import imread_rgb01, imread_rgba01
    rgba = make_rgba(9, 11, 'noise')
    path = lambda n: str(tmp_path / n)
    Image.fromarray(rgba, 'RGBA').save(path('rgba.png'))
    got, opaque = imread_rgba01(path('rgba.png'))
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 9, 11) and not opaque
    assert torch.equal(got, torch.from_numpy(rgba.astype(np.float32) / 255.0).permute(2, 0, 1))
    # an RGBA file whose alpha is 255 everywhere is opaque
    full = rgba.copy()
    full[:, :, 3] = 255
    Image.fromarray(full, 'RGBA').save(path('full.png'))
    got, opaque = imread_rgba01(path('full.png'))
    assert opaque and torch.equal(got[3], torch.ones(9, 11)) and torch.equal(got[:3], imread_rgb01(path('full.png')))
    # LA: grey + alpha
    la = np.stack([rgba[:, :, 0], rgba[:, :, 3]], axis=-1)
    Image.fromarray(la, 'LA').save(path('la.png'))
    got, opaque = imread_rgba01(path('la.png'))
    assert not opaque and torch.equal(got[3], torch.from_numpy(la[:, :, 1].astype(np.float32) / 255.0))
    for c in range(3):
        assert torch.equal(got[c], torch.from_numpy(la[:, :, 0].astype(np.float32) / 255.0))
    # palette with a tRNS chunk: index 0 is fully transparent
    pal = Image.fromarray((np.arange(99).reshape(9, 11) % 4).astype(np.uint8), 'P')
    pal.putpalette([10, 20, 30, 200, 100, 0, 0, 0, 255, 255, 255, 255] + [0] * (3 * 252))
    pal.save(path('pal.png'), transparency=0)
    assert b'tRNS' in open(path('pal.png'), 'rb').read()
    got, opaque = imread_rgba01(path('pal.png'))
    idx = torch.from_numpy((np.arange(99).reshape(9, 11) % 4).astype(np.int64))
    assert not opaque and torch.equal(got[3], (idx != 0).float())
    assert torch.equal(got[0], torch.tensor([10, 200, 0, 255], dtype=torch.float32)[idx] / 255.0)
    # a palette file without tRNS and an RGB file: alpha 1, opaque
    pal.save(path('pal_opaque.png'))
    assert imread_rgba01(path('pal_opaque.png'))[1]
    Image.fromarray(rgba[:, :, :3].copy(), 'RGB').save(path('rgb.png'))
    got, opaque = imread_rgba01(path('rgb.png'))
    assert opaque and torch.equal(got[3], torch.ones(9, 11)) and torch.equal(got[:3], imread_rgb01(path('rgb.png')))


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the shared library fails the test: the errors under test come before it."""
    from ciaosr_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', refuse)
    monkeypatch.setattr(_lib, 'call', refuse)


def test_value_errors_before_the_library(no_library):
    from ciaosr_amd import metrics_hip, png_hip
    from ciaosr_amd._lib import CiaoSRHipError
    rgba = torch.zeros(5, 7, 4, dtype=torch.uint8)
    rgb = torch.zeros(5, 7, 3, dtype=torch.uint8)
    rects = [(0, 0, 2, 2)]
    for img, order in ((rgba, 'bgr'), (rgba, 'rgb'), (rgba, 'abgr'), (rgb, 'bgra'), (rgb, 'rgba'), (rgb, 'xyz')):
        for call in (lambda: png_hip.encode_png(img, order), lambda: png_hip.encode_zlib(img, order), lambda: png_hip.filter_u8(img, order),
                     lambda: png_hip.encode_png_tiles(img, rects, order), lambda: png_hip.encode_zlib_tiles(img, rects, order),
                     lambda: png_hip.encode_tiles_device(img, rects, order), lambda: png_hip.imwrite_gpu(img, '/nonexistent/x.png', order)):
            with pytest.raises(ValueError):
                call()
    # the right order on a host tensor is refused as before: no CPU fallback
    for img, order in ((rgba, 'bgra'), (rgba, 'rgba'), (rgb, 'bgr')):
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(img, order)
    # five channels, two channels, floats: not an image of this module
    for img in (torch.zeros(5, 7, 5, dtype=torch.uint8), torch.zeros(5, 7, 2, dtype=torch.uint8), torch.zeros(5, 7, 4)):
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(img, 'bgra')
    # the pack helpers
    for bad in (torch.zeros(1, 3, 5, 7), torch.zeros(2, 4, 5, 7), torch.zeros(3, 3, 5, 7), torch.zeros(2, 3, 5), np.zeros((2, 3, 5, 7))):
        with pytest.raises(ValueError):
            metrics_hip.tensor2img_bgra_u8(bad)
    for a, b in ((rgb, rgba), (rgba, rgb), (rgb, torch.zeros(5, 8, 3, dtype=torch.uint8)), (rgb.float(), rgb), (rgb, rgb.numpy())):
        with pytest.raises(ValueError):
            metrics_hip.pack_bgra_u8(a, b)
    # the three-channel entry points keep refusing four channels
    with pytest.raises(CiaoSRHipError):
        metrics_hip._check_image(rgba)


def test_encode_rgba_shape_errors(no_library):
    from ciaosr_amd import scene_render
    for bad in (torch.zeros(1, 3, 5, 7), torch.zeros(2, 4, 5, 7), torch.zeros(4, 5, 7), np.zeros((1, 4, 5, 7))):
        with pytest.raises(ValueError):
            scene_render.encode_rgba(None, bad)


def test_cli_refuses_alpha_with_jpeg(capsys):
    from tools import render
    base = ['cfg.py', 'None', 'img.png', '--scale', '2', '--out', 'o']
    assert render.parse_args(base + ['--alpha']).alpha and not render.parse_args(base).alpha
    with pytest.raises(SystemExit):
        render.parse_args(base + ['--alpha', '--jpeg', '90'])
    assert '--alpha' in capsys.readouterr().err
    assert '--alpha' in render.__doc__


def test_jpeg_pyramid_refuses_alpha(no_library, tmp_path):
    from ciaosr_amd import pyramid

    class Enc:
        alpha = True
        x = torch.zeros(2, 3, 4, 4)

    class Model:
        def render_pyramid(self, *a, **k):
            raise AssertionError('rendered before the format was checked')
    with pytest.raises(ValueError, match='alpha'):
        pyramid.write_dzi(Model(), Enc(), str(tmp_path), 'img', scale=2, fmt='jpg')
    levels = [torch.zeros(1, 1, 4, dtype=torch.uint8), torch.zeros(2, 2, 4, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='alpha'):
        pyramid.write_levels(levels, str(tmp_path), 'img', fmt='jpg')
    assert os.listdir(str(tmp_path)) == []


def test_abi_surface():
    from ciaosr_amd import _lib
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    lib = _lib.load()
    assert lib.ciaosr_version() >= 320
    for name in NEW_SYMBOLS:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for w in (1, 7, 300, 32767, 65535):
        assert lib.ciaosr_png_rgba_rows_per_band(w, 0) == ref.rows_per_band(w)
        assert lib.ciaosr_png_rgba_rows_per_band(w, 5) == 5
        assert lib.ciaosr_png_rows_per_band(w, 0) == max(1, 131072 // (3 * w + 1))      # the three-byte rule is unchanged
    assert lib.ciaosr_png_rgba_rows_per_band(0, 0) == 0 and lib.ciaosr_png_rgba_rows_per_band(65536, 0) == 0
    assert lib.ciaosr_png_rgba_workspace_bytes(0, 5, 0) == 0 and lib.ciaosr_png_rgba_capacity_bytes(5, 65536, 0) == 0
    # the longer rows are sized for: capacity and workspace hold H (4 W + 1) bytes
    assert lib.ciaosr_png_rgba_capacity_bytes(70, 300, 0) >= 70 * 1201 and lib.ciaosr_png_rgba_workspace_bytes(70, 300, 0) >= 70 * 1201
    assert lib.ciaosr_png_rgba_capacity_bytes(70, 300, 0) > lib.ciaosr_png_capacity_bytes(70, 300, 0)
    # null pointers and a misaligned four-byte source are refused before any launch (CIAOSR_ERR_BAD_ARG = whatever null gives)
    bad = lib.ciaosr_png_rgba_filter_u8(None, 28, 5, 7, 1, 0, None, None, None, None)
    assert bad != 0
    assert lib.ciaosr_tensor2img_bgra_u8(None, None, 5, 7, None, 28, None) == bad
    assert lib.ciaosr_pack_bgra_u8(None, 21, None, 21, 5, 7, None, 28, None) == bad
