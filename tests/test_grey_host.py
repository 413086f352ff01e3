"""Host-side tests of the grey feature (CiaoSR.encode_grey, png_hip and jpeg_hip on [H, W] images, tools/render.py --grey): the grey
byte against Pillow's convert('L'), `imread_grey01`, the one-component JPEG header and the colour type 0 container against the bytes
Pillow writes, the ValueErrors that must come before the library is touched, the sizes of the new ABI entries against their formulae,
and the CLI's rules.  Also the image makers that tests/test_grey_gpu.py shares."""
import io
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import grey_ref as ref
from tests.test_rgba_host import no_library  # noqa: F401  (the fixture that fails a test when the shared library is touched)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG_SYMBOLS = ['ciaosr_png_grey_rows_per_band', 'ciaosr_png_grey_filter_u8', 'ciaosr_png_grey_workspace_bytes',
               'ciaosr_png_grey_capacity_bytes', 'ciaosr_png_grey_encode_u8', 'ciaosr_png_grey_tiles_workspace_bytes',
               'ciaosr_png_grey_tiles_capacity_bytes', 'ciaosr_png_grey_encode_tiles_u8', 'ciaosr_png_grey_lz_workspace_bytes',
               'ciaosr_png_grey_lz_encode_u8', 'ciaosr_png_grey_lz_tiles_workspace_bytes', 'ciaosr_png_grey_lz_encode_tiles_u8']
NEW_SYMBOLS = ['ciaosr_tensor2img_grey_u8', 'ciaosr_grey_from_bgr_u8'] + PNG_SYMBOLS
CONTENTS = ['noise', 'ramp', 'flat', 'hstripes', 'vstripes']
JPEG_CONTENTS = ['noise', 'ramp', 'flat0', 'flat255', 'checker']
GREY = 4                                                     # CIAOSR_JPEG_GREY


def make_grey(h, w, content, seed=0):
    """uint8 [h, w].  'noise': seeded uniform bytes (None or Paeth wins); 'ramp': a smooth diagonal ramp (Sub / Average / Paeth);
    'flat', 'flat0', 'flat255': one value; 'hstripes': rows alternate between two values (Sub wins: a row is constant);
    'vstripes': columns of period 3 (Up wins below the first row); 'checker': single pixels of 0 and 255."""
    rng = np.random.RandomState(1000 * seed + 31 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    if content == 'noise':
        return rng.randint(0, 256, (h, w), dtype=np.uint8)
    if content == 'ramp':
        return ((3 * x + 2 * y) % 256).astype(np.uint8)
    if content in ('flat', 'flat0', 'flat255'):
        return np.full((h, w), {'flat': 77, 'flat0': 0, 'flat255': 255}[content], dtype=np.uint8)
    if content == 'hstripes':
        return np.where(y % 2 == 0, 30, 220).astype(np.uint8)
    if content == 'vstripes':
        return np.array([10, 128, 250], dtype=np.uint8)[x % 3] + np.zeros((h, 1), dtype=np.uint8)
    if content == 'checker':
        return (255 * ((x + y) % 2)).astype(np.uint8)
    raise KeyError(content)


def pil_grey(png):
    """The pixels of a PNG or JPEG file that Pillow opens as mode L."""
    from PIL import Image
    im = Image.open(io.BytesIO(png))
    assert im.mode == 'L', im.mode
    return np.asarray(im)


def pil_jpeg_grey(grey, quality, optimize=False):
    """Pillow's mode-L JPEG file (for `optimize` with its output buffer raised, as tests/test_jpeg_opt_host.py does)."""
    import PIL.ImageFile
    from PIL import Image
    mp = pytest.MonkeyPatch()
    mp.setattr(PIL.ImageFile, 'MAXBLOCK', 1 << 24)
    try:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(grey), 'L').save(bio, format='JPEG', quality=quality, **(dict(optimize=True) if optimize else {}))
    finally:
        mp.undo()
    return bio.getvalue()


# -- the grey byte ----------------------------------------------------------------------------------------------------------------------
def test_grey_formula_is_pillows_convert_l():
    from PIL import Image
    rgb = np.random.RandomState(7).randint(0, 256, (300, 300, 3), dtype=np.uint8)
    assert np.array_equal(ref.grey_of_bgr(rgb[:, :, ::-1]), np.asarray(Image.fromarray(rgb).convert('L')))
    v = np.arange(256, dtype=np.uint8)
    assert 19595 + 38470 + 7471 == 65536 and np.array_equal(ref.grey_of_bgr(np.stack([v, v, v], axis=-1)), v)      # neutral stays
    # where the alpha formula disagrees, Pillow sides with the grey one: 39 135 triples, each off by one
    bgr = ref.disagreement_set()
    assert len(bgr) == 39135
    u8 = bgr.astype(np.uint8)
    assert (ref.grey_of_bgr(u8) != ref.alpha_of_bgr(u8)).all()
    pad = np.zeros((198 * 198 - len(u8), 3), dtype=np.uint8)
    rgb = np.concatenate([u8[:, ::-1], pad]).reshape(198, 198, 3)
    pil = np.asarray(Image.fromarray(np.ascontiguousarray(rgb)).convert('L')).reshape(-1)[:len(u8)]
    assert np.array_equal(pil, ref.grey_of_bgr(u8))


def test_reference_filter_against_itself_and_zlib():
    seen = set()
    for h, w in ((1, 1), (1, 7), (5, 1), (7, 5), (33, 17)):
        for content in CONTENTS:
            img = make_grey(h, w, content)
            stream, kinds, costs = ref.filter_rows(img)
            assert len(stream) == h * (1 + w) and all(stream[y * (1 + w)] == k for y, k in enumerate(kinds))
            for k, cost in zip(kinds, costs):
                assert cost[k] == min(cost) and k == cost.index(min(cost))
            seen |= set(kinds)
    assert seen == {0, 1, 2, 3, 4}, seen                     # each of the five filters wins some row of the material
    hist, adler = ref.band_tables(stream, 33, 17, 5)
    assert hist.shape == (7, 260) and hist[:, :256].sum() == len(stream) and (hist[:, 256] == 1).all()
    a = b = 0
    for i in range(7):                                       # the partials combine to zlib's Adler-32
        n = int(hist[i, :256].sum())
        b = (b + int(adler[i, 1]) + n * a) % ref.ADLER
        a = (a + int(adler[i, 0])) % ref.ADLER
    assert ((len(stream) + b) % ref.ADLER) << 16 | (1 + a) % ref.ADLER == zlib.adler32(bytes(stream))
    assert ref.band_offsets(33, 17, 5) == [0, 90, 180, 270, 360, 450, 540, 594]


# -- files ------------------------------------------------------------------------------------------------------------------------------
def test_imread_grey01(tmp_path):
    from PIL import Image
    from ciaosr_amd.imageio import imread_grey01
    g = make_grey(9, 11, 'noise')
    want = torch.from_numpy(g.astype(np.float32) / 255.0).unsqueeze(0)
    path = lambda n: str(tmp_path / n)
    Image.fromarray(g, 'L').save(path('l.png'))
    got, was_grey = imread_grey01(path('l.png'))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 9, 11) and was_grey and torch.equal(got, want)
    Image.fromarray(np.stack([g, g, g], axis=-1), 'RGB').save(path('neutral.png'))
    got, was_grey = imread_grey01(path('neutral.png'))
    assert was_grey and torch.equal(got, want)
    rgb = np.random.RandomState(3).randint(0, 256, (9, 11, 3), dtype=np.uint8)
    Image.fromarray(rgb, 'RGB').save(path('colour.png'))
    got, was_grey = imread_grey01(path('colour.png'))
    assert not was_grey and torch.equal(got, torch.from_numpy(ref.grey_of_bgr(rgb[:, :, ::-1]).astype(np.float32) / 255.0).unsqueeze(0))
    pal = Image.fromarray((np.arange(99).reshape(9, 11) % 4).astype(np.uint8), 'P')
    pal.putpalette([10, 10, 10, 200, 200, 200, 0, 0, 0, 255, 255, 255] + [0] * (3 * 252))
    pal.save(path('pal_grey.png'))
    got, was_grey = imread_grey01(path('pal_grey.png'))
    idx = torch.from_numpy((np.arange(99).reshape(9, 11) % 4).astype(np.int64))
    assert was_grey and torch.equal(got[0], torch.tensor([10, 200, 0, 255], dtype=torch.float32)[idx] / 255.0)
    pal.putpalette([10, 20, 30, 200, 100, 0, 0, 0, 255, 255, 255, 255] + [0] * (3 * 252))
    pal.save(path('pal_colour.png'))
    assert not imread_grey01(path('pal_colour.png'))[1]
    la = np.stack([g, 255 - g], axis=-1)
    Image.fromarray(la, 'LA').save(path('la.png'))
    got, was_grey = imread_grey01(path('la.png'))
    assert was_grey and torch.equal(got, want)               # the alpha band is dropped, the grey band kept


@pytest.mark.parametrize('h,w,q', [(1, 1, 1), (37, 53, 90), (250, 253, 100)])
def test_jpeg_header_is_pillows(h, w, q):
    from ciaosr_amd import jpeg_hip
    grey = make_grey(h, w, 'noise')
    for optimize in (False, True):
        pil = pil_jpeg_grey(grey, q, optimize)
        sos = pil.index(b'\xff\xda')
        front = pil[:sos + 2 + 8]                            # up to and including the one-component SOS header
        assert pil[sos + 2:sos + 10] == bytes((0, 8, 1, 1, 0x00, 0, 0x3f, 0))
        frame = jpeg_hip._frame(h, w, q, '444', b'\xff\xc0', grey=True)
        assert front.startswith(frame) and frame[-13:-11] == b'\xff\xc0' and frame[-3:] == bytes((1, 0x11, 0))
        assert frame.count(b'\xff\xdb') == 1
        if not optimize:
            assert jpeg_hip.header(h, w, q, grey=True) == front
            assert front.count(b'\xff\xc4') == 2
            continue
        # the optimised file: Pillow's two tables, handed to header() as an optimised call returns them (records 2, 3 all zero)
        tables, i = [], len(frame)
        while pil[i:i + 2] == b'\xff\xc4':
            n = int.from_bytes(pil[i + 2:i + 4], 'big')
            tables.append((tuple(pil[i + 5:i + 21]), tuple(pil[i + 21:i + 2 + n])))
            assert pil[i + 4] == (0x00, 0x10)[len(tables) - 1]
            i += 2 + n
        assert len(tables) == 2 and i == sos
        empty = ((0,) * 16, ())
        assert jpeg_hip.header(h, w, q, tables=tables + [empty, empty], grey=True) == front
        assert jpeg_hip.header(h, w, q, tables=tables, grey=True) == front
    # the colour header is unchanged by the new keyword
    assert jpeg_hip.header(h, w, q, '444') == jpeg_hip.header(h, w, q, '444', None, False) and jpeg_hip.header(h, w, q, '444')[-14:-10] == b'\xff\xda\x00\x0c'


def test_png_container_colour_type_0():
    from ciaosr_amd import png_hip
    for content in CONTENTS:
        img = make_grey(33, 17, content)
        z = zlib.compress(bytes(ref.filter_rows(img)[0]))
        for idat_max in (png_hip.IDAT_MAX, 100):
            png = png_hip.container(33, 17, z, idat_max=idat_max, grey=True)
            assert png[25] == 0 and np.array_equal(pil_grey(png), img)
    assert png_hip.container(33, 17, z)[25] == 2 and png_hip.container(33, 17, z, grey=False) == png_hip.container(33, 17, z)
    for bad in (1, 0, 2):
        with pytest.raises(ValueError):
            png_hip.container(33, 17, z, channels=bad)       # channels=1 stays refused: grey is its own keyword
    with pytest.raises(ValueError):
        png_hip.container(33, 17, z, grey=1)


# -- errors before the library ----------------------------------------------------------------------------------------------------------
def test_value_errors_before_the_library(no_library, tmp_path):  # noqa: F811
    from ciaosr_amd import jpeg_hip, metrics_hip, png_hip, pyramid, scene_render
    from ciaosr_amd._lib import CiaoSRHipError
    grey = torch.zeros(5, 7, dtype=torch.uint8)
    rgb = torch.zeros(5, 7, 3, dtype=torch.uint8)
    rects = [(0, 0, 2, 2)]
    png_calls = lambda img, order: (
        lambda: png_hip.encode_png(img, order), lambda: png_hip.encode_zlib(img, order), lambda: png_hip.filter_u8(img, order),
        lambda: png_hip.encode_png_tiles(img, rects, order), lambda: png_hip.encode_zlib_tiles(img, rects, order),
        lambda: png_hip.encode_tiles_device(img, rects, order), lambda: png_hip.imwrite_gpu(img, '/nonexistent/x.png', order),
        lambda: png_hip.encode_png(img, order, matches=True), lambda: png_hip.encode_png_tiles(img, rects, order, matches=True))
    for img, order in ((grey, 'rgb'), (grey, 'bgra'), (grey, 'l'), (rgb, 'grey'), (torch.zeros(5, 7, 4, dtype=torch.uint8), 'grey')):
        for call in png_calls(img, order):
            with pytest.raises(ValueError):
                call()
    # the right order on a host tensor is refused as every host image is: no CPU fallback; two channels stay what they were
    for order in ('bgr', 'grey'):
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(grey, order)
    for bad in (torch.zeros(5, 7, 2, dtype=torch.uint8), torch.zeros(5, 7)):
        with pytest.raises(CiaoSRHipError):
            png_hip.encode_png(bad)
    # JPEG: no subsampling, no 'gray', no progressive form, no colour order on a 2-D image
    jpeg_calls = lambda **kw: (
        lambda: jpeg_hip.encode_jpeg(grey, **kw), lambda: jpeg_hip.encode_jpeg_tiles(grey, rects, **kw), lambda: jpeg_hip.encode_scan(grey, **kw),
        lambda: jpeg_hip.encode_scans(grey, rects, **kw), lambda: jpeg_hip.encode_scans_device(grey, rects, **kw),
        lambda: jpeg_hip.imwrite_gpu_jpeg(grey, '/nonexistent/x.jpg', **kw))
    for kw in (dict(subsampling='420'), dict(subsampling='gray'), dict(progressive=True), dict(progressive=True, optimize=True),
               dict(order='rgb'), dict(quality=0)):
        for call in jpeg_calls(**kw):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        jpeg_hip.encode_jpeg(rgb, subsampling='gray')
    with pytest.raises(ValueError):
        jpeg_hip.encode_jpeg(rgb, order='grey')
    with pytest.raises(CiaoSRHipError):
        jpeg_hip.encode_jpeg(grey)                           # a host image: refused after the arguments, without a library call
    with pytest.raises(ValueError):
        jpeg_hip.header(8, 8, 90, '420', grey=True)
    # the quantisers' shapes
    for bad in (torch.zeros(2, 3, 5, 7), torch.zeros(1, 1, 5, 7), torch.zeros(1, 5, 7), torch.zeros(5, 7), np.zeros((3, 5, 7))):
        with pytest.raises(ValueError):
            metrics_hip.tensor2img_grey_u8(bad)
    with pytest.raises(ValueError):
        metrics_hip.tensor2img_grey_u8(torch.zeros(3, 5, 7), out=torch.zeros(5, 8, dtype=torch.uint8))
    for bad in (grey, torch.zeros(5, 7, 4, dtype=torch.uint8), rgb.float(), rgb.numpy()):
        with pytest.raises(ValueError):
            metrics_hip.grey_from_bgr_u8(bad)
    with pytest.raises(ValueError):
        metrics_hip.grey_from_bgr_u8(rgb, order='grey')
    # the renderer's encodes
    for bad in (torch.zeros(1, 3, 5, 7), torch.zeros(1, 2, 5, 7), torch.zeros(1, 5, 7), np.zeros((1, 1, 5, 7))):
        with pytest.raises(ValueError):
            scene_render.encode_grey(None, bad)
    with pytest.raises(ValueError, match='grey'):
        scene_render.encode_rgba(None, torch.zeros(1, 2, 5, 7))                 # grey + alpha

    # the pyramid writer: progressive grey tiles and subsampled ones are refused before anything is rendered or written
    class Enc:
        alpha, grey = False, True
        x = torch.zeros(1, 3, 4, 4)

    class Model:
        def render_pyramid(self, *a, **k):
            raise AssertionError('rendered before the format was checked')
    levels = [torch.zeros(1, 1, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8)]
    for kw in (dict(progressive=True), dict(subsampling='420')):
        with pytest.raises(ValueError):
            pyramid.write_dzi(Model(), Enc(), str(tmp_path), 'img', scale=2, fmt='jpg', **kw)
        with pytest.raises(ValueError):
            pyramid.write_levels(levels, str(tmp_path), 'img', fmt='jpg', **kw)
    with pytest.raises(ValueError):
        pyramid.write_levels(levels, str(tmp_path), 'img', order='rgb')
    with pytest.raises(ValueError):
        pyramid.write_levels([levels[0], torch.zeros(2, 2, 3, dtype=torch.uint8)], str(tmp_path), 'img')
    assert os.listdir(str(tmp_path)) == []


# -- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_surface_and_sizes():
    from ciaosr_amd import _lib, jpeg_hip
    import ctypes as C
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    png_header = open(os.path.join(REPO, 'include', 'ciaosr_hip_png_grey.h')).read()
    lib = _lib.load()
    assert lib.ciaosr_version() >= 340 and f'#define CIAOSR_JPEG_GREY {GREY}' in header and jpeg_hip.GREY == GREY
    for name in NEW_SYMBOLS[:2]:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the grey PNG family: its own header, which ciaosr_hip.h includes, and its own ctypes table, which `load` binds -- each
    # declaration is exported and bound, the two list the same names, with the arguments of the four-byte namesakes
    assert re.search(r'^#include "ciaosr_hip_png_grey.h"$', header, flags=re.M)
    protos = re.findall(r'^\s*(int|size_t)\s+(ciaosr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', re.sub(r'/\*.*?\*/', '', png_header, flags=re.S), flags=re.M)
    assert sorted(n for _, n, _ in protos) == sorted(PNG_SYMBOLS) == sorted(_lib.GREY_PNG_SIGNATURES)
    assert not set(PNG_SYMBOLS) & set(_lib.SIGNATURES)
    for ret, name, args in protos:
        res, argtypes = _lib.GREY_PNG_SIGNATURES[name]
        assert _lib.GREY_PNG_SIGNATURES[name] == _lib.SIGNATURES[name.replace('_grey_', '_rgba_')], name
        assert (C.c_int if ret == 'int' else C.c_size_t) is res and len(args.split(',')) == len(argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == argtypes, name
    # PNG: the default band is max(1, 131072 / (W + 1)) rows; refusals are 0
    for w in (1, 7, 300, 8160, 32767, 65535):
        assert lib.ciaosr_png_grey_rows_per_band(w, 0) == ref.rows_per_band(w) == max(1, 131072 // (w + 1))
        assert lib.ciaosr_png_grey_rows_per_band(w, 5) == 5
    assert lib.ciaosr_png_grey_rows_per_band(0, 0) == 0 and lib.ciaosr_png_grey_rows_per_band(65536, 0) == 0
    assert lib.ciaosr_png_grey_rows_per_band(5, -1) == 0
    # sizes follow the scanline bytes H (W + 1): the capacity is the three-byte coder's of an image with as many bytes in as many bands
    for h, w, rows in ((1, 1, 0), (70, 300, 0), (70, 300, 7), (1000, 8160, 0), (65535, 65535, 0), (31, 64, 3)):
        total, nb = h * (w + 1), -(-h // ref.rows_per_band(w, rows))
        cap = lib.ciaosr_png_grey_capacity_bytes(h, w, rows)
        assert cap == total + 5 * (total // 65535 + nb) + 6 + 8, (h, w, rows)
        assert lib.ciaosr_png_grey_workspace_bytes(h, w, rows) >= total
        assert lib.ciaosr_png_grey_lz_workspace_bytes(h, w, rows) >= lib.ciaosr_png_grey_workspace_bytes(h, w, rows) + 2 * total
        rect = (C.c_int * 4)(0, 0, h, w)
        assert lib.ciaosr_png_grey_tiles_capacity_bytes(rect, 1, rows) == cap
        assert lib.ciaosr_png_grey_tiles_workspace_bytes(rect, 1, rows) >= total
        assert lib.ciaosr_png_grey_lz_tiles_workspace_bytes(rect, 1, rows) >= lib.ciaosr_png_grey_tiles_workspace_bytes(rect, 1, rows) + 2 * total
    assert lib.ciaosr_png_grey_capacity_bytes(70, 300, 0) < lib.ciaosr_png_capacity_bytes(70, 300, 0)
    for h, w, rows in ((0, 5, 0), (5, 0, 0), (65536, 5, 0), (5, 65536, 0), (5, 5, -1)):
        for fn in (lib.ciaosr_png_grey_capacity_bytes, lib.ciaosr_png_grey_workspace_bytes, lib.ciaosr_png_grey_lz_workspace_bytes):
            assert fn(h, w, rows) == 0, (h, w, rows)
    for rects in ([0, 0, 0, 5], [0, -1, 5, 5], [0, 0, 65536, 5]):
        arr = (C.c_int * 4)(*rects)
        assert lib.ciaosr_png_grey_tiles_capacity_bytes(arr, 1, 0) == 0 and lib.ciaosr_png_grey_tiles_workspace_bytes(arr, 1, 0) == 0
        assert lib.ciaosr_png_grey_lz_tiles_workspace_bytes(arr, 1, 0) == 0
    assert lib.ciaosr_png_grey_tiles_capacity_bytes(None, 1, 0) == 0
    # JPEG: 416 bytes per block, optimised 2 x ceil(1665 x blocks / 8); the progressive entries refuse the value; 1 and 3 stay invalid
    for h, w in ((1, 1), (8, 8), (9, 17), (37, 53), (250, 253), (5424, 8160), (65535, 3)):
        blocks = -(-h // 8) * -(-w // 8)
        assert jpeg_hip.scan_block_count(h, w, '444', grey=True) == blocks
        assert lib.ciaosr_jpeg_capacity_bytes(h, w, GREY) == 416 * blocks
        assert lib.ciaosr_jpeg_opt_capacity_bytes(h, w, GREY) == 2 * -(-1665 * blocks // 8)
        rect = (C.c_int * 8)(0, 0, h, w, 0, 0, 1, 1)
        assert lib.ciaosr_jpeg_tiles_capacity_bytes(rect, 2, GREY) == 416 * (blocks + 1)
        assert lib.ciaosr_jpeg_opt_tiles_capacity_bytes(rect, 2, GREY) == 2 * (-(-1665 * blocks // 8) + -(-1665 // 8))
        for mcus in (0, 1, 3):
            assert lib.ciaosr_jpeg_workspace_bytes(h, w, GREY, mcus) >= 128 * blocks + 208 * blocks
            assert lib.ciaosr_jpeg_opt_workspace_bytes(h, w, GREY, mcus) >= 128 * blocks + -(-1665 * blocks // 8)
            assert lib.ciaosr_jpeg_tiles_workspace_bytes(rect, 2, GREY, mcus) > 0 and lib.ciaosr_jpeg_opt_tiles_workspace_bytes(rect, 2, GREY, mcus) > 0
        assert lib.ciaosr_jpeg_prog_capacity_bytes(h, w, GREY) == 0 and lib.ciaosr_jpeg_prog_workspace_bytes(h, w, GREY, 0) == 0
        assert lib.ciaosr_jpeg_prog_tiles_capacity_bytes(rect, 2, GREY) == 0 and lib.ciaosr_jpeg_prog_tiles_workspace_bytes(rect, 2, GREY, 0) == 0
        for bad in (1, 3, 5, -1):
            assert lib.ciaosr_jpeg_capacity_bytes(h, w, bad) == 0 and lib.ciaosr_jpeg_workspace_bytes(h, w, bad, 0) == 0
            assert lib.ciaosr_jpeg_opt_capacity_bytes(h, w, bad) == 0 and lib.ciaosr_jpeg_opt_workspace_bytes(h, w, bad, 0) == 0
            assert lib.ciaosr_jpeg_prog_capacity_bytes(h, w, bad) == 0
        assert lib.ciaosr_jpeg_capacity_bytes(h, w, 0) == 3 * 416 * blocks                       # the colour sizes are what they were
    # the grey chunk default: 768 MCUs of one block, as the colour chunks hold 768 blocks -- the sizes of 0 and 768 agree
    assert lib.ciaosr_jpeg_workspace_bytes(250, 253, GREY, 0) == lib.ciaosr_jpeg_workspace_bytes(250, 253, GREY, 768)
    # the progressive call refuses the value before anything else is looked at: no launch, no pointer read
    rc = lib.ciaosr_jpeg_prog_encode_u8(None, 8, 8, 8, 0, 90, GREY, 0, None, 0, None, None, 0, None)
    assert rc != 0 and b'unsupported' in lib.ciaosr_error_string(rc).lower()
    rc_bad = lib.ciaosr_jpeg_prog_encode_u8(None, 8, 8, 8, 0, 90, 3, 0, None, 0, None, None, 0, None)
    assert rc_bad not in (0, rc)
    # null pointers are refused before any launch
    bad = lib.ciaosr_png_grey_filter_u8(None, 7, 5, 7, 0, 0, None, None, None, None)
    assert bad != 0 and lib.ciaosr_tensor2img_grey_u8(None, 5, 7, None, 7, None) == bad
    assert lib.ciaosr_grey_from_bgr_u8(None, 21, 1, 5, 7, None, 7, None) == bad


# -- tools/render.py --grey -------------------------------------------------------------------------------------------------------------
def test_cli_rules(capsys):
    from tools import render
    base = ['cfg.py', 'None', 'img.png', '--scale', '2', '--out', 'o']
    assert render.parse_args(base + ['--grey']).grey and not render.parse_args(base).grey
    for extra, word in ((['--alpha'], '--alpha'), (['--jpeg', '90', '--jpeg-progressive'], '--jpeg-progressive'),
                        (['--jpeg', '90', '--jpeg-subsampling', '420'], '--jpeg-subsampling')):
        with pytest.raises(SystemExit):
            render.parse_args(base + ['--grey'] + extra)
        err = capsys.readouterr().err
        assert '--grey' in err and word in err
    with pytest.raises(SystemExit):
        render.parse_args(base + ['--png-matches'])           # still the device coder's option only
    capsys.readouterr()
    # what works as for colour
    args = render.parse_args(base + ['--grey', '--png-matches', '--self-ensemble', '--niqe', 'p.npz'])
    assert args.png_matches and args.self_ensemble and render.output_format(args) == dict(fmt='png', ext='.png')
    args = render.parse_args(base + ['--grey', '--jpeg', '85', '--jpeg-optimize', '--dzi', '2'])
    assert render.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=85, subsampling='444', optimize=True)
    assert render.output_format(render.parse_args(base + ['--grey', '--jpeg', '85'])) == dict(fmt='jpg', ext='.jpg', quality=85, subsampling='444')
    assert '--grey' in render.__doc__
