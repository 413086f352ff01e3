"""16-bit samples, host side (no GPU): the depth-16 PNG reader against Pillow (grey) and against the reference writer of
tests/png16_ref.py (RGB, every filter forced), the 16-bit image readers, the container's depth keyword, the new exports against the
header and their size functions' refusals, the reference's own filter coverage on the contents the GPU tests use, and the refusals of
tools/render.py --depth16.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import png16_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER_SIZES = [(1, 1), (1, 300), (5, 1), (33, 17), (9, 300)]      # what tests/test_depth16_gpu.py filters
READER_SIZES = [(1, 1), (1, 9), (7, 1), (6, 11)]
FAMILY = ('rows_per_band', 'filter_u16', 'workspace_bytes', 'lz_workspace_bytes', 'capacity_bytes', 'encode_u16', 'lz_encode_u16',
          'tiles_workspace_bytes', 'lz_tiles_workspace_bytes', 'tiles_capacity_bytes', 'encode_tiles_u16', 'lz_encode_tiles_u16')
NEW_EXPORTS = ['ciaosr_tensor2img_u16', 'ciaosr_tensor2img_grey_u16', 'ciaosr_grey_from_bgr_u16'] + \
              [pre + n for pre in ('ciaosr_png16_', 'ciaosr_png16_grey_') for n in FAMILY]


def _write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(data)
    return path


# -- the reader ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', READER_SIZES + [(40, 33)])
def test_read_png16_grey_is_pillows_array(tmp_path, h, w):
    from PIL import Image
    from ciaosr_amd.imageio import read_png16
    for content in ('noise', 'smooth', 'bytes'):
        img = ref.make16(h, w, 1, content)
        path = str(tmp_path / f'{content}.png')
        Image.fromarray(img).save(path)                       # mode I;16: Pillow writes a colour type 0 file of bit depth 16
        with Image.open(path) as f:
            assert f.mode.startswith('I;16')
            want = np.asarray(f).astype(np.uint16)
        assert np.array_equal(want, img)
        got = read_png16(path)
        assert got.dtype == np.uint16 and got.shape == (h, w) and np.array_equal(got, want), content


@pytest.mark.parametrize('h,w', READER_SIZES)
@pytest.mark.parametrize('c', [1, 3])
def test_read_png16_every_filter(tmp_path, h, w, c):
    from ciaosr_amd.imageio import read_png16
    for content in ('noise', 'diagonal', 'bytes'):
        img = ref.make16(h, w, c, content)
        for force in (0, 1, 2, 3, 4, [y % 5 for y in range(h)], None):
            png = ref.write_png16(img, force)
            assert np.array_equal(ref.decode_png16(png), img)             # the reference reads its own files
            got = read_png16(_write(tmp_path, 'f.png', png))
            assert got.dtype == np.uint16 and got.shape == img.shape and np.array_equal(got, img), (content, force)
    png = ref.write_png16(img, [(y + 3) % 5 for y in range(h)], idat_sizes=5)                  # many IDAT chunks
    assert sum(tag == b'IDAT' for tag, _ in ref.chunks(png)) >= 3
    assert np.array_equal(read_png16(_write(tmp_path, 'split.png', png)), img)


def test_read_png16_refusals(tmp_path):
    from PIL import Image
    from ciaosr_amd.imageio import read_png16
    img = ref.make16(4, 5, 3, 'noise')
    with pytest.raises(ValueError, match='interlace'):
        read_png16(_write(tmp_path, 'i.png', ref.write_png16(img, interlace=1)))
    for colour_type in (4, 6):
        with pytest.raises(ValueError, match=f'colour type {colour_type}'):
            read_png16(_write(tmp_path, 'a.png', ref.write_png16(img, colour_type=colour_type)))
    path = str(tmp_path / 'eight.png')
    Image.fromarray((img >> 8).astype(np.uint8), 'RGB').save(path)
    with pytest.raises(ValueError, match='bit depth 8'):
        read_png16(path)
    with pytest.raises(ValueError, match='not a PNG'):
        read_png16(_write(tmp_path, 'x.png', b'not a png file at all, but long enough'))


# -- the 16-bit image readers ----------------------------------------------------------------------------------------------------------
def test_imread16_is_imread_on_8_bit_files(tmp_path):
    from PIL import Image
    from ciaosr_amd.imageio import imread16_grey01, imread16_rgb01, imread_grey01, imread_rgb01
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, (9, 13, 3), dtype=np.uint8)
    files = {'rgb.png': Image.fromarray(rgb, 'RGB'), 'l.png': Image.fromarray(rgb[:, :, 0], 'L'),
             'p.png': Image.fromarray(rgb, 'RGB').quantize(16), 'rgb.bmp': Image.fromarray(rgb, 'RGB'),
             'la.png': Image.fromarray(rgb[:, :, :2], 'LA')}
    for name, im in files.items():
        path = str(tmp_path / name)
        im.save(path)
        t, bits = imread16_rgb01(path)
        assert bits == 8 and t.dtype == torch.float32 and torch.equal(t, imread_rgb01(path)), name
        g, was_grey, bits = imread16_grey01(path)
        want, want_grey = imread_grey01(path)
        assert bits == 8 and was_grey == want_grey and g.dtype == torch.float32 and torch.equal(g, want), name


def test_imread16_reads_sample_over_65535(tmp_path):
    from PIL import Image
    from ciaosr_amd.imageio import imread16_grey01, imread16_rgb01
    rgb = ref.make16(7, 9, 3, 'noise')
    rgb[0, 0], rgb[0, 1], rgb[0, 2] = (65535, 65535, 65535), (0, 0, 0), (1, 2, 65534)
    as_f32 = lambda a: torch.from_numpy((a.astype(np.float64) / 65535).astype(np.float32))     # fp32(sample / 65535), by way of float64
    path = _write(tmp_path, 'rgb16.png', ref.write_png16(rgb))
    with Image.open(path) as f:
        assert f.mode == 'RGB'                                # what Pillow makes of it: 8 bits, the reason for read_png16
    t, bits = imread16_rgb01(path)
    assert bits == 16 and t.dtype == torch.float32 and tuple(t.shape) == (3, 7, 9)
    assert torch.equal(t, as_f32(rgb).permute(2, 0, 1))
    truncated = torch.from_numpy((rgb >> 8).astype(np.float32) / 255).permute(2, 0, 1)
    assert not torch.equal(t, truncated)
    # a 16-bit RGB file read as grey: the L16 formula on the samples
    g, was_grey, bits = imread16_grey01(path)
    l16 = ref.grey16(rgb[:, :, ::-1])
    assert bits == 16 and not was_grey and tuple(g.shape) == (1, 7, 9) and torch.equal(g[0], as_f32(l16))
    assert l16[0, 0] == 65535 and l16[0, 1] == 0
    # 16-bit grey: a PNG through read_png16, a TIFF through Pillow's I;16
    grey = ref.make16(7, 9, 1, 'bytes')
    for name in ('g.png', 'g.tif'):
        path = str(tmp_path / name)
        Image.fromarray(grey).save(path)
        g, was_grey, bits = imread16_grey01(path)
        assert bits == 16 and was_grey and torch.equal(g[0], as_f32(grey)), name
        t, bits = imread16_rgb01(path)
        assert bits == 16 and all(torch.equal(t[k], as_f32(grey)) for k in range(3)), name
    neutral = np.repeat(grey[:, :, None], 3, axis=2)
    g, was_grey, _ = imread16_grey01(_write(tmp_path, 'n.png', ref.write_png16(neutral)))
    assert was_grey and torch.equal(g[0], as_f32(grey))       # a neutral (v, v, v) gives v


def test_k_over_255_is_257_k_over_65535():
    k = np.arange(256)
    a = (k.astype(np.float64) / 255).astype(np.float32)
    b = ((257 * k).astype(np.float64) / 65535).astype(np.float32)
    assert np.array_equal(a, b)
    t = torch.from_numpy(a)
    assert np.array_equal(ref.q16(t).numpy(), 257 * k)


# -- the container ---------------------------------------------------------------------------------------------------------------------
def test_container_depth():
    from ciaosr_amd import png_hip
    z = b'\x78\x01\x03\x00\x00\x00\x00\x01'
    for kw, colour_type in ((dict(), 2), (dict(grey=True), 0)):
        png = png_hip.container(33, 17, z, depth=16, **kw)
        assert ref.ihdr(png) == (17, 33, 16, colour_type, 0, 0, 0) and ref.idat(png) == z
        assert png_hip.container(33, 17, z, depth=8, **kw) == png_hip.container(33, 17, z, **kw)
        assert ref.ihdr(png_hip.container(33, 17, z, **kw)) == (17, 33, 8, colour_type, 0, 0, 0)
    # without `depth`: today's bytes, written out here
    import struct
    import zlib
    ch = lambda tag, d: struct.pack('>I', len(d)) + tag + d + struct.pack('>I', zlib.crc32(tag + d) & 0xffffffff)
    for kw, colour_type in ((dict(), 2), (dict(channels=4), 6), (dict(grey=True), 0)):
        want = b'\x89PNG\r\n\x1a\n' + ch(b'IHDR', struct.pack('>IIBBBBB', 17, 33, 8, colour_type, 0, 0, 0)) + ch(b'IDAT', z) + ch(b'IEND', b'')
        assert png_hip.container(33, 17, z, **kw) == want
    for bad in (0, 1, 4, 12, 15, 32, '16', None, True, 16.5):
        with pytest.raises(ValueError):
            png_hip.container(33, 17, z, depth=bad)
    with pytest.raises(ValueError, match='alpha'):
        png_hip.container(33, 17, z, channels=4, depth=16)


# -- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_size_functions_refuse():
    from ciaosr_amd import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read(), flags=re.S)
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert lib.ciaosr_version() >= 350
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r'\b' + name + r'\s*\(', header), name
        assert 'png_' not in name and 'deflate_' not in name and 'jpeg_' not in name, name
    assert 'ciaosr_png16_' in integration and 'ciaosr_tensor2img_u16' in integration
    for pre, bpp, namesake in (('ciaosr_png16_', 6, 'ciaosr_png_'), ('ciaosr_png16_grey_', 2, 'ciaosr_png_grey_')):
        sigs = {**_lib.SIGNATURES, **_lib.GREY_PNG_SIGNATURES}
        for n in FAMILY:
            assert _lib.SIGNATURES[pre + n] == sigs[namesake + n.replace('_u16', '_u8')], pre + n
        f = lambda n: getattr(lib, pre + n)
        for w in (0, 65536, -1):
            assert f('rows_per_band')(w, 0) == 0
            for n in ('workspace_bytes', 'lz_workspace_bytes', 'capacity_bytes'):
                assert f(n)(10, w, 0) == 0 and f(n)(w, 10, 0) == 0, (pre, n, w)
            rect = (C.c_int * 4)(0, 0, 10, w)
            for n in ('tiles_workspace_bytes', 'lz_tiles_workspace_bytes', 'tiles_capacity_bytes'):
                assert f(n)(rect, 1, 0) == 0, (pre, n, w)
        assert f('rows_per_band')(65535, 0) == 1 and f('rows_per_band')(17, 0) == 131072 // (bpp * 17 + 1) and f('rows_per_band')(17, 5) == 5
        assert f('workspace_bytes')(10, 10, -1) == 0
        # sizes: the filtered image lies in the workspace, the capacity is the all-stored worst case of its bytes
        total = 33 * (bpp * 17 + 1)
        assert f('workspace_bytes')(33, 17, 5) >= total and f('lz_workspace_bytes')(33, 17, 5) >= f('workspace_bytes')(33, 17, 5) + 2 * total
        assert f('capacity_bytes')(33, 17, 5) >= total + 5 * 7 + 6
        rect = (C.c_int * 4)(3, 5, 33, 17)
        assert f('tiles_capacity_bytes')(rect, 1, 5) == f('capacity_bytes')(33, 17, 5)


# -- the reference's filter coverage on the GPU tests' contents ---------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
def test_reference_chooses_every_filter(c):
    seen = {}
    for h, w in FILTER_SIZES:
        for content in ref.CONTENTS:
            for k in ref.filter_rows(ref.make16(h, w, c, content))[1]:
                seen.setdefault(k, set()).add(content)
    assert sorted(seen) == [0, 1, 2, 3, 4], seen
    # the ramp whose low byte wraps while its high byte steps
    ramp = ref.make16(9, 300, c, 'wrap_ramp')
    rows = ref.byte_rows(ramp)
    lo, hi = rows[0, 1::2].astype(int), rows[0, 0::2].astype(int)
    step = slice(None, None, c)
    assert (np.diff(lo[step]) < 0).any() and (np.diff(hi[step]) > 0).any()
    assert set(ref.filter_rows(ramp)[1][0::2]) == {1}          # the ramp rows: Sub, per BYTE -- low bytes 37, high bytes 0 or 1, no borrow
    sub = ref.filter_rows(ramp, 1)[0].reshape(9, -1)[0, 1 + 2 * c:]
    assert set(sub[1::2].tolist()) == {37} and set(sub[0::2].tolist()) == {0, 1}
    # a filter that subtracted 16-bit samples and split the difference would write other bytes
    v = ramp.astype(np.int64).reshape(9, -1)
    left = np.zeros_like(v)
    left[:, c:] = v[:, :-c]
    d = (v - left) % 65536
    borrowed = np.stack([d >> 8, d & 255], axis=-1).reshape(9, -1)
    assert not np.array_equal(borrowed, ref.filter_rows(ramp, 1)[0].reshape(9, -1)[:, 1:])


def test_reference_rows_are_big_endian():
    img = np.array([[0x1234, 0xFF01]], dtype=np.uint16)
    assert ref.byte_rows(img).tolist() == [[0x12, 0x34, 0xFF, 0x01]]
    rgb = np.array([[[0x0102, 0x0304, 0x0506]]], dtype=np.uint16)
    assert ref.byte_rows(rgb).tolist() == [[1, 2, 3, 4, 5, 6]]
    assert ref.filter_rows(rgb, 0)[0].tolist() == [0, 1, 2, 3, 4, 5, 6]
    b = ref.make16(5, 7, 3, 'bytes')
    assert ((b >> 8) != (b & 255)).all() and ((b >> 8) != 255 - (b & 255)).all()


# -- tools/render.py --depth16 ---------------------------------------------------------------------------------------------------------
def test_render_cli_depth16_refusals(capsys):
    from tools import render
    base = ['cfg.py', 'None', 'img.png', '--scale', '2', '--out', 'out', '--depth16']
    for extra in (['--jpeg', '90'], ['--alpha'], ['--dzi', '2'], ['--niqe', 'params.npz']):
        with pytest.raises(SystemExit) as e:
            render.parse_args(base + extra)
        assert e.value.code == 2 and '--depth16' in capsys.readouterr().err
    args = render.parse_args(base + ['--grey', '--png-matches', '--self-ensemble', '--window', '1', '2', '3', '4'])
    assert args.depth16 and args.grey and args.png_matches and args.self_ensemble
    assert render.parse_args(base + ['--png-matches']).png_matches            # --depth16 implies the device coder
    assert not render.parse_args(base[:-1]).depth16
