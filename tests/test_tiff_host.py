"""Pyramidal tiled TIFF, host side (no GPU): the container `tiff_hip.plan_file` lays out, read by Pillow and by the reference reader of
tests/tiff_ref.py (itself held to Pillow here); the level sizes; the 4 GiB refusal from lengths alone; every ValueError of the public
path before any device work; the new exports against the header and their refusals; the refusals of tools/render.py --tiff.
"""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import tiff_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (16, 16), (17, 33), (77, 131)]
TILES = [16, 32]
PILLOW_MODES = {'rgb8': 'RGB', 'grey8': 'L', 'grey16': 'I;16', 'rgba8': 'RGBA'}
NEW_EXPORTS = ['ciaosr_tiff_rows_per_band', 'ciaosr_tiff_tiles_workspace_bytes', 'ciaosr_tiff_lz_tiles_workspace_bytes',
               'ciaosr_tiff_tiles_capacity_bytes', 'ciaosr_tiff_encode_tiles', 'ciaosr_tiff_lz_encode_tiles', 'ciaosr_halve_box_u16']


def planned_file(levels, tile, level=6):
    """The file of the numpy `levels` (stream order): `plan_file` around zlib.compress of the reference's tile bytes -> (bytes, plan)"""
    from ciaosr_amd import tiff_hip
    streams = [[zlib.compress(t, level) for t in ref.tiles_bytes(lv, tile)] for lv in levels]
    plan = tiff_hip.plan_file([ref.meta_of(lv, tile) for lv in levels], [[len(z) for z in zs] for zs in streams])
    out = bytearray(plan['header'])
    for lv, zs in zip(plan['levels'], streams):
        for off, z in zip(lv['tile_offsets'], zs):
            out += b'\0' * (off - len(out))
            assert len(out) == off
            out += z
        out += b'\0' * (lv['extra_offset'] - len(out))
        assert len(out) == lv['extra_offset']
        out += lv['extra']
        assert len(out) == lv['ifd_offset']
        out += lv['ifd']
    assert len(out) == plan['total']
    return bytes(out), plan


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('kind', ref.KINDS)
def test_pillow_and_the_reference_reader_read_the_planned_file(kind, h, w, tile):
    from ciaosr_amd import tiff_hip
    levels = ref.pyramid_of(ref.make_image(h, w, kind, seed=tile), tile)
    assert [lv.shape[:2] for lv in levels] == tiff_hip.tiff_level_sizes(h, w, tile) == ref.level_sizes(h, w, tile)
    data, plan = planned_file(levels, tile)
    # the structure: exactly the contract's tags, ascending (the reader asserts that), every offset even
    ifds = ref.read_ifds(data)
    assert len(ifds) == len(levels)
    samples = ref.kind_shape(kind)[0]
    want_tags = [t for t in tiff_hip.TAGS if t != 338 or samples == 4]
    for k, (off, tags) in enumerate(ifds):
        assert sorted(tags) == want_tags and off % 2 == 0 and off == plan['levels'][k]['ifd_offset']
        assert tags[254][1] == [1 if k else 0] and tags[324][0] == tags[325][0] == 4                     # LONG
        assert all(o % 2 == 0 for o in tags[324][1]) and tags[324][1] == plan['levels'][k]['tile_offsets']
        assert plan['levels'][k]['extra_offset'] % 2 == 0
    # the reference reader returns every level bit for bit
    got = ref.read_tiff(data)
    assert len(got) == len(levels)
    for a, b in zip(got, levels):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    # Pillow: the kinds it reads bit for bit; RGB 16 it opens (as 8-bit RGB), page count and sizes only
    pages = ref.pillow_pages(data)
    assert len(pages) == len(levels)
    for page, lv in zip(pages, levels):
        assert page.shape[:2] == lv.shape[:2]
        if kind in PILLOW_MODES:
            assert page.dtype == lv.dtype and np.array_equal(page, lv), kind
    if kind in PILLOW_MODES:
        import io
        from PIL import Image
        assert Image.open(io.BytesIO(data)).mode == PILLOW_MODES[kind]


def test_reference_predictor_works_on_samples_and_stores_low_byte_first():
    p = np.array([[[0], [65535], [0], [0x1234]]], dtype=np.uint16).repeat(1, axis=0)
    tile = np.zeros((4, 4, 1), dtype=np.uint16)
    tile[:] = p
    raw = ref.predicted_bytes(tile)
    assert list(raw[:8]) == [0, 0, 0xFF, 0xFF, 0x01, 0x00, 0x34, 0x12]           # 0, 65535 - 0, 0 - 65535 = 1, 0x1234 - 0
    bytewise = np.frombuffer(tile.tobytes(), dtype=np.uint8).reshape(4, 8).astype(int)
    d = bytewise.copy()
    d[:, 2:] = (bytewise[:, 2:] - bytewise[:, :-2]) % 256
    assert bytes(d.astype(np.uint8).reshape(-1)) != raw                          # a predictor on bytes writes other bytes
    assert np.array_equal(ref.unpredict(raw, 4, 1, 16), tile)
    rgb = ref.make_image(5, 7, 'rgb16')
    assert np.array_equal(ref.unpredict(ref.predicted_bytes(ref.padded_tile(rgb, 0, 0, 16)), 16, 3, 16)[:5, :7], rgb)


def test_reference_padding_and_halving():
    img = ref.make_image(5, 7, 'rgb8')
    p = ref.padded_tile(img, 0, 0, 16)
    assert np.array_equal(p[:5, :7], img) and (p[5:] == p[4]).all() and (p[:, 7:] == p[:, 6:7]).all()
    a = np.array([[0, 1, 65535], [2, 3, 65535], [65535, 65534, 1]], dtype=np.uint16)
    assert ref.halve_box(a).tolist() == [[(0 + 1 + 2 + 3 + 2) >> 2, 65535], [(65535 + 65534 + 65535 + 65534 + 2) >> 2, 1]]
    assert ref.halve_box(np.array([[7, 8, 10]], dtype=np.uint16)).tolist() == [[(7 + 8 + 7 + 8 + 2) >> 2, 10]]
    assert ref.halve_box(np.array([[9]], dtype=np.uint16)).tolist() == [[9]]


def test_level_sizes():
    from ciaosr_amd import pyramid, tiff_hip
    f = tiff_hip.tiff_level_sizes
    assert f(1, 1, 16) == [(1, 1)] and f(16, 16, 16) == [(16, 16)] and f(256, 100, 256) == [(256, 100)]
    assert f(17, 33, 16) == [(17, 33), (9, 17), (5, 9)]
    assert f(77, 131, 32) == [(77, 131), (39, 66), (20, 33), (10, 17)]
    assert f(5424, 8160) == [(5424, 8160), (2712, 4080), (1356, 2040), (678, 1020), (339, 510), (170, 255)]
    assert f(1, 1025, 256) == [(1, 1025), (1, 513), (1, 257), (1, 129)]
    for h, w, t in ((77, 131, 32), (1001, 3, 16), (5424, 8160, 256)):
        sizes = f(h, w, t)
        assert sizes == pyramid.level_sizes(h, w)[::-1][:len(sizes)]             # the sizes render_pyramid renders, top first
        assert max(sizes[-1]) <= t and all(max(s) > t for s in sizes[:-1])
    for bad in ((0, 5), (5, 0)):
        with pytest.raises(ValueError):
            f(*bad, 16)


def test_plan_file_refuses_4gib_from_lengths_alone():
    from ciaosr_amd import tiff_hip
    meta = dict(height=64, width=64, samples=3, bits=8, tile=32)
    ok = tiff_hip.plan_file([meta], [[1 << 30, 1 << 30, 1 << 30, (1 << 30) - 4096]])
    assert ok['total'] <= tiff_hip.MAX_OFFSET and ok['levels'][0]['tile_offsets'][3] == 8 + 3 * (1 << 30)
    with pytest.raises(ValueError, match='2\\^32'):
        tiff_hip.plan_file([meta], [[1 << 30] * 4])
    small = dict(height=32, width=32, samples=3, bits=8, tile=32)
    with pytest.raises(ValueError, match='2\\^32'):                               # the second level's IFD would lie past the limit
        tiff_hip.plan_file([meta, small], [[1 << 30, 1 << 30, 1 << 30, (1 << 30) - 4096], [8192]])
    with pytest.raises(ValueError):                                              # the wrong number of tiles
        tiff_hip.plan_file([meta], [[10, 10, 10]])
    with pytest.raises(ValueError):
        tiff_hip.plan_file([meta, small], [[10, 10, 10, 10]])
    for bad in (dict(meta, samples=2), dict(meta, bits=12), dict(meta, samples=4, bits=16), dict(meta, tile=24)):
        with pytest.raises(ValueError):
            tiff_hip.plan_file([bad], [[10, 10, 10, 10]])
    odd = tiff_hip.plan_file([meta], [[3, 5, 8, 1]])                             # odd lengths: the next tile moves to an even offset
    assert odd['levels'][0]['tile_offsets'] == [8, 12, 18, 26] and odd['levels'][0]['extra_offset'] == 28


class _Enc:
    def __init__(self, alpha=False, grey=False):
        self.alpha, self.grey = alpha, grey


def test_value_errors_before_any_device_work(tmp_path):
    from ciaosr_amd import pyramid, scene, tiff_hip
    from ciaosr_amd._lib import CiaoSRHipError
    for bad in (0, 8, 15, 24, 250, 4097, 4112, -16, 16.0, '256', None, True):
        with pytest.raises(ValueError, match='tile'):
            tiff_hip.check_tile(bad)
        with pytest.raises(ValueError, match='tile'):
            pyramid.check_tiff(_Enc(), tile=bad)
        with pytest.raises(ValueError, match='tile'):
            tiff_hip.tiff_level_sizes(10, 10, bad)
    for good in (16, 32, 256, 4096):
        assert tiff_hip.check_tile(good) == good
    with pytest.raises(ValueError, match='alpha'):
        pyramid.check_tiff(_Enc(alpha=True), depth=16)
    with pytest.raises(ValueError, match='grey'):
        pyramid.check_tiff(_Enc(alpha=True, grey=True))
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='matches'):
            pyramid.check_tiff(_Enc(), matches=bad)
        with pytest.raises(ValueError, match='matches'):
            tiff_hip.encode_tiff_tiles(torch.zeros(4, 4, 3, dtype=torch.uint8), matches=bad)
    for bad in (12, '8', True, None):
        with pytest.raises(ValueError, match='depth'):
            pyramid.check_tiff(_Enc(), depth=bad)
    ens = scene.EnsembleEncoded((0, 1), [None, None], (1, 3, 8, 8))
    with pytest.raises(ValueError, match='ensemble'):
        pyramid.check_tiff(ens)
    pyramid.check_tiff(_Enc()), pyramid.check_tiff(_Enc(grey=True), depth=16, matches=True), pyramid.check_tiff(_Enc(alpha=True))
    # write_tiff raises them itself, with a model that must not be touched
    with pytest.raises(ValueError, match='tile'):
        pyramid.write_tiff(None, _Enc(), str(tmp_path / 'a.tif'), scale=2, tile=100)
    with pytest.raises(ValueError, match='alpha'):
        pyramid.write_tiff(None, _Enc(alpha=True), str(tmp_path / 'a.tif'), scale=2, depth=16)
    with pytest.raises(ValueError, match='ensemble'):
        pyramid.write_tiff(None, ens, str(tmp_path / 'a.tif'), scale=2)
    assert not os.path.exists(str(tmp_path / 'a.tif'))
    # images: a wrong order and a wrong tile are ValueErrors, a host array raises (no CPU fallback), no 16-bit alpha
    host = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        tiff_hip.encode_tiff_tiles(host, order='grb')
    with pytest.raises(ValueError, match='tile'):
        tiff_hip.encode_tiff_tiles(host, tile=20)
    for call in (lambda: tiff_hip.encode_tiff_tiles(host), lambda: tiff_hip.encode_tiff([host]),
                 lambda: tiff_hip.imwrite_gpu_tiff(host, str(tmp_path / 'b.tif')),
                 lambda: tiff_hip.imwrite_gpu_tiff(np.zeros((4, 4, 3), np.uint8), str(tmp_path / 'b.tif')),
                 lambda: tiff_hip.encode_tiff_tiles(torch.zeros(4, 4, 4, dtype=torch.uint16)),
                 lambda: tiff_hip.halve_box_u16(torch.zeros(4, 4, dtype=torch.uint16))):
        with pytest.raises(CiaoSRHipError):
            call()
    assert not os.path.exists(str(tmp_path / 'b.tif'))
    with pytest.raises(ValueError):
        tiff_hip.halve_box_u16(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='halving'):
        tiff_hip.encode_tiff([torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(5, 4, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match='kind'):
        tiff_hip.encode_tiff([torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        tiff_hip.encode_tiff([])


def test_new_exports_are_declared_and_refuse():
    from ciaosr_amd import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read(), flags=re.S)
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert lib.ciaosr_version() >= 360
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r'\b' + name + r'\s*\(', header), name
        assert 'png_' not in name and 'deflate_' not in name and 'jpeg_' not in name, name
        assert name in integration, name
    rows, cap = lib.ciaosr_tiff_rows_per_band, lib.ciaosr_tiff_tiles_capacity_bytes
    sizes = (lib.ciaosr_tiff_tiles_workspace_bytes, lib.ciaosr_tiff_lz_tiles_workspace_bytes, cap)
    assert rows(3, 256, 0) == 131072 // 768 and rows(3, 256, 5) == 5 and rows(1, 16, 0) == 16 and rows(6, 4096, 0) == 5
    assert rows(3, 32, 100) == 32                                                # at most the tile
    for bpp in (0, 5, 7, 8, -1):
        assert rows(bpp, 256, 0) == 0 and all(f(bpp, 64, 64, 32, 0) == 0 for f in sizes)
    for tile in (0, 8, 24, 4112, -16):
        assert rows(3, tile, 0) == 0 and all(f(3, 64, 64, tile, 0) == 0 for f in sizes)
    for side in (0, -1, 65536):
        assert all(f(3, side, 64, 32, 0) == 0 and f(3, 64, side, 32, 0) == 0 for f in sizes)
    assert rows(3, 32, -1) == 0 and all(f(3, 64, 64, 32, -1) == 0 for f in sizes)
    # sizes: the predicted tiles lie in the workspace (padding included), the capacity is their all-stored worst case
    for bpp in (1, 2, 3, 4, 6):
        total = 3 * 5 * 32 * 32 * bpp                                            # a 77 x 131 level at T = 32: 3 x 5 tiles
        ws, lz = lib.ciaosr_tiff_tiles_workspace_bytes(bpp, 77, 131, 32, 5), lib.ciaosr_tiff_lz_tiles_workspace_bytes(bpp, 77, 131, 32, 5)
        assert ws >= total and lz >= ws + 2 * total
        assert cap(bpp, 77, 131, 32, 5) >= total + 15 * (5 * 7 + 6)
    # the calls refuse bad arguments with an error code before any launch (null pointers, a bad tile, a bad pixel size)
    null = C.c_void_p(0)
    one = C.c_void_p(256)                                                        # never dereferenced: the checks come first
    args = lambda bpp=3, img=one, pitch=3 * 64, T=32, out=one, offs=one, ws=one: (
        bpp, img, C.c_size_t(pitch), 64, 64, 1, T, 0, out, C.c_size_t(1 << 20), offs, ws, C.c_size_t(1 << 20), null)
    for f in (lib.ciaosr_tiff_encode_tiles, lib.ciaosr_tiff_lz_encode_tiles):
        for bad in (args(bpp=5), args(img=null), args(T=24), args(out=null), args(offs=null), args(ws=null), args(pitch=100),
                    args(bpp=4, img=C.c_void_p(258), pitch=256), args(bpp=6, img=C.c_void_p(257), pitch=384), args(bpp=2, pitch=129)):
            assert f(*bad) == -1, bad
        assert f(*args()[:9], C.c_size_t(16), *args()[10:]) == -4                 # an output below the capacity: workspace error
        assert f(*args()[:12], C.c_size_t(16), null) == -4
    h = lib.ciaosr_halve_box_u16
    assert h(null, C.c_size_t(8), 2, 2, 1, one, C.c_size_t(2), null) == -1 and h(one, C.c_size_t(8), 2, 2, 2, one, C.c_size_t(2), null) == -1
    assert h(one, C.c_size_t(2), 2, 2, 1, one, C.c_size_t(2), null) == -1 and h(one, C.c_size_t(8), 2, 2, 1, one, C.c_size_t(1), null) == -1
    assert h(one, C.c_size_t(8), 0, 2, 1, one, C.c_size_t(2), null) == -1 and h(C.c_void_p(257), C.c_size_t(8), 2, 2, 1, one, C.c_size_t(2), null) == -1


def test_render_cli_tiff_refusals(capsys):
    from tools import render
    base = ['cfg.py', 'None', 'img.png', '--scale', '2', '--out', 'out', '--tiff']
    for extra in (['--jpeg', '90'], ['--view', '1', '2', '3', '4', '--size', '8', '8'], ['--window', '1', '2', '3', '4'],
                  ['--niqe', 'params.npz'], ['--self-ensemble'], ['--dzi', '2'], ['--tiff-tile', '100'], ['--tiff-tile', '8'],
                  ['--tiff-tile', '8192']):
        with pytest.raises(SystemExit) as e:
            render.parse_args(base + extra)
        assert e.value.code == 2 and '--tiff' in capsys.readouterr().err, extra
    for extra in (['--alpha', '--depth16'], ['--grey', '--alpha']):
        with pytest.raises(SystemExit):
            render.parse_args(base + extra)
        capsys.readouterr()
    with pytest.raises(SystemExit):
        render.parse_args(['cfg.py', 'None', 'img.png', '--dzi', '2', '--out', 'out', '--tiff'])         # no --scale to write
    capsys.readouterr()
    args = render.parse_args(base + ['--depth16', '--grey', '--png-matches', '--tiff-tile', '64'])
    assert args.tiff and args.tiff_tile == 64 and args.depth16 and args.grey and args.png_matches
    assert render.parse_args(base + ['--alpha', '--png-matches']).alpha
    assert render.parse_args(base + ['--png-matches']).png_matches               # --tiff implies the device coder
    assert render.parse_args(base).tiff_tile == 256 and not render.parse_args(base[:-1]).tiff
