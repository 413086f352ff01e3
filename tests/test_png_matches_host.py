"""Host tests of the PNG coder's opt-in LZ77 matches: the restatement of the contract (tests/png_match_ref.py) against itself and
`zlib`, the ABI surface, and the argument errors that come before any device work.  No GPU.
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from tests import png_match_ref as mref
from tests import png_reference as ref
from tests import rgba_ref
from tests.test_rgba_host import no_library                    # noqa: F401  (a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['ciaosr_png_lz_workspace_bytes', 'ciaosr_png_lz_encode_u8', 'ciaosr_png_lz_tiles_workspace_bytes',
               'ciaosr_png_lz_encode_tiles_u8', 'ciaosr_png_rgba_lz_workspace_bytes', 'ciaosr_png_rgba_lz_encode_u8',
               'ciaosr_png_rgba_lz_tiles_workspace_bytes', 'ciaosr_png_rgba_lz_encode_tiles_u8', 'ciaosr_deflate_lz_workspace_bytes',
               'ciaosr_deflate_lz_u8']


def _buffers():
    rng = np.random.RandomState(1)
    periodic = bytes(range(7)) * 1500
    return dict(random=rng.randint(0, 256, 9000, dtype=np.uint8).tobytes(), periodic=periodic, zeros=b'\x00' * 10000,
                few=(rng.randint(0, 2, 12000) * 9).astype(np.uint8).tobytes(), one=b'x', rows=(b'\x01' + bytes(range(40))) * 300)


@pytest.mark.parametrize('name', ['random', 'periodic', 'zeros', 'few', 'one', 'rows'])
@pytest.mark.parametrize('line,bpp', [(0, 1), (41, 4), (7, 3)])
def test_the_parse_expands_to_its_input(name, line, bpp):
    data = _buffers()[name]
    tokens = mref.parse(data, line, bpp)
    assert mref.expand(tokens) == data
    allowed = set(mref.distances(line, bpp))
    at = 0
    for t in tokens:
        if isinstance(t, tuple):
            length, d = t
            assert 8 <= length <= 258 and d in allowed and d <= at
            assert at // mref.CHUNK == (at + length - 1) // mref.CHUNK             # no match crosses a parse chunk
            at += length
        else:
            at += 1
    repeats = name == 'zeros' or (name, line) in (('periodic', 7), ('rows', 41))       # the period is a candidate distance
    if repeats:
        assert sum(isinstance(t, tuple) for t in tokens) >= len(data) // 258
        assert mref.model_bits(tokens) < ref.band_model_bits(data)[0] // 4
    if name in ('random', 'periodic', 'rows') and not repeats:
        assert not any(isinstance(t, tuple) for t in tokens)
    if name == 'periodic' and line == 7:
        assert {t[1] for t in tokens if isinstance(t, tuple)} == {7}                 # 4 = line - bpp does not repeat; 7 = line does
    if name == 'zeros':
        assert tokens[:3] == [0, (258, 1), (258, 1)] and tokens[-3:] == [(258, 1), 0, 0]    # the last chunk: 1808 = 7 x 258 + 2


def test_ties_go_to_the_earliest_candidate():
    data = b'ab' * 40
    assert mref.parse(data, 0, 1)[:3] == [ord('a'), ord('b'), (78, 2)]                # 2, 4, 6, 8, 12, 16 all reach the end: 2 wins
    assert mref.parse(b'q' + data, 4, 2)[:4] == [ord('q'), ord('a'), ord('b'), (78, 2)]


@pytest.mark.parametrize('level', [1, 6, 9])
def test_the_token_inflate_agrees_with_zlib(level):
    rng = np.random.RandomState(level)
    img = (np.add.outer(np.arange(120), np.arange(160)) // 3 % 256).astype(np.uint8)[:, :, None].repeat(3, axis=2)
    img[40:80] += rng.randint(0, 3, (40, 160, 3)).astype(np.uint8)
    data = ref.filter_stream(img)[0] + rng.randint(0, 256, 3000, dtype=np.uint8).tobytes() + b'\x00' * 5000
    z = zlib.compress(data, level)
    blocks, out, end = mref.inflate_tokens(z, 2)
    assert out == zlib.decompress(z) == data and end == len(z) - 4
    assert blocks[-1]['final'] == 1 and all(b['final'] == 0 for b in blocks[:-1])
    assert mref.expand([t for b in blocks for t in b['tokens']]) == data
    assert any(isinstance(t, tuple) for b in blocks for t in b['tokens'])
    stored = zlib.compress(data[:70000], 0)
    blocks, out, _ = mref.inflate_tokens(stored, 2)
    assert out == data[:70000] and {b['type'] for b in blocks} == {0}


def test_the_sprite_fixture_leaves_the_gate_room():
    """The size gate of the GPU tests holds the device file of the 256 x 256 sprite to Pillow's: the model itself must be well below."""
    from tests.test_png_matches_gpu import _pil_size, sprite0
    img = sprite0(256, 256)
    stream = rgba_ref.filter_rows(img)[0].tobytes()
    line = 1 + 4 * 256
    offs = ref.band_split(256, line, rgba_ref.rows_per_band(256))
    model = mref.model_bytes(stream, offs, line, 4) + ref.png_overhead()
    assert model < 0.97 * _pil_size(img), (model, _pil_size(img))


def test_abi_surface():
    from ciaosr_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    doc = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + '(' in header and name in doc, name
    # the old entry points keep their signatures
    assert _lib.SIGNATURES['ciaosr_png_lz_encode_u8'] == _lib.SIGNATURES['ciaosr_png_encode_u8']
    assert _lib.SIGNATURES['ciaosr_png_rgba_lz_encode_tiles_u8'] == _lib.SIGNATURES['ciaosr_png_encode_tiles_u8']
    assert len(_lib.SIGNATURES['ciaosr_deflate_lz_u8'][1]) == len(_lib.SIGNATURES['ciaosr_deflate_huff_u8'][1]) + 2


def test_workspace_is_monotone_and_never_zero_where_the_parent_codes():
    from ciaosr_amd import _lib
    lib = _lib.load()
    for bpp, pre in ((3, 'ciaosr_png_'), (4, 'ciaosr_png_rgba_')):
        lz, lit = getattr(lib, pre + 'lz_workspace_bytes'), getattr(lib, pre + 'workspace_bytes')
        for rows in (0, 1, 7):
            prev = 0
            for h, w in [(1, 1), (1, 300), (33, 17), (256, 384), (300, 1), (1024, 1024), (5424, 8160), (65535, 3), (3, 65535)]:
                got, base = lz(h, w, rows), lit(h, w, rows)
                assert base > 0 and got >= base + 2 * h * (bpp * w + 1), (h, w, rows)        # 16 bits of token per filtered byte
            for h in (1, 2, 50, 51, 400, 4000):
                got = lz(h, 333, rows)
                assert got > prev, (h, rows)
                prev = got
        assert lz(0, 4, 0) == 0 and lz(4, 65536, 0) == 0 and lz(4, 4, -1) == 0
        rects = (C.c_int * 12)(0, 0, 5, 7, 3, 3, 200, 300, 9, 9, 1, 1)
        tl, tp = getattr(lib, pre + 'lz_tiles_workspace_bytes'), getattr(lib, pre + 'tiles_workspace_bytes')
        assert tl(rects, 3, 0) > tl(rects, 2, 0) > tl(rects, 1, 0) >= tp(rects, 1, 0) + 2 * 5 * (7 * bpp + 1)
        assert tl(rects, 3, 0) >= tp(rects, 3, 0) + 2 * (5 * (7 * bpp + 1) + 200 * (300 * bpp + 1) + bpp + 1)
        bad = (C.c_int * 4)(0, 0, 0, 7)
        assert tl(bad, 1, 0) == 0 and tp(bad, 1, 0) == 0
    f = lib.ciaosr_deflate_lz_workspace_bytes
    assert f(C.c_size_t(1), 1) > 0 and f(C.c_size_t(0), 1) == 0 and f(C.c_size_t(10), 0) == 0
    assert f(C.c_size_t(1 << 20), 3) > f(C.c_size_t(1 << 19), 3) > f(C.c_size_t(1 << 19), 2) >= (1 << 20)


def test_bad_arguments_are_refused_before_any_launch():
    """The library's "bad argument" status for the new entry points: null pointers and a line that is no line."""
    from ciaosr_amd import _lib
    from ciaosr_amd._lib import CiaoSRHipError
    _lib.load()
    offs = (C.c_ulonglong * 2)(0, 10)
    one = C.c_void_p(256)                                             # aligned, never dereferenced: the arguments are refused first
    for line, bpp in ((-1, 1), (5, 0), (3, 3), (2, 4)):
        with pytest.raises(CiaoSRHipError, match='bad argument'):
            _lib.call('ciaosr_deflate_lz_u8', one, offs, 1, line, bpp, one, C.c_size_t(1 << 20), one, one, C.c_size_t(1 << 20), None)
    with pytest.raises(CiaoSRHipError, match='bad argument'):
        _lib.call('ciaosr_deflate_lz_u8', None, offs, 1, 0, 1, one, C.c_size_t(1 << 20), one, one, C.c_size_t(1 << 20), None)
    with pytest.raises(CiaoSRHipError, match='bad argument'):
        _lib.call('ciaosr_png_lz_encode_u8', None, C.c_size_t(12), 4, 4, 0, 0, one, C.c_size_t(1 << 20), one, one, C.c_size_t(1 << 20), None)
    with pytest.raises(CiaoSRHipError, match='bad argument'):
        _lib.call('ciaosr_png_rgba_lz_encode_tiles_u8', one, C.c_size_t(16), 4, 4, 0, None, 1, 0, one, C.c_size_t(1 << 20), one, one,
                  C.c_size_t(1 << 20), None)


def test_value_errors_before_the_library(no_library, tmp_path):        # noqa: F811
    import torch
    from ciaosr_amd import png_hip, pyramid
    img = torch.zeros(4, 4, 3, dtype=torch.uint8)
    for bad in (1, 0, None, 'yes', np.bool_(True)):
        for fn in (lambda: png_hip.encode_zlib(img, matches=bad), lambda: png_hip.encode_png(img, matches=bad),
                   lambda: png_hip.encode_tiles_device(img, [(0, 0, 2, 2)], matches=bad),
                   lambda: png_hip.encode_zlib_tiles(img, [(0, 0, 2, 2)], matches=bad),
                   lambda: png_hip.encode_png_tiles(img, [(0, 0, 2, 2)], matches=bad),
                   lambda: png_hip.imwrite_gpu(img, str(tmp_path / 'x.png'), matches=bad),
                   lambda: png_hip.deflate_huff(img.reshape(-1), [0, 48], matches=bad),
                   lambda: pyramid.write_levels([img], str(tmp_path / 'p'), 'p', matches=bad),
                   lambda: pyramid.write_dzi(None, None, str(tmp_path / 'p'), 'p', scale=2, matches=bad)):
            with pytest.raises(ValueError, match='matches'):
                fn()
    with pytest.raises(ValueError, match='matches'):
        pyramid.write_levels([img], str(tmp_path / 'p'), 'p', fmt='jpg', matches=True)
    with pytest.raises(ValueError, match='matches'):
        pyramid.write_dzi(None, None, str(tmp_path / 'p'), 'p', scale=2, fmt='jpg', matches=True)
    for line, bpp in ((-1, 1), (5, 0), (3, 3)):
        with pytest.raises(ValueError, match='line'):
            png_hip.deflate_huff(img.reshape(-1), [0, 48], matches=True, line=line, bpp=bpp)
    assert not (tmp_path / 'p').exists() and not (tmp_path / 'x.png').exists()


def test_cli_flags(capsys):
    import ciaosr_amd
    import tools.test as cli
    from ciaosr_amd.config import Config
    from tools import render
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    for argv, png, lz in ([], False, False), (['--gpu-png'], True, False), (['--gpu-png-matches'], True, True):
        cfg = cli.apply_overrides(Config.fromfile(path), cli.parse_args([path, 'None'] + argv))
        model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        assert model.gpu_png() is png and model.gpu_png_matches() is lz
    model.test_cfg['gpu_png'] = False
    assert model.gpu_png_matches() is False                            # only read with gpu_png
    base = ['cfg.py', 'None', 'img.png', '--scale', '2', '--out', 'o']
    assert not render.parse_args(base).png_matches
    assert render.parse_args(base + ['--gpu-png', '--png-matches']).png_matches
    assert render.parse_args(base + ['--alpha', '--png-matches']).png_matches
    for bad in (['--png-matches'], ['--png-matches', '--jpeg', '90'], ['--png-matches', '--gpu-png', '--jpeg', '90']):
        with pytest.raises(SystemExit):
            render.parse_args(base + bad)
        assert '--png-matches' in capsys.readouterr().err
    assert '--png-matches' in render.__doc__
