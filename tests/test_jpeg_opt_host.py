"""Host-side tests of JPEG files with optimised Huffman tables (ciaosr_amd/jpeg_hip.py `optimize=True`): the plain
Python restatement of libjpeg's table rule (tests/jpeg_opt_ref.py) against Pillow's `optimize=True` files byte for byte, an image whose
Huffman trees are deeper than 16 levels before limiting, the header with tables of the caller's, the refusals, the CLI flag, the ABI
surface and the capacity formula.  Also the helpers that tests/test_jpeg_opt_gpu.py shares."""
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_opt_ref as opt
from tests.test_jpeg_host import CONTENTS, PIL_SUBSAMPLING, QUALITIES, SIZES, SUBSAMPLINGS, first_difference, make_image, segments

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_jpeg_opt(rgb, quality, subsampling):
    """Pillow's optimize=True file.  Pillow codes an optimised file into one buffer of max(ImageFile.MAXBLOCK, w h) bytes (2 w h from
    quality 95) and refuses ("broken data stream") what does not fit, as noise at quality 100 does not: the buffer is raised for the
    call.  A file that Pillow still refuses is an error."""
    import PIL.ImageFile
    from PIL import Image
    mp = pytest.MonkeyPatch()
    mp.setattr(PIL.ImageFile, 'MAXBLOCK', 1 << 24)
    try:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(rgb)).save(bio, format='JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[subsampling],
                                                        optimize=True)
    finally:
        mp.undo()
    return bio.getvalue()


def craft(h, w, seed, p):
    """An image whose blocks fall into classes of geometrically falling frequency and doubling amplitude, so that the AC symbols'
    frequencies fall off fast enough for Huffman trees deeper than 16 levels."""
    rng = np.random.RandomState(seed)
    cls = np.minimum(rng.geometric(p, (h // 8, w // 8)) - 1, 8)
    amp = np.where(cls == 0, 0.0, 2.0 ** (cls - 1)).repeat(8, axis=0).repeat(8, axis=1)[:, :, None]
    return np.clip(np.rint(128 + amp * rng.uniform(-1, 1, (h, w, 3))), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def crafted_image():
    return craft(512, 512, seed=1, p=0.4)


@functools.lru_cache(maxsize=None)
def crafted_want(subsampling):
    """(the file, the depths of its four trees before limiting) of the crafted image at quality 100; the file is Pillow's."""
    rgb = crafted_image()
    depths = opt.scan(rgb, 100, subsampling)[2]
    want = opt.encode(rgb, 100, subsampling)
    assert want == pil_jpeg_opt(rgb, 100, subsampling)
    return want, depths


def dht_tables(data):
    """The four (counts, symbols) pairs of a file's DHT segments, in the file's order."""
    dht = [p for m, p in segments(data)[0] if m == 0xc4]
    assert [p[0] for p in dht] == list(opt.TABLE_IDS)
    return [(tuple(p[1:17]), tuple(p[17:])) for p in dht]


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('content', CONTENTS)
def test_reference_is_pillows_optimised_file(content, subsampling):
    bad = []
    for h, w in SIZES:
        rgb = make_image(h, w, content)
        for q in QUALITIES:
            mine, pil = opt.encode(rgb, q, subsampling), pil_jpeg_opt(rgb, q, subsampling)
            if mine != pil:
                bad.append(f'{h}x{w} {content} q{q} {subsampling}: first difference at byte {first_difference(mine, pil)}, '
                           f'{len(mine)} against {len(pil)} bytes')
    assert not bad, '\n'.join(bad)


def test_pillows_buffer_rule_is_lifted():
    """160 x 200 noise at quality 100 in 4:4:4 is larger than 2 w h bytes: Pillow refuses it with its own buffer, writes it with the
    raised one, and the file is the reference's."""
    from PIL import Image
    rgb = make_image(160, 200, 'noise')
    with pytest.raises(OSError):
        Image.fromarray(rgb).save(io.BytesIO(), format='JPEG', quality=100, subsampling=0, optimize=True)
    pil = pil_jpeg_opt(rgb, 100, '444')
    assert len(pil) > 2 * 160 * 200 and pil == opt.encode(rgb, 100, '444')


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_length_limiting(subsampling):
    """The crafted image has a tree deeper than 16 levels in both subsamplings (4:4:4: 9 / 17 / 9 / 18, 4:2:0: 9 / 17 / 6 / 15 for the
    four tables), so the limiting step runs; every code of the file is at most 16 bits and the file is Pillow's."""
    want, depths = crafted_want(subsampling)
    print(subsampling, 'depths before limiting', depths)
    assert max(depths) > 16, depths
    assert depths == ([9, 17, 9, 18] if subsampling == '444' else [9, 17, 6, 15])
    for counts, symbols in dht_tables(want):
        assert len(counts) == 16 and sum(counts) == len(symbols)
        assert sum(c << (16 - n) for n, c in enumerate(counts, 1)) < 1 << 16              # Kraft, with room for the reserved code


def test_table_rule_on_small_histograms():
    # one real symbol: it and the reserved code share length 1, the symbol gets code 0
    assert opt.table_from_histogram([0] * 5 + [7] + [0] * 250) == ([1] + [0] * 15, [5], 1)
    # ties go to the larger index: of four symbols of frequency 1 and the pseudo-symbol, 3 is merged with 256 first
    hist = [1, 1, 1, 1] + [0] * 252
    counts, symbols, depth = opt.table_from_histogram(hist)
    assert (counts[:3], symbols, depth) == ([0, 3, 1], [0, 1, 2, 3], 3)
    # frequencies 1, 1, 2, 4, ... : a chain as deep as the symbols are many; 20 symbols are limited to 16 bits
    chain = [1 << max(k - 1, 0) for k in range(20)] + [0] * 236
    counts, symbols, depth = opt.table_from_histogram(chain)
    assert depth == 20 and sum(counts) == 20 and symbols[:3] == [19, 18, 17]
    assert sum(c << (16 - n) for n, c in enumerate(counts, 1)) < 1 << 16
    with pytest.raises(ValueError):
        opt.table_from_histogram([opt.FREQUENCY_LIMIT] + [0] * 255)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_header_with_tables_is_pillows(subsampling):
    from ciaosr_amd import jpeg_hip
    for (h, w), q, content in [((1, 1), 1, 'flat'), ((17, 33), 10, 'ramp'), ((100, 75), 50, 'noise'), ((64, 64), 90, 'saturated'),
                               ((300, 7), 100, 'ramp_noise')]:
        rgb = make_image(h, w, content)
        pil = pil_jpeg_opt(rgb, q, subsampling)
        segs, start = segments(pil)
        assert [m for m, _ in segs] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xda]
        tables = dht_tables(pil)
        assert jpeg_hip.header(h, w, q, subsampling, tables) == pil[:start] == opt.header(h, w, q, subsampling, tables), (h, w, q)
        assert jpeg_hip.header(h, w, q, subsampling, tables=[(list(c), list(v)) for c, v in tables]) == pil[:start]
        assert [(list(c), list(v)) for c, v in tables] == opt.scan(rgb, q, subsampling)[1]
        # without tables: the Annex K header, as before
        from tests import jpeg_ref
        from tests.test_jpeg_host import pil_jpeg
        plain = pil_jpeg(rgb, q, subsampling)
        assert jpeg_hip.header(h, w, q, subsampling) == jpeg_hip.header(h, w, q, subsampling, None) == jpeg_ref.header(h, w, q, subsampling)
        assert jpeg_hip.header(h, w, q, subsampling) == plain[:segments(plain)[1]]
    annex_k = [(c, v) for _, c, v in jpeg_hip.HUFFMAN]
    assert jpeg_hip.header(8, 8, 90, '444', annex_k) == jpeg_hip.header(8, 8, 90, '444')
    for bad in (annex_k[:3], annex_k + annex_k[:1], [(c[:15], v) for c, v in annex_k], [(c, v[:-1]) for c, v in annex_k],
                [((0,) * 16, ())] * 4):
        with pytest.raises(ValueError):
            jpeg_hip.header(8, 8, 90, '444', bad)
    assert jpeg_hip.TABLE_IDS == opt.TABLE_IDS and jpeg_hip.FREQUENCY_LIMIT == opt.FREQUENCY_LIMIT


def test_split_result():
    import struct
    from ciaosr_amd import jpeg_hip
    records = []
    for k in range(8):
        counts = [0] * 16
        counts[k] = 2
        counts[k + 3] = 1
        records.append((tuple(counts), (k, 200 + k, 17)))
    raw = struct.pack('<3q', 0, 40, 77) + b''.join(bytes(c) + bytes(v) + bytes(256 - len(v)) for c, v in records)
    assert len(raw) == 8 * 3 + 2 * 4 * jpeg_hip.DHT_RECORD_BYTES
    offsets, tables = jpeg_hip.split_result(torch.from_numpy(np.frombuffer(raw, dtype=np.int64).copy()), 2)
    assert offsets == [0, 40, 77] and tables == [records[:4], records[4:]]


def test_refusals():
    from ciaosr_amd import jpeg_hip, pyramid
    from ciaosr_amd._lib import CiaoSRHipError
    img = make_image(7, 5, 'noise')
    for bad in ('yes', 1, 0, None, 'True'):
        for fn in (jpeg_hip.encode_jpeg, jpeg_hip.encode_scan):
            with pytest.raises(ValueError):
                fn(img, optimize=bad)
        for fn in (jpeg_hip.encode_jpeg_tiles, jpeg_hip.encode_scans, jpeg_hip.encode_scans_device):
            with pytest.raises(ValueError):
                fn(img, [(0, 0, 2, 2)], optimize=bad)
        with pytest.raises(ValueError):
            jpeg_hip.imwrite_gpu_jpeg(img, 'never_written.jpg', optimize=bad)
        with pytest.raises(ValueError):
            pyramid.write_levels([torch.zeros((5, 9, 3), dtype=torch.uint8)], 'never_written', 'q', fmt='jpg', optimize=bad)
    assert not os.path.exists('never_written.jpg') and not os.path.exists('never_written')
    # no CPU fallback: a host array raises, as without the flag
    for fn in (jpeg_hip.encode_jpeg, jpeg_hip.encode_scan):
        with pytest.raises(CiaoSRHipError):
            fn(torch.from_numpy(img), optimize=True)
    with pytest.raises(CiaoSRHipError):
        jpeg_hip.encode_jpeg_tiles(torch.from_numpy(img), [(0, 0, 2, 2)], optimize=True)
    # the frequency limit: 64 x blocks (all components, dummy blocks included) stays below 1e9
    assert jpeg_hip.scan_block_count(72, 136, '444') == 3 * 9 * 17 and jpeg_hip.scan_block_count(72, 136, '420') == 6 * 5 * 9
    assert jpeg_hip.check_frequency_limit(5424, 8160, '444') == 3 * 678 * 1020                # the bench image: 1.3e8 symbols at most
    assert 64 * 3 * 678 * 1020 < jpeg_hip.FREQUENCY_LIMIT
    assert jpeg_hip.check_frequency_limit(18256, 18256, '444') == 3 * 2282 * 2282            # 64 x 15 622 572 = 999 844 608
    assert 64 * 3 * 2282 * 2283 == 1_000_282_752                                              # one more column of blocks: refused
    for h, w, sub in [(18256, 18264, '444'), (65535, 65535, '444'), (65535, 65535, '420'), (36528, 18264, '420')]:
        assert 64 * jpeg_hip.scan_block_count(h, w, sub) >= jpeg_hip.FREQUENCY_LIMIT
        with pytest.raises(ValueError, match='64 x blocks'):
            jpeg_hip.check_frequency_limit(h, w, sub)


def test_cli_flag(tmp_path, monkeypatch):
    import tools.render as render_cli
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    base = [path, 'None', 'x.png', '--scale', '2', '--out', 'o']
    args = render_cli.parse_args(base + ['--jpeg', '90'])
    assert args.jpeg_optimize is False and render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=90, subsampling='444')
    args = render_cli.parse_args(base + ['--jpeg', '35', '--jpeg-subsampling', '420', '--jpeg-optimize', '--dzi', '2'])
    assert render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=35, subsampling='420', optimize=True)
    for bad in (['--jpeg-optimize'], ['--jpeg-optimize', '--gpu-png'], ['--jpeg-optimize', '--jpeg-subsampling', '420']):
        with pytest.raises(SystemExit):
            render_cli.parse_args(base + bad)
    # the pyramid's level writer hands the flag to encode_jpeg_tiles, one call per level; the manifest is the plain one
    from ciaosr_amd import jpeg_hip, pyramid
    calls = []

    def fake(img, rects, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0, optimize=False):
        calls.append((tuple(img.shape), len(rects), quality, subsampling, order, optimize))
        return [b'jpeg'] * len(rects)

    monkeypatch.setattr(jpeg_hip, 'encode_jpeg_tiles', fake)
    levels = [torch.zeros((hl, wl, 3), dtype=torch.uint8) for hl, wl in pyramid.level_sizes(5, 9)]
    pyramid.write_levels(levels, str(tmp_path / 'a'), 'p', tile_size=4, overlap=1, fmt='jpg', quality=35, subsampling='420', optimize=True)
    plan = pyramid.dzi_plan(5, 9, 4, 1)
    assert calls == [((lv['height'], lv['width'], 3), len(lv['tiles']), 35, '420', 'bgr', True) for lv in plan]
    calls.clear()
    pyramid.write_levels(levels, str(tmp_path / 'b'), 'p', tile_size=4, overlap=1, fmt='jpg', quality=35, subsampling='420')
    assert [c[-1] for c in calls] == [False] * len(plan)
    assert (tmp_path / 'a' / 'p.dzi').read_text() == (tmp_path / 'b' / 'p.dzi').read_text()


def test_abi_surface_and_capacity():
    import ctypes as C
    from ciaosr_amd import _lib, jpeg_hip
    lib = _lib.load()
    assert lib.ciaosr_version() >= 290
    names = ['ciaosr_jpeg_opt_result_bytes', 'ciaosr_jpeg_opt_workspace_bytes', 'ciaosr_jpeg_opt_capacity_bytes', 'ciaosr_jpeg_opt_encode_u8',
             'ciaosr_jpeg_opt_tiles_workspace_bytes', 'ciaosr_jpeg_opt_tiles_capacity_bytes', 'ciaosr_jpeg_opt_encode_tiles_u8']
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    assert f'#define CIAOSR_JPEG_DHT_RECORD_BYTES {jpeg_hip.DHT_RECORD_BYTES}' in header
    assert [lib.ciaosr_jpeg_opt_result_bytes(n) for n in (0, 1, 3, 726)] == [0, 16 + 1088, 32 + 3 * 1088, 8 * 727 + 726 * 1088]
    # the capacity is the worst case of arbitrary 16-bit codes: 2 x ceil(1665 x blocks / 8) per crop, dummy blocks included
    assert 16 + 11 + 63 * (16 + 10) == 1665

    def need(blocks):
        return 2 * -(-1665 * blocks // 8)

    for h, w in [(1, 1), (8, 8), (72, 136), (200, 264), (5424, 8160), (65535, 3)]:
        b444, b420 = 3 * -(-h // 8) * -(-w // 8), 6 * -(-h // 16) * -(-w // 16)
        assert lib.ciaosr_jpeg_opt_capacity_bytes(h, w, 0) == need(b444) > lib.ciaosr_jpeg_capacity_bytes(h, w, 0) == 416 * b444
        assert lib.ciaosr_jpeg_opt_capacity_bytes(h, w, 2) == need(b420) > lib.ciaosr_jpeg_capacity_bytes(h, w, 2) == 416 * b420
        for sub, blocks in ((0, b444), (2, b420)):
            plain = lib.ciaosr_jpeg_workspace_bytes(h, w, sub, 0)
            assert lib.ciaosr_jpeg_opt_workspace_bytes(h, w, sub, 0) >= plain + 4 * 256 * 4 + 2 * 272 * 4
            assert lib.ciaosr_jpeg_opt_workspace_bytes(h, w, sub, 0) >= blocks * (128 + 4) + need(blocks) // 2
    # per crop: an odd number of blocks rounds up in every crop of its own
    rects = (C.c_int * 12)(0, 0, 8, 8, 3, 5, 1, 1, 0, 0, 72, 136)
    assert lib.ciaosr_jpeg_opt_tiles_capacity_bytes(rects, 3, 0) == 2 * need(3) + need(3 * 9 * 17) == 2 * 1250 + need(459)
    assert lib.ciaosr_jpeg_opt_tiles_capacity_bytes(rects, 3, 2) == 2 * need(6) + need(6 * 5 * 9)
    assert lib.ciaosr_jpeg_opt_tiles_workspace_bytes(rects, 3, 0, 0) > lib.ciaosr_jpeg_tiles_workspace_bytes(rects, 3, 0, 0)
    # what the size functions cannot take: as the plain ones, and a crop at the frequency limit
    assert lib.ciaosr_jpeg_opt_capacity_bytes(65536, 4, 0) == 0 and lib.ciaosr_jpeg_opt_workspace_bytes(4, 0, 0, 0) == 0
    assert lib.ciaosr_jpeg_opt_capacity_bytes(8, 8, 1) == 0 and lib.ciaosr_jpeg_opt_workspace_bytes(8, 8, 3, 0) == 0
    assert lib.ciaosr_jpeg_opt_workspace_bytes(8, 8, 0, -1) == 0 and lib.ciaosr_jpeg_opt_tiles_capacity_bytes(rects, 0, 0) == 0
    assert lib.ciaosr_jpeg_opt_capacity_bytes(18256, 18256, 0) == need(3 * 2282 * 2282)
    assert lib.ciaosr_jpeg_opt_capacity_bytes(18256, 18264, 0) == 0 and lib.ciaosr_jpeg_opt_workspace_bytes(18256, 18264, 0, 0) == 0
    assert lib.ciaosr_jpeg_capacity_bytes(18256, 18264, 0) == 416 * 3 * 2282 * 2283                # the plain call still takes it
    big = (C.c_int * 8)(0, 0, 8, 8, 0, 0, 18256, 18264)
    assert lib.ciaosr_jpeg_opt_tiles_capacity_bytes(big, 2, 0) == 0 and lib.ciaosr_jpeg_opt_tiles_capacity_bytes(big, 1, 0) == need(3)
