"""Host-side tests of progressive JPEG files (ciaosr_amd/jpeg_hip.py `progressive=True`): the plain Python restatement
of libjpeg's progressive entropy coder (tests/jpeg_prog_ref.py) against Pillow's `progressive=True` files byte for byte -- the host
grid, images whose buffered correction bits force a flush, a flat image whose EOB runs reach 32767 blocks -- the host's assembly of
the file, the refusals, the CLI flag, the ABI surface and the capacity formula.  Also the helpers that tests/test_jpeg_prog_gpu.py
shares."""
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_prog_ref as prog
from tests.test_jpeg_host import CONTENTS, PIL_SUBSAMPLING, SIZES, SUBSAMPLINGS, first_difference, make_image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_QUALITIES = [1, 50, 90, 100]
CORR_SIZES = [(8, 320), (16, 128), (24, 136)]
FLAT_SIDE = 1456                            # 182 x 182 = 33 124 blocks per full-size component: one more than 32767 + 356


def pil_jpeg_prog(rgb, quality, subsampling, **more):
    """Pillow's progressive=True file; its one output buffer is raised for the call, as in tests/test_jpeg_opt_host.py."""
    import PIL.ImageFile
    from PIL import Image
    mp = pytest.MonkeyPatch()
    mp.setattr(PIL.ImageFile, 'MAXBLOCK', 1 << 24)
    try:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(rgb)).save(bio, format='JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[subsampling],
                                                        progressive=True, **more)
    finally:
        mp.undo()
    return bio.getvalue()


def _dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.cos((2 * n + 1) * k * np.pi / 16) / 2
    c[0] /= np.sqrt(2)
    return c


@functools.lru_cache(maxsize=None)
def corr_image(h, w, seed=7):
    """Grey; every coefficient of every block but the DC is +-6 at quality 100: no scan after the first meets a coefficient that
    becomes non-zero, so a refinement scan is one EOB run whose every block buffers up to 63 correction bits."""
    rng = np.random.RandomState(seed)
    c = _dct_matrix()
    img = np.zeros((h, w), dtype=np.uint8)
    for by in range(h // 8):
        for bx in range(w // 8):
            k = 6.0 * rng.choice([-1.0, 1.0], (8, 8))
            k[0, 0] = 0.0
            img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = np.clip(np.rint(128 + c.T @ k @ c), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def corr_want(h, w, subsampling):
    """(file, scans, tables, counters) of the crafted image at quality 100; the file is Pillow's."""
    rgb = corr_image(h, w)
    scans, tables, stats = prog.code(rgb, 100, subsampling)
    want = prog.assemble(h, w, 100, subsampling, scans, tables)
    assert want == pil_jpeg_prog(rgb, 100, subsampling)
    return want, scans, tables, stats


@functools.lru_cache(maxsize=None)
def flat_want(subsampling):
    """(file, counters) of the flat FLAT_SIDE x FLAT_SIDE image at quality 90; the file is Pillow's."""
    rgb = np.full((FLAT_SIDE, FLAT_SIDE, 3), 77, dtype=np.uint8)
    stats = {}
    want = prog.encode(rgb, 90, subsampling, stats)
    assert want == pil_jpeg_prog(rgb, 90, subsampling)
    return want, stats


def parse(data):
    """A whole file -> ([marker or (marker, payload)] in order, SOI and EOI bare; the entropy-coded data behind every SOS)."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    segs, datas, i = [0xd8], [], 2
    while i < len(data) - 2:
        assert data[i] == 0xff
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        segs.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xda:
            j = i
            while not (data[j] == 0xff and data[j + 1] != 0x00):
                j += 1
            datas.append(data[i:j])
            i = j
    return segs + [0xd9], datas


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('content', CONTENTS)
def test_reference_is_pillows_progressive_file(content, subsampling):
    for h, w in SIZES:
        rgb = make_image(h, w, content)
        for q in HOST_QUALITIES:
            got, want = prog.encode(rgb, q, subsampling), pil_jpeg_prog(rgb, q, subsampling)
            assert got == want, (h, w, content, q, subsampling, first_difference(got, want), len(got), len(want))


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_optimize_does_not_change_a_progressive_file(subsampling):
    for content in CONTENTS:
        for h, w in ((17, 33), (64, 64)):
            rgb = make_image(h, w, content)
            for q in (50, 100):
                assert pil_jpeg_prog(rgb, q, subsampling, optimize=True) == pil_jpeg_prog(rgb, q, subsampling)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('size', CORR_SIZES)
def test_correction_bits_force_flushes(size, subsampling):
    """The rule `more than 937 buffered bits` cuts the runs of these images (asserted from the reference's own counter, so that a seed
    which reaches none fails here); corr_want holds the files to Pillow."""
    stats = corr_want(*size, subsampling)[3]
    assert stats['corr_flushes'] >= 1 and stats['full_flushes'] == 0, stats
    print(size, subsampling, stats)


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_flat_image_reaches_the_run_limit(subsampling):
    """33 124 blocks of nothing but EOB: every AC scan of a full-size component is one run, cut at 32767 blocks."""
    stats = flat_want(subsampling)[1]
    assert stats['longest_run'] == 32767 and stats['corr_flushes'] == 0, stats
    if subsampling == '444':
        assert stats['full_flushes'] == 4 and stats['first_full_flushes'] == 4, stats        # one per AC scan
    else:
        assert stats['full_flushes'] == 2 and stats['first_full_flushes'] == 2, stats        # 4:2:0: luma alone has that many blocks


def test_the_file_layout():
    """SOF2, ten scans with the script's headers, ten tables in front of the scans that use them."""
    rgb = make_image(17, 33, 'noise')
    for subsampling in SUBSAMPLINGS:
        scans, tables, _ = prog.code(rgb, 90, subsampling)
        segs, datas = parse(prog.assemble(17, 33, 90, subsampling, scans, tables))
        assert datas == scans
        markers = [s if isinstance(s, int) else s[0] for s in segs]
        assert markers[:5] == [0xd8, 0xe0, 0xdb, 0xdb, 0xc2] and markers[-1] == 0xd9
        assert markers[5:-1] == [0xc4, 0xc4, 0xda] + [0xc4, 0xda] * 5 + [0xda] + [0xc4, 0xda] * 3
        segs = [s for s in segs if not isinstance(s, int)]
        assert [p[0] for m, p in segs if m == 0xc4] == list(prog.TABLE_IDS)
        assert [(tuple(p[1:17]), tuple(p[17:])) for m, p in segs if m == 0xc4] == [(tuple(c), tuple(v)) for c, v in tables]
        sos = [p for m, p in segs if m == 0xda]
        assert [p[0] for p in sos] == [3, 1, 1, 1, 1, 1, 3, 1, 1, 1]
        assert [p[1] for p in sos[1:6] + sos[7:]] == [1, 3, 2, 1, 1, 3, 2, 1]                # Cr before Cb
        assert [tuple(p[-3:]) for p in sos] == [(ss, se, (ah << 4) | al) for _, ss, se, ah, al in prog.SCRIPT]
        assert len(datas) == 10


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_host_assembly_is_the_references(subsampling):
    from ciaosr_amd import jpeg_hip
    assert jpeg_hip.SCAN_SCRIPT == prog.SCRIPT and jpeg_hip.PROGRESSIVE_TABLE_IDS == prog.TABLE_IDS
    for (h, w), q in (((17, 33), 90), ((1, 1), 1), ((100, 75), 100)):
        rgb = make_image(h, w, 'ramp_noise')
        scans, tables, _ = prog.code(rgb, q, subsampling)
        assert jpeg_hip.progressive_header(h, w, q, subsampling) == prog.frame_header(h, w, q, subsampling)
        for s in range(10):
            assert jpeg_hip.scan_header(s, tables) == prog.scan_header(s, tables), s
        assert jpeg_hip.assemble_progressive(h, w, q, subsampling, scans, tables) == pil_jpeg_prog(rgb, q, subsampling)
    with pytest.raises(ValueError):
        jpeg_hip.assemble_progressive(8, 8, 90, subsampling, scans[:9], tables)
    with pytest.raises(ValueError):
        jpeg_hip.assemble_progressive(8, 8, 90, subsampling, scans, tables[:9])
    with pytest.raises(ValueError):
        jpeg_hip.scan_header(1, [((0,) * 16, (1,))] * 10)


def test_split_progressive_result():
    import struct
    from ciaosr_amd import jpeg_hip
    records = []
    for k in range(20):
        counts = [0] * 16
        counts[k % 13] = 2
        counts[k % 13 + 3] = 1
        records.append((tuple(counts), (k, 200 + k, 17)))
    offs = list(range(0, 21 * 5, 5))
    raw = struct.pack('<21q', *offs) + b''.join(bytes(c) + bytes(v) + bytes(256 - len(v)) for c, v in records)
    assert len(raw) == 8 * 21 + 2 * 10 * jpeg_hip.DHT_RECORD_BYTES
    offsets, tables = jpeg_hip.split_progressive_result(torch.from_numpy(np.frombuffer(raw, dtype=np.int64).copy()), 2)
    assert offsets == offs and tables == [records[:10], records[10:]]


def test_refusals():
    from ciaosr_amd import jpeg_hip, pyramid
    from ciaosr_amd._lib import CiaoSRHipError
    img = make_image(7, 5, 'noise')
    for bad in ('yes', 1, 0, None, 'True'):
        with pytest.raises(ValueError):
            jpeg_hip.check_progressive(bad)
        for fn in (jpeg_hip.encode_jpeg, jpeg_hip.encode_scan):
            with pytest.raises(ValueError):
                fn(img, progressive=bad)
        for fn in (jpeg_hip.encode_jpeg_tiles, jpeg_hip.encode_scans, jpeg_hip.encode_scans_device):
            with pytest.raises(ValueError):
                fn(img, [(0, 0, 2, 2)], progressive=bad)
        with pytest.raises(ValueError):
            jpeg_hip.imwrite_gpu_jpeg(img, 'never_written.jpg', progressive=bad)
        with pytest.raises(ValueError):
            pyramid.write_levels([torch.zeros((5, 9, 3), dtype=torch.uint8)], 'never_written', 'q', fmt='jpg', progressive=bad)
    assert jpeg_hip.check_progressive(True) is True and jpeg_hip.check_progressive(False) is False
    for kw in (dict(quality=0), dict(subsampling='422'), dict(order='gbr'), dict(mcus_per_chunk=-2), dict(optimize='yes')):
        with pytest.raises(ValueError):
            jpeg_hip.encode_jpeg(img, progressive=True, **kw)
    assert not os.path.exists('never_written.jpg') and not os.path.exists('never_written')
    # no CPU fallback: a host array raises, as without the flag
    for fn in (jpeg_hip.encode_jpeg, jpeg_hip.encode_scan):
        with pytest.raises(CiaoSRHipError):
            fn(torch.from_numpy(img), progressive=True)
    with pytest.raises(CiaoSRHipError):
        jpeg_hip.encode_jpeg_tiles(torch.from_numpy(img), [(0, 0, 2, 2)], progressive=True)


def test_cli_flag(tmp_path, monkeypatch):
    import tools.render as render_cli
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    base = [path, 'None', 'x.png', '--scale', '2', '--out', 'o']
    args = render_cli.parse_args(base + ['--jpeg', '90'])
    assert args.jpeg_progressive is False and render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=90, subsampling='444')
    args = render_cli.parse_args(base + ['--jpeg', '35', '--jpeg-subsampling', '420', '--jpeg-progressive', '--dzi', '2'])
    assert render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=35, subsampling='420', progressive=True)
    args = render_cli.parse_args(base + ['--jpeg', '35', '--jpeg-progressive', '--jpeg-optimize'])
    assert render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=35, subsampling='444', optimize=True, progressive=True)
    for bad in (['--jpeg-progressive'], ['--jpeg-progressive', '--gpu-png'], ['--jpeg-progressive', '--jpeg-subsampling', '420']):
        with pytest.raises(SystemExit):
            render_cli.parse_args(base + bad)
    # the pyramid's level writer hands the flag to encode_jpeg_tiles, one call per level; the manifest is the plain one
    from ciaosr_amd import jpeg_hip, pyramid
    calls = []

    def fake(img, rects, **kw):
        calls.append(kw)
        return [b'jpeg'] * len(rects)

    monkeypatch.setattr(jpeg_hip, 'encode_jpeg_tiles', fake)
    levels = [torch.zeros((hl, wl, 3), dtype=torch.uint8) for hl, wl in pyramid.level_sizes(5, 9)]
    pyramid.write_levels(levels, str(tmp_path / 'a'), 'p', tile_size=4, overlap=1, fmt='jpg', quality=35, subsampling='420', progressive=True)
    plan = pyramid.dzi_plan(5, 9, 4, 1)
    assert calls == [dict(quality=35, subsampling='420', order='bgr', progressive=True)] * len(plan)
    calls.clear()
    pyramid.write_levels(levels, str(tmp_path / 'b'), 'p', tile_size=4, overlap=1, fmt='jpg', quality=35, subsampling='420')
    assert calls == [dict(quality=35, subsampling='420', order='bgr')] * len(plan)         # without the flag: the call as it was
    assert (tmp_path / 'a' / 'p.dzi').read_text() == (tmp_path / 'b' / 'p.dzi').read_text()


def capacity_need(h, w, subsampling):
    """The closed form of DESIGN 4.1i-e: twice the sum over the ten scans of ceil(bits per block x blocks of the scan / 8)."""
    luma = -(-h // 8) * -(-w // 8)
    if subsampling == '444':
        inter, chroma = 3 * luma, luma
    else:
        chroma = -(-h // 16) * -(-w // 16)
        inter = 6 * chroma
    total = 0
    for comp, ss, se, ah, al in prog.SCRIPT:
        if comp is None:
            bits, blocks = (1 if ah else 16 + 11), inter
        else:
            bits, blocks = (17 * 63 + 60 if ah else 26 * (se - ss + 1) + 60), (luma if comp == 0 else chroma)
        total += -(-bits * blocks // 8)
    return 2 * total


def test_abi_surface_and_capacity():
    import ctypes as C
    from ciaosr_amd import _lib, jpeg_hip
    lib = _lib.load()
    assert lib.ciaosr_version() >= 300
    names = ['ciaosr_jpeg_prog_result_bytes', 'ciaosr_jpeg_prog_workspace_bytes', 'ciaosr_jpeg_prog_capacity_bytes', 'ciaosr_jpeg_prog_encode_u8',
             'ciaosr_jpeg_prog_tiles_workspace_bytes', 'ciaosr_jpeg_prog_tiles_capacity_bytes', 'ciaosr_jpeg_prog_encode_tiles_u8']
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + '(' in header and name in integration, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('_prog_', '_opt_')]
    # 10 n + 1 offsets, then ten DHT records per crop
    assert [lib.ciaosr_jpeg_prog_result_bytes(n) for n in (0, 1, 3, 726)] == [0, 88 + 2720, 8 * 31 + 3 * 2720, 8 * 7261 + 726 * 2720]
    assert capacity_need(8, 8, '444') == 2 * (-(-81 // 8) + 1 + -(-190 // 8) + 2 * -(-1698 // 8) + 1568 // 8 + 4 * -(-1131 // 8))
    for h, w in [(1, 1), (8, 8), (9, 40), (72, 136), (200, 264), (5424, 8160), (65535, 3)]:
        for sub, name in ((0, '444'), (2, '420')):
            need = capacity_need(h, w, name)
            assert lib.ciaosr_jpeg_prog_capacity_bytes(h, w, sub) == need, (h, w, name)
            if name == '444':                               # 4:2:0: the AC scans skip the dummy blocks, which the one baseline scan codes
                assert need > lib.ciaosr_jpeg_opt_capacity_bytes(h, w, sub), (h, w)
            blocks = jpeg_hip.scan_block_count(h, w, name)
            assert lib.ciaosr_jpeg_prog_workspace_bytes(h, w, sub, 0) >= 128 * blocks + need // 2
    rects = (C.c_int * 12)(0, 0, 8, 8, 3, 5, 1, 1, 0, 0, 72, 136)
    for sub, name in ((0, '444'), (2, '420')):
        assert lib.ciaosr_jpeg_prog_tiles_capacity_bytes(rects, 3, sub) == 2 * capacity_need(8, 8, name) + capacity_need(72, 136, name)
        assert lib.ciaosr_jpeg_prog_tiles_workspace_bytes(rects, 3, sub, 0) > lib.ciaosr_jpeg_opt_tiles_workspace_bytes(rects, 3, sub, 0)
    # what the size functions cannot take: as the optimised ones
    assert lib.ciaosr_jpeg_prog_capacity_bytes(65536, 4, 0) == 0 and lib.ciaosr_jpeg_prog_workspace_bytes(4, 0, 0, 0) == 0
    assert lib.ciaosr_jpeg_prog_capacity_bytes(8, 8, 1) == 0 and lib.ciaosr_jpeg_prog_workspace_bytes(8, 8, 3, 0) == 0
    assert lib.ciaosr_jpeg_prog_workspace_bytes(8, 8, 0, -1) == 0 and lib.ciaosr_jpeg_prog_tiles_capacity_bytes(rects, 0, 0) == 0
    assert lib.ciaosr_jpeg_prog_capacity_bytes(18256, 18256, 0) == capacity_need(18256, 18256, '444')
    assert lib.ciaosr_jpeg_prog_capacity_bytes(18256, 18264, 0) == 0 and lib.ciaosr_jpeg_prog_workspace_bytes(18256, 18264, 0, 0) == 0
    big = (C.c_int * 8)(0, 0, 8, 8, 0, 0, 18256, 18264)
    assert lib.ciaosr_jpeg_prog_tiles_capacity_bytes(big, 2, 0) == 0 and lib.ciaosr_jpeg_prog_tiles_capacity_bytes(big, 1, 0) == capacity_need(8, 8, '444')
