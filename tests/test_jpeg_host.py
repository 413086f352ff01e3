"""Host-side tests of the device JPEG encoder's contract (ciaosr_amd/jpeg_hip.py, csrc/jpeg_u8.hip): the numpy
restatement of libjpeg's baseline pipeline (tests/jpeg_ref.py) against Pillow's files byte for byte, the header and tables of the module
against Pillow's, the manifest, the CLI flags, the refusals and the ABI surface.  Also the image makers that tests/test_jpeg_gpu.py
shares."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 9), (8, 8), (17, 33), (9, 40), (40, 9), (24, 24), (64, 64), (100, 75)]
CONTENTS = ['noise', 'ramp', 'saturated', 'flat', 'ramp_noise']
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
SUBSAMPLINGS = ['444', '420']
PIL_SUBSAMPLING = {'444': 0, '420': 2}


def make_image(h, w, content, seed=0):
    """uint8 [h, w, 3] RGB.  'noise': uniform bytes; 'ramp': smooth; 'saturated': 0 / 255 only -- 8 x 8 blocks that are flat 0, flat 255,
    random per pixel, or split into a black and a white half (DC differences of category 11 and AC of category 10 at quality 100); 'flat': 255 everywhere (6-bit
    blocks: many blocks share a word); 'ramp_noise': ramp +- 2."""
    rng = np.random.RandomState(seed * 7919 + 131 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(2 * yy + xx) % 256, (yy + 3 * xx) // 2 % 256, 255 - (yy + xx) % 256], axis=-1)
    if content == 'noise':
        return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    if content == 'ramp':
        return ramp.astype(np.uint8)
    if content == 'saturated':
        pixels = rng.randint(0, 2, (h, w, 1)).repeat(3, axis=2)
        blocks = rng.randint(0, 4, (-(-h // 8), -(-w // 8), 1)).repeat(8, axis=0).repeat(8, axis=1)[:h, :w]       # 0, 1: flat
        split = (xx % 8 >= 4)[:, :, None]
        return (np.where(blocks == 2, pixels, np.where(blocks == 3, split, blocks)) * 255).astype(np.uint8)
    if content == 'flat':
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if content == 'ramp_noise':
        return np.clip(ramp + rng.randint(-2, 3, ramp.shape), 0, 255).astype(np.uint8)
    raise KeyError(content)


def pil_jpeg(rgb, quality, subsampling):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(bio, format='JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[subsampling])
    return bio.getvalue()


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def segments(data):
    """[(marker, payload)] of a JPEG file up to and including SOS, and the offset where the entropy-coded data begins."""
    assert data[:2] == b'\xff\xd8'
    out, i = [], 2
    while True:
        assert data[i] == 0xff
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xda:
            return out, i


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('content', CONTENTS)
def test_reference_is_pillow_byte_for_byte(content, subsampling):
    bad = []
    for h, w in SIZES:
        rgb = make_image(h, w, content)
        for q in QUALITIES:
            mine, pil = ref.encode(rgb, q, subsampling), pil_jpeg(rgb, q, subsampling)
            if mine != pil:
                bad.append(f'{h}x{w} {content} q{q} {subsampling}: first difference at byte {first_difference(mine, pil)}, '
                           f'{len(mine)} against {len(pil)} bytes')
    assert not bad, '\n'.join(bad)


def test_the_grid_reaches_the_large_categories_and_the_stuffing():
    blocks = ref.scan_blocks(make_image(64, 64, 'saturated'), 100, '444')
    pred, cats_dc, cats_ac = [0, 0, 0], set(), set()
    for comp, blk in blocks:
        cats_dc.add(abs(int(blk[0]) - pred[comp]).bit_length())
        pred[comp] = int(blk[0])
        cats_ac |= {abs(int(v)).bit_length() for v in blk[1:]}
    assert 11 in cats_dc and 10 in cats_ac, (cats_dc, cats_ac)
    assert b'\xff' in ref.unstuffed(ref.scan_blocks(make_image(64, 64, 'noise'), 100, '444'))
    # 24 x 24 in 4:2:0: columns are repeated BEFORE the halving (the last column alone), rows AFTER it (the last halved row)
    rgb = make_image(24, 24, 'noise')
    full = ref.ycc(rgb)[1]
    cb = ref.planes(rgb, '420')[1]
    assert cb.shape == (16, 16)
    from_last_column = (2 * (full[0::2, 23] + full[1::2, 23])[:, None] + np.array([1, 2, 1, 2])) >> 2
    assert np.array_equal(cb[:12, 12:], from_last_column)
    assert np.array_equal(cb[12:], np.repeat(cb[11:12], 4, axis=0))
    assert not np.array_equal(cb[:12, 12:], np.repeat(cb[:12, 11:12], 4, axis=1))         # the row rule on columns would differ


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_header_and_tables_are_pillows(subsampling):
    from ciaosr_amd import jpeg_hip
    for (h, w), q in [((1, 1), 1), ((17, 33), 10), ((100, 75), 50), ((64, 64), 90), ((300, 7), 100)]:
        pil = pil_jpeg(make_image(h, w, 'ramp'), q, subsampling)
        segs, start = segments(pil)
        assert jpeg_hip.header(h, w, q, subsampling) == pil[:start] == ref.header(h, w, q, subsampling), (h, w, q)
        assert [m for m, _ in segs] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xda]
        dht = [p for m, p in segs if m == 0xc4]
        assert [(p[0], tuple(p[1:17]), tuple(p[17:])) for p in dht] == list(jpeg_hip.HUFFMAN)
        assert [(list(p[1:17]), list(p[17:])) for p in dht] == [(list(b), list(v)) for b, v in
                                                                (ref.DC_LUMA, ref.AC_LUMA, ref.DC_CHROMA, ref.AC_CHROMA)]
        dqt = [p for m, p in segs if m == 0xdb]
        for k, table in enumerate(jpeg_hip.quant_tables(q)):
            assert dqt[k][0] == k and list(dqt[k][1:]) == [table[i] for i in jpeg_hip.ZIGZAG]
            assert list(table) == [int(v) for v in ref.quant_tables(q)[k]]
    assert list(jpeg_hip.ZIGZAG) == ref.ZIGZAG.tolist()
    assert jpeg_hip.SUBSAMPLINGS == PIL_SUBSAMPLING


def test_manifest_format():
    from ciaosr_amd.pyramid import DZI_NS, dzi_manifest
    old = (f'<?xml version="1.0" encoding="UTF-8"?><Image xmlns="{DZI_NS}" Format="png" Overlap="1" TileSize="254">'
           f'<Size Width="300" Height="200"/></Image>')
    assert dzi_manifest(200, 300) == dzi_manifest(200, 300, 254, 1) == dzi_manifest(200, 300, fmt='png') == old
    assert dzi_manifest(200, 300, fmt='jpg') == old.replace('Format="png"', 'Format="jpg"')
    with pytest.raises(ValueError):
        dzi_manifest(200, 300, fmt='jpeg')


def test_cli_flags_reach_the_writer(tmp_path, monkeypatch):
    import tools.render as render_cli
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    base = [path, 'None', 'x.png', '--scale', '2', '--out', 'o']
    args = render_cli.parse_args(base)
    assert args.jpeg is None and render_cli.output_format(args) == dict(fmt='png', ext='.png')
    args = render_cli.parse_args(base + ['--jpeg', '90'])
    assert render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=90, subsampling='444')
    args = render_cli.parse_args(base + ['--jpeg', '35', '--jpeg-subsampling', '420', '--dzi', '2'])
    assert render_cli.output_format(args) == dict(fmt='jpg', ext='.jpg', quality=35, subsampling='420')
    for bad in (['--jpeg', '0'], ['--jpeg', '101'], ['--jpeg', '90', '--jpeg-subsampling', '422']):
        with pytest.raises(SystemExit):
            render_cli.parse_args(base + bad)
    # the pyramid's level writer hands quality and subsampling to encode_jpeg_tiles, one call per level, and names the files .jpg
    from ciaosr_amd import jpeg_hip, pyramid
    calls = []

    def fake(img, rects, quality=90, subsampling='444', order='bgr', mcus_per_chunk=0):
        calls.append((tuple(img.shape), len(rects), quality, subsampling, order))
        return [b'jpeg'] * len(rects)

    monkeypatch.setattr(jpeg_hip, 'encode_jpeg_tiles', fake)
    levels = [torch.zeros((hl, wl, 3), dtype=torch.uint8) for hl, wl in pyramid.level_sizes(5, 9)]
    res = pyramid.write_levels(levels, str(tmp_path), 'p', tile_size=4, overlap=1, fmt='jpg', quality=35, subsampling='420')
    plan = pyramid.dzi_plan(5, 9, 4, 1)
    assert calls == [((lv['height'], lv['width'], 3), len(lv['tiles']), 35, '420', 'bgr') for lv in plan]
    assert res['files'] == 1 + sum(len(lv['tiles']) for lv in plan)
    assert 'Format="jpg"' in (tmp_path / 'p.dzi').read_text()
    assert sorted(os.listdir(tmp_path / 'p_files' / str(plan[-1]['level']))) == sorted(f'{c}_{r}.jpg' for c, r, *_ in plan[-1]['tiles'])
    with pytest.raises(ValueError):
        pyramid.write_levels(levels, str(tmp_path), 'q', tile_size=4, overlap=1, fmt='jpg', quality=0)
    with pytest.raises(ValueError):
        pyramid.write_levels(levels, str(tmp_path), 'q', tile_size=4, overlap=1, fmt='gif')


def test_bad_arguments_are_value_errors():
    from ciaosr_amd import jpeg_hip
    img = make_image(7, 5, 'noise')
    for q in (0, 101, -3, 50.5, 1000):
        with pytest.raises(ValueError):
            jpeg_hip.encode_jpeg(img, quality=q)
        with pytest.raises(ValueError):
            jpeg_hip.header(8, 8, q, '444')
    for s in ('422', 'gray', 0, 2, None):
        with pytest.raises(ValueError):
            jpeg_hip.encode_jpeg(img, subsampling=s)
        with pytest.raises(ValueError):
            jpeg_hip.encode_jpeg_tiles(img, [(0, 0, 2, 2)], subsampling=s)
    with pytest.raises(ValueError):
        jpeg_hip.encode_jpeg(img, order='gbr')
    with pytest.raises(ValueError):
        jpeg_hip.encode_scan(img, mcus_per_chunk=-1)
    with pytest.raises(ValueError):
        jpeg_hip.header(0, 8, 90, '444')
    with pytest.raises(ValueError):
        jpeg_hip.header(8, 65536, 90, '444')
    for bad in ([(0, 0, 8, 5)], [(0, 3, 5, 3)], [(0, 0, 0, 5)], [(3, 3, 2, 0)], [(-1, 0, 2, 2)], [(0, 0, 2, 2), (6, 4, 2, 1)], [], [(0, 0, 2.5, 2)]):
        with pytest.raises(ValueError):
            jpeg_hip.check_rects(bad, 7, 5)


def test_host_arrays_are_refused(tmp_path):
    from ciaosr_amd import jpeg_hip
    from ciaosr_amd._lib import CiaoSRHipError
    img = make_image(7, 5, 'noise')
    for fn in (jpeg_hip.encode_jpeg, jpeg_hip.encode_scan):
        with pytest.raises(CiaoSRHipError):
            fn(img)
        with pytest.raises(CiaoSRHipError):
            fn(torch.from_numpy(img))
    for fn in (jpeg_hip.encode_jpeg_tiles, jpeg_hip.encode_scans, jpeg_hip.encode_scans_device):
        with pytest.raises(CiaoSRHipError):
            fn(torch.from_numpy(img), [(0, 0, 2, 2)])
    with pytest.raises(CiaoSRHipError):
        jpeg_hip.imwrite_gpu_jpeg(torch.from_numpy(img), str(tmp_path / 'never_written.jpg'))
    assert not (tmp_path / 'never_written.jpg').exists()


def test_abi_surface():
    import ctypes as C
    from ciaosr_amd import _lib
    lib = _lib.load()
    assert lib.ciaosr_version() >= 280
    names = ['ciaosr_jpeg_workspace_bytes', 'ciaosr_jpeg_capacity_bytes', 'ciaosr_jpeg_encode_u8', 'ciaosr_jpeg_tiles_workspace_bytes',
             'ciaosr_jpeg_tiles_capacity_bytes', 'ciaosr_jpeg_encode_tiles_u8']
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    assert '#define CIAOSR_JPEG_444 0' in header and '#define CIAOSR_JPEG_420 2' in header
    # the capacity is the worst case: 2 x 208 bytes for every block of the scan, dummy blocks included
    for h, w in [(1, 1), (72, 136), (200, 264), (5424, 8160), (65535, 3)]:
        assert lib.ciaosr_jpeg_capacity_bytes(h, w, 0) == 416 * 3 * -(-h // 8) * -(-w // 8)
        assert lib.ciaosr_jpeg_capacity_bytes(h, w, 2) == 416 * 6 * -(-h // 16) * -(-w // 16)
        for sub in (0, 2):
            blocks = lib.ciaosr_jpeg_capacity_bytes(h, w, sub) // 416
            assert lib.ciaosr_jpeg_workspace_bytes(h, w, sub, 0) >= blocks * (128 + 4 + 208)
            assert lib.ciaosr_jpeg_workspace_bytes(h, w, sub, 1) > lib.ciaosr_jpeg_workspace_bytes(h, w, sub, 0) or h * w <= 256
    rects = (C.c_int * 8)(0, 0, 72, 136, 3, 5, 1, 1)
    assert lib.ciaosr_jpeg_tiles_capacity_bytes(rects, 2, 2) == lib.ciaosr_jpeg_capacity_bytes(72, 136, 2) + 416 * 6
    assert lib.ciaosr_jpeg_tiles_workspace_bytes(rects, 2, 0, 0) > 0
    # what the size functions cannot take: a side outside 1..65535, an unknown subsampling, no tiles, an empty rect
    assert lib.ciaosr_jpeg_capacity_bytes(65536, 4, 0) == 0 and lib.ciaosr_jpeg_workspace_bytes(4, 0, 0, 0) == 0
    assert lib.ciaosr_jpeg_capacity_bytes(8, 8, 1) == 0 and lib.ciaosr_jpeg_workspace_bytes(8, 8, 3, 0) == 0
    assert lib.ciaosr_jpeg_workspace_bytes(8, 8, 0, -1) == 0
    assert lib.ciaosr_jpeg_tiles_capacity_bytes(rects, 0, 0) == 0
    empty = (C.c_int * 4)(0, 0, 0, 4)
    assert lib.ciaosr_jpeg_tiles_capacity_bytes(empty, 1, 0) == 0 and lib.ciaosr_jpeg_tiles_workspace_bytes(empty, 1, 0, 0) == 0
