"""GPU tests of the PNG coder's opt-in LZ77 matches (`matches=True`: csrc/png_u8.hip's *_lz_* entry points, ciaosr_amd/png_hip.py).
The judges are Python's `zlib`, Pillow's decoder and the restatement of the contract in tests/png_match_ref.py -- never the device
against itself.
Run on the GPU box:  python -m pytest tests/test_png_matches_gpu.py -m gpu -q
"""
import io
import os
import zlib

import numpy as np
import pytest
import torch

from tests import png_match_ref as mref
from tests import png_reference as ref
from tests.test_png_host import make_image, pil_pixels
from tests.test_rgba_host import pil_rgba

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_SIZES = [(1, 1), (1, 300), (300, 1), (33, 17), (96, 128), (256, 384)]
RGBA_SIZES = [(7, 5), (64, 64), (256, 256)]
FINAL = b'\x01\x00\x00\xff\xff'                            # an empty stored block with BFINAL: ends a segment that is not the last


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


# ---- images --------------------------------------------------------------------------------------------------------------------------
def sprite0(h, w, seed=5):
    """uint8 [h, w, 4] R G B A: an ellipse of four-level noise (about 30 % of the pixels) with an edge eight pixels wide in alpha; the
    pixels under A = 0 hold colour 0.  On the CPU the restatement's model of the 256 x 256 one is 0.93 x Pillow's default file."""
    rng = np.random.RandomState(seed)
    colour = (rng.randint(0, 4, (h, w, 3)) * 85).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w] + 0.5
    r = np.sqrt(((y - h / 2) / (0.309 * h)) ** 2 + ((x - w / 2) / (0.309 * w)) ** 2)
    alpha = np.rint(255 * np.clip((1.0 - r) * (0.309 * min(h, w)) / 8.0 + 0.5, 0, 1)).astype(np.uint8)
    img = np.concatenate([colour, alpha[:, :, None]], axis=-1)
    img[alpha == 0] = 0
    return img


def rotated_view(h, w, channels=3, angle=30.0):
    """The smooth test image seen rotated by `angle` degrees about its centre (nearest pixel), 0 outside; with four channels A = 255
    inside and 0 outside."""
    src = make_image(h, w, 'noisy')
    t = np.deg2rad(angle)
    y, x = np.mgrid[0:h, 0:w] - np.array([h / 2 - 0.5, w / 2 - 0.5]).reshape(2, 1, 1)
    sy, sx = np.cos(t) * y - np.sin(t) * x + h / 2 - 0.5, np.sin(t) * y + np.cos(t) * x + w / 2 - 0.5
    iy, ix = np.rint(sy).astype(int), np.rint(sx).astype(int)
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    out = np.zeros((h, w, channels), dtype=np.uint8)
    out[inside, :3] = src[iy[inside], ix[inside]]
    if channels == 4:
        out[inside, 3] = 255
    return out


def stripes(h, w):
    """uint8 [h, w, 3]: vertical stripes of period 5."""
    colours = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [240, 240, 10], [5, 5, 5]], dtype=np.uint8)
    return np.ascontiguousarray(np.broadcast_to(colours[np.arange(w) % 5][None], (h, w, 3)))


def token_image(name):
    if name == 'random':
        return make_image(33, 17, 'random')
    if name == 'smooth':
        return make_image(96, 128, 'smooth')
    if name == 'sprite0':
        return sprite0(256, 256)
    if name == 'transparent':
        return np.zeros((256, 256, 4), dtype=np.uint8)
    if name == 'stripes':
        return stripes(60, 70)
    raise KeyError(name)


TOKEN_IMAGES = ['random', 'smooth', 'sprite0', 'transparent', 'stripes']
MUST_MATCH = {'sprite0', 'transparent', 'stripes'}


def _dev_img(img, dev, order=None):
    """The device tensor of an R G B (A) image in byte order `order` (default: 'rgb' / 'rgba')."""
    ch = img.shape[2]
    if order in ('bgr', 'bgra'):
        img = img[:, :, [2, 1, 0] + ([3] if ch == 4 else [])]
    return torch.from_numpy(np.ascontiguousarray(img)).to(dev)


def _order(img):
    return 'rgb' if img.shape[2] == 3 else 'rgba'


def _pixels(png, channels):
    return pil_pixels(png) if channels == 3 else pil_rgba(png)


def _pil_size(img):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(img, 'RGB' if img.shape[2] == 3 else 'RGBA').save(bio, format='PNG')
    return len(bio.getvalue())


def _rows(img, rows=0):
    from ciaosr_amd import _lib
    h, w, ch = img.shape
    name = 'ciaosr_png_rows_per_band' if ch == 3 else 'ciaosr_png_rgba_rows_per_band'
    return getattr(_lib.load(), name)(w, rows)


_cache = {}


def _coded(name, dev):
    """Everything the tests want of a token image, made once: the device's filtered stream, its bands, the match coder's and the
    literal coder's segments and zlib streams."""
    if name not in _cache:
        from ciaosr_amd import png_hip
        img = token_image(name)
        h, w, ch = img.shape
        t = _dev_img(img, dev)
        line = 1 + ch * w
        stream, _, adler = png_hip.filter_u8(t, order=_order(img))
        offs = ref.band_split(h, line, _rows(img))
        lz = png_hip.deflate_huff(stream, offs, matches=True, line=line, bpp=ch)
        lit = png_hip.deflate_huff(stream, offs)
        partials = [(int(a), int(b), offs[i + 1] - offs[i]) for i, (a, b) in enumerate(adler.cpu().tolist())]
        _cache[name] = dict(img=img, t=t, line=line, bpp=ch, offs=offs, stream=stream.cpu().numpy().tobytes(), lz=lz, lit=lit,
                            partials=partials, z_lz=png_hip.encode_zlib(t, _order(img), matches=True),
                            z_lit=png_hip.encode_zlib(t, _order(img)))
    return _cache[name]


# ---- 1: round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', RGB_SIZES)
def test_rgb_files_decode_to_the_pixels(dev, h, w):
    from ciaosr_amd.png_hip import encode_png, encode_zlib
    for img in (make_image(h, w, 'smooth'), make_image(h, w, 'two'), rotated_view(h, w), make_image(h, w, 'random')):
        for order in ('rgb', 'bgr'):
            t = _dev_img(img, dev, order)
            png = encode_png(t, order=order, matches=True)
            assert np.array_equal(pil_pixels(png), img), order
            assert len(encode_zlib(t, order, matches=True)) <= len(encode_zlib(t, order))          # 4: never larger


@pytest.mark.parametrize('h,w', RGBA_SIZES)
def test_rgba_files_decode_to_the_pixels(dev, h, w):
    from ciaosr_amd.png_hip import encode_png, encode_zlib
    for img in (sprite0(h, w), rotated_view(h, w, 4), np.zeros((h, w, 4), dtype=np.uint8)):
        for order in ('rgba', 'bgra'):
            t = _dev_img(img, dev, order)
            png = encode_png(t, order=order, matches=True)
            assert np.array_equal(pil_rgba(png), img), order
            assert len(encode_zlib(t, order, matches=True)) <= len(encode_zlib(t, order))


@pytest.mark.parametrize('rows', [1, 2, 7, 0])
def test_band_seams(dev, rows):
    from ciaosr_amd.png_hip import encode_png
    for img in (rotated_view(37, 45), sprite0(37, 45), stripes(23, 31)):
        png = encode_png(_dev_img(img, dev), order=_order(img), rows_per_band=rows, matches=True)
        assert np.array_equal(_pixels(png, img.shape[2]), img), rows


def test_pitched_crop(dev):
    from ciaosr_amd.png_hip import encode_png
    for big in (rotated_view(61, 90), sprite0(61, 90)):
        t = _dev_img(big, dev)
        view = t[9:48, 12:78]
        assert not view.is_contiguous()
        png = encode_png(view, order=_order(big), matches=True)
        assert np.array_equal(_pixels(png, big.shape[2]), big[9:48, 12:78])
        assert png == encode_png(view.contiguous(), order=_order(big), matches=True)


# ---- 2: tokens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TOKEN_IMAGES)
def test_tokens_are_the_contracts_parse(dev, name):
    from ciaosr_amd import png_hip
    c = _coded(name, dev)
    assert zlib.decompress(c['z_lz']) == c['stream']
    assert png_hip.zlib_stream(c['lz'], c['partials']) == c['z_lz']                # the stages compose to the one-call encoder
    assert png_hip.zlib_stream(c['lit'], c['partials']) == c['z_lit']
    in_match_mode = 0
    for i, (seg, lit) in enumerate(zip(c['lz'], c['lit'])):
        band = c['stream'][c['offs'][i]:c['offs'][i + 1]]
        assert len(seg) <= len(lit), i                                             # 4: never larger, per band
        if seg == lit:                                                             # the parent's literal-only or stored block
            continue
        last = i == len(c['lz']) - 1
        blocks, data, end = mref.inflate_tokens(seg if last else seg + FINAL)
        assert data == band, i
        assert [b['type'] for b in blocks[:2]] == [2, 0] and blocks[1]['tokens'] == [] and blocks[1]['end'] == len(seg), i
        assert blocks[0]['tokens'] == mref.parse(band, c['line'], c['bpp']), i
        assert any(isinstance(t, tuple) for t in blocks[0]['tokens'])
        used = [v for v in blocks[0]['dist'] if v]
        assert blocks[0]['dist'][-1] != 0 and (len(blocks[0]['ll']) == 257 or blocks[0]['ll'][-1] != 0)     # HLIT, HDIST trimmed
        assert used == [1] or sum(2.0 ** -v for v in used) == 1.0                  # one lone code of one bit, or a complete code
        in_match_mode += 1
    print(f'{name}: {in_match_mode} of {len(c["lz"])} bands in match mode')
    if name in MUST_MATCH:
        assert in_match_mode >= 1


# ---- 3: edges of the contract ----------------------------------------------------------------------------------------------------------
def _deflate(data, offsets, dev, line=0, bpp=1, matches=True):
    from ciaosr_amd.png_hip import deflate_huff
    return deflate_huff(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev), offsets, matches=matches, line=line, bpp=bpp)


def _tokens(seg, last=True):
    blocks, data, _ = mref.inflate_tokens(seg if last else seg + FINAL)
    return blocks[0]['type'], blocks[0]['tokens'], data


def _noise(n, seed, values=256):
    return np.random.RandomState(seed).randint(0, values, n, dtype=np.uint8).tobytes()


def _filler(n, seed):
    """n bytes of a compressible kind without runs: successive bytes always differ, and by more than the near distances repeat."""
    v = np.random.RandomState(seed).randint(1, 9, n).cumsum() % 64
    return v.astype(np.uint8).tobytes()


def _edge_case(data, dev, line=0, bpp=1):
    """One band, the match coder: the tokens must be the contract's parse (or the block the literal coder's)."""
    seg, = _deflate(data, [0, len(data)], dev, line, bpp)
    lit, = _deflate(data, [0, len(data)], dev, matches=False)
    assert zlib.decompress(seg, wbits=-15) == data and len(seg) <= len(lit)
    kind, tokens, _ = _tokens(seg)
    if seg != lit:
        assert kind == 2 and tokens == mref.parse(data, line, bpp)
    return seg, lit, tokens


def test_runs_of_seven_and_eight(dev):
    # a run of k equal bytes behind its first byte offers a match of k - 1 at distance 1
    body = _filler(3000, 1)
    for run, want in ((8, False), (9, True)):                       # 7 repeated bytes: no match; 8: a match of 8
        data = body[:1500] + b'\xee' * run + body[1500:] + b'\x00' * 600       # the zeros make the band a match band in both cases
        seg, lit, tokens = _edge_case(data, dev)
        assert seg != lit
        at = tokens.index(0xee)
        assert (tokens[at + 1] == (8, 1)) is want
        assert tokens[at + 1] == ((8, 1) if want else 0xee)


def test_run_of_258_plus_8(dev):
    data = _filler(100, 2) + b'\x91' * (1 + 258 + 8) + _filler(100, 3)
    seg, lit, tokens = _edge_case(data, dev)
    at = tokens.index(0x91)
    assert seg != lit and tokens[at + 1:at + 3] == [(258, 1), (8, 1)]


def test_run_across_a_chunk_boundary(dev):
    data = _filler(4000, 4) + b'\xa2' * 200 + _filler(500, 5)       # the run covers 4000 .. 4199; the chunk ends at 4096
    seg, lit, tokens = _edge_case(data, dev)
    at = tokens.index(0xa2)
    assert seg != lit and tokens[at + 1:at + 3] == [(95, 1), (104, 1)]           # 4001 .. 4095, then a new match from 4096
    data = _filler(4090, 6) + b'\xb3' * 10 + _filler(500, 7) + b'\x00' * 300    # 4090 .. 4099: 5 left before the end, 4 behind it
    seg, lit, tokens = _edge_case(data, dev)
    at = tokens.index(0xb3)
    assert seg != lit and tokens[at:at + 10] == [0xb3] * 10                       # capped below 8 on both sides: literals


def test_a_source_before_the_band_is_not_taken(dev):
    block = _noise(40, 8)
    data = block + block + b'\x00' * 300 + _filler(200, 9)          # band 1 repeats band 0 at distance 40 = line: only from before it
    segs = _deflate(data, [0, 40, len(data)], dev, line=40, bpp=4)
    assert zlib.decompress(b''.join(segs), wbits=-15) == data
    kind, tokens, out = _tokens(segs[1])
    assert out == data[40:] and kind == 2 and tokens == mref.parse(data[40:], 40, 4)
    assert tokens[:40] == list(block)
    # the same bytes as ONE band: the second block is a match at the line distance
    seg, lit, tokens = _edge_case(data, dev, line=40, bpp=4)
    assert seg != lit and tokens[40] == (40, 40)


def test_line_above_32768_and_line_zero(dev):
    row = _filler(33000, 10)
    data = row + row[:3000]                                          # repeats at distance 33000 only
    for line in (33000, 0):
        seg, lit, tokens = _edge_case(data, dev, line=line, bpp=1)
        assert not any(isinstance(t, tuple) for t in mref.parse(data, line, 1)) and seg == lit
    row = _filler(5000, 11)
    data = row + row[:3000]
    seg, lit, tokens = _edge_case(data, dev, line=5000, bpp=3)
    assert seg != lit and any(isinstance(t, tuple) and t[1] == 5000 for t in tokens)
    seg0, lit0, _ = _edge_case(data, dev, line=0)
    assert seg0 == lit0 == lit


def test_a_single_distance_symbol(dev):
    data = _filler(300, 12) + b'\xc4' * 700 + _filler(300, 13) + b'\xd5' * 90
    seg, lit, tokens = _edge_case(data, dev)
    assert seg != lit and {t[1] for t in tokens if isinstance(t, tuple)} == {1}
    blocks, _, _ = mref.inflate_tokens(seg)
    assert blocks[0]['dist'] == [1]                                  # HDIST = 1 and the one code has one bit
    assert zlib.decompress(seg, wbits=-15) == data


def test_random_bytes_fall_back(dev):
    n = 70001
    data = _noise(n, 14)
    seg, lit, _ = _edge_case(data, dev, line=301, bpp=3)
    assert seg == lit and len(seg) <= n + 5 * -(-n // 65535)


def test_several_bands_not_from_zero(dev):
    parts = [_filler(5000, 15), b'\x00' * 9000, b'z', _noise(70001, 16), (b'abcde' * 2000), _noise(17, 17), b'\x07' * 8200, b'q']
    data = b'junk' + b''.join(parts) + b'tail'
    offs = [4]
    for p in parts:
        offs.append(offs[-1] + len(p))
    segs = _deflate(data, offs, dev, line=25, bpp=5)
    lits = _deflate(data, offs, dev, matches=False)
    assert zlib.decompress(b''.join(segs), wbits=-15) == b''.join(parts)
    modes = []
    for i, (s, lit, p) in enumerate(zip(segs, lits, parts)):
        assert len(s) <= len(lit), i
        kind, tokens, out = _tokens(s, last=i == len(parts) - 1)
        assert out == p, i
        modes.append(s != lit)
        if s != lit:
            assert kind == 2 and tokens == mref.parse(p, 25, 5), i
    assert modes == [False, True, False, False, True, False, True, False]


# ---- 5: sizes ------------------------------------------------------------------------------------------------------------------------
def test_transparent_tile_is_a_twentieth(dev):
    c = _coded('transparent', dev)
    print(f'transparent 256 x 256: matches {len(c["z_lz"])} B, literals {len(c["z_lit"])} B ({len(c["z_lz"]) / len(c["z_lit"]):.4f})')
    assert 20 * len(c['z_lz']) <= len(c['z_lit'])


@pytest.mark.parametrize('name', TOKEN_IMAGES)
def test_size_against_the_model_and_pillow(dev, name):
    c = _coded(name, dev)
    model = mref.model_bytes(c['stream'], c['offs'], c['line'], c['bpp'])
    pil = _pil_size(c['img']) - ref.png_overhead()
    print(f'{name}: matches {len(c["z_lz"])} B, literals {len(c["z_lit"])} B ({len(c["z_lz"]) / len(c["z_lit"]):.4f}), model {model} B '
          f'({len(c["z_lz"]) / model:.4f}), Pillow IDAT {pil} B ({len(c["z_lz"]) / pil:.4f})')
    assert len(c['z_lz']) <= len(c['z_lit'])
    assert len(c['z_lz']) <= 1.01 * model
    if name == 'sprite0':
        from ciaosr_amd.png_hip import encode_png
        assert len(encode_png(c['t'], 'rgba', matches=True)) <= _pil_size(c['img'])


# ---- 6: tiles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [3, 4])
def test_tiles_are_the_single_encoder(dev, channels):
    from ciaosr_amd.png_hip import encode_png, encode_png_tiles
    img = rotated_view(150, 170, channels)
    img[100:, 120:] = 0                                              # a corner block that is wholly fill / transparent
    order = _order(img)
    t = _dev_img(img, dev)
    rects = [(0, 0, 150, 170), (0, 0, 64, 64), (60, 50, 70, 33), (63, 49, 66, 120), (5, 7, 1, 1), (110, 125, 40, 45), (149, 0, 1, 170),
             (0, 169, 150, 1)]
    for rows in (0, 5):
        files = encode_png_tiles(t, rects, order, rows, matches=True)
        plain = encode_png_tiles(t, rects, order, rows)
        for k, (y0, x0, h, w) in enumerate(rects):
            assert files[k] == encode_png(t[y0:y0 + h, x0:x0 + w], order, rows, matches=True), (rows, k)
            assert np.array_equal(_pixels(files[k], channels), img[y0:y0 + h, x0:x0 + w]), (rows, k)
            assert len(files[k]) <= len(plain[k]), (rows, k)
        # the empty 40 x 45 corner, n = 5440 (RGB) filtered bytes: literals cost at least n / 8 = 680 B; 22 matches of 258 at no more
        # than 4 bits each, a header of under 30 B and 10 B of framing stay below a tenth of that
        z_lz, z_lit = len(files[5]) - ref.png_overhead(), len(plain[5]) - ref.png_overhead()
        assert rows or 10 * z_lz <= z_lit, (z_lz, z_lit)             # (rows = 5: eight bands, each with a header and framing)


# ---- 7: repeatability, launches, copies ------------------------------------------------------------------------------------------------
def _profile_of(fn):
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        out = fn()
    return out, {k: v['launches'] for k, v in hip_ops.profile.results().items()}


def test_launches_copies_and_repeatability(dev, monkeypatch):
    from ciaosr_amd import png_hip
    img = sprite0(120, 130)
    t = _dev_img(img, dev)
    rects = [(0, 0, 120, 130), (0, 0, 60, 60), (30, 30, 60, 70), (100, 100, 20, 30), (0, 0, 1, 1), (7, 9, 50, 3), (60, 0, 60, 130),
             (0, 65, 120, 65), (59, 64, 2, 2)]
    first = png_hip.encode_png_tiles(t, rects, 'rgba', matches=True)
    _, one = _profile_of(lambda: png_hip.encode_png_tiles(t, rects[:1], 'rgba', matches=True))
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
    second, nine = _profile_of(lambda: png_hip.encode_png_tiles(t, rects, 'rgba', matches=True))
    monkeypatch.undo()
    assert [c[0] for c in copies] == ['cpu', 'cpu'] and copies[0][1] == (10,), copies           # the offsets, then the streams
    assert one == nine == dict(png_rgba_filter_tiles_u8=1, deflate_lz_match=1, deflate_plan=1, deflate_lz_plan=1, png_tiles_scan=1,
                               deflate_pack=1, deflate_lz_pack=1)
    assert second == first
    copies.clear()
    for name in ('cpu', 'item', 'tolist', 'numpy', 'to', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    single, launches = _profile_of(lambda: png_hip.encode_png(t, 'rgba', matches=True))
    monkeypatch.undo()
    assert [c[0] for c in copies] == ['item', 'cpu'], copies                                       # the size, then the stream
    assert launches == dict(png_rgba_filter_u8=1, deflate_lz_match=1, deflate_plan=1, deflate_lz_plan=1, deflate_scan=1, deflate_pack=1,
                            deflate_lz_pack=1)
    assert single == first[0]
    torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(0xA5)                              # other bytes in freed memory
    assert png_hip.encode_png_tiles(t, rects, 'rgba', matches=True) == first
    assert png_hip.encode_png(t, 'rgba', matches=True) == single


# ---- 8: off is off -------------------------------------------------------------------------------------------------------------------
def test_without_matches_the_files_are_the_parents(dev):
    from ciaosr_amd import png_hip
    from tools.make_png_parent_golden import RECTS, SMALL, WIDE, image
    gold = np.load(os.path.join(REPO, 'tests', 'golden', 'png_rgb_parent.npz'))
    small, wide = torch.from_numpy(image(*SMALL)).to(dev), torch.from_numpy(image(*WIDE)).to(dev)
    for order in ('bgr', 'rgb'):
        for off in ({}, dict(matches=False)):
            assert png_hip.encode_png(small, order, **off) == gold[f'small_{order}'].tobytes(), order
            assert png_hip.encode_png(small, order, 3, **off) == gold[f'small_{order}_rows3'].tobytes(), order
            for k, data in enumerate(png_hip.encode_png_tiles(wide, RECTS, order, 7, **off)):
                assert data == gold[f'wide_{order}_tile{k}'].tobytes(), (order, k)


# ---- 9: integration ------------------------------------------------------------------------------------------------------------------
def test_forward_test_with_gpu_png_matches(dev, tmp_path):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.coords import make_cell, make_coord
    from ciaosr_amd.imageio import imread_u8
    from ciaosr_amd.init_utils import synthetic_pair
    from tests.test_png_gpu import _restorer
    scale = 2
    lq, gt = synthetic_pair(20, 26, scale)
    h, w = gt.shape[-2:]
    gt_q3 = gt[0].permute(1, 2, 0).reshape(1, h * w, 3).contiguous()
    coord, cell = make_coord((h, w)).unsqueeze(0), make_cell((h, w)).unsqueeze(0)
    files, prof = {}, {}
    for name, extra in (('off', {}), ('png', dict(gpu_png=True)), ('lz', dict(gpu_png=True, gpu_png_matches=True)),
                        ('alone', dict(gpu_png_matches=True))):
        model = _restorer(dict(scale=scale, metrics=['PSNR', 'SSIM'], crop_border=2, convert_to='y', **extra)).to(dev)
        assert model.gpu_png_matches() is (name == 'lz')
        with hip_ops.profile():
            model(lq=lq.to(dev), gt=gt_q3.to(dev), test_mode=True, coord=coord.to(dev), cell=cell.to(dev),
                  meta=[dict(gt_path='/data/img7.png')], save_image=True, save_path=str(tmp_path / name))
        prof[name] = hip_ops.profile.results()
        files[name] = open(str(tmp_path / name / 'img7.png'), 'rb').read()
    want = imread_u8(str(tmp_path / 'off' / 'img7.png'))
    for name in ('png', 'lz', 'alone'):
        assert np.array_equal(imread_u8(str(tmp_path / name / 'img7.png')), want), name
    assert files['alone'] == files['off']                            # the key is read only with gpu_png
    assert len(files['lz']) <= len(files['png'])
    assert prof['lz']['deflate_lz_match']['launches'] == 1 and 'deflate_lz_match' not in prof['png']


def test_render_cli_png_matches(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model
    from ciaosr_amd.config import Config
    from ciaosr_amd.init_utils import seeded_init_
    from tests.test_rgba_gpu import _rgba_input
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    x4 = _rgba_input('cpu', 24, 30)
    x4[:, :3] *= (x4[:, 3:] > 0)                                     # a sprite as files store it: colour 0 under A = 0
    Image.fromarray((x4[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8), 'RGBA').save(png)
    flags = [config, ckpt, png, '--alpha', '--dzi', '4', '--dzi-tile', '32']
    render.main(flags + ['--out', str(tmp_path / 'a')])
    render.main(flags + ['--png-matches', '--out', str(tmp_path / 'b')])
    sizes, n = {'a': 0, 'b': 0}, 0
    for root, _, names in os.walk(str(tmp_path / 'a' / 'img_files')):
        for f in names:
            other = os.path.join(str(tmp_path / 'b'), os.path.relpath(os.path.join(root, f), str(tmp_path / 'a')))
            da, db = open(os.path.join(root, f), 'rb').read(), open(other, 'rb').read()
            assert np.array_equal(pil_rgba(da), pil_rgba(db)), f
            assert len(db) <= len(da), f
            sizes['a'] += len(da)
            sizes['b'] += len(db)
            n += 1
    print(f'{n} tiles: {sizes["a"]} B without --png-matches, {sizes["b"]} B with')
    assert n >= 12 and sizes['b'] < sizes['a']
    assert open(str(tmp_path / 'a' / 'img.dzi'), 'rb').read() == open(str(tmp_path / 'b' / 'img.dzi'), 'rb').read()
