"""Host-side tests of the opt-in PNG encoder (`test_cfg.gpu_png`, ciaosr_amd/png_hip.py, csrc/png_u8.hip): the ABI surface, the numpy
reference validating itself, the container assembly with Python's `zlib` and Pillow's decoder as judges, the CLI flags and the refusal
of host arrays.  Also the image makers that tests/test_png_gpu.py shares."""
import ctypes as C
import io
import os
import zlib

import numpy as np
import pytest
import torch

from tests import png_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTENTS = ['smooth', 'noisy', 'random', 'constant', 'two']


def make_image(h, w, content, seed=0):
    """uint8 [h, w, 3] RGB: 'smooth' = init_utils.synthetic_gt, 'noisy' = the same plus 2 grey levels of noise, 'random' = uniform
    bytes, 'constant', 'two' = two values in random runs."""
    from ciaosr_amd import metrics
    from ciaosr_amd.init_utils import synthetic_gt
    rng = np.random.RandomState(seed * 9973 + 31 * h + w)
    if content in ('smooth', 'noisy'):
        img = np.ascontiguousarray(metrics.tensor2img(synthetic_gt(h, w, seed=1234 + seed))[:, :, ::-1]).reshape(h, w, 3)
        if content == 'noisy':
            img = np.clip(img.astype(np.int64) + rng.randint(-2, 3, img.shape), 0, 255).astype(np.uint8)
        return img
    if content == 'random':
        return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    if content == 'constant':
        return np.full((h, w, 3), 77, dtype=np.uint8)
    if content == 'two':
        return np.where(rng.rand(h, w, 1) < 0.3, np.uint8(200), np.uint8(13)).repeat(3, axis=2).astype(np.uint8)
    raise KeyError(content)


def five_filter_image(w=24, seed=5):
    """uint8 [10, w, 3]: rows built so that each of the five filters wins at least one row under the rule (asserted below, with the
    reference).  Row pairs: an unrelated random row, then a row that one predictor explains up to noise of +-1."""
    rng = np.random.RandomState(seed)
    n = 3 * w
    rows = []
    noise = lambda: rng.randint(-1, 2, n)
    for kind in range(5):
        above = rng.randint(0, 256, n)
        rows.append(above)
        if kind == 0:                                       # None: small values; every predictor adds the neighbour's noise
            cur = (rng.randint(-2, 3, n)) & 255
        elif kind == 1:                                     # Sub: a steep ramp per channel
            cur = (40 + 7 * (np.arange(n) // 3) + noise()) & 255
        elif kind == 2:                                     # Up
            cur = (above + noise()) & 255
        else:
            cur = np.zeros(n, dtype=np.int64)
            e = noise()
            for i in range(n):
                a = cur[i - 3] if i >= 3 else 0
                b = above[i]
                c = above[i - 3] if i >= 3 else 0
                if kind == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (pred + e[i]) & 255
        rows.append(cur)
    return np.stack(rows).astype(np.uint8).reshape(10, w, 3)


def pil_pixels(png_bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(png_bytes))
    assert im.mode == 'RGB'
    return np.asarray(im)


def pil_default_size(rgb):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(rgb).save(bio, format='PNG')
    return len(bio.getvalue())


def band_partials(stream, offsets):
    """(sum of bytes, sum of byte x bytes-to-the-band's-end, length) of each band, the first two mod 65521."""
    out = []
    for i in range(len(offsets) - 1):
        d = np.frombuffer(stream[offsets[i]:offsets[i + 1]], dtype=np.uint8).astype(np.int64)
        n = len(d)
        out.append((int(d.sum() % 65521), int((d * (n - np.arange(n))).sum() % 65521), n))
    return out


def test_abi_surface():
    from ciaosr_amd import _lib
    lib = _lib.load()
    assert lib.ciaosr_version() >= 270
    for name in ('ciaosr_png_filter_u8', 'ciaosr_deflate_huff_u8', 'ciaosr_png_encode_u8'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # the default band: about 128 KiB of scanline bytes; 5 rows at 8160 pixels
    assert lib.ciaosr_png_rows_per_band(8160, 0) == 5 and lib.ciaosr_png_rows_per_band(384, 0) == 131072 // 1153
    assert lib.ciaosr_png_rows_per_band(65535, 0) == 1 and lib.ciaosr_png_rows_per_band(8160, 7) == 7
    assert lib.ciaosr_png_rows_per_band(0, 0) == 0 and lib.ciaosr_png_rows_per_band(65536, 0) == 0
    # capacity covers the all-stored worst case: raw bytes + 5 per started 65535 of every band + zlib framing
    for h, w, r in [(1, 1, 0), (256, 384, 0), (256, 384, 1), (5424, 8160, 0), (65535, 3, 1)]:
        rows = lib.ciaosr_png_rows_per_band(w, r)
        line, nb = 3 * w + 1, -(-h // rows)
        worst = sum(n + 5 * -(-n // 65535) for n in [rows * line] * (nb - 1) + [(h - (nb - 1) * rows) * line]) + 6
        assert lib.ciaosr_png_capacity_bytes(h, w, r) >= worst, (h, w, r)
        assert lib.ciaosr_png_workspace_bytes(h, w, r) >= h * line + nb * (2 * 260 * 4 + 64 * 4)
    assert lib.ciaosr_png_capacity_bytes(65536, 4, 0) == 0 and lib.ciaosr_png_workspace_bytes(4, 65536, 0) == 0
    assert lib.ciaosr_deflate_huff_capacity_bytes(C.c_size_t(65536), 1) >= 65536 + 10
    assert lib.ciaosr_deflate_huff_workspace_bytes(0) == 0 and lib.ciaosr_deflate_huff_workspace_bytes(3) > 0


@pytest.mark.parametrize('h,w,content', [(1, 1, 'random'), (7, 5, 'random'), (33, 17, 'smooth'), (33, 17, 'two'), (10, 24, 'five')])
def test_reference_validates_itself(h, w, content):
    img = five_filter_image(w) if content == 'five' else make_image(h, w, content)
    stream, best = ref.filter_stream(img)
    assert len(stream) == h * (3 * w + 1) and list(stream[::3 * w + 1]) == list(best)
    assert np.array_equal(ref.unfilter(stream, h, w), img)
    assert np.array_equal(pil_pixels(ref.png_from_stream(stream, h, w)), img)
    if content == 'five':
        assert set(best.tolist()) == {0, 1, 2, 3, 4}, best
    # the rule, restated for one row without the vectorised code: smallest sum of min(b, 256 - b), ties to the lowest number
    y = h - 1
    cand = ref.filtered_candidates(img)[:, y]
    sums = [int(sum(min(int(b), 256 - int(b)) for b in cand[k])) for k in range(5)]
    assert int(best[y]) == sums.index(min(sums))


def test_optimal_huffman_model():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    depth = ref.huffman_lengths(fib)
    assert max(depth.values()) == 23 and sum(2.0 ** -d for d in depth.values()) == 1.0
    assert ref.huffman_lengths([0, 5, 0]) == {1: 1}
    flat = ref.huffman_lengths([3] * 256)
    assert set(flat.values()) == {8}
    stream = bytes(range(256)) * 4
    assert ref.band_split(5, 10, 2) == [0, 20, 40, 50] and ref.band_split(4, 10, 2) == [0, 20, 40] and ref.band_split(3, 7, 5) == [0, 21]
    # 256 symbols of count 4 and one end-of-block: the payload is a little over 8 bits per byte
    bits, deepest = ref.band_model_bits(stream)
    assert 8 * len(stream) < bits < 8 * len(stream) + 1200 and deepest in (8, 9, 10)


def test_container_from_made_up_segments():
    from PIL import Image
    from ciaosr_amd import png_hip
    h, w = 33, 17
    img = make_image(h, w, 'noisy')
    stream, _ = ref.filter_stream(img)
    offsets = ref.band_split(h, 3 * w + 1, 7)
    # made-up band segments: zlib's own raw deflate, flushed to a byte boundary at every seam (an empty stored block, as the device's)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    segments = []
    for i in range(len(offsets) - 1):
        part = co.compress(stream[offsets[i]:offsets[i + 1]])
        part += co.flush(zlib.Z_FINISH if i == len(offsets) - 2 else zlib.Z_FULL_FLUSH)
        segments.append(part)
    partials = band_partials(stream, offsets)
    assert png_hip.adler32_combine(partials) == zlib.adler32(stream)
    assert png_hip.adler32_combine(band_partials(stream, [0, len(stream)])) == zlib.adler32(stream)
    z = png_hip.zlib_stream(segments, partials)
    assert zlib.decompress(z) == stream
    bad = png_hip.zlib_stream(segments, partials[:-1] + [(partials[-1][0] ^ 1, partials[-1][1], partials[-1][2])])
    with pytest.raises(zlib.error):
        zlib.decompress(bad)
    for idat_max in (png_hip.IDAT_MAX, 100, 1):
        png = png_hip.container(h, w, z, idat_max=idat_max)
        assert png.count(b'IDAT') >= -(-len(z) // idat_max)
        hh, ww, payload = ref.idat_payload(png)                      # checks every CRC with zlib.crc32
        assert (hh, ww) == (h, w) and payload == z
        assert np.array_equal(pil_pixels(png), img)
    # Pillow verifies the CRC of the chunks it parses (IHDR here; it skips over the IDAT CRCs, which idat_payload checked above)
    good = png_hip.container(h, w, z, idat_max=100)
    png = bytearray(good)
    png[8 + 8 + 13] ^= 0x40                                          # IHDR's CRC
    with pytest.raises(Exception):
        Image.open(io.BytesIO(bytes(png))).load()
    png = bytearray(good)
    png[png.index(b'IDAT') + 4 + 100] ^= 0x40                        # the first IDAT chunk's CRC
    with pytest.raises(AssertionError):
        ref.idat_payload(bytes(png))
    with pytest.raises(ValueError):
        png_hip.container(h, w, z, idat_max=1 << 31)


def test_cli_flags_reach_test_cfg():
    import ciaosr_amd
    import tools.render as render_cli
    import tools.test as cli
    from ciaosr_amd.config import Config
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    for argv, want in ([], False), (['--gpu-png'], True), (['--gpu-png', '--gpu-metrics'], True):
        args = cli.parse_args([path, 'None'] + argv)
        assert args.gpu_png is want
        cfg = cli.apply_overrides(Config.fromfile(path), args)
        model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        assert bool(model.test_cfg.get('gpu_png', False)) is want and model.gpu_png() is want
        assert model.gpu_metrics() is ('--gpu-metrics' in argv)
    assert render_cli.parse_args([path, 'None', 'x.png', '--scale', '2', '--out', 'o']).gpu_png is False
    assert render_cli.parse_args([path, 'None', 'x.png', '--scale', '2', '--out', 'o', '--gpu-png']).gpu_png is True


def test_encode_png_refuses_host_arrays(tmp_path):
    from ciaosr_amd import png_hip
    from ciaosr_amd._lib import CiaoSRHipError
    img = make_image(7, 5, 'random')
    with pytest.raises(CiaoSRHipError):
        png_hip.encode_png(img)
    with pytest.raises(CiaoSRHipError):
        png_hip.encode_png(torch.from_numpy(img))
    with pytest.raises(CiaoSRHipError):
        png_hip.imwrite_gpu(torch.from_numpy(img), str(tmp_path / 'never_written.png'))
    assert not (tmp_path / 'never_written.png').exists()
    with pytest.raises(CiaoSRHipError):
        png_hip.deflate_huff(torch.zeros(10, dtype=torch.uint8), [0, 10])
