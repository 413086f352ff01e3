"""GPU tests of the opt-in PNG encoder (csrc/png_u8.hip, ciaosr_amd/png_hip.py, `test_cfg.gpu_png`).  The judges are Pillow's decoder,
Python's `zlib` and the numpy reference of tests/png_reference.py -- never the device against itself.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import png_reference as ref
from tests.test_png_host import CONTENTS, band_partials, five_filter_image, make_image, pil_default_size, pil_pixels

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (5, 1), (7, 5), (33, 17), (96, 128), (256, 384)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _dev_img(rgb, order, dev):
    """The device tensor `encode_png(..., order)` takes for the RGB image `rgb`."""
    arr = rgb[:, :, ::-1] if order == 'bgr' else rgb
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


# ---- round trip ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
def test_round_trip_is_bit_exact(dev, h, w):
    from ciaosr_amd.png_hip import encode_png
    for content in CONTENTS:
        rgb = make_image(h, w, content)
        for order in ('bgr', 'rgb'):
            png = encode_png(_dev_img(rgb, order, dev), order=order)
            assert np.array_equal(pil_pixels(png), rgb), (content, order)
            hh, ww, z = ref.idat_payload(png)
            assert (hh, ww) == (h, w) and len(zlib.decompress(z)) == h * (3 * w + 1)


def test_round_trip_of_a_pitched_crop(dev):
    from ciaosr_amd.png_hip import encode_png
    big = make_image(61, 90, 'noisy')
    t = _dev_img(big, 'bgr', dev)
    view = t[9:48, 11:78]                                   # 39 x 67 inside 61 x 90: pitch 270 bytes, rows of 201
    assert not view.is_contiguous()
    png = encode_png(view)
    assert np.array_equal(pil_pixels(png), big[9:48, 11:78])
    assert png == encode_png(view.contiguous())            # the bytes do not depend on the pitch


@pytest.mark.parametrize('rows', [1, 2, 7, 0])
def test_band_seams(dev, rows):
    """Images R - 1, R, R + 1 and 2 R + 1 rows high for R = rows_per_band (the default's R comes from the library)."""
    from ciaosr_amd import _lib
    from ciaosr_amd.png_hip import encode_png, encode_zlib
    w = 384 if rows == 0 else 23
    r = _lib.load().ciaosr_png_rows_per_band(w, rows)
    assert r == (rows or 131072 // (3 * w + 1))
    for h in (r - 1, r, r + 1, 2 * r + 1):
        if h < 1:
            continue
        rgb = make_image(h, w, 'noisy', seed=rows)
        t = _dev_img(rgb, 'bgr', dev)
        assert np.array_equal(pil_pixels(encode_png(t, rows_per_band=rows)), rgb), (rows, h)
        assert zlib.decompress(encode_zlib(t, rows_per_band=rows)) == ref.filter_stream(rgb)[0]


# ---- the filter stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,content', [(10, 24, 'five'), (33, 17, 'random'), (33, 17, 'two'), (7, 5, 'constant'), (96, 128, 'smooth'),
                                         (256, 384, 'noisy'), (1, 1, 'random'), (300, 5, 'random')])
def test_filter_stage_is_the_reference_stream(dev, h, w, content):
    from ciaosr_amd.png_hip import encode_png, filter_u8
    rgb = five_filter_image(w) if content == 'five' else make_image(h, w, content)
    want, best = ref.filter_stream(rgb)
    if content in ('five', 'random') and h >= 10 and w > 1:
        assert len(set(best.tolist())) == 5 if content == 'five' else len(set(best.tolist())) >= 3
    for order in ('bgr', 'rgb'):
        t = _dev_img(rgb, order, dev)
        _, _, z = ref.idat_payload(encode_png(t, order=order, rows_per_band=3))
        assert zlib.decompress(z) == want, (content, order)
    # the stage on its own: stream, per-band histograms (with one end-of-block) and Adler partial sums
    stream, hist, adler = filter_u8(_dev_img(rgb, 'bgr', dev), rows_per_band=3)
    assert stream.cpu().numpy().tobytes() == want
    offs = ref.band_split(h, 3 * w + 1, 3)
    hist, adler = hist.cpu().numpy(), adler.cpu().numpy()
    for i, (s1, s2, n) in enumerate(band_partials(want, offs)):
        assert hist[i, :257].tolist() == ref.band_histogram(want[offs[i]:offs[i + 1]]), i
        assert (int(adler[i, 0]), int(adler[i, 1])) == (s1, s2), i


# ---- the deflate stage on crafted buffers -----------------------------------------------------------------------------------------------
def _fibonacci_buffer():
    """24 byte values with the Fibonacci counts 1, 2, 3, 5, ...: unlimited Huffman depth 23, and 24 once the coder's end-of-block
    (count 1) joins them -- far beyond deflate's 15, so the length limiter has to act."""
    fib = [1, 2]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert max(ref.huffman_lengths(fib).values()) == 23 and max(ref.huffman_lengths(fib + [1]).values()) == 24
    rng = np.random.RandomState(3)
    buf = np.concatenate([np.full(f, 10 * i + 3, dtype=np.uint8) for i, f in enumerate(fib)])
    rng.shuffle(buf)
    return buf.tobytes()


def _deflate(data, offsets, dev):
    from ciaosr_amd.png_hip import deflate_huff
    return deflate_huff(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev), offsets)


def _stored_bound(n):
    return n + 5 * -(-n // 65535)


def test_deflate_length_limiter(dev):
    data = _fibonacci_buffer()
    seg, = _deflate(data, [0, len(data)], dev)
    assert zlib.decompress(seg, wbits=-15) == data
    assert len(seg) < 0.45 * len(data)                                   # entropy 2.6 bits per byte; a broken limiter falls back to stored


@pytest.mark.parametrize('case', ['one_value', 'all_values', 'len1', 'len65535', 'len65536', 'len65537'])
def test_deflate_crafted_buffers(dev, case):
    rng = np.random.RandomState(11)
    if case == 'one_value':
        data = b'\x07' * 5000
    elif case == 'all_values':
        data = rng.permutation(np.arange(256, dtype=np.uint8).repeat(40)).tobytes()
    else:
        data = (rng.randint(0, 6, int(case[3:])) * 41).astype(np.uint8).tobytes()          # six values: compressible at any length
    seg, = _deflate(data, [0, len(data)], dev)
    assert zlib.decompress(seg, wbits=-15) == data
    assert len(seg) <= _stored_bound(len(data))
    if case == 'one_value':
        assert len(seg) < 5000 // 8 + 120
    if case.startswith('len6'):
        assert len(seg) < 0.4 * len(data)


@pytest.mark.parametrize('n', [1, 300, 65535, 65536, 65537, 140000])
def test_deflate_incompressible_falls_back_to_stored(dev, n):
    data = np.random.RandomState(n).randint(0, 256, n, dtype=np.uint8).tobytes()
    seg, = _deflate(data, [0, n], dev)
    assert zlib.decompress(seg, wbits=-15) == data
    assert len(seg) <= _stored_bound(n)                                   # input + 5 bytes per started 65535, no other framing


def test_deflate_several_bands_and_empty_band(dev):
    from ciaosr_amd._lib import CiaoSRHipError
    rng = np.random.RandomState(5)
    parts = [_fibonacci_buffer()[:5000], rng.randint(0, 256, 70001, dtype=np.uint8).tobytes(), b'\x00' * 3,
             (rng.randint(0, 3, 65536) * 100).astype(np.uint8).tobytes(), rng.randint(0, 256, 17, dtype=np.uint8).tobytes(), b'z']
    data = b'junk' + b''.join(parts) + b'tail'                             # bands need not start at 0 or end at the buffer's end
    offs = [4]
    for p in parts:
        offs.append(offs[-1] + len(p))
    segs = _deflate(data, offs, dev)
    assert len(segs) == len(parts)
    assert zlib.decompress(b''.join(segs), wbits=-15) == b''.join(parts)
    for i, (s, p) in enumerate(zip(segs, parts)):
        assert len(s) <= _stored_bound(len(p)), i
        if i < len(parts) - 1:                                              # not final: decodable only with a final block behind it
            assert zlib.decompress(s + b'\x01\x00\x00\xff\xff', wbits=-15) == p, i
        else:
            assert zlib.decompress(s, wbits=-15) == p
    for bad in ([4, 9, 9, 20], [4, 4, 20], [9, 4]):
        with pytest.raises(CiaoSRHipError, match='bad argument'):
            _deflate(data, bad, dev)


def test_stages_compose_to_the_encoder(dev):
    """filter_u8 + deflate_huff assembled on the host (png_hip.zlib_stream) give the bytes of the one-call encoder."""
    from ciaosr_amd import png_hip
    rgb = make_image(33, 17, 'noisy')
    t = _dev_img(rgb, 'bgr', dev)
    stream, _, adler = png_hip.filter_u8(t, rows_per_band=7)
    offs = ref.band_split(33, 52, 7)
    segs = png_hip.deflate_huff(stream, offs)
    partials = [(int(a), int(b), offs[i + 1] - offs[i]) for i, (a, b) in enumerate(adler.cpu().tolist())]
    assert png_hip.zlib_stream(segs, partials) == png_hip.encode_zlib(t, rows_per_band=7)


# ---- repeatability and size ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(dev):
    from ciaosr_amd.png_hip import encode_png
    for content, rows in (('noisy', 0), ('smooth', 5), ('random', 2)):
        t = _dev_img(make_image(256, 384, content), 'bgr', dev)
        first = encode_png(t, rows_per_band=rows)
        torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(0xA5)      # other bytes in freed memory
        assert encode_png(t, rows_per_band=rows) == first


@pytest.mark.parametrize('content', ['smooth', 'noisy'])
def test_size_against_pillow_and_the_huffman_model(dev, content):
    from ciaosr_amd import _lib
    from ciaosr_amd.png_hip import encode_png
    h, w = 256, 384
    rgb = make_image(h, w, content)
    png = encode_png(_dev_img(rgb, 'bgr', dev))
    pil = pil_default_size(rgb)
    stream, _ = ref.filter_stream(rgb)
    offs = ref.band_split(h, 3 * w + 1, _lib.load().ciaosr_png_rows_per_band(w, 0))
    model = ref.model_bytes(stream, offs) + ref.png_overhead()
    deepest = max(ref.band_model_bits(stream[offs[i]:offs[i + 1]])[1] for i in range(len(offs) - 1))
    print(f'{content}: device {len(png)} B, Pillow {pil} B ({len(png) / pil:.4f}), model {model} B ({len(png) / model:.4f}), '
          f'{len(offs) - 1} bands, unlimited depth {deepest}')
    assert len(png) <= 1.02 * pil
    assert len(png) <= 1.01 * model


# ---- integration ------------------------------------------------------------------------------------------------------------------------
def _restorer(test_cfg):
    """The small EDSR model of __graft_entry__.smoke()."""
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    from ciaosr_amd.init_utils import seeded_init_
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[64, 64])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=16, num_blocks=2),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                   test_cfg=test_cfg).eval()
    seeded_init_(model, seed=3, gain=2.0, head_gain=6 ** 0.5)
    return model


def test_forward_test_writes_the_same_pixels(dev, tmp_path):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.coords import make_cell, make_coord
    from ciaosr_amd.imageio import imread_u8
    from ciaosr_amd.init_utils import synthetic_pair
    scale = 2
    lq, gt = synthetic_pair(20, 26, scale)
    h, w = gt.shape[-2:]
    gt_q3 = gt[0].permute(1, 2, 0).reshape(1, h * w, 3).contiguous()
    coord, cell = make_coord((h, w)).unsqueeze(0), make_cell((h, w)).unsqueeze(0)
    res, files, prof = {}, {}, {}
    for name, extra in (('off', {}), ('png', dict(gpu_png=True)), ('metrics', dict(gpu_metrics=True)),
                        ('both', dict(gpu_png=True, gpu_metrics=True))):
        model = _restorer(dict(scale=scale, metrics=['PSNR', 'SSIM'], crop_border=2, convert_to='y', **extra))
        model = model.to(dev)
        out = tmp_path / name
        with hip_ops.profile():
            res[name] = model(lq=lq.to(dev), gt=gt_q3.to(dev), test_mode=True, coord=coord.to(dev), cell=cell.to(dev),
                              meta=[dict(gt_path='/data/img7.png')], save_image=True, save_path=str(out))['eval_result']
        prof[name] = hip_ops.profile.results()
        files[name] = str(out / 'img7.png')
        assert os.path.exists(files[name])
    want = imread_u8(files['off'])
    assert want.shape == (h, w, 3)
    for name in ('png', 'metrics', 'both'):
        assert np.array_equal(imread_u8(files[name]), want), name
    assert open(files['metrics'], 'rb').read() == open(files['off'], 'rb').read()        # the default writer, unchanged
    assert open(files['png'], 'rb').read() == open(files['both'], 'rb').read() != open(files['off'], 'rb').read()
    for name in ('off', 'metrics'):
        assert 'png_filter_u8' not in prof[name] and 'deflate_pack' not in prof[name]
    for name in ('png', 'both'):
        assert prof[name]['png_filter_u8']['launches'] == 1 and prof[name]['deflate_pack']['launches'] == 1
    assert 'tensor2img_u8' not in prof['off'] and prof['png']['tensor2img_u8']['launches'] == 1
    assert prof['both']['tensor2img_u8']['launches'] == 2                               # the output ONCE, for metrics and file; the GT
    assert res['png'] == res['off'] and res['both'] == res['metrics']


def test_render_cli_gpu_png(dev, tmp_path):
    from PIL import Image
    from ciaosr_amd import build_model, hip_ops
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread_u8
    from ciaosr_amd.init_utils import seeded_init_
    from tools import render
    config = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    cfg = Config.fromfile(config)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=23, gain=1.2, head_gain=6 ** 0.5)
    ckpt, png = str(tmp_path / 'w.pth'), str(tmp_path / 'img.png')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    Image.fromarray(make_image(24, 30, 'smooth')).save(png)
    argv = [config, ckpt, png, '--scale', '2.5', '--view', '11.0', '14.5', '2.2', '20', '--size', '37', '45']
    plain = render.main(argv + ['--out', str(tmp_path / 'plain')])
    with hip_ops.profile():
        fast = render.main(argv + ['--gpu-png', '--out', str(tmp_path / 'fast')])
    prof = hip_ops.profile.results()
    assert [os.path.basename(p) for p in fast] == [os.path.basename(p) for p in plain] == ['img_x2p5.png', 'img_view0.png']
    assert prof['png_filter_u8']['launches'] == 2 and prof['tensor2img_u8']['launches'] == 2
    for a, b in zip(plain, fast):
        assert np.array_equal(imread_u8(a), imread_u8(b)), b
    assert imread_u8(fast[0]).shape == (60, 75, 3) and imread_u8(fast[1]).shape == (37, 45, 3)
