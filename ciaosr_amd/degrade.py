"""GT -> LR degradation of the reference's GT-only test data (configs/001_*.py, `val_scale > 4`): mmedit 0.x's
`RandomDownSampling` with `patch_size=None`, whose resize is `mmcv.imresize(gt, (w, h), 'bicubic', backend='pillow')`, i.e.
`PIL.Image.fromarray(gt_u8).resize((w, h), Image.BICUBIC)`.

The resize runs on the MI355X (ciaosr_resample_u8, csrc/resample_u8.hip) and is bitwise equal to Pillow's 8-bit resample, which
is integer arithmetic once the coefficient tables are fixed.  The tables are built here, on the host, in float64 and in Pillow's
operation order (Resample.c: precompute_coeffs + normalize_coeffs_8bpc): computing them on the device would let the compiler
contract a multiply-add into an FMA, and one changed double flips a rounded coefficient.

mmedit and mmcv are not dependencies of this project: the RandomDownSampling rules below are restated from the public mmedit 0.x
source (mmedit/datasets/pipelines/random_down_sampling.py) and could not be checked against it offline.  The Pillow rules are
checked against Pillow itself (tests/test_degrade_host.py, tests/test_degrade_gpu.py).
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import CiaoSRHipError

PRECISION_BITS = 22           # Pillow's 8-bit resample: 32 - 8 - 2 fractional bits
BICUBIC_A = -0.5
BICUBIC_SUPPORT = 2.0


def bicubic_filter(x):
    """Pillow's bicubic kernel (a = -0.5), same operation order as Resample.c."""
    a = BICUBIC_A
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def pillow_bicubic_tables(n_in, n_out):
    """Coefficient tables of one axis of Pillow's bicubic resample from n_in to n_out samples.

    Returns (bounds int32 [n_out, 2] = (xmin, count), coef int32 [n_out, ksize], ksize); tap t of output o reads input
    xmin + t with the fixed-point weight coef[o, t] (22 fractional bits), for t < count; coef is 0 beyond count."""
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f'resample sizes must be positive, got {n_in} -> {n_out}')
    scale = float(n_in) / n_out
    filterscale = max(scale, 1.0)
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[o, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds[o] = (xmin, xmax)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef, ksize


_dev_tables = {}


def _device_tables(n_in, n_out, device):
    """(bounds, coef, ksize) of pillow_bicubic_tables on `device`, cached per (n_in, n_out, device)."""
    key = (n_in, n_out, device.index)
    hit = _dev_tables.get(key)
    if hit is None:
        b, k, ks = pillow_bicubic_tables(n_in, n_out)
        if len(_dev_tables) > 64:
            _dev_tables.clear()
        hit = _dev_tables[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(k.copy()).to(device), ks)
    return hit


def _check_image(img):
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise CiaoSRHipError('resize_bicubic_u8 runs on the MI355X only: pass a uint8 HxWx3 cuda tensor (no CPU fallback)')
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise CiaoSRHipError(f'expected a uint8 HxWx3 image, got {img.dtype} {tuple(img.shape)}')
    if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * img.shape[1]:
        raise CiaoSRHipError('expected HWC rows of 3*W contiguous bytes (a top-left crop of a wider image is fine)')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')


def resample_u8(img, size, want_u8=True, want_chw=False):
    """Pillow-exact bicubic resize of a uint8 HWC image on the GPU.  `size` = (w, h) as in PIL.  Returns
    (dst_u8 [h, w, 3] uint8 or None, dst_chw [3, h, w] float32 = dst_u8 / 255 or None)."""
    from . import hip_ops
    _check_image(img)
    w_out, h_out = int(size[0]), int(size[1])
    h_in, w_in = img.shape[0], img.shape[1]
    if w_out <= 0 or h_out <= 0 or h_in <= 0 or w_in <= 0:
        raise ValueError(f'resize of a {w_in}x{h_in} image to {w_out}x{h_out}')
    dev = img.device
    bx, kx, ksx = _device_tables(w_in, w_out, dev) if w_out != w_in else (None, None, 0)
    by, ky, ksy = _device_tables(h_in, h_out, dev) if h_out != h_in else (None, None, 0)
    dst = torch.empty((h_out, w_out, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    chw = torch.empty((3, h_out, w_out), dtype=torch.float32, device=dev) if want_chw else None
    lib = _lib.load()
    nbytes = lib.ciaosr_resample_u8_workspace_bytes(h_in, w_in, h_out, w_out)
    ws = hip_ops.workspace(nbytes, dev, slot='resample_u8')
    _lib.call('ciaosr_resample_u8', hip_ops.ptr(img), C.c_size_t(img.stride(0)), h_in, w_in, h_out, w_out,
              hip_ops.ptr(bx), hip_ops.ptr(kx), ksx, hip_ops.ptr(by), hip_ops.ptr(ky), ksy,
              hip_ops.ptr(dst), hip_ops.ptr(chw), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return dst, chw


def resize_bicubic_u8(img, size):
    """`PIL.Image.fromarray(img).resize(size, Image.BICUBIC)` of a uint8 HxWx3 cuda tensor, on the GPU; size = (w, h)."""
    return resample_u8(img, size)[0]


def down_size(h, w, scale):
    """mmedit RandomDownSampling (patch_size=None): LR size and the GT crop it comes from.
    Returns (h_lr, w_lr, h_crop, w_crop)."""
    h_lr = math.floor(h / scale + 1e-9)
    w_lr = math.floor(w / scale + 1e-9)
    return h_lr, w_lr, round(h_lr * scale), round(w_lr * scale)


class RandomDownSampling:
    """mmedit 0.x RandomDownSampling, test form only (rules restated from the public mmedit source, not checked offline):

        scale = uniform(scale_min, scale_max)                  # scale_min == scale_max here
        h_lr, w_lr = floor(H / scale + 1e-9), floor(W / scale + 1e-9)
        gt = gt[:round(h_lr * scale), :round(w_lr * scale), :]
        lq = imresize(gt, (w_lr, h_lr), 'bicubic', backend='pillow')

    The GT arrives as uint8 (LoadImageFromFile does not convert; the pillow backend requires uint8).  `patch_size` (the
    training crop), a scale range, and any other interpolation or backend are refused."""

    def __init__(self, scale_min=1.0, scale_max=4.0, patch_size=None, interpolation='bicubic', backend='pillow'):
        if patch_size is not None:
            raise ValueError(f'RandomDownSampling: patch_size={patch_size!r} is a training crop; only patch_size=None '
                             f'(the whole GT, test form) is supported')
        if scale_min != scale_max:
            raise ValueError(f'RandomDownSampling: scale range [{scale_min}, {scale_max}] is random; only a fixed scale '
                             f'(scale_min == scale_max) is supported')
        if interpolation != 'bicubic' or backend != 'pillow':
            raise ValueError(f'RandomDownSampling: interpolation={interpolation!r}, backend={backend!r}; only '
                             f"interpolation='bicubic' with backend='pillow' is supported")
        if not scale_min > 0:
            raise ValueError(f'RandomDownSampling: scale must be positive, got {scale_min}')
        self.scale = float(scale_min)

    def sizes(self, h, w):
        return down_size(h, w, self.scale)

    def apply(self, gt_u8, want_u8=True, want_chw=False):
        """gt_u8 [H, W, 3] uint8 on the GPU -> (gt crop view [Hc, Wc, 3], lq_u8 [h, w, 3] or None, lq_chw [3, h, w] float32
        = lq_u8 / 255 or None).  The crop is a view: its rows reach the kernel through their pitch."""
        h_lr, w_lr, hc, wc = self.sizes(gt_u8.shape[0], gt_u8.shape[1])
        if h_lr <= 0 or w_lr <= 0:
            raise ValueError(f'a {gt_u8.shape[1]}x{gt_u8.shape[0]} GT is smaller than one LR pixel at scale {self.scale}')
        crop = gt_u8[:hc, :wc, :]
        lq_u8, lq_chw = resample_u8(crop, (w_lr, h_lr), want_u8, want_chw)
        return crop, lq_u8, lq_chw

    def __call__(self, results):
        crop, lq, _ = self.apply(results['gt'])
        results['gt'], results['lq'], results['scale'] = crop, lq, self.scale
        return results
