"""PSNR / SSIM of `BasicRestorer.evaluate` on the MI355X (csrc/metrics_u8.hip), opt-in through `test_cfg.gpu_metrics`.

Same definitions as ciaosr_amd/metrics.py (basic_restorer.py:101-124 -> mmedited/core/evaluation/metrics.py:181-226, :229-318):
both images are quantised to 8 bits first (`tensor2img`), then compared.  `tensor2img_u8` is bitwise `metrics.tensor2img`;
`psnr_ssim_u8` evaluates both metrics in one pass over the two byte images and leaves twelve doubles on the device, which the
host finishes with a mean and a log10 -- that copy is the only synchronisation.  There is no CPU fallback.
"""
import ctypes as C
import math

import torch

from . import _lib, hip_ops
from ._lib import CiaoSRHipError

WANT_BITS = {'PSNR': 1, 'SSIM': 2}        # CIAOSR_METRIC_PSNR / CIAOSR_METRIC_SSIM
SSIM_WINDOW = 11


def tensor2img_u8(t):
    """`metrics.tensor2img` on the device: [1, 3, H, W] or [3, H, W] RGB in [0, 1] -> uint8 [H, W, 3] BGR (x255, round half even)."""
    t = t.detach()
    while t.dim() > 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f'tensor2img_u8 expects [1, 3, H, W] or [3, H, W], got {tuple(t.shape)}')
    t = t.float().contiguous()
    hip_ops.require_gpu(t)
    h, w = t.shape[1], t.shape[2]
    img = torch.empty((h, w, 3), dtype=torch.uint8, device=t.device)
    _lib.call('ciaosr_tensor2img_u8', hip_ops.ptr(t), h, w, hip_ops.ptr(img), C.c_size_t(img.stride(0)), hip_ops.stream_ptr(t.device))
    return img


def tensor2img_bgra_u8(out2):
    """The 8-bit image of an RGBA render: [2, 3, H, W] = (colour, alpha as grey), RGB in [0, 1] -> uint8 [H, W, 4] with bytes B G R A.
    B G R are `tensor2img_u8`'s bytes of item 0; with (B, G, R) = `tensor2img_u8`'s bytes of item 1,
    A = (4899 R + 9617 G + 1868 B + 8192) >> 14.  One pass."""
    if not isinstance(out2, torch.Tensor) or out2.dim() != 4 or out2.shape[0] != 2 or out2.shape[1] != 3:
        shape = tuple(out2.shape) if isinstance(out2, torch.Tensor) else type(out2).__name__
        raise ValueError(f'tensor2img_bgra_u8 expects [2, 3, H, W] (colour, alpha as grey), got {shape}')
    t = out2.detach().float().contiguous()
    hip_ops.require_gpu(t)
    h, w = t.shape[2], t.shape[3]
    img = torch.empty((h, w, 4), dtype=torch.uint8, device=t.device)
    _lib.call('ciaosr_tensor2img_bgra_u8', hip_ops.ptr(t[0]), hip_ops.ptr(t[1]), h, w, hip_ops.ptr(img), C.c_size_t(img.stride(0)),
              hip_ops.stream_ptr(t.device))
    return img


def pack_bgra_u8(bgr_u8, grey_u8):
    """uint8 [H, W, 4] B G R A from two uint8 [H, W, 3] BGR device images: the colour bytes of the first, the alpha
    (4899 R + 9617 G + 1868 B + 8192) >> 14 of the second's.  Rows may be pitched."""
    for img in (bgr_u8, grey_u8):
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            what = f'{img.dtype} {tuple(img.shape)}' if isinstance(img, torch.Tensor) else type(img).__name__
            raise ValueError(f'pack_bgra_u8 expects two uint8 [H, W, 3] images, got {what}')
    if bgr_u8.shape != grey_u8.shape:
        raise ValueError(f'pack_bgra_u8: the images differ in size, {tuple(bgr_u8.shape)} and {tuple(grey_u8.shape)}')
    _check_image(bgr_u8)
    _check_image(grey_u8)
    h, w = bgr_u8.shape[0], bgr_u8.shape[1]
    img = torch.empty((h, w, 4), dtype=torch.uint8, device=bgr_u8.device)
    _lib.call('ciaosr_pack_bgra_u8', hip_ops.ptr(bgr_u8), C.c_size_t(bgr_u8.stride(0)), hip_ops.ptr(grey_u8), C.c_size_t(grey_u8.stride(0)),
              h, w, hip_ops.ptr(img), C.c_size_t(img.stride(0)), hip_ops.stream_ptr(bgr_u8.device))
    return img


def tensor2img_grey_u8(t, out=None):
    """The 8-bit GREY image of a render: [1, 3, H, W] or [3, H, W] RGB in [0, 1] -> uint8 [H, W].  With (B, G, R) = `tensor2img_u8`'s
    bytes of the pixel, L = (19595 R + 38470 G + 7471 B + 32768) >> 16: `Image.convert('L')` of the colour image, and v for a neutral
    (v, v, v).  One pass.  `out`: a uint8 [H, W] device view to write into (rows may be pitched, any alignment)."""
    shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.shape[-3] != 3 or (t.dim() == 4 and t.shape[0] != 1):
        raise ValueError(f'tensor2img_grey_u8 expects [1, 3, H, W] or [3, H, W], got {shape}')
    h, w = t.shape[-2], t.shape[-1]
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or (w > 1 and out.stride(1) != 1) \
                or (h > 1 and out.stride(0) < w):
            raise ValueError(f'tensor2img_grey_u8: out must be a uint8 [{h}, {w}] view with contiguous rows')
    t = t.detach().reshape(3, h, w).float().contiguous()
    hip_ops.require_gpu(t)
    if out is not None and out.device != t.device:
        raise CiaoSRHipError(f'tensor2img_grey_u8: out on {out.device} but the render on {t.device}')
    img = torch.empty((h, w), dtype=torch.uint8, device=t.device) if out is None else out
    _lib.call('ciaosr_tensor2img_grey_u8', hip_ops.ptr(t), h, w, hip_ops.ptr(img), C.c_size_t(img.stride(0) if h > 1 else w),
              hip_ops.stream_ptr(t.device))
    return img


def grey_from_bgr_u8(img_u8, order='bgr'):
    """uint8 [H, W] grey image of a uint8 [H, W, 3] device image (`order` 'bgr' or 'rgb'; rows may be pitched) by the formula of
    `tensor2img_grey_u8`: `Image.convert('L')`."""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        what = f'{img_u8.dtype} {tuple(img_u8.shape)}' if isinstance(img_u8, torch.Tensor) else type(img_u8).__name__
        raise ValueError(f'grey_from_bgr_u8 expects a uint8 [H, W, 3] image, got {what}')
    if order not in ('bgr', 'rgb'):
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    _check_image(img_u8)
    h, w = img_u8.shape[0], img_u8.shape[1]
    img = torch.empty((h, w), dtype=torch.uint8, device=img_u8.device)
    _lib.call('ciaosr_grey_from_bgr_u8', hip_ops.ptr(img_u8), C.c_size_t(img_u8.stride(0)), 1 if order == 'bgr' else 0, h, w,
              hip_ops.ptr(img), C.c_size_t(w), hip_ops.stream_ptr(img_u8.device))
    return img


def tensor2img_u16(t):
    """`tensor2img_u8` with 16-bit samples: [1, 3, H, W] or [3, H, W] RGB in [0, 1] -> torch.uint16 [H, W, 3] BGR, each sample
    rint(fp32(clamp(v, 0, 1) * 65535)) (one fp32 multiply, round half to even): bitwise `(t.clamp(0, 1) * 65535).round()`.  A level
    k / 255 becomes 257 k; otherwise this is NOT the 8-bit image shifted left, and a sample's high byte is NOT `tensor2img_u8`'s."""
    t = t.detach()
    while t.dim() > 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f'tensor2img_u16 expects [1, 3, H, W] or [3, H, W], got {tuple(t.shape)}')
    t = t.float().contiguous()
    hip_ops.require_gpu(t)
    h, w = t.shape[1], t.shape[2]
    img = torch.empty((h, w, 3), dtype=torch.uint16, device=t.device)
    _lib.call('ciaosr_tensor2img_u16', hip_ops.ptr(t), h, w, hip_ops.ptr(img), C.c_size_t(6 * w), hip_ops.stream_ptr(t.device))
    return img


def tensor2img_grey_u16(t, out=None):
    """The 16-bit GREY image of a render: [1, 3, H, W] or [3, H, W] RGB in [0, 1] -> torch.uint16 [H, W].  With (B, G, R) =
    `tensor2img_u16`'s samples of the pixel, L16 = (19595 R + 38470 G + 7471 B + 32768) >> 16 in unsigned 32-bit arithmetic: the
    weights of `tensor2img_grey_u8`, and v for a neutral (v, v, v).  One pass.  `out`: a uint16 [H, W] device view to write into
    (rows may be pitched; a crop may start at any pixel)."""
    shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.shape[-3] != 3 or (t.dim() == 4 and t.shape[0] != 1):
        raise ValueError(f'tensor2img_grey_u16 expects [1, 3, H, W] or [3, H, W], got {shape}')
    h, w = t.shape[-2], t.shape[-1]
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint16 or tuple(out.shape) != (h, w) or (w > 1 and out.stride(1) != 1) \
                or (h > 1 and out.stride(0) < w):
            raise ValueError(f'tensor2img_grey_u16: out must be a uint16 [{h}, {w}] view with contiguous rows')
    t = t.detach().reshape(3, h, w).float().contiguous()
    hip_ops.require_gpu(t)
    if out is not None and out.device != t.device:
        raise CiaoSRHipError(f'tensor2img_grey_u16: out on {out.device} but the render on {t.device}')
    img = torch.empty((h, w), dtype=torch.uint16, device=t.device) if out is None else out
    _lib.call('ciaosr_tensor2img_grey_u16', hip_ops.ptr(t), h, w, hip_ops.ptr(img), C.c_size_t(2 * (img.stride(0) if h > 1 else w)),
              hip_ops.stream_ptr(t.device))
    return img


def grey_from_bgr_u16(img_u16, order='bgr'):
    """uint16 [H, W] grey image of a uint16 [H, W, 3] device image (`order` 'bgr' or 'rgb'; rows may be pitched) by the formula of
    `tensor2img_grey_u16`."""
    if not isinstance(img_u16, torch.Tensor) or img_u16.dtype != torch.uint16 or img_u16.dim() != 3 or img_u16.shape[2] != 3:
        what = f'{img_u16.dtype} {tuple(img_u16.shape)}' if isinstance(img_u16, torch.Tensor) else type(img_u16).__name__
        raise ValueError(f'grey_from_bgr_u16 expects a uint16 [H, W, 3] image, got {what}')
    if order not in ('bgr', 'rgb'):
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    _check_image_u16(img_u16)
    h, w = img_u16.shape[0], img_u16.shape[1]
    img = torch.empty((h, w), dtype=torch.uint16, device=img_u16.device)
    _lib.call('ciaosr_grey_from_bgr_u16', hip_ops.ptr(img_u16), C.c_size_t(2 * img_u16.stride(0)), 1 if order == 'bgr' else 0, h, w,
              hip_ops.ptr(img), C.c_size_t(2 * w), hip_ops.stream_ptr(img_u16.device))
    return img


def _check_image_u16(img):
    """`_check_image` for a uint16 [H, W, 3] tensor (dtype and shape are the caller's to check): strides count samples."""
    if not img.is_cuda:
        hip_ops.require_gpu(img)              # raises: no CPU fallback
    if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * img.shape[1]:
        raise CiaoSRHipError('expected HWC rows of 3*W contiguous samples (a crop of a larger image is fine)')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')


def _check_image(img):
    if not isinstance(img, torch.Tensor):
        raise CiaoSRHipError(f'expected a uint8 HxWx3 cuda tensor, got {type(img).__name__}')
    if not img.is_cuda:
        hip_ops.require_gpu(img)              # raises: no CPU fallback
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise CiaoSRHipError(f'expected a uint8 HxWx3 image, got {img.dtype} {tuple(img.shape)}')
    if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * img.shape[1]:
        raise CiaoSRHipError('expected HWC rows of 3*W contiguous bytes (a crop of a larger image is fine)')
    if img.device.index != torch.cuda.current_device():
        raise CiaoSRHipError(f'image on cuda:{img.device.index} but the current device is cuda:{torch.cuda.current_device()}')


def finish(sums, want):
    """{name: float} from the kernel's [3][sse, pixels, ssim sum, map pixels] (a host list of 12 floats), as metrics.psnr / .ssim."""
    res = {}
    for name in want:
        if name == 'PSNR':
            n = sum(sums[4 * c + 1] for c in range(3))
            mse = sum(sums[4 * c] for c in range(3)) / n
            res[name] = float('inf') if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))
        else:
            vals = [sums[4 * c + 2] / sums[4 * c + 3] for c in range(3) if sums[4 * c + 3] > 0]
            res[name] = float(sum(vals) / len(vals))
    return res


def launch_psnr_ssim_u8(a, b, crop_border=0, convert_to=None, want=('PSNR', 'SSIM')):
    """Checks + the two launches of `psnr_ssim_u8` without the result copy: returns the 12 doubles on the device
    ([3][sse, pixels, ssim sum, map pixels]) and does not synchronise."""
    _check_image(a)
    _check_image(b)
    assert a.shape == b.shape, f'Image shapes are different: {a.shape}, {b.shape}.'
    if isinstance(convert_to, str) and convert_to.lower() == 'y':
        to_y = 1
    elif convert_to is not None:
        raise ValueError('Wrong color model. Supported values are "Y" and None.')
    else:
        to_y = 0
    h, w = a.shape[0], a.shape[1]
    crop = int(crop_border)
    if crop < 0 or 2 * crop >= h or 2 * crop >= w:
        raise ValueError(f'crop_border={crop_border} leaves nothing of a {h}x{w} image')
    if 'SSIM' in want and (h - 2 * crop < SSIM_WINDOW or w - 2 * crop < SSIM_WINDOW):
        raise ValueError(f'SSIM needs at least {SSIM_WINDOW}x{SSIM_WINDOW} pixels after the crop, got {h - 2 * crop}x{w - 2 * crop}')
    bits = 0
    for name in want:
        bits |= WANT_BITS[name]
    dev = a.device
    lib = _lib.load()
    nbytes = lib.ciaosr_psnr_ssim_u8_workspace_bytes(h, w, crop, to_y)
    if nbytes == 0:
        raise CiaoSRHipError(f'psnr_ssim_u8: a {h}x{w} image with crop_border={crop} is beyond the kernel\'s index range')
    ws = hip_ops.workspace(nbytes, dev, slot='metrics')
    out = torch.empty(12, dtype=torch.float64, device=dev)
    _lib.call('ciaosr_psnr_ssim_u8', hip_ops.ptr(a), C.c_size_t(a.stride(0)), hip_ops.ptr(b), C.c_size_t(b.stride(0)), h, w, crop,
              to_y, bits, hip_ops.ptr(out), hip_ops.ptr(ws), C.c_size_t(nbytes), hip_ops.stream_ptr(dev))
    return out


def psnr_ssim_u8(a, b, crop_border=0, convert_to=None, want=('PSNR', 'SSIM')):
    """`metrics.psnr` / `metrics.ssim` of two uint8 [H, W, 3] BGR images on the device -> {name: python float} in the order of
    `want`.  PSNR is inf for identical images.  Rows may be pitched (a crop view of a larger image).  The copy of the twelve
    doubles to the host is the only synchronisation."""
    want = (want,) if isinstance(want, str) else tuple(want)
    for name in want:
        if name not in WANT_BITS:
            raise KeyError(name)
    if not want:
        return {}
    return finish(launch_psnr_ssim_u8(a, b, crop_border, convert_to, want).cpu().tolist(), want)
