"""Image file I/O for the test pipeline (LoadImageFromFile / mmcv.imwrite counterparts; mmcv is external).
Files are read as RGB (`channel_order='rgb'`, configs/001_*_rdn_*.py:100-112); `tensor2img` output is BGR."""
import os

import numpy as np
import torch


def imread_rgb01(path):
    """-> float32 tensor [3,H,W] in [0,1] (LoadImageFromFile + RescaleToZeroOne + ImageToTensor)."""
    from PIL import Image
    img = np.asarray(Image.open(path).convert('RGB'), dtype=np.float32) / 255.0
    return torch.from_numpy(img).permute(2, 0, 1).contiguous()


def imread_rgba01(path):
    """-> (float32 tensor [4,H,W] in [0,1], R G B A, not premultiplied; opaque): the file through Pillow's convert('RGBA') -- RGBA, LA,
    palette files with a tRNS chunk; a file without transparency gets alpha 1.  `opaque`: every alpha byte is 255."""
    from PIL import Image
    img = np.asarray(Image.open(path).convert('RGBA'), dtype=np.uint8)
    opaque = bool((img[:, :, 3] == 255).all())
    return torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).contiguous(), opaque


def imread_grey01(path):
    """-> (float32 tensor [1,H,W] in [0,1], was_grey): the file through Pillow's convert('L') -- L, LA, palette and colour files alike.
    `was_grey`: the file's convert('RGB') has three equal channels, so nothing but the grey values was there to lose."""
    from PIL import Image
    with Image.open(path) as f:
        rgb = np.asarray(f.convert('RGB'), dtype=np.uint8)
        grey = np.asarray(f.convert('L'), dtype=np.uint8)
    was_grey = bool((rgb[:, :, 0] == rgb[:, :, 1]).all() and (rgb[:, :, 1] == rgb[:, :, 2]).all())
    return torch.from_numpy(grey.astype(np.float32) / 255.0).unsqueeze(0).contiguous(), was_grey


def imread_u8(path):
    """-> HxWx3 uint8 RGB array: LoadImageFromFile(flag='color', channel_order='rgb') before any conversion."""
    from PIL import Image
    return np.array(Image.open(path).convert('RGB'), dtype=np.uint8)


def imwrite(img_bgr_u8, path):
    """mmcv.imwrite of a tensor2img result (HxWx3 BGR uint8)."""
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    arr = np.asarray(img_bgr_u8)
    if arr.ndim == 3:
        arr = arr[:, :, ::-1]
    Image.fromarray(np.ascontiguousarray(arr.astype(np.uint8))).save(path)
