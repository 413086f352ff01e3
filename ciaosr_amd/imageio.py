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


PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def png_header(path):
    """(width, height, bit depth, colour type, interlace) of a PNG file's IHDR, or None for a file that is not a PNG."""
    import struct
    with open(path, 'rb') as f:
        head = f.read(33)
    if len(head) < 33 or head[:8] != PNG_SIGNATURE or head[12:16] != b'IHDR':
        return None
    w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', head[16:29])
    return w, h, depth, colour, interlace


def _unfilter16(raw, h, line, bpp):
    """The scanlines of `raw` (h rows of 1 + line bytes) with their PNG filters undone, per byte, `bpp` bytes to the left
    predecessor -> uint8 [h, line]."""
    out = np.zeros((h, line), dtype=np.uint8)
    prev = np.zeros(line, dtype=np.uint8)
    for y in range(h):
        ft = raw[y * (line + 1)]
        row = np.frombuffer(raw, dtype=np.uint8, count=line, offset=y * (line + 1) + 1)
        if ft == 0:
            cur = row.copy()
        elif ft == 1:                                         # Sub: a running sum per byte lane, mod 256
            pad = (-line) % bpp
            lanes = np.concatenate([row, np.zeros(pad, dtype=np.uint8)]).reshape(-1, bpp)
            cur = np.cumsum(lanes, axis=0, dtype=np.uint8).reshape(-1)[:line]
        elif ft == 2:
            cur = row + prev                                  # uint8 wraps
        elif ft in (3, 4):                                    # Average, Paeth: every byte needs the one bpp before it
            r, up, c = row.tolist(), prev.tolist(), [0] * line
            for i in range(line):
                a = c[i - bpp] if i >= bpp else 0
                b = up[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    cc = up[i - bpp] if i >= bpp else 0
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                c[i] = (r[i] + pred) & 255
            cur = np.array(c, dtype=np.uint8)
        else:
            raise ValueError(f'row {y} has filter type {ft}: not a PNG filter')
        out[y] = cur
        prev = cur
    return out


def read_png16(path):
    """-> uint16 [h, w] (colour type 0) or [h, w, 3] (colour type 2, R G B) of a non-interlaced PNG file of bit depth 16, every sample
    exact.  Pure numpy and zlib: Pillow opens a 16-bit RGB file as 8-bit RGB and drops the low bytes.  Ancillary chunks are skipped.
    An interlaced file, colour type 4 or 6 (alpha) at depth 16, or any other depth is a ValueError that names what was found.  NOT a
    fast path: the Average and Paeth rows are undone byte by byte in Python -- meant for LR inputs."""
    import struct
    import zlib
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != PNG_SIGNATURE:
        raise ValueError(f'{path}: not a PNG file')
    pos, ihdr, idat = 8, None, []
    while pos + 8 <= len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b'IHDR':
            ihdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat.append(body)
        elif tag == b'IEND':
            break
    if ihdr is None:
        raise ValueError(f'{path}: no IHDR chunk')
    w, h, depth, colour, _, _, interlace = ihdr
    if depth != 16:
        raise ValueError(f'{path}: bit depth {depth}, read_png16 reads bit depth 16')
    if colour not in (0, 2):
        raise ValueError(f'{path}: colour type {colour} at bit depth 16 (alpha) is not read: no 16-bit alpha')
    if interlace != 0:
        raise ValueError(f'{path}: interlace method {interlace} (Adam7) is not read')
    ch = 1 if colour == 0 else 3
    line = 2 * ch * w
    raw = zlib.decompress(b''.join(idat))
    if len(raw) != h * (line + 1):
        raise ValueError(f'{path}: {len(raw)} bytes of scanlines, expected {h * (line + 1)}')
    samples = _unfilter16(raw, h, line, 2 * ch).view('>u2').astype(np.uint16)
    return samples.reshape(h, w) if ch == 1 else samples.reshape(h, w, 3)


def grey16_of_rgb(rgb16):
    """L16 = (19595 R + 38470 G + 7471 B + 32768) >> 16 of a uint16 [h, w, 3] R G B array, in unsigned 32-bit arithmetic (at most
    65535 * 65536 + 32768 < 2^32) -> uint16 [h, w]: the 8-bit grey byte's weights; a neutral (v, v, v) gives v."""
    c = rgb16.astype(np.uint32)
    return ((np.uint32(19595) * c[..., 0] + np.uint32(38470) * c[..., 1] + np.uint32(7471) * c[..., 2] + np.uint32(32768)) >> 16).astype(np.uint16)


def _read16(path):
    """uint16 [h, w] or [h, w, 3] of a file with 16-bit samples -- a depth-16 PNG (`read_png16`) or a file Pillow opens in an I;16
    mode (16-bit grey TIFF) -- or None for every other file."""
    from PIL import Image
    hdr = png_header(path)
    if hdr is not None and hdr[2] == 16:
        return read_png16(path)
    with Image.open(path) as f:
        if f.mode.startswith('I;16'):
            return np.asarray(f).astype(np.uint16)
    return None


def imread16_rgb01(path):
    """-> (float32 tensor [3,H,W] in [0,1], bits).  A file with 16-bit samples (see `_read16`) is read as sample / 65535 in fp32, a grey
    one into three equal channels, bits = 16; every other file exactly as `imread_rgb01` reads it, bit for bit, bits = 8."""
    s = _read16(path)
    if s is None:
        return imread_rgb01(path), 8
    if s.ndim == 2:
        s = np.repeat(s[:, :, None], 3, axis=2)
    img = s.astype(np.float32) / np.float32(65535.0)
    return torch.from_numpy(img).permute(2, 0, 1).contiguous(), 16


def imread16_grey01(path):
    """-> (float32 tensor [1,H,W] in [0,1], was_grey, bits).  A file with 16-bit samples is read as sample / 65535 in fp32 -- a colour
    one through `grey16_of_rgb` first -- with bits = 16; every other file exactly as `imread_grey01` reads it, bit for bit, bits = 8.
    `was_grey`: the file held one channel, or three equal ones."""
    s = _read16(path)
    if s is None:
        t, was_grey = imread_grey01(path)
        return t, was_grey, 8
    was_grey = True
    if s.ndim == 3:
        was_grey = bool((s[:, :, 0] == s[:, :, 1]).all() and (s[:, :, 1] == s[:, :, 2]).all())
        s = grey16_of_rgb(s)
    img = s.astype(np.float32) / np.float32(65535.0)
    return torch.from_numpy(img).unsqueeze(0).contiguous(), was_grey, 16


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
