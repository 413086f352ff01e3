"""The baseline JPEG contract of DESIGN 4.1i-d in numpy and plain Python: libjpeg's integer pipeline as Pillow drives it (JFIF header,
Annex K tables scaled by the quality, the 16-bit fixed-point RGB -> YCbCr, h2v2 box downsampling with the alternating bias, the
"islow" forward DCT, division rounding half away from zero, the Annex K Huffman codes, one interleaved scan).  It knows nothing of
the HIP code; tests/test_jpeg_host.py holds it to Pillow's files byte for byte, tests/test_jpeg_gpu.py holds the device to it."""
import struct

import numpy as np

SUBSAMPLINGS = ('444', '420')

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
                       + [99] * 36, dtype=np.int64)


def _zigzag():
    order = []
    for s in range(15):
        diag = [(i, s - i) for i in range(8) if 0 <= s - i < 8]
        order += diag if s % 2 else diag[::-1]
    return np.array([r * 8 + c for r, c in order])


ZIGZAG = _zigzag()                       # ZIGZAG[k] = natural index (row * 8 + column) of the k-th coefficient in zigzag order

# Annex K "typical" Huffman tables: (bits[1..16], vals)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
            0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
            0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
              0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa])


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of the canonical code that a DHT segment's (bits, vals) describe."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _check(quality, subsampling):
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f'quality={quality!r}')
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f'subsampling={subsampling!r}')


def quant_tables(quality):
    """(luma, chroma) int64 [64] in natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def header(h, w, quality, subsampling):
    """The file from SOI up to and including the SOS header."""
    _check(quality, subsampling)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f'{h} x {w}')
    out = [b'\xff\xd8', b'\xff\xe0', struct.pack('>H5sBBBHHBB', 16, b'JFIF\0', 1, 1, 0, 1, 1, 0, 0)]
    for k, q in enumerate(quant_tables(quality)):
        out += [b'\xff\xdb', struct.pack('>HB', 67, k), bytes(int(v) for v in q[ZIGZAG])]
    out += [b'\xff\xc0', struct.pack('>HBHHB', 17, 8, h, w, 3), bytes([1, 0x22 if subsampling == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])]
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += [b'\xff\xc4', struct.pack('>HB', 19 + len(vals), tc_th), bytes(bits), bytes(vals)]
    out += [b'\xff\xda', struct.pack('>HB', 12, 3), bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3f, 0])]
    return b''.join(out)


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    """Repeat the last row / column up to rows x cols."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode='edge')


def _up(n, m):
    return -(-n // m) * m


def planes(rgb, subsampling):
    """(Y, Cb, Cr) planes padded to whole blocks (4:2:0: luma to whole blocks, NOT whole MCUs: the rest is dummy blocks)."""
    h, w = rgb.shape[:2]
    y, cb, cr = ycc(rgb)
    y = _extend(y, _up(h, 8), _up(w, 8))
    if subsampling == '444':
        return y, _extend(cb, _up(h, 8), _up(w, 8)), _extend(cr, _up(h, 8), _up(w, 8))
    out = [y]
    for c in (cb, cr):
        c = _extend(c, _up(h, 2), _up(w, 16))
        bias = np.where(np.arange(c.shape[1] // 2) % 2 == 0, 1, 2)[None, :]
        c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_extend(c, _up(c.shape[0], 8), c.shape[1]))
    return tuple(out)


F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """jfdctint on the last axis of int64 [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F['f0_541']
    out[2] = _descale(z1 + t13 * F['f0_765'], n)
    out[6] = _descale(z1 - t12 * F['f1_847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f1_175']
    t4, t5, t6, t7 = t4 * F['f0_298'], t5 * F['f2_053'], t6 * F['f3_072'], t7 * F['f1_501']
    z1, z2, z3, z4 = -z1 * F['f0_899'], -z2 * F['f2_562'], -z3 * F['f1_961'] + z5, -z4 * F['f0_390'] + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def blocks_of(plane, qtable):
    """Quantised coefficients int64 [rows of blocks, columns of blocks, 64] in ZIGZAG order."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128                     # [hb, wb, row, column]
    d = _dct_pass(d, True)
    d = _dct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    c = d.reshape(hb, wb, 64)
    div = 8 * qtable
    q = np.sign(c) * ((np.abs(c) + (div >> 1)) // div)
    return q[:, :, ZIGZAG]


def scan_blocks(rgb, quality, subsampling):
    """The blocks of the interleaved scan in coding order: [(component 0 / 1 / 2, int coefficients [64] in zigzag order)], dummy blocks
    included."""
    _check(quality, subsampling)
    ql, qc = quant_tables(quality)
    y, cb, cr = planes(rgb, subsampling)
    by, bcb, bcr = blocks_of(y, ql), blocks_of(cb, qc), blocks_of(cr, qc)
    out = []
    if subsampling == '444':
        for i in range(by.shape[0]):
            for j in range(by.shape[1]):
                out += [(0, by[i, j]), (1, bcb[i, j]), (2, bcr[i, j])]
        return out
    for i in range(bcb.shape[0]):
        for j in range(bcb.shape[1]):
            for v in (0, 1):
                for u in (0, 1):
                    r, c = 2 * i + v, 2 * j + u
                    if r < by.shape[0] and c < by.shape[1]:
                        out.append((0, by[r, c]))
                    else:                                   # dummy: the DC of the block coded just before it, no AC
                        blk = np.zeros(64, dtype=np.int64)
                        blk[0] = out[-1][1][0]
                        out.append((0, blk))
            out += [(1, bcb[i, j]), (2, bcr[i, j])]
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = [(huffman_codes(*DC_LUMA), huffman_codes(*AC_LUMA)), (huffman_codes(*DC_CHROMA), huffman_codes(*AC_CHROMA))]
    return _TABLES


def _put_value(bw, table, run, v):
    n = abs(v).bit_length()
    bw.put(*table[(run << 4) | n])
    if n:
        bw.put(v if v > 0 else v + (1 << n) - 1, n)


def unstuffed(blocks):
    """The scan's bytes before 0xFF stuffing, padded with 1-bits."""
    bw = BitWriter()
    pred = [0, 0, 0]
    for comp, blk in blocks:
        dc, ac = _tables()[0 if comp == 0 else 1]
        v = int(blk[0])
        _put_value(bw, dc, 0, v - pred[comp])
        pred[comp] = v
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                bw.put(*ac[0xf0])
                run -= 16
            _put_value(bw, ac, run, v)
            run = 0
        if run:
            bw.put(*ac[0x00])
    return bw.finish()


def stuff(data):
    return data.replace(b'\xff', b'\xff\x00')


def scan(rgb, quality, subsampling):
    """The entropy-coded scan of the uint8 [h, w, 3] RGB image, stuffed and padded: the file between the SOS header and EOI."""
    return stuff(unstuffed(scan_blocks(rgb, quality, subsampling)))


def encode(rgb, quality, subsampling):
    """The whole file."""
    h, w = rgb.shape[:2]
    return header(h, w, quality, subsampling) + scan(rgb, quality, subsampling) + b'\xff\xd9'
