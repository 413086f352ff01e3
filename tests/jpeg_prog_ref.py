"""The progressive contract of DESIGN 4.1i-e in plain Python, on top of tests/jpeg_ref.py (coefficients, bit writer, stuffing) and
tests/jpeg_opt_ref.py (libjpeg's table from a histogram): libjpeg's progressive entropy coder under the ten-scan script that Pillow's
`progressive=True` selects, every scan coded with a table made from its own symbols.  It knows nothing of the HIP code;
tests/test_jpeg_prog_host.py holds it to Pillow's files byte for byte, tests/test_jpeg_prog_gpu.py holds the device to it.
`code` returns the ten scans, the ten tables (two for the first scan, none for the seventh) and counters of the EOB runs."""
import struct

from tests import jpeg_opt_ref as opt
from tests import jpeg_ref as ref

# (component: None = Y, Cb, Cr interleaved, else 0 Y / 1 Cb / 2 Cr; Ss, Se, Ah, Al) -- note Cr before Cb
SCRIPT = ((None, 0, 0, 0, 1), (0, 1, 5, 0, 2), (2, 1, 63, 0, 1), (1, 1, 63, 0, 1), (0, 6, 63, 0, 2), (0, 1, 63, 2, 1),
          (None, 0, 0, 1, 0), (2, 1, 63, 1, 0), (1, 1, 63, 1, 0), (0, 1, 63, 1, 0))
# class << 4 | id of the ten DHT segments in the file's order: two before scan 1, one before every AC scan
TABLE_IDS = (0x00, 0x01, 0x10, 0x11, 0x11, 0x10, 0x10, 0x11, 0x11, 0x10)
MAX_RUN = 0x7fff
MAX_CORR = 937                              # libjpeg's MAX_CORR_BITS - DCTSIZE2 + 1
# EOB runs emitted; the longest; runs cut at MAX_RUN blocks in a refinement scan and in a first scan; runs cut by the correction bits
COUNTERS = ('runs', 'longest_run', 'full_flushes', 'first_full_flushes', 'corr_flushes')


def component_grids(rgb, quality, subsampling):
    """[Y, Cb, Cr] -> coefficients [rows of blocks, columns of blocks, 64]: the real blocks only, in raster order."""
    ql, qc = ref.quant_tables(quality)
    y, cb, cr = ref.planes(rgb, subsampling)
    return [ref.blocks_of(y, ql), ref.blocks_of(cb, qc), ref.blocks_of(cr, qc)]


def dc_first(blocks, al):
    """[(table 0 / 1, symbol, extra bits, their number)] of the interleaved blocks."""
    out, pred = [], [0, 0, 0]
    for comp, blk in blocks:
        v = int(blk[0]) >> al
        d = v - pred[comp]
        pred[comp] = v
        n = abs(d).bit_length()
        out.append((0 if comp == 0 else 1, n, (d if d > 0 else d + (1 << n) - 1) if n else 0, n))
    return out


class _Run:
    """The EOB run of a scan: blocks that end without a symbol, and the correction bits they buffered."""

    def __init__(self, out, stats, full='full_flushes'):
        self.out, self.stats, self.full, self.blocks, self.bits = out, stats, full, 0, []

    def flush(self):
        if self.blocks:
            n = self.blocks.bit_length() - 1
            self.out.append((0, n << 4, self.blocks & ((1 << n) - 1), n))
            self.out += [(None, None, bit, 1) for bit in self.bits]
            self.stats['runs'] += 1
            self.stats['longest_run'] = max(self.stats['longest_run'], self.blocks)
            self.blocks, self.bits = 0, []

    def end_block(self, bits):
        self.blocks += 1
        self.bits += bits
        if self.blocks == MAX_RUN:
            self.stats[self.full] += 1
            self.flush()
        elif len(self.bits) > MAX_CORR:
            self.stats['corr_flushes'] += 1
            self.flush()


def ac_first(blocks, ss, se, al, stats):
    out = []
    run = _Run(out, stats, 'first_full_flushes')
    for blk in blocks:
        r = 0
        for k in range(ss, se + 1):
            v = int(blk[k])
            a = abs(v) >> al
            if a == 0:
                r += 1
                continue
            run.flush()
            while r > 15:
                out.append((0, 0xf0, 0, 0))
                r -= 16
            n = a.bit_length()
            out.append((0, (r << 4) | n, a if v > 0 else ~a & ((1 << n) - 1), n))
            r = 0
        if r > 0:
            run.end_block([])
    run.flush()
    return out


def ac_refine(blocks, ss, se, al, stats):
    out = []
    run = _Run(out, stats)
    for blk in blocks:
        a = [abs(int(v)) >> al for v in blk]
        eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=0)
        r, br = 0, []
        for k in range(ss, se + 1):
            if a[k] == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                run.flush()
                out.append((0, 0xf0, 0, 0))
                r -= 16
                out += [(None, None, bit, 1) for bit in br]
                br = []
            if a[k] > 1:
                br.append(a[k] & 1)
                continue
            run.flush()
            out.append((0, (r << 4) | 1, 0 if blk[k] < 0 else 1, 1))
            out += [(None, None, bit, 1) for bit in br]
            r, br = 0, []
        if r > 0 or br:
            run.end_block(br)
    run.flush()
    return out


def entropy_code(syms, n_tables):
    """-> ([(counts, symbols)] per table, the scan stuffed and padded); a symbol of table None is raw bits."""
    hist = [[0] * 256 for _ in range(n_tables)]
    for table, symbol, _, _ in syms:
        if table is not None:
            hist[table][symbol] += 1
    tables = [tuple(opt.table_from_histogram(h)[:2]) for h in hist]
    codes = [ref.huffman_codes(c, v) for c, v in tables]
    bw = ref.BitWriter()
    for table, symbol, extra, n in syms:
        if table is not None:
            bw.put(*codes[table][symbol])
        if n:
            bw.put(extra, n)
    return tables, ref.stuff(bw.finish())


def code(rgb, quality, subsampling):
    """-> (scans [10] bytes, tables [10] of (counts, symbols) in the file's order, counters dict)."""
    stats = dict.fromkeys(COUNTERS, 0)
    grids = component_grids(rgb, quality, subsampling)
    inter = ref.scan_blocks(rgb, quality, subsampling)
    scans, tables = [], []
    for comp, ss, se, ah, al in SCRIPT:
        if comp is None and ah == 0:
            made, data = entropy_code(dc_first(inter, al), 2)
        elif comp is None:
            made, data = entropy_code([(None, None, (int(blk[0]) >> al) & 1, 1) for _, blk in inter], 0)
        else:
            g = grids[comp]
            blocks = [g[i, j] for i in range(g.shape[0]) for j in range(g.shape[1])]
            made, data = entropy_code((ac_refine if ah else ac_first)(blocks, ss, se, al, stats), 1)
        scans.append(data)
        tables += made
    return scans, tables, stats


def frame_header(h, w, quality, subsampling):
    """SOI, APP0, two DQT, SOF2."""
    out = [b'\xff\xd8', b'\xff\xe0', struct.pack('>H5sBBBHHBB', 16, b'JFIF\0', 1, 1, 0, 1, 1, 0, 0)]
    for k, q in enumerate(ref.quant_tables(quality)):
        out += [b'\xff\xdb', struct.pack('>HB', 67, k), bytes(int(v) for v in q[ref.ZIGZAG])]
    out += [b'\xff\xc2', struct.pack('>HBHHB', 17, 8, h, w, 3), bytes([1, 0x22 if subsampling == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])]
    return b''.join(out)


def dht(tc_th, table):
    counts, vals = table
    assert len(counts) == 16 and len(vals) == sum(counts)
    return b'\xff\xc4' + struct.pack('>HB', 19 + len(vals), tc_th) + bytes(counts) + bytes(vals)


def scan_header(s, tables):
    """The DHT segments and the SOS header in front of scan s = 0..9; `tables`: the file's ten."""
    comp, ss, se, ah, al = SCRIPT[s]
    if comp is None:
        first = [dht(0x00, tables[0]), dht(0x01, tables[1])] if ah == 0 else []
        sel = 0x10 if ah == 0 else 0x00
        return b''.join(first) + b'\xff\xda' + struct.pack('>HB', 12, 3) + bytes((1, 0x00, 2, sel, 3, sel, ss, se, (ah << 4) | al))
    slot = s + 1 if s < 6 else s                             # scan 7 has no table
    tid = 0 if comp == 0 else 1
    return dht(0x10 | tid, tables[slot]) + b'\xff\xda' + struct.pack('>HB', 8, 1) + bytes((comp + 1, tid, ss, se, (ah << 4) | al))


def assemble(h, w, quality, subsampling, scans, tables):
    out = [frame_header(h, w, quality, subsampling)]
    for s in range(10):
        out += [scan_header(s, tables), scans[s]]
    return b''.join(out) + b'\xff\xd9'


def encode(rgb, quality, subsampling, stats=None):
    """The whole progressive file; `stats` (a dict) receives the counters."""
    scans, tables, counted = code(rgb, quality, subsampling)
    if stats is not None:
        stats.update(counted)
    return assemble(rgb.shape[0], rgb.shape[1], quality, subsampling, scans, tables)
