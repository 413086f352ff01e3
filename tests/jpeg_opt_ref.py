"""The optimised-Huffman contract of DESIGN 4.1i-d in plain Python, on top of tests/jpeg_ref.py: the histograms of the symbols that a
file's scan emits, libjpeg's rule that makes a table from a histogram (its tie-breaks, its limiting to 16 bits, the reserved all-ones
code), the coding with those tables and the header with the four DHT segments.  It knows nothing of the HIP code;
tests/test_jpeg_opt_host.py holds it to Pillow's `optimize=True` files byte for byte, tests/test_jpeg_opt_gpu.py holds the device to
it.  It also reports how deep each table's tree is BEFORE limiting."""
import heapq
import struct

from tests import jpeg_ref as ref

TABLE_IDS = (0x00, 0x10, 0x01, 0x11)        # the file's order of DHT segments: DC luma, AC luma, DC chroma, AC chroma
FREQUENCY_LIMIT = 1_000_000_000


def symbols(blocks):
    """The symbols of the scan in coding order: [(table 0..3 in the file's order, symbol, extra bits, their number)]."""
    out, pred = [], [0, 0, 0]
    for comp, blk in blocks:
        dc_table = 0 if comp == 0 else 2
        v = int(blk[0])
        d = v - pred[comp]
        pred[comp] = v
        n = abs(d).bit_length()
        out.append((dc_table, n, (d if d > 0 else d + (1 << n) - 1) if n else 0, n))
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append((dc_table + 1, 0xf0, 0, 0))
                run -= 16
            n = abs(v).bit_length()
            out.append((dc_table + 1, (run << 4) | n, v if v > 0 else v + (1 << n) - 1, n))
            run = 0
        if run:
            out.append((dc_table + 1, 0x00, 0, 0))
    return out


def histograms(syms):
    hist = [[0] * 256 for _ in range(4)]
    for table, symbol, _, _ in syms:
        hist[table][symbol] += 1
    return hist


def code_sizes(freq256):
    """codesize[0..256] of libjpeg's merging: the two smallest non-zero frequencies, ties to the LARGER index, merge until one is left."""
    freq = list(freq256) + [1]                               # the pseudo-symbol 256 reserves the all-ones code
    if sum(freq) > FREQUENCY_LIMIT:
        raise ValueError('more symbols than the contract allows')
    size = [0] * 257
    members = {i: [i] for i, f in enumerate(freq) if f}      # the symbols of the group that index i addresses
    live = [(f, -i) for i, f in enumerate(freq) if f]        # smallest frequency first, the larger index on ties
    heapq.heapify(live)
    while len(live) > 1:
        f1, i1 = heapq.heappop(live)
        f2, i2 = heapq.heappop(live)
        c1, c2 = -i1, -i2
        members[c1] += members.pop(c2)
        for s in members[c1]:
            size[s] += 1
        heapq.heappush(live, (f1 + f2, -c1))
    return size


def table_from_histogram(freq256):
    """-> (counts [16], symbols in code order, the tree's depth before limiting)."""
    size = code_sizes(freq256)
    depth = max(size)
    bits = [0] * (max(depth, 32) + 2)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                             # the reserved code leaves
    order = sorted((size[s], s) for s in range(256) if size[s])
    return bits[1:17], [s for _, s in order], depth


def tables_of(blocks):
    """-> ([(counts, symbols)] x 4 in the file's order, [depth before limiting] x 4)."""
    made = [table_from_histogram(h) for h in histograms(symbols(blocks))]
    return [(c, v) for c, v, _ in made], [d for _, _, d in made]


def header(h, w, quality, subsampling, tables):
    """The file from SOI up to and including the SOS header, the four DHT segments holding `tables`."""
    out = [b'\xff\xd8', b'\xff\xe0', struct.pack('>H5sBBBHHBB', 16, b'JFIF\0', 1, 1, 0, 1, 1, 0, 0)]
    for k, q in enumerate(ref.quant_tables(quality)):
        out += [b'\xff\xdb', struct.pack('>HB', 67, k), bytes(int(v) for v in q[ref.ZIGZAG])]
    out += [b'\xff\xc0', struct.pack('>HBHHB', 17, 8, h, w, 3), bytes([1, 0x22 if subsampling == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])]
    for tc_th, (counts, vals) in zip(TABLE_IDS, tables):
        assert len(counts) == 16 and len(vals) == sum(counts)
        out += [b'\xff\xc4', struct.pack('>HB', 19 + len(vals), tc_th), bytes(counts), bytes(vals)]
    out += [b'\xff\xda', struct.pack('>HB', 12, 3), bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3f, 0])]
    return b''.join(out)


def unstuffed(blocks, tables):
    codes = [ref.huffman_codes(c, v) for c, v in tables]
    bw = ref.BitWriter()
    for table, symbol, extra, n in symbols(blocks):
        bw.put(*codes[table][symbol])
        if n:
            bw.put(extra, n)
    return bw.finish()


def scan(rgb, quality, subsampling):
    """-> (the entropy-coded scan, stuffed and padded; the four tables; their depths before limiting)."""
    blocks = ref.scan_blocks(rgb, quality, subsampling)
    tables, depths = tables_of(blocks)
    return ref.stuff(unstuffed(blocks, tables)), tables, depths


def encode(rgb, quality, subsampling):
    """The whole optimised file."""
    h, w = rgb.shape[:2]
    data, tables, _ = scan(rgb, quality, subsampling)
    return header(h, w, quality, subsampling, tables) + data + b'\xff\xd9'
