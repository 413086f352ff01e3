"""A plain Python / numpy restatement of the match coder's contract (csrc/png_u8.hip, the *_lz_* entry points), written for the tests
(not product code):

* `parse`        band bytes, scanline length `line`, bytes per pixel `bpp` -> the token list the device must emit: an int is a literal,
                 a tuple is (length, distance);
* `expand`       the bytes such a token list stands for;
* `model_bits`   the size of one dynamic block for a token list with optimal, unlimited-depth Huffman codes for both alphabets, the
                 extra bits of RFC 1951 section 3.2.5 and a plain header (code lengths sent one by one);
* `inflate_tokens`  an inflate that records, per block, its type and its tokens instead of only the bytes.

The judges of a stream's validity stay `zlib.decompress` and Pillow's decoder.
"""
import numpy as np

from tests.png_reference import band_model_bits, huffman_lengths

CHUNK = 4096
MIN_MATCH, MAX_MATCH = 8, 258
NEAR = (1, 2, 3, 4, 6, 8, 12, 16)

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def distances(line, bpp):
    """The candidate distances in the contract's order; `line = 0` drops the three scanline candidates."""
    return NEAR + ((line - bpp, line, line + bpp) if line else ())


def _run_lengths(eq):
    """run[i] = the number of consecutive True from i on."""
    n = len(eq)
    idx = np.arange(n)
    stop = np.where(~eq, idx, n)                     # the next False at or after i
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    return nxt - idx


def best_matches(band, line, bpp):
    """(length int [n], distance int [n]): per position the longest candidate, ties to the earliest in D; lengths are capped at 258
    and at the end of the position's parse chunk; a candidate above 32768 or above the position's offset is skipped."""
    a = np.frombuffer(bytes(band), dtype=np.uint8)
    n = len(a)
    pos = np.arange(n)
    room = np.minimum(MAX_MATCH, np.minimum(n, (pos // CHUNK + 1) * CHUNK) - pos)
    best_len = np.zeros(n, dtype=np.int64)
    best_d = np.zeros(n, dtype=np.int64)
    for d in distances(line, bpp):
        if d > 32768 or d >= n or d < 1:
            continue
        eq = np.zeros(n, dtype=bool)
        eq[d:] = a[d:] == a[:-d]
        length = np.minimum(_run_lengths(eq), room)
        better = length > best_len                   # strict: ties stay with the earlier candidate
        best_len[better] = length[better]
        best_d[better] = d
    return best_len, best_d


def parse(band, line, bpp):
    """The contract's greedy parse: from every chunk's start, a match of 8 or more is taken, else a literal."""
    a = bytes(band)
    length, dist = best_matches(a, line, bpp)
    out, i, n = [], 0, len(a)
    while i < n:
        if length[i] >= MIN_MATCH:
            out.append((int(length[i]), int(dist[i])))
            i += int(length[i])
        else:
            out.append(a[i])
            i += 1
    return out


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            length, d = t
            assert 1 <= d <= len(out), (t, len(out))
            for _ in range(length):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)


def length_symbol(length):
    s = max(k for k in range(29) if LENGTH_BASE[k] <= length)
    return 257 + s, LENGTH_EXTRA[s]


def distance_symbol(d):
    s = max(k for k in range(30) if DIST_BASE[k] <= d)
    return s, DIST_EXTRA[s]


def model_bits(tokens):
    """Bits of one dynamic block for the token list: optimal unlimited-depth codes for the literal / length and the distance alphabet,
    extra bits, and a plain header: 3 + 14 bits, 19 x 3 bits, and every code length up to the last used symbol of both alphabets sent
    as itself under the lengths' own optimal code."""
    ll, dd, extra = [0] * 286, [0] * 30, 0
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            s, e = length_symbol(t[0])
            ll[s] += 1
            extra += e
            s, e = distance_symbol(t[1])
            dd[s] += 1
            extra += e
        else:
            ll[t] += 1
    dl, ddp = huffman_lengths(ll), huffman_lengths(dd) if any(dd) else {}
    payload = sum(ll[s] * v for s, v in dl.items()) + sum(dd[s] * v for s, v in ddp.items()) + extra
    hlit = max(257, max(dl) + 1)
    hdist = max(1, max(ddp) + 1 if ddp else 1)
    lens = [dl.get(s, 0) for s in range(hlit)] + [ddp.get(s, 0) for s in range(hdist)]
    cl = {}
    for v in lens:
        cl[v] = cl.get(v, 0) + 1
    keys = sorted(cl)
    cl_depth = huffman_lengths([cl[k] for k in keys])
    return 3 + 14 + 19 * 3 + sum(cl[keys[i]] * v for i, v in cl_depth.items()) + payload


def model_bytes(stream, offsets, line, bpp):
    """zlib-stream bytes under the model: per band the smaller of its match block and png_reference's literal-only block, byte-aligned
    by an empty stored block (3 bits, pad, 4 bytes); 2 + 4 bytes of framing."""
    total = 6
    for i in range(len(offsets) - 1):
        band = stream[offsets[i]:offsets[i + 1]]
        bits = min(model_bits(parse(band, line, bpp)), band_model_bits(band)[0])
        total += (bits + 3 + 7) // 8 + 4
    return total


# ---- a token-recording inflate (RFC 1951) ----------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, pos=0):
        self.d, self.p = data, 8 * pos

    def take(self, n):
        v = 0
        for k in range(n):
            v |= (self.d[self.p >> 3] >> (self.p & 7) & 1) << k
            self.p += 1
        return v

    def align(self):
        self.p = (self.p + 7) & ~7


def _decoder(lengths):
    """{(length, code): symbol} of the canonical code with these lengths."""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, v in enumerate(lengths):
        if v:
            table[(v, nxt[v])] = s
            nxt[v] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = code << 1 | bits.take(1)
        if (n, code) in table:
            return table[(n, code)]
    raise ValueError('no such code')


def inflate_tokens(data, pos=0):
    """The blocks of the raw deflate stream at data[pos:] -> (blocks, bytes, end): a block is a dict with `type` (0 stored, 1 fixed,
    2 dynamic), `final`, `start` / `end` (byte offsets of its first bit and past its last bit, rounded outwards), `tokens` (ints and
    (length, distance) pairs; a stored block's bytes are literals) and, for a dynamic block, `ll` and `dist` code lengths."""
    bits, out, blocks = _Bits(data, pos), bytearray(), []
    while True:
        start = bits.p >> 3
        final, kind = bits.take(1), bits.take(2)
        blk = dict(type=kind, final=final, start=start, tokens=[])
        if kind == 0:
            bits.align()
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xffff
            at = bits.p >> 3
            blk['tokens'] = list(data[at:at + n])
            out += data[at:at + n]
            bits.p += 8 * n
        elif kind in (1, 2):
            if kind == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                blk['ll'], blk['dist'] = ll, dl
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = _symbol(bits, lt)
                if s < 256:
                    blk['tokens'].append(s)
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    ds = _symbol(bits, dt)
                    d = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                    blk['tokens'].append((length, d))
                    for _ in range(length):
                        out.append(out[-d])
        else:
            raise ValueError('block type 3')
        blk['end'] = (bits.p + 7) >> 3
        blocks.append(blk)
        if final:
            return blocks, bytes(out), blk['end']
