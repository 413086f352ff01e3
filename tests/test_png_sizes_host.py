"""The PNG coder's exported sizes, pinned: callers allocate what `*_workspace_bytes` and `*_capacity_bytes` return and the drivers carve
it up, and `*_rows_per_band` decides the bands of both.  tests/golden/png_sizes.json records what the library returned before the
coder's four workspace layouts became one (recorded from the build of the commit before that change, library version 330); the exports
must still return exactly these numbers, the refusals (0) included -- no GPU: the size functions are host code.

    python tests/test_png_sizes_host.py --record     rewrites the fixture from the library in use (CIAOSR_HIP_LIB selects one)
"""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciaosr_amd import _lib  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'png_sizes.json')
KINDS = ('ciaosr_png_', 'ciaosr_png_rgba_')
ROWS = (0, 1, 3, 7)
SIDES_H = (1, 31, 64, 1000, 65535)                          # 31, 64 and 1000 are no multiples of 3, 7 or the default rows per band
SIDES_W = (1, 31, 200, 8160, 65535)
# refused: a side of 0 or 65536, negative rows; the last one only by the match coder (a band above 2^31 bytes)
REFUSED_IMAGES = [(0, 5, 0), (5, 0, 0), (65536, 5, 0), (5, 65536, 0), (5, 5, -1), (65535, 65535, 65535)]
RECT_LISTS = [[(0, 0, 1, 1)], [(0, 0, 64, 200)], [(0, 0, 64, 200), (5, 7, 33, 65), (63, 199, 1, 1)],
              [(0, 0, 1000, 8160), (3, 5, 255, 255), (10, 10, 1, 1), (0, 0, 65535, 1), (7, 7, 1, 65535)]]
# refused: an empty side, a side of 65536, a negative origin
REFUSED_RECTS = [[(0, 0, 0, 5)], [(0, 0, 5, 0)], [(0, 0, 65536, 5)], [(0, 0, 5, 5), (0, -1, 5, 5)], [(-1, 0, 5, 5)]]
BANDS = (-1, 0, 1, 2, 3, 17, 1000, 100000)
TOTALS = (0, 1, 16, 4096, 65535, 65536, 10 ** 6, 1 << 33, 1 << 44)


def image_cases():
    good = list(itertools.product(SIDES_H, SIDES_W, ROWS))
    for kind, lz, what in itertools.product(KINDS, ('', 'lz_'), ('workspace_bytes', 'capacity_bytes')):
        if lz and what == 'capacity_bytes':                  # the match coder has the literal coder's capacities
            continue
        for h, w, rows in good + REFUSED_IMAGES:
            yield [kind + lz + what, h, w, rows]
    for kind in KINDS:
        for w, rows in itertools.product(SIDES_W + (0, 65536), ROWS + (-1,)):
            yield [kind + 'rows_per_band', w, rows]


def tile_cases():
    for kind, lz, what in itertools.product(KINDS, ('', 'lz_'), ('workspace_bytes', 'capacity_bytes')):
        if lz and what == 'capacity_bytes':
            continue
        name = kind + lz + 'tiles_' + what
        for rects, rows in itertools.product(RECT_LISTS, ROWS):
            yield [name, [list(r) for r in rects], len(rects), rows]
        for rects in REFUSED_RECTS:
            yield [name, [list(r) for r in rects], len(rects), 0]
        one = [list(RECT_LISTS[0][0])]
        yield [name, None, 1, 0]                             # a null rect list
        yield [name, one, 0, 0]                              # no tiles
        yield [name, one, 1, -1]                             # negative rows


def deflate_cases():
    for nb in BANDS:
        yield ['ciaosr_deflate_huff_workspace_bytes', nb]
    for name in ('ciaosr_deflate_huff_capacity_bytes', 'ciaosr_deflate_lz_workspace_bytes'):
        for total, nb in itertools.product(TOTALS, BANDS):
            yield [name, total, nb]


def call(lib, case):
    name, args = case[0], case[1:]
    fn = getattr(lib, name)
    if 'tiles_' in name:
        rects, n, rows = args
        host = None if rects is None else (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
        return fn(host, n, rows)
    if name.startswith('ciaosr_deflate_') and len(args) == 2:
        return fn(C.c_size_t(args[0]), args[1])
    return fn(*args)


FAMILIES = {'image': image_cases, 'tiles': tile_cases, 'deflate': deflate_cases}


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_exported_png_sizes_are_the_recorded_ones(family):
    lib = _lib.load()
    rows = _recorded()[family]
    assert [r[:-1] for r in rows] == list(FAMILIES[family]()), 'the fixture no longer lists the cases of this module'
    wrong = [(r[:-1], r[-1], call(lib, r[:-1])) for r in rows if call(lib, r[:-1]) != r[-1]]
    assert not wrong, f'{len(wrong)} of {len(rows)} sizes differ from the recorded ones (case, recorded, now): {wrong[:5]}'


def test_the_recorded_cases_cover_every_export_and_the_refusals():
    rec = _recorded()
    names = {r[0] for rows in rec.values() for r in rows}
    lib = _lib.load()
    exported = {n for n in _lib.SIGNATURES if ('png_' in n or 'deflate_' in n) and n.endswith(('_bytes', 'rows_per_band'))}
    assert names == exported and all(hasattr(lib, n) for n in names)
    for rows in rec.values():
        for name in {r[0] for r in rows}:
            values = [r[-1] for r in rows if r[0] == name]
            assert 0 in values and max(values) > 0, name      # every export is held to refusals and to sizes
    image = [r for r in rec['image'] if r[0] == 'ciaosr_png_workspace_bytes']
    assert {1, 65535} <= {r[2] for r in image} and {1, 3, 7} <= {r[3] for r in image}
    per_band = {(r[1], r[2]): r[3] for r in rec['image'] if r[0] == 'ciaosr_png_rows_per_band'}
    assert any(r[1] % per_band[(r[2], r[3])] for r in image if r[-1])                       # a short last band
    assert {len(r[1]) for r in rec['tiles'] if r[1]} >= {1, 3} and any([0, 0, 1, 1] in r[1] for r in rec['tiles'] if r[1])


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    out = {name: [case + [call(_lib.load(), case)] for case in cases()] for name, cases in sorted(FAMILIES.items())}
    with open(FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join(f' "{k}": [\n  ' + ',\n  '.join(json.dumps(r, separators=(',', ':')) for r in v) + '\n ]' for k, v in out.items()) + '\n}\n')
    print({k: len(v) for k, v in out.items()}, os.path.getsize(FIXTURE), 'bytes')
