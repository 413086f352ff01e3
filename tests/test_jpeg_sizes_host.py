"""The JPEG coders' exported sizes, pinned: callers allocate what the fourteen `ciaosr_jpeg_*{workspace,capacity,result}_bytes` exports
return and the drivers carve it up.  tests/golden/jpeg_sizes.json records what the library returned before the three coders' host
plans, workspace carves and drivers became one set of parts in csrc/jpeg_u8.h (recorded from the build of the commit before that
change, library version 340); the exports must still return exactly these numbers, the refusals (0) included -- no GPU: the size
functions are host code.

    python tests/test_jpeg_sizes_host.py --record     rewrites the fixture from the library in use (CIAOSR_HIP_LIB selects one)
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

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_sizes.json')
KINDS = ('ciaosr_jpeg_', 'ciaosr_jpeg_opt_', 'ciaosr_jpeg_prog_')
SUBS = (0, 2, 4)                                            # 4:4:4, 4:2:0, grey (which the progressive family refuses)
REFUSED_SUBS = (1, 3, -1)
MCUS = (0, 1, 5, 128)
SIDES = (1, 8, 9, 31, 64, 1000, 18256, 65535)               # 9 and 31 are no multiples of an MCU's side, 1000 of no 4:2:0 MCU's
# every side squared, both ways across, and the frequency-limit pair: 64 x the blocks of 18256 x 18256 in 4:4:4 stay below 10^9,
# those of 18256 x 18264 do not (refused by the optimised and the progressive family only)
IMAGES = [(s, s) for s in SIDES] + [(1, 65535), (65535, 1), (9, 1000), (1000, 31), (31, 8), (64, 18256), (8, 9), (18256, 18264)]
REFUSED_IMAGES = [(0, 5), (5, 0), (65536, 5), (5, 65536)]
RECT_LISTS = [[(0, 0, 1, 1)],
              [(0, 0, 64, 31), (5, 7, 33, 65), (63, 199, 1, 1)],
              [(0, 0, 1000, 18256), (3, 5, 255, 255), (10, 10, 1, 1), (0, 0, 65535, 1), (7, 7, 9, 65535)]]
# refused: an empty side, a side of 65536, a negative origin
REFUSED_RECTS = [[(0, 0, 0, 5)], [(0, 0, 5, 0)], [(0, 0, 65536, 5)], [(0, 0, 5, 5), (0, -1, 5, 5)], [(-1, 0, 5, 5)]]
RESULTS = (-1, 0, 1, 3, 1000)


def image_cases():
    for kind in KINDS:
        for (h, w), sub, mcus in itertools.product(IMAGES, SUBS, MCUS):
            yield [kind + 'workspace_bytes', h, w, sub, mcus]
        for (h, w), sub in itertools.product(IMAGES, SUBS):
            yield [kind + 'capacity_bytes', h, w, sub]
        for sub in REFUSED_SUBS:
            yield [kind + 'workspace_bytes', 64, 31, sub, 0]
            yield [kind + 'capacity_bytes', 64, 31, sub]
        for (h, w), sub in itertools.product(REFUSED_IMAGES, SUBS[:2]):
            yield [kind + 'workspace_bytes', h, w, sub, 0]
            yield [kind + 'capacity_bytes', h, w, sub]
        for sub in SUBS:
            yield [kind + 'workspace_bytes', 64, 31, sub, -1]


def tile_cases():
    one = [list(RECT_LISTS[0][0])]
    for kind in KINDS:
        ws, cap = kind + 'tiles_workspace_bytes', kind + 'tiles_capacity_bytes'
        for rects, sub in itertools.product(RECT_LISTS, SUBS):
            for mcus in MCUS:
                yield [ws, [list(r) for r in rects], len(rects), sub, mcus]
            yield [cap, [list(r) for r in rects], len(rects), sub]
        for rects, sub in itertools.product(REFUSED_RECTS, SUBS[:2]):
            yield [ws, [list(r) for r in rects], len(rects), sub, 0]
            yield [cap, [list(r) for r in rects], len(rects), sub]
        for sub in REFUSED_SUBS:
            yield [ws, one, 1, sub, 0]
            yield [cap, one, 1, sub]
        yield [ws, None, 1, 0, 0]                            # a null rect list
        yield [cap, None, 1, 0]
        yield [ws, one, 0, 0, 0]                             # no tiles
        yield [cap, one, 0, 0]
        yield [ws, one, 1, 0, -1]                            # negative MCUs per chunk


def result_cases():
    for kind in KINDS[1:]:
        for n in RESULTS:
            yield [kind + 'result_bytes', n]


def call(lib, case):
    name, args = case[0], case[1:]
    fn = getattr(lib, name)
    if 'tiles_' in name:
        rects = args[0]
        host = None if rects is None else (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
        return fn(host, *args[1:])
    return fn(*args)


FAMILIES = {'image': image_cases, 'tiles': tile_cases, 'result': result_cases}


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_exported_jpeg_sizes_are_the_recorded_ones(family):
    lib = _lib.load()
    rows = _recorded()[family]
    assert [r[:-1] for r in rows] == list(FAMILIES[family]()), 'the fixture no longer lists the cases of this module'
    wrong = [(r[:-1], r[-1], call(lib, r[:-1])) for r in rows if call(lib, r[:-1]) != r[-1]]
    assert not wrong, f'{len(wrong)} of {len(rows)} sizes differ from the recorded ones (case, recorded, now): {wrong[:5]}'


def test_the_recorded_cases_cover_every_export_and_the_refusals():
    rec = _recorded()
    names = {r[0] for rows in rec.values() for r in rows}
    lib = _lib.load()
    exported = {n for n in _lib.SIGNATURES if 'jpeg_' in n and n.endswith('_bytes')}
    assert names == exported and len(names) == 14 and all(hasattr(lib, n) for n in names)     # 4 baseline, 5 optimised, 5 progressive
    for rows in rec.values():
        for name in {r[0] for r in rows}:
            values = [r[-1] for r in rows if r[0] == name]
            assert 0 in values and max(values) > 0, name      # every export is held to refusals and to sizes
    assert sum(len(rows) for rows in rec.values()) >= 1000
    size = {tuple(r[:-1]): r[-1] for r in rec['image']}
    for kind in KINDS:
        for sub in SUBS:                                     # grey: sizes of its own, and none in the progressive family
            assert (size[(kind + 'workspace_bytes', 64, 64, sub, 0)] > 0) == (sub != 4 or 'prog_' not in kind)
        assert size[(kind + 'workspace_bytes', 18256, 18256, 0, 0)] > 0                     # the frequency limit, from both sides
        assert (size[(kind + 'workspace_bytes', 18256, 18264, 0, 0)] > 0) == (kind == KINDS[0])
        assert len({size[(kind + 'workspace_bytes', 1000, 1000, 0, m)] for m in MCUS}) == len(MCUS)
    assert {len(r[1]) for r in rec['tiles'] if r[1]} >= {1, 3, 5} and any([0, 0, 1, 1] in r[1] for r in rec['tiles'] if r[1])


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    out = {name: [case + [call(_lib.load(), case)] for case in cases()] for name, cases in sorted(FAMILIES.items())}
    with open(FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join(f' "{k}": [\n  ' + ',\n  '.join(json.dumps(r, separators=(',', ':')) for r in v) + '\n ]' for k, v in out.items()) + '\n}\n')
    print({k: len(v) for k, v in out.items()}, os.path.getsize(FIXTURE), 'bytes')
