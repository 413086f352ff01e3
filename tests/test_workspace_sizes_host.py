"""The exported workspace sizes, pinned: callers allocate what these functions return and the drivers carve it up, so a size that
shrinks under a later edit is a device buffer overrun.  tests/golden/workspace_sizes.json records, for a few hundred argument sets, the
bytes the library returned when the drivers' carve lists were unified (recorded from the build before that change); the exports must
still return them -- no GPU: the size functions read only scalar fields of the weight structs.

    python tests/test_workspace_sizes_host.py --record     rewrites the fixture from the library in use (CIAOSR_HIP_LIB selects one)
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

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_sizes.json')
MAPS = [(8, 8), (48, 48), (37, 51), (192, 192)]
HIDDEN = {'wide': [256, 256, 256, 256], 'narrow': [64, 32]}
_DUMMY = 0x1000       # a non-null pointer that nothing dereferences (ciaosr_mlp_workspace_bytes_16 refuses an MLP without weights)


def _mlp(in_dim, hidden, out_dim):
    m = _lib.MlpT()
    widths = list(hidden) + [out_dim]
    m.n_layers, m.act, m.in_dim = len(widths), _lib.ACT_RELU, in_dim
    k = in_dim
    for i, n in enumerate(widths):
        m.width[i], m.ld[i], m.weight[i], m.bias[i] = n, (k + 3) // 4 * 4, _DUMMY, _DUMMY
        k = n
    return m


def _options(block_mb):
    opt = _lib.OptionsT()
    opt.csa_block_mb = block_mb
    return C.byref(opt)


def head_cases(stride=1):
    """(C, non-local scales, nonlocal_max_scale, local_size, no_unfold, H, W, Q, hidden widths, csa_block_mb or None = no options)"""
    grid = itertools.product((4, 64, 180), ((0, 0), (1, 0), (1, 4), (3, 4)), (1, 2, 3), (0, 1), MAPS,
                             (1000, 65535, 65537, 589824, (1 << 20) - 1, (1 << 20) + 1), sorted(HIDDEN), (None, 0, 256))
    for c, (n_sc, max_sc), ls, nu, (h, w), q, hid, mb in itertools.islice(grid, 0, None, stride):
        yield [c, n_sc, max_sc, ls, nu, h, w, q, hid, mb]


def head_bytes(lib, case):
    c, n_sc, max_sc, ls, nu, h, w, q, hid, mb = case
    hw = _lib.HeadWeightsT()
    hw.channels, hw.nonlocal_channels, hw.nonlocal_max_scale, hw.local_size, hw.no_unfold = c, n_sc * c, max_sc, ls, nu
    d = (1 if nu else 9) * c
    hw.k, hw.v, hw.q = _mlp(d + 4, HIDDEN[hid], d), _mlp(d + n_sc * c + 4, HIDDEN[hid], d + n_sc * c), _mlp(d + n_sc * c, HIDDEN[hid], 3)
    if mb is None:
        n = lib.ciaosr_head_workspace_bytes(h, w, C.byref(hw), q)
        assert lib.ciaosr_head_workspace_bytes_opt(h, w, C.byref(hw), q, None) == n
        return n
    return lib.ciaosr_head_workspace_bytes_opt(h, w, C.byref(hw), q, _options(mb))


def rdn_cases():
    """(B, H, W, mid_channels, growth, num_blocks, num_layers)"""
    for b, (h, w), cfg in itertools.product((1, 7, 16), MAPS, ((64, 64, 16, 8), (32, 32, 4, 4))):
        yield [b, h, w] + list(cfg)


def rdn_bytes(lib, case):
    b, h, w, c, g, nb, nl = case
    rw = _lib.RdnWeightsT()
    rw.mid_channels, rw.growth, rw.num_blocks, rw.num_layers = c, g, nb, nl
    return lib.ciaosr_rdn_workspace_bytes_batch(b, h, w, C.byref(rw))


def mlp_cases():
    """(in_dim, hidden widths, out_dim, rows, 16-bit)"""
    for (i, o), hid, rows, h16 in itertools.product(((580, 576), (644, 640), (36, 3), (1624, 3)), sorted(HIDDEN), (1, 1000, 262144), (0, 1)):
        yield [i, hid, o, rows, h16]


def mlp_bytes(lib, case):
    i, hid, o, rows, h16 = case
    return (lib.ciaosr_mlp_workspace_bytes_16 if h16 else lib.ciaosr_mlp_workspace_bytes)(C.byref(_mlp(i, HIDDEN[hid], o)), rows)


FAMILIES = {'head': (lambda: head_cases(stride=41), head_bytes), 'rdn': (rdn_cases, rdn_bytes), 'mlp': (mlp_cases, mlp_bytes)}


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_exported_workspace_sizes_are_the_recorded_ones(family):
    lib = _lib.load()
    cases, fn = FAMILIES[family]
    rows = _recorded()[family]
    assert [r[:-1] for r in rows] == list(cases()), 'the fixture no longer lists the cases of this module'
    assert len(rows) >= 24 and all(r[-1] > 0 for r in rows)
    wrong = [(r[:-1], r[-1], fn(lib, r[:-1])) for r in rows if fn(lib, r[:-1]) != r[-1]]
    assert not wrong, f'{len(wrong)} of {len(rows)} sizes differ from the recorded ones (case, recorded, now): {wrong[:5]}'


def test_the_recorded_cases_vary_what_the_sizes_depend_on():
    head = _recorded()['head']
    assert 200 <= len(head) <= 600
    for col, want in enumerate([{4, 64, 180}, {0, 1, 3}, {0, 4}, {1, 2, 3}, {0, 1}]):
        assert {r[col] for r in head} == want, col
    assert {(r[5], r[6]) for r in head} == set(MAPS) and {r[9] for r in head} == {None, 0, 256}
    qs = {r[7] for r in head}
    assert min(qs) < 65536 < max(qs) and any(65536 < q < 1 << 20 for q in qs) and max(qs) > 1 << 20
    assert {r[0] for r in _recorded()['rdn']} == {1, 7, 16}


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    out = {name: [case + [fn(_lib.load(), case)] for case in cases()] for name, (cases, fn) in sorted(FAMILIES.items())}
    with open(FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join(f' "{k}": [\n  ' + ',\n  '.join(json.dumps(r, separators=(',', ':')) for r in v) + '\n ]' for k, v in out.items()) + '\n}\n')
    print({k: len(v) for k, v in out.items()}, os.path.getsize(FIXTURE), 'bytes')
