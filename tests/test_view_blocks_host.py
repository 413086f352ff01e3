"""The host side of `test_cfg.view_blocks` (no GPU): `scene.view_blocks_fit`, the numpy reference of the block-ordered member lists
(tests/view_blocks_reference.py) on the inputs of tests/test_view_blocks_gpu.py, the new exports' host arithmetic, and the refusal of
`ciaosr_head_query_flag_offset`'s arguments."""
import math

import numpy as np

from ciaosr_amd import scene
from tests import view_blocks_reference as br
from tests import view_reference as vr


def _m(zoom, angle, size=(64, 64)):
    return scene.view_matrix((20.0, 20.0), zoom, angle, size)


def test_view_blocks_fit_bound():
    for angle in (0, 30, 45, 90):
        assert scene.view_blocks_fit(_m(4.0, angle)), angle
    assert not scene.view_blocks_fit(_m(1.45, 0))                      # 3 / 1.45 > 2 (3 / 1.5 = 2 is the boundary)
    worst = math.degrees(math.atan(1.0 / 3.0))                         # 3 |sin| + |cos| = sqrt(10)
    assert scene.view_blocks_fit(_m(1.6, worst)) and not scene.view_blocks_fit(_m(1.55, worst))
    assert scene.view_blocks_fit(_m(1.6, -worst)) and scene.view_blocks_fit(_m(1.6, 180 - worst))
    # the two rows are tested on their own, and the translation does not matter
    assert scene.view_blocks_fit((0.5, 0.0, -7.0, 0.0, 0.5, 1e6))
    assert not scene.view_blocks_fit((0.5, 0.0, 0.0, 0.0, 0.7, 0.0)) and not scene.view_blocks_fit((0.3, 0.6, 0.0, 0.0, 0.5, 0.0))
    assert scene.view_blocks_fit((2.0, 0.0, 0.0, 0.0, 2.0 / 3.0 - 1e-9, 0.0)) and not scene.view_blocks_fit((2.0 + 1e-9, 0.0, 0.0, 0.0, 0.5, 0.0))


def _inputs():
    m = scene.view_matrix(*br.ARGS, br.SIZE)
    one = [(0, 0, *br.ONE_LR)]
    tiled = scene.plan_view(*br.TILED_LR, br.TILE, br.OVERLAP, any_scale=True)
    return m, one, tiled


def test_the_gpu_inputs_exercise_blocks_and_pads():
    """An input that exercises nothing cannot pass: cut views, full and padded blocks, a list longer than index order, and the bound."""
    m, one, tiled = _inputs()
    hv, wv = br.SIZE
    n_q = hv * wv
    assert hv % 2 == 1 and wv % 4 != 0 and scene.view_blocks_fit(m)
    assert tiled == [(0, 0, 32, 32), (0, 24, 32, 32), (8, 0, 32, 32), (8, 24, 32, 32)]
    y, x = vr.lr_points(m, hv, wv)
    for frames in (one, tiled):
        lists = [br.block_list(m, hv, wv, f) for f in frames]
        assert all(0 < b['members'] < n_q for b in lists), [b['members'] for b in lists]
        assert all(b['full'] > 0 and b['padded'] > 0 and b['full'] + b['padded'] == b['blocks'] for b in lists)
        for f, b in zip(frames, lists):
            mem = vr.members(y, x, f)
            assert b['members'] == int(mem.sum()) and b['q_index'].shape == (8 * b['blocks'],) and 8 * b['blocks'] > b['members']
            qs = b['q_index'][b['q_index'] >= 0]
            assert np.array_equal(np.sort(qs), np.flatnonzero(mem))                       # every member once, nothing else
            # member entries: exactly the index-order list's coordinates; pads: a copy of a member of the same block
            want = vr.coord_in(y, x, f)
            assert np.array_equal(b['coord'][b['q_index'] >= 0].view(np.int32), want[qs].view(np.int32))
            blocks = b['q_index'].reshape(-1, 8)
            coords = b['coord'].reshape(-1, 8, 2)
            for qb, cb in zip(blocks, coords):
                first = int(np.argmax(qb >= 0))
                assert np.array_equal(cb[qb < 0].view(np.int32), np.broadcast_to(cb[first], (int((qb < 0).sum()), 2)).view(np.int32))
                # entry e is pixel (row e >> 2, column e & 3) of a block aligned to (2, 4)
                i, j = qb[first] // wv - (first >> 2), qb[first] % wv - (first & 3)
                assert i % 2 == 0 and j % 4 == 0
                assert all(q == (i + (e >> 2)) * wv + j + (e & 3) for e, q in enumerate(qb) if q >= 0)
            # blocks in increasing block index
            order = [(qb[qb >= 0][0] // wv // 2) * ((wv + 3) // 4) + (qb[qb >= 0][0] % wv) // 4 for qb in blocks]
            assert order == sorted(order) and len(set(order)) == len(order)
    # the bottom row of blocks and the right column hold pixels outside the 45 x 53 grid: pads that are no query at all
    q = br.block_pixels(hv, wv)
    assert q.shape == (23 * 14, 8) and (q[-1] < 0).sum() >= 4 and (q[13] < 0).sum() == 6 and (q >= 0).sum() == n_q
    # a 1 x 1 grid: one block of one member and seven pads -- a list longer than the grid
    tiny = br.block_list(scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1)), 1, 1, (0, 0, 40, 56))
    assert tiny['members'] == 1 and tiny['blocks'] == 1 and tiny['q_index'].tolist() == [0] + [-1] * 7


def test_block_extent_stays_inside_the_window_under_the_bound():
    """The derivation of the bound, checked on the inputs: under `view_blocks_fit` the LR positions of a block's members span at most
    2 LR pixels along each axis."""
    m, one, _ = _inputs()
    hv, wv = br.SIZE
    y, x = vr.lr_points(m, hv, wv)
    q = br.block_pixels(hv, wv)
    for qb in q:
        qs = qb[qb >= 0]
        assert np.ptp(y[qs]) <= 2.0 and np.ptp(x[qs]) <= 2.0
    full = q[(q >= 0).all(1)]                                           # the full blocks reach the extent the bound is about
    assert abs(max(np.ptp(y[qb]) for qb in full) - (3 * abs(m[1]) + abs(m[0]))) < 1e-12


def test_block_exports_are_declared():
    import ctypes as C
    from ciaosr_amd import _lib
    lib = _lib.load()
    sig = _lib.SIGNATURES
    assert sig['ciaosr_view_count_blocks_i32'] == sig['ciaosr_view_count_i32']
    assert sig['ciaosr_view_count_blocks_many_i32'] == sig['ciaosr_view_count_many_i32']
    assert sig['ciaosr_view_select_blocks_f32'] == sig['ciaosr_view_select_f32']
    assert sig['ciaosr_head_query_flag_offset'][1][-1] is not None and len(sig['ciaosr_head_query_flag_offset'][1]) == 5
    per_wg = lib.ciaosr_view_block_blocks()
    assert per_wg == 256
    # two rows (members, live blocks) of one int per workgroup and tile; a thread per 4 x 2 block
    for (hv, wv), n_tiles in (((45, 53), 4), ((1, 1), 1), ((2, 4 * per_wg), 3), ((2, 4 * per_wg + 1), 3), ((3, 700), 117)):
        blocks = -(-hv // 2) * -(-wv // 4)
        assert lib.ciaosr_view_blocks_workspace_bytes(hv, wv, n_tiles) == 2 * n_tiles * 4 * -(-blocks // per_wg), (hv, wv)
    assert lib.ciaosr_view_blocks_workspace_bytes(0, 5, 1) == 0 and lib.ciaosr_view_blocks_workspace_bytes(5, 5, 0) == 0
    assert lib.ciaosr_view_blocks_workspace_bytes(1 << 16, 1 << 16, 1) == 0
    assert lib.ciaosr_view_blocks_workspace_bytes(1, 2 ** 31 - 1, 1) == 2 * 4 * (2 ** 29 // per_wg)
    sizes = [(45, 53), (1, 1), (3, 700)]
    arr = (C.c_int * 6)(*[v for s in sizes for v in s])
    off = 0
    for v, (hv, wv) in enumerate(sizes):
        assert lib.ciaosr_view_blocks_many_workspace_offset(arr, 3, 4, v) == off and off % 256 == 0
        off += -(-lib.ciaosr_view_blocks_workspace_bytes(hv, wv, 4) // 256) * 256
    assert lib.ciaosr_view_blocks_many_workspace_bytes(arr, 3, 4) == off
    assert lib.ciaosr_view_blocks_many_workspace_bytes(arr, 0, 4) == 0 and lib.ciaosr_view_blocks_many_workspace_offset(arr, 3, 4, 3) == 0
    # the flag offset refuses what the query refuses, before anything else
    off = C.c_size_t(7)
    assert lib.ciaosr_head_query_flag_offset(None, None, 16, None, C.byref(off)) == -1 and off.value == 7
    desc = _lib.HeadSceneT()
    assert lib.ciaosr_head_query_flag_offset(C.byref(desc), None, 16, None, None) == -1


def test_render_cli_passes_view_blocks():
    from tools import render
    argv = ['cfg.py', 'None', 'img.png', '--view', '12', '12', '2.5', '30', '--size', '40', '52', '--out', 'out']
    assert render.parse_args(argv).view_blocks is False
    assert render.parse_args(argv + ['--view-blocks']).view_blocks is True
