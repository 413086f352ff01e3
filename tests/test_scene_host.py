"""The persistent head scene, host side (no GPU): the size and route exports, the descriptor's mirror, the window planner against brute
force over tile_plan.plan, and the scene cache."""
import ctypes as C
import itertools

import pytest

from ciaosr_amd import _lib, scene, tile_plan
from tests.test_workspace_sizes_host import HIDDEN, _mlp, head_cases


def _weights(case):
    c, n_sc, max_sc, ls, nu = case[:5]
    hw = _lib.HeadWeightsT()
    hw.channels, hw.nonlocal_channels, hw.nonlocal_max_scale, hw.local_size, hw.no_unfold = c, n_sc * c, max_sc, ls, nu
    hw.softmax_scale = 1.0
    d = (1 if nu else 9) * c
    hid = HIDDEN[case[8]]
    hw.k, hw.v, hw.q = _mlp(d + 4, hid, d), _mlp(d + n_sc * c + 4, hid, d + n_sc * c), _mlp(d + n_sc * c, hid, 3)
    return hw


def _opt(mb):
    if mb is None:
        return None
    o = _lib.OptionsT()
    o.csa_block_mb = mb
    return C.byref(o)


def _fused_weights(c=64):
    """A head the fp32 fused route accepts: hidden 256 x 4, local_size 2, a (never dereferenced) fragment pointer per fused layer."""
    hw = _weights([c, 1, 0, 2, 0, 0, 0, 0, 'wide', None])
    for m, layers in ((hw.k, range(1, 5)), (hw.v, range(1, 5)), (hw.q, range(0, 4))):
        for i in layers:
            m.frag[i] = 0x1000
    return hw


def test_scene_exports_are_declared():
    lib = _lib.load()
    assert lib.ciaosr_version() >= 230
    for name, res, n_args in (('ciaosr_head_scene_bytes', C.c_size_t, 5), ('ciaosr_head_prepare_workspace_bytes', C.c_size_t, 5),
                              ('ciaosr_head_query_workspace_bytes', C.c_size_t, 4), ('ciaosr_head_route_code', C.c_int, 6),
                              ('ciaosr_make_coord_cell_window_f32', C.c_int, 10)):
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
    for sfx in ('f32', 'bf16', 'f16'):
        assert len(_lib.SIGNATURES['ciaosr_head_prepare_' + sfx][1]) == 13 and hasattr(lib, 'ciaosr_head_prepare_' + sfx)
        assert len(_lib.SIGNATURES['ciaosr_head_query_' + sfx][1]) == 14 and hasattr(lib, 'ciaosr_head_query_' + sfx)


def test_descriptor_mirror_matches_the_library():
    assert _lib.load().ciaosr_sizeof(b'ciaosr_head_scene_t') == C.sizeof(_lib.HeadSceneT) > 0
    assert _lib.STRUCTS['ciaosr_head_scene_t'] is _lib.HeadSceneT


def test_scene_sizes_over_the_workspace_grid():
    """scene_bytes > 0; a function of (H, W, w, route), not of Q beyond the route; the query's scratch is part of head_forward's."""
    lib = _lib.load()
    by_route = {}
    n = 0
    for case in head_cases(stride=41):
        c, n_sc, max_sc, ls, nu, h, w, q, hid, mb = case
        hw, opt = _weights(case), _opt(mb)
        sb = lib.ciaosr_head_scene_bytes(h, w, C.byref(hw), q, opt)
        assert sb > 0, case
        route = lib.ciaosr_head_route_code(h, w, C.byref(hw), q, 0, opt)
        assert route >= 0, case
        d = (1 if nu else 9) * c
        floor = h * w * (d + n_sc * c + 2 * HIDDEN[hid][0]) * 4                      # U, Tk, Tv
        assert floor <= sb <= floor + h * w * 9 * 260 * 4 + 4 * 256, case
        key = (c, n_sc, max_sc, ls, nu, h, w, hid, route)
        assert by_route.setdefault(key, sb) == sb, case
        assert lib.ciaosr_head_prepare_workspace_bytes(h, w, C.byref(hw), q, opt) > 0, case
        # a descriptor as prepare would write it is needed for the query size: take the one the sizes imply
        desc = _lib.HeadSceneT()
        desc.magic, desc.H, desc.W, desc.C, desc.Cn, desc.D, desc.Dv = 0x43530001, h, w, c, n_sc * c, d, d + n_sc * c
        desc.J, desc.q_plan, desc.precision, desc.route = {1: 1, 2: 4, 3: 9}[ls], q, 0, route
        qb = lib.ciaosr_head_query_workspace_bytes(C.byref(desc), C.byref(hw), q, opt)
        assert 0 < qb <= lib.ciaosr_head_workspace_bytes_opt(h, w, C.byref(hw), q, opt), case
        small = lib.ciaosr_head_query_workspace_bytes(C.byref(desc), C.byref(hw), 1, opt)
        assert 0 < small <= qb, case
        n += 1
    assert n >= 200


def test_scene_bytes_per_pixel_are_the_documented_ones():
    lib = _lib.load()
    hw = _fused_weights()
    for h, w in ((48, 48), (192, 192)):
        hwn = h * w
        with_g = lib.ciaosr_head_scene_bytes(h, w, C.byref(hw), 16 * hwn, None)
        without = lib.ciaosr_head_scene_bytes(h, w, C.byref(hw), hwn, None)
        assert 0 <= with_g - 13968 * hwn <= 4 * 256 and 0 <= without - 4608 * hwn <= 4 * 256, (h, w, with_g, without)
    assert round(13968 * 192 * 192 / 1e6) == 515 and round(13968 * 48 * 48 / 1e6) == 32


def test_route_code_changes_only_across_the_logit_table_threshold():
    """The logit table exists iff Q * J > 9 * HW: J = 4, HW = 24 * 20 = 480 -> Q > 1080."""
    lib = _lib.load()
    hw = _fused_weights()
    code = lambda q: lib.ciaosr_head_route_code(24, 20, C.byref(hw), q, 0, None)
    assert code(1) == code(500) == code(1080) >= 0
    assert code(1081) == code(3510) == code(1 << 20) >= 0
    assert code(1080) != code(1081)
    assert (code(1080) >> 3) & 7 == 0 and (code(1081) >> 3) & 7 != 0 and code(1081) & 1 == 1
    assert lib.ciaosr_head_scene_bytes(24, 20, C.byref(hw), 1081, None) - lib.ciaosr_head_scene_bytes(24, 20, C.byref(hw), 1080, None) == 480 * 9 * 260 * 4
    # refusals are the call's error codes: a 16-bit precision without 16-bit fragments, a precision that does not exist
    assert lib.ciaosr_head_route_code(24, 20, C.byref(hw), 3510, 2, None) == -3
    assert lib.ciaosr_head_route_code(24, 20, C.byref(hw), 3510, 3, None) == -1
    assert lib.ciaosr_head_route_code(24, 20, C.byref(hw), 0, 0, None) == -1


def test_query_size_refuses_a_descriptor_that_does_not_fit():
    lib = _lib.load()
    hw = _fused_weights()
    desc = _lib.HeadSceneT()
    desc.magic, desc.H, desc.W, desc.C, desc.Cn, desc.D, desc.Dv, desc.J = 0x43530001, 24, 20, 64, 64, 576, 640, 4
    desc.q_plan, desc.precision = 3510, 0
    desc.route = lib.ciaosr_head_route_code(24, 20, C.byref(hw), 3510, 0, None)
    assert lib.ciaosr_head_query_workspace_bytes(C.byref(desc), C.byref(hw), 100, None) > 0
    for field, value in (('magic', 0), ('C', 32), ('Dv', 576), ('precision', 2), ('route', desc.route ^ 8), ('q_plan', 100)):
        bad = _lib.HeadSceneT.from_buffer_copy(desc)
        setattr(bad, field, value)
        assert lib.ciaosr_head_query_workspace_bytes(C.byref(bad), C.byref(hw), 100, None) == 0, field
    no_table = _lib.OptionsT()
    no_table.head_route = _lib.HEAD_NO_LOGIT_TABLE                                  # a route-changing option bit
    assert lib.ciaosr_head_query_workspace_bytes(C.byref(desc), C.byref(hw), 100, C.byref(no_table)) == 0


# ---- the window planner ----------------------------------------------------------------------------------------------------------------
def _brute(h, w, tile, overlap, ht, wt, window):
    """Per tile of tile_plan.plan that meets the window: (y0, x0) -> the set of HR pixels, and the tile order."""
    wi0, wj0, wh, ww = window
    out = []
    for t in tile_plan.plan(h, w, ht, wt, tile, overlap):
        px = {(i, j) for i in range(max(t['i0'], wi0), min(t['i1'], wi0 + wh)) for j in range(max(t['j0'], wj0), min(t['j1'], wj0 + ww))}
        if px:
            out.append(((t['y0'], t['x0']), px))
    return out


@pytest.mark.parametrize('ht,wt,any_scale,window', [(80, 112, False, (9, 41, 61, 35)), (80, 112, False, (0, 0, 1, 1)), (80, 112, False, None),
                                                    (80, 112, True, (9, 41, 61, 35)), (108, 151, True, (9, 41, 61, 35)),
                                                    (108, 151, True, (0, 0, 1, 1)), (108, 151, True, (107, 150, 1, 1)), (108, 151, True, None)])
def test_window_planner_against_brute_force(ht, wt, any_scale, window):
    h, w, tile, overlap = 40, 56, 32, 8
    got = scene.plan_window(h, w, tile, overlap, ht, wt, window, scale=2, any_scale=any_scale)
    want = _brute(h, w, tile, overlap, ht, wt, window or (0, 0, ht, wt))
    assert [(t['y0'], t['x0']) for t in got] == [o for o, _ in want]                 # the touched tiles, in the blend order
    origins = [(y0, x0) for y0 in tile_plan.tile_starts(h, tile, overlap) for x0 in tile_plan.tile_starts(w, tile, overlap)]
    for t, (_, px) in zip(got, want):
        assert {(i, j) for i in range(t['a0'], t['a1']) for j in range(t['b0'], t['b1'])} == px
        assert origins[t['index']] == (t['y0'], t['x0']) and (t['th'], t['tw']) == (tile, tile)
        gh, gw, r0, r1, c0, c1, frame = t['grid']
        assert (r1 - r0, c1 - c0) == (t['a1'] - t['a0'], t['b1'] - t['b0']) and 0 <= r0 < r1 <= gh and 0 <= c0 < c1 <= gw
        if any_scale:
            assert (gh, gw, r0, c0) == (ht, wt, t['a0'], t['b0']) and frame == (h, t['y0'], tile, w, t['x0'], tile)
        else:
            assert (gh, gw) == (64, 64) and frame is None and (r0, c0) == (t['a0'] - 2 * t['y0'], t['b0'] - 2 * t['x0'])
    if window == (9, 41, 61, 35):
        assert len(got) == 4                                                        # crosses both seams
    if window == (0, 0, 1, 1):
        assert len(got) == 1


def test_window_planner_refusals():
    for bad in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (76, 0, 5, 5), (0, 108, 5, 5), (80, 0, 1, 1)):
        with pytest.raises(ValueError):
            scene.plan_window(40, 56, 32, 8, 80, 112, bad, scale=2)
        with pytest.raises(ValueError):
            scene.check_window(80, 112, bad)
    assert scene.check_window(80, 112, None) == (0, 0, 80, 112)
    # the size rule: without tile_any_scale only the (h * s) x (w * s) image of the integer test_cfg.scale exists
    for ht, wt, s in ((108, 151, 2), (80, 112, None), (80, 112, 2.5), (120, 168, 2), (80, 113, 2)):
        with pytest.raises(ValueError):
            scene.plan_window(40, 56, 32, 8, ht, wt, None, scale=s)
    assert len(scene.plan_window(40, 56, 32, 8, 108, 151, None, scale=2, any_scale=True)) == 4
    assert scene.target_size(40, 56, scale=2.7) == (108, 151) and scene.target_size(40, 56, size=(7, 9)) == (7, 9)
    for kw in (dict(), dict(size=(4, 4), scale=2), dict(size=(0, 4))):
        with pytest.raises(ValueError):
            scene.target_size(40, 56, **kw)


# ---- the scene cache -------------------------------------------------------------------------------------------------------------------
class _Fake:
    def __init__(self, key, nbytes):
        self.key, self.nbytes = key, nbytes


def _cache(budget, size=100):
    built = []

    def build(key):
        built.append(key)
        return _Fake(key, size)
    return scene.SceneCache(budget, build), built


def test_scene_cache_evicts_the_least_recently_used_under_its_budget():
    cache, built = _cache(300)
    for k in 'abc':
        assert cache.get(k).key == k
    assert cache.get('a').key == 'a' and built == list('abc')                       # a hit builds nothing and makes 'a' the most recent
    cache.get('d')                                                                  # 'b' is now the oldest
    assert list(cache.entries) == ['c', 'a', 'd'] and cache.nbytes == 300
    cache.get('b')
    assert list(cache.entries) == ['a', 'd', 'b'] and built == list('abcdb') and cache.builds == 5      # the rebuilt entry is counted
    for k in itertools.islice(itertools.cycle('abcdef'), 40):
        cache.get(k)
        assert cache.nbytes <= 300 and cache.nbytes == 100 * len(cache.entries)


def test_scene_cache_always_holds_the_entry_in_use():
    cache, built = _cache(50)                                                       # smaller than one scene: works by rebuilding
    for k in 'abab':
        hit = cache.get(k)
        assert hit.key == k and list(cache.entries) == [k] and cache.entries[k] is hit
    assert cache.builds == 4 and built == list('abab')
    cache, _ = _cache(100)
    cache.get('a')
    assert cache.get('a') is cache.get('a') and cache.builds == 1
    cache.clear()
    assert cache.nbytes == 0 and not cache.entries
