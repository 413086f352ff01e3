"""The host side of CiaoSR.render_many / prefetch (no GPU): which tiles the targets touch, the tile-major plan (`scene.plan_union`,
`scene.group_missing`), the scene cache under entries built outside it (`make_room` / `put` / `hold` / `room`), and the `Grid` / `View`
records' refusals against the single calls'."""
import pytest

from ciaosr_amd import scene

LR = (40, 56)                   # tile 32, overlap 8, tile_any_scale: 2 x 2 tiles
TILES = [(0, 0), (0, 24), (8, 0), (8, 24)]
HR = (108, 151)                 # x2.7


def _touched(window=None, size=HR):
    plan = scene.plan_window(*LR, 32, 8, *size, window, any_scale=True)
    return [t['index'] for t in plan], [(t['y0'], t['x0']) for t in plan]


def test_the_inputs_touch_the_tiles_the_plan_is_tested_on():
    assert scene.plan_view(*LR, 32, 8, any_scale=True) == [(y, x, 32, 32) for y, x in TILES]
    assert _touched() == ([0, 1, 2, 3], TILES)
    assert _touched((0, 0, 5, 7)) == ([0], TILES[:1])
    assert _touched((0, 0, 20, 151)) == ([0, 1], TILES[:2])
    assert _touched(size=(80, 112)) == ([0, 1, 2, 3], TILES)


def test_union_order_users_and_groups():
    full, corner, top = _touched()[0], _touched((0, 0, 5, 7))[0], _touched((0, 0, 20, 151))[0]
    union, users = scene.plan_union([corner, top])
    assert union == [0, 1] and users == {0: [0, 1], 1: [1]}
    union, users = scene.plan_union([top, full, corner])
    assert union == [0, 1, 2, 3] and list(users) == union                        # row-major, whatever order the targets come in
    assert users == {0: [0, 1, 2], 1: [0, 1], 2: [1], 3: [1]}                    # per tile: the targets in list order
    union, users = scene.plan_union([[3, 1], [], [1]])                           # a view: any subset, and a target may touch nothing
    assert union == [1, 3] and users == {1: [0, 2], 3: [0]}
    assert scene.plan_union([]) == ([], {}) and scene.plan_union([[2, 2]]) == ([2], {2: [0]})
    # groups of 3 from 4 missing tiles: 3 + 1
    assert scene.group_missing(full, set(), 3) == [[0, 1, 2], [3]]
    assert scene.group_missing(full, set(), 1) == [[0], [1], [2], [3]]
    assert scene.group_missing(full, set(), 4) == scene.group_missing(full, set(), 7) == [[0, 1, 2, 3]]
    # cached tiles are skipped: a group is consecutive MISSING tiles
    assert scene.group_missing(full, {1}, 2) == [[0, 2], [3]]
    assert scene.group_missing(full, {0, 1}, 3) == [[2, 3]]
    assert scene.group_missing(full, set(full), 3) == [] and scene.group_missing([], set(), 3) == []
    assert scene.group_missing(full, set(), 0) == [[0], [1], [2], [3]]           # never a group of nothing


class _Entry:
    def __init__(self, nbytes):
        self.nbytes = nbytes


def test_cache_takes_entries_built_outside_it():
    built = []

    def build(key):
        built.append(key)
        return _Entry(10)

    cache = scene.SceneCache(25, build)
    assert cache.room() is None                                                 # no scene seen yet: its size is unknown
    for key in 'ab':
        cache.make_room()
        assert cache.put(key, _Entry(10)).nbytes == 10
    assert cache.builds == 2 and cache.nbytes == 20 and list(cache.entries) == ['a', 'b'] and built == [] and cache.room() == 0
    # the third entry: room is made BEFORE it exists (the peak stays at the budget), least recently used first
    cache.make_room()
    assert list(cache.entries) == ['b'] and cache.nbytes == 10 and cache.room() == 1
    cache.put('c', _Entry(10))
    assert cache.builds == 3 and cache.nbytes == 20 and list(cache.entries) == ['b', 'c']
    # `get` is the same rule, and counts in the same `builds`
    assert cache.get('b').nbytes == 10 and list(cache.entries) == ['c', 'b'] and cache.builds == 3
    cache.get('d')
    assert built == ['d'] and cache.builds == 4 and list(cache.entries) == ['b', 'd'] and cache.nbytes == 20
    # the entry in use is never evicted, whatever its size: a budget below one scene still works
    big = cache.put('e', _Entry(40))
    assert list(cache.entries) == ['e'] and cache.nbytes == 40 and cache.entries['e'] is big and cache.builds == 5
    tiny = scene.SceneCache(5, build)
    tiny.put('a', _Entry(10))
    tiny.make_room()
    tiny.put('b', _Entry(10))
    assert list(tiny.entries) == ['b'] and tiny.nbytes == 10 and tiny.builds == 2
    cache.clear()
    assert cache.nbytes == 0 and not cache.entries and cache.builds == 5


def test_cache_evicts_what_a_walk_still_needs_last():
    cache = scene.SceneCache(30, lambda key: _Entry(10))
    for key in (2, 3, 9):
        cache.get(key)
    cache.hold = {2, 3}                    # a walk over tiles 0 .. 3 has 2 and 3 cached and still in front of it
    cache.make_room()
    cache.put(0, _Entry(10))
    assert list(cache.entries) == [2, 3, 0]                                      # 9, not the older 2
    cache.make_room()
    cache.put(1, _Entry(10))
    assert list(cache.entries) == [2, 3, 1]                                      # 0 has been used: it goes before a held entry
    cache.hold = set()
    cache.make_room()
    assert list(cache.entries) == [3, 1]                                         # nothing on hold: plain least-recently-used
    # when only held entries are left, they go too (the walk then rebuilds them): the budget wins
    cache = scene.SceneCache(20, lambda key: _Entry(10))
    cache.get(2)
    cache.get(3)
    cache.hold = {2, 3}
    cache.make_room()
    cache.put(0, _Entry(10))
    assert list(cache.entries) == [3, 0] and cache.nbytes == 20


def _cpu_model(test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[16, 16])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=8, num_blocks=1),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    return CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=test_cfg).eval()


class _Enc:
    """An encode result on the HOST: any device work on it raises CiaoSRHipError, not the ValueError these tests expect."""
    max_scale, view_tiles, options = 2.7, None, None

    def __init__(self, tile):
        import torch
        self.x = torch.zeros(1, 3, *LR)
        self.tile = tile
        self.cache = scene.SceneCache(1 << 30, lambda key: pytest.fail('a refused target builds nothing'))


def _error(fn):
    with pytest.raises(ValueError) as err:
        fn()
    return str(err.value)


def test_records_refuse_what_the_single_calls_refuse():
    tiled = dict(tile=32, tile_overlap=8, tile_any_scale=True)
    m = scene.view_matrix((20.0, 28.0), 2.0, 30, (16, 16))
    ok = scene.Grid(scale=2)
    grids = [(tiled, dict()), (tiled, dict(size=(80, 112), scale=2)), (tiled, dict(size=(0, 5))), (tiled, dict(scale=0.001)),
             (tiled, dict(scale=2.7, window=(0, 0, 200, 10))), (tiled, dict(scale=2, window=(3, 4, 0, 5))),
             (dict(scale=2, tile=32, tile_overlap=8), dict(size=HR)), (dict(scale=2), dict(scale=2.7, window=(-1, 0, 4, 4)))]
    for cfg, kw in grids:
        model = _cpu_model(dict(cfg))
        enc = _Enc(32 if cfg.get('tile') else None)
        single = _error(lambda: model.render(enc, **kw))
        assert _error(lambda: model.render_many(enc, [ok, scene.Grid(**kw)])) == single, kw
        assert _error(lambda: model.prefetch(enc, [scene.Grid(**kw)])) == single, kw
    views = [(dict(scale=2, tile=32, tile_overlap=8), dict(matrix=m, size=(16, 16)), 'tile_any_scale'),
             (tiled, dict(matrix=m, size=(0, 16)), 'empty view grid'),
             (tiled, dict(matrix=(0.5, 0.5, 0.0, 0.5, 0.5, 0.0), size=(16, 16)), 'singular'),
             (dict(scale=2), dict(matrix=(30.0, 0.0, 0.0, 0.0, 0.5, 0.0), size=(16, 16)), 'cell'),
             (tiled, dict(matrix=m, size=(16, 16), fill=1.5), 'fill'), (tiled, dict(matrix=m, size=(16, 16), fill=(0.1, 0.2)), 'fill')]
    for cfg, kw, word in views:
        model = _cpu_model(dict(cfg))
        enc = _Enc(32 if cfg.get('tile') else None)
        single = _error(lambda: model.render_view(enc, **kw))
        assert word in single
        assert _error(lambda: model.render_many(enc, [ok, scene.View(**kw)])) == single, kw
        assert _error(lambda: model.prefetch(enc, [scene.View(**kw)])) == single, kw
    model = _cpu_model(dict(tiled))
    with pytest.raises(ValueError, match='no targets'):
        model.render_many(_Enc(32), [])
    with pytest.raises(TypeError, match='Grid'):
        model.render_many(_Enc(32), [dict(scale=2)])
    # the records keep what they are given and resolve like the single calls
    g = scene.Grid(size=HR, window=(9, 41, 61, 35))
    assert (g.size, g.scale, g.window) == (HR, None, (9, 41, 61, 35)) and g.resolve(*LR) == (108, 151, (9, 41, 61, 35))
    assert scene.Grid(scale=2.7).resolve(*LR) == (108, 151, (0, 0, 108, 151))
    v = scene.View(m, (16, 16))
    got_m, size, fill, frames = v.resolve(*LR, 32, 8, True)
    assert got_m == tuple(m) and size == (16, 16) and fill == (0.0, 0.0, 0.0) and len(frames) == 4
    assert scene.View(m, (16, 16), fill=(0.25, 0.5, 1)).resolve(*LR)[2:] == ((0.25, 0.5, 1.0), [(0, 0, *LR)])


def test_many_view_exports_are_declared():
    import ctypes as C
    from ciaosr_amd import _lib
    lib = _lib.load()
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    sig = _lib.SIGNATURES
    assert sig['ciaosr_view_count_many_max_views'] == (C.c_int, [])
    assert sig['ciaosr_view_many_workspace_bytes'][0] is C.c_size_t and sig['ciaosr_view_many_workspace_bytes'][1][0] is I
    assert sig['ciaosr_view_many_workspace_offset'][0] is C.c_size_t and len(sig['ciaosr_view_many_workspace_offset'][1]) == 4
    assert sig['ciaosr_view_count_many_i32'][1][:2] == [D, I] and len(sig['ciaosr_view_count_many_i32'][1]) == 9
    # the workspace is the views' single-view part arrays at 256-byte-aligned offsets (host arithmetic: no GPU needed)
    assert lib.ciaosr_view_count_many_max_views() >= 2
    chunk = lib.ciaosr_view_block_queries()
    sizes = [(61, 83), (1, 1), (3, 700), (2 * chunk, 1)]
    arr = (C.c_int * 8)(*[v for s in sizes for v in s])
    off = 0
    for v, (hv, wv) in enumerate(sizes):
        assert lib.ciaosr_view_many_workspace_offset(arr, 4, 4, v) == off and off % 256 == 0
        one = lib.ciaosr_view_workspace_bytes(hv, wv, 4)
        assert one == 4 * 4 * -(-hv * wv // chunk)
        off += -(-one // 256) * 256
    assert lib.ciaosr_view_many_workspace_bytes(arr, 4, 4) == off
    assert lib.ciaosr_view_many_workspace_bytes(arr, 0, 4) == 0 and lib.ciaosr_view_many_workspace_bytes(arr, 4, 0) == 0
    bad = (C.c_int * 4)(61, 83, 0, 5)
    assert lib.ciaosr_view_many_workspace_bytes(bad, 2, 4) == 0
