"""`test_cfg.view_blocks` on the GPU: ciaosr_view_count_blocks_i32 / _many / ciaosr_view_select_blocks_f32 against the definition in
numpy float64 (tests/view_blocks_reference.py), the flag of the chained 16-bit head kernel on a grid, a block list and an index-order
list, and CiaoSR.render_view / render_many with the option on against a composition from full-grid queries.  Every comparison is
bitwise."""
import numpy as np
import pytest
import torch

from tests import view_blocks_reference as br
from tests.helpers import SQRT6, randn

pytestmark = pytest.mark.gpu

TILED = dict(tile=br.TILE, tile_overlap=br.OVERLAP, tile_any_scale=True)
HV, WV = br.SIZE


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_models = {}


def _model(dev):
    """A random-init RDN restorer with the real head widths (C = 64, 256-wide MLPs: what the chained kernel needs), as
    tests/test_render_many_gpu.py builds it; test_cfg is set per test."""
    if 'rdn' not in _models:
        from ciaosr_amd.init_utils import seeded_init_
        from tests.test_hip_parity import _restorer
        model = _restorer('rdn', 4, dev, dict(), blocks=3, layers=4)
        seeded_init_(model, seed=17, gain=1.2, head_gain=SQRT6)
        _models['rdn'] = model.to(dev)
    return _models['rdn']


def _lq(h, w, dev, seed=5):
    return (randn((1, 3, h, w), seed) * 0.2 + 0.45).clamp(0, 1).to(dev)


def _matrix():
    from ciaosr_amd import scene
    return scene.view_matrix(*br.ARGS, br.SIZE)


def _frames(tiled):
    from ciaosr_amd import scene
    return scene.plan_view(*br.TILED_LR, br.TILE, br.OVERLAP, any_scale=True) if tiled else [(0, 0, *br.ONE_LR)]


def _tiles(frames, dev):
    return torch.tensor(frames, dtype=torch.int32).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np_bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


_refs = {}


def _ref(m, hv, wv, frames):
    """The numpy block lists of a view, made once per input."""
    key = (tuple(m), hv, wv, tuple(frames))
    if key not in _refs:
        _refs[key] = [br.block_list(m, hv, wv, f) for f in frames]
    return _refs[key]


def _check_blocks_against_numpy(m, hv, wv, frames, dev):
    from ciaosr_amd import hip_ops
    tiles = _tiles(frames, dev)
    want = _ref(m, hv, wv, frames)
    counts, ws = hip_ops.view_count_blocks(m, hv, wv, tiles)
    assert counts.shape == (len(frames), 2) and counts.dtype == torch.int32
    counts = counts.tolist()
    assert counts == [[b['members'], b['blocks']] for b in want], counts
    plain, ws_plain = hip_ops.view_count(m, hv, wv, tiles)
    assert plain.tolist() == [c[0] for c in counts]
    out = []
    for k, (frame, b) in enumerate(zip(frames, want)):
        if b['blocks'] == 0:
            continue
        q_index, coord, cell = hip_ops.view_select_blocks(m, hv, wv, frame, k, len(frames), ws, b['blocks'])
        assert q_index.shape == (8 * b['blocks'],) and coord.shape == cell.shape == (8 * b['blocks'], 2)
        assert np.array_equal(q_index.cpu().numpy(), b['q_index']), frame
        assert np.array_equal(_np_bits(coord), b['coord'].view(np.int32)), frame
        assert np.array_equal(_np_bits(cell), b['cell'].view(np.int32)), frame
        assert hip_ops.grid_width_of(coord) == 0                                 # a list, not a grid: eight entries are one row tile
        # member entries: the coordinates and cells view_select writes for the same q
        qi, ci, li = hip_ops.view_select(m, hv, wv, frame, k, len(frames), ws_plain, b['members'])
        member = q_index >= 0
        order = torch.argsort(q_index[member])
        assert torch.equal(q_index[member][order], qi)
        assert torch.equal(_bits(coord[member][order]), _bits(ci)) and torch.equal(_bits(cell[member][order]), _bits(li))
        out += [q_index, coord, cell]
    return counts, out


@pytest.mark.parametrize('tiled', [False, True])
def test_count_and_select_blocks_against_the_definition(dev, tiled):
    from ciaosr_amd import _lib
    m, frames = _matrix(), _frames(tiled)
    assert -(-HV // 2) * -(-WV // 4) > _lib.load().ciaosr_view_block_blocks()    # more than one workgroup, the last one ragged
    a = _check_blocks_against_numpy(m, HV, WV, frames, dev)
    b = _check_blocks_against_numpy(m, HV, WV, frames, dev)
    assert a[0] == b[0] and all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a[1], b[1]))         # repeatable
    assert all(0 < n < HV * WV and 8 * nb > n for n, nb in a[0])


def test_blocks_of_small_and_wide_grids(dev):
    from ciaosr_amd import hip_ops, scene
    frames = _frames(True)
    # one query in the two upper tiles: a list of 8 for a grid of 1, blended with seven pads
    m1 = scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1))
    counts, out = _check_blocks_against_numpy(m1, 1, 1, frames, dev)
    assert counts == [[1, 1], [1, 1], [0, 0], [0, 0]]
    E, Wt = torch.zeros(3, 1, device=dev), torch.zeros(1, device=dev)
    rgb = randn((8, 3), 3).to(dev)
    hip_ops.view_blend(E, Wt, out[0], rgb)                                        # n = 8 > Q = 1
    assert torch.equal(E, rgb[:1].t()) and Wt.tolist() == [1.0]
    # three very wide rows: two rows of blocks over several workgroups, members of all four tiles, the lower block row half outside
    wide = 2100
    m = scene.view_matrix((20.0, 28.0), 33.0, 7, (3, wide))
    counts, _ = _check_blocks_against_numpy(m, 3, wide, frames, dev)
    assert 2 * -(-wide // 4) > 4 * 256 and all(n > 0 for n, _ in counts) and max(n for n, _ in counts) < 3 * wide


def test_count_blocks_many_is_the_single_count(dev):
    from ciaosr_amd import _lib, hip_ops, scene
    lib = _lib.load()
    frames = _frames(True)
    tiles = _tiles(frames, dev)
    views = [(_matrix(), br.SIZE), (scene.view_matrix((5.0, 30.0), 2.7, -32, (1, 1)), (1, 1)),
             (scene.view_matrix((20.0, 28.0), 33.0, 7, (3, 2100)), (3, 2100))]
    n_max = lib.ciaosr_view_count_many_max_views()
    for k in range(n_max):                                                        # tiny views: the list crosses a launch group
        size = (2 + k % 3, 3 + k % 5)
        views.append((scene.view_matrix((4.0 + 0.9 * k, 50.0 - 1.3 * k), 1.7 + 0.05 * k, 11 * k, size), size))
    ms, sizes = [v[0] for v in views], [v[1] for v in views]
    counts, ws, offsets = hip_ops.view_count_blocks_many(ms, sizes, tiles)
    assert counts.shape == (len(views), len(frames), 2)
    counts = counts.tolist()
    assert counts[0] == [[b['members'], b['blocks']] for b in _ref(ms[0], HV, WV, frames)]
    assert sum(1 for c in counts[3:] if any(n for n, _ in c)) > n_max // 2
    for v, ((m, (hv, wv)), off) in enumerate(zip(views, offsets)):
        one, ws1 = hip_ops.view_count_blocks(m, hv, wv, tiles)
        assert one.tolist() == counts[v], v
        nbytes = lib.ciaosr_view_blocks_workspace_bytes(hv, wv, len(frames))
        assert off % 256 == 0 and torch.equal(ws[off:off + nbytes], ws1[:nbytes]), v
        for k, (n, nb) in enumerate(counts[v]):
            if v < 3 and nb:
                got = hip_ops.view_select_blocks(m, hv, wv, frames[k], k, len(frames), ws[off:], nb)
                ref = hip_ops.view_select_blocks(m, hv, wv, frames[k], k, len(frames), ws1, nb)
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, ref)), (v, k)


def _one_frame_lists(dev):
    """The three query lists of the head tests on the one-frame input: the whole grid, the block list, the index-order list."""
    from ciaosr_amd import hip_ops
    m = _matrix()
    frame = (0, 0, *br.ONE_LR)
    tiles = _tiles([frame], dev)
    counts, ws = hip_ops.view_count_blocks(m, HV, WV, tiles)
    n, nb = counts.tolist()[0]
    blk = hip_ops.view_select_blocks(m, HV, WV, frame, 0, 1, ws, nb)
    _, ws_plain = hip_ops.view_count(m, HV, WV, tiles)
    idx = hip_ops.view_select(m, HV, WV, frame, 0, 1, ws_plain, n)
    return m, frame, n, blk, idx


@pytest.mark.parametrize('precision', ['f16', 'bf16'])
def test_chain_flag_on_grid_blocks_and_index_order(dev, precision):
    """(a) the grid-walked view: flag 0; (b) the block list: flag 0, and at its members bit for bit the rows of (a); (c) the index-order
    list of the same members: flag 1 -- the chained kernel gives the launch up to the gated 128-row kernel."""
    from ciaosr_amd import hip_ops, scene
    model = _model(dev)
    model.test_cfg = dict(precision=precision)
    gen = model.generator
    m, frame, n, (qb, cb, lb), (qi, ci, li) = _one_frame_lists(dev)
    assert scene.view_blocks_fit(m) and 0 < n < HV * WV
    enc = model.encode(_lq(*br.ONE_LR, dev), max_scale=scene.view_max_scale(m))
    feats = enc.cache.get((0, None))
    assert feats.scenes[0].chained
    coord, cell = hip_ops.make_coord_cell_view(m, HV, WV, frame, dev)
    assert hip_ops.grid_width_of(coord) == WV
    rgb_a, flag_a = gen.render(feats, coord, cell, return_flags=True)
    rgb_b, flag_b = gen.render(feats, cb, lb, return_flags=True)
    rgb_c, flag_c = gen.render(feats, ci, li, return_flags=True)
    assert flag_a.dtype == torch.int32 and flag_a.shape == (1,) and flag_a.is_cuda
    flags = (flag_a.item(), flag_b.item(), flag_c.item())
    print(f'{precision}: flags grid / blocks / index order = {flags}')
    assert flags == (0, 0, 1), flags
    member = qb >= 0
    assert int(member.sum()) == n
    assert torch.equal(_bits(rgb_b[0][member]), _bits(rgb_a[0][qb[member].long()]))
    assert torch.equal(gen.render(feats, cb, lb), rgb_b)                          # the flag is read, nothing else changes


def test_fp32_blocks_equal_index_order_and_have_no_flag(dev):
    from ciaosr_amd import scene
    from ciaosr_amd._lib import CiaoSRHipError
    model = _model(dev)
    model.test_cfg = dict(precision='fp32')
    gen = model.generator
    m, frame, n, (qb, cb, lb), (qi, ci, li) = _one_frame_lists(dev)
    enc = model.encode(_lq(*br.ONE_LR, dev), max_scale=scene.view_max_scale(m))
    feats = enc.cache.get((0, None))
    assert not feats.scenes[0].chained
    rgb_b, rgb_c = gen.render(feats, cb, lb)[0], gen.render(feats, ci, li)[0]
    member = qb >= 0
    order = torch.argsort(qb[member])
    assert torch.equal(qb[member][order], qi)
    assert torch.equal(_bits(rgb_b[member][order]), _bits(rgb_c))
    with pytest.raises(CiaoSRHipError, match='unsupported'):
        gen.render(feats, cb, lb, return_flags=True)


def _composition(model, enc, m, frames, tiled, dev):
    """Per tile in row-major order the full-grid query in the tile's frame, its members picked with the index list, blended and
    finalised with the existing calls."""
    from ciaosr_amd import hip_ops
    n_q = HV * WV
    tiles = _tiles(frames, dev)
    counts, ws = hip_ops.view_count(m, HV, WV, tiles)
    E, Wt = torch.zeros(3, n_q, device=dev), torch.zeros(n_q, device=dev)
    for k, (frame, n) in enumerate(zip(frames, counts.tolist())):
        if n == 0:
            continue
        feats = enc.cache.get((0, (frame[0], frame[1]) if tiled else None))
        q_index, _, _ = hip_ops.view_select(m, HV, WV, frame, k, len(frames), ws, n)
        coord, cell = hip_ops.make_coord_cell_view(m, HV, WV, frame, dev)
        full = model.generator.render(feats, coord, cell)[0]
        hip_ops.view_blend(E, Wt, q_index, full[q_index.long()].contiguous())
    pred = hip_ops.view_finalize(E, Wt, (0.0,) * 3, model.rgb_mean, model.rgb_std)
    return hip_ops.denorm_clamp(pred, HV, WV, model.rgb_mean, model.rgb_std).unsqueeze(0)


@pytest.mark.parametrize('tiled', [False, True])
def test_f16_view_blocks_end_to_end(dev, tiled):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.scene import View
    model = _model(dev)
    cfg = dict(TILED if tiled else {}, precision='f16')
    m, frames = _matrix(), _frames(tiled)
    lq = _lq(*(br.TILED_LR if tiled else br.ONE_LR), dev)
    model.test_cfg = dict(cfg, view_blocks=True)
    enc = model.encode(lq)
    with hip_ops.profile():
        got = model.render_view(enc, m, br.SIZE)
    prof = hip_ops.profile.results()
    partial = sum(1 for b in _ref(m, HV, WV, frames) if b['members'])
    assert partial == len(frames)
    assert prof['view_count_blocks']['launches'] == 1 and prof['view_select_blocks']['launches'] == partial
    assert 'view_count' not in prof and 'view_select' not in prof
    many = model.render_many(enc, [View(m, br.SIZE)])
    assert len(many) == 1 and torch.equal(_bits(many[0]), _bits(got))
    fresh = model.encode(lq)
    assert torch.equal(_bits(model.render_many(fresh, [View(m, br.SIZE)])[0]), _bits(got))
    model.test_cfg = dict(cfg)                                                    # the composition runs with the option off
    want = _composition(model, enc, m, frames, tiled, dev)
    assert got.shape == want.shape == (1, 3, HV, WV)
    assert torch.equal(_bits(got), _bits(want)), (got - want).abs().max().item()
    assert (got.view(3, -1).sum(0) == 0).any() and (got.view(3, -1).sum(0) != 0).any()       # the border cuts the view: fill and picture
    # a view under the bound's other side keeps the index-order list
    from ciaosr_amd import scene
    m_low = scene.view_matrix(br.ARGS[0], 1.0, 30, br.SIZE)               # 3 sin 30 + cos 30 = 2.37 > 2
    assert not scene.view_blocks_fit(m_low)
    model.test_cfg = dict(cfg, view_blocks=True)
    with hip_ops.profile():
        model.render_view(model.encode(lq, max_scale=3.3), m_low, br.SIZE)
    prof = hip_ops.profile.results()
    assert 'view_count_blocks' not in prof and 'view_select_blocks' not in prof and prof['view_count']['launches'] == 1


@pytest.mark.parametrize('tiled', [False, True])
def test_fp32_view_blocks_is_inert(dev, tiled):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.scene import View
    model = _model(dev)
    cfg = dict(TILED if tiled else {}, precision='fp32')
    m = _matrix()
    lq = _lq(*(br.TILED_LR if tiled else br.ONE_LR), dev)
    outs, tags = [], []
    for on in (False, True):
        model.test_cfg = dict(cfg, view_blocks=on)
        with hip_ops.profile():
            enc = model.encode(lq)
            a = model.render_view(enc, m, br.SIZE)
            b = model.render_many(model.encode(lq), [View(m, br.SIZE)])[0]
        prof = hip_ops.profile.results()
        outs.append((a, b))
        tags.append({k: r['launches'] for k, r in prof.items()})
    assert tags[0] == tags[1] and not any('blocks' in k for k in tags[1]), (tags[0], tags[1])
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert torch.equal(_bits(outs[1][0]), _bits(outs[1][1]))


def test_route_bits_that_disable_the_chain_keep_the_index_order(dev):
    """Decided from the route code, not from the precision's name: f16 under head_route's no-chain bit selects in index order."""
    from ciaosr_amd import hip_ops
    model = _model(dev)
    m = _matrix()
    lq = _lq(*br.TILED_LR, dev)
    model.test_cfg = dict(TILED, precision='f16', view_blocks=True)
    opts = hip_ops.Options('f16', head_route=32)                                  # CIAOSR_HEAD_NO_CHAIN (include/ciaosr_hip.h)
    enc = model.encode(lq, options=opts)
    with hip_ops.profile():
        model.render_view(enc, m, br.SIZE)
    prof = hip_ops.profile.results()
    assert 'view_select_blocks' not in prof and prof['view_select']['launches'] == 4
    assert not enc.cache.get((0, (0, 0))).scenes[0].chained


def test_render_many_mixes_block_and_index_order_views(dev):
    """Views that fit the bound and one that does not, in one render_many on the tiled image: one count per kind, one copy of the
    counts to the host, every output bitwise its own render_view."""
    from ciaosr_amd import hip_ops, scene
    from ciaosr_amd.scene import Grid, View
    model = _model(dev)
    model.test_cfg = dict(TILED, precision='f16', view_blocks=True)
    lq = _lq(*br.TILED_LR, dev)
    m = _matrix()
    m_low = scene.view_matrix(br.ARGS[0], 1.0, 30, (21, 30))
    m_pan = scene.view_matrix((22.5, 30.25), 3.3, -75, (31, 27))
    assert scene.view_blocks_fit(m) and scene.view_blocks_fit(m_pan) and not scene.view_blocks_fit(m_low)
    targets = [View(m_low, (21, 30), fill=0.5), View(m, br.SIZE), Grid(size=(66, 92), window=(20, 30, 33, 41)), View(m_pan, (31, 27))]
    wants = []
    for t in targets:
        enc = model.encode(lq, max_scale=3.3)
        wants.append(model.render(enc, size=t.size, window=t.window) if isinstance(t, Grid) else model.render_view(enc, t.matrix, t.size, t.fill))
    enc = model.encode(lq, max_scale=3.3)
    copies = []
    tolist = torch.Tensor.tolist

    def counting(t):
        copies.append(tuple(t.shape))
        return tolist(t)

    torch.Tensor.tolist = counting
    try:
        with hip_ops.profile():
            outs = model.render_many(enc, targets)
    finally:
        torch.Tensor.tolist = tolist
    prof = hip_ops.profile.results()
    assert prof['view_count_many']['launches'] == 1 and prof['view_count_blocks_many']['launches'] == 1
    assert prof['view_select_blocks']['launches'] > 0 and prof['view_select']['launches'] > 0
    assert copies == [(4 + 2 * 2 * 4,)], copies                                   # counts of one plain view + (members, blocks) of two
    assert len(outs) == len(wants) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, wants))
