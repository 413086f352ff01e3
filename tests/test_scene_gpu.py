"""The persistent head scene through the C ABI: prepare + query against ciaosr_head_forward_* (bitwise: the same kernels on the same
operands, and the head kernels are row-independent), windows and repeated renders from one scene, the window-coordinate kernel against
the host's make_coord / tile_plan.axis_local, and the refusals."""
import ctypes as C

import pytest
import torch

from tests.helpers import randn, seeded_head
from tests.test_hip_parity import _my_generator

pytestmark = pytest.mark.gpu

S = 2.7                     # odd target sizes
WINDOW = (5, 11, 37, 53)    # 1961 queries: a multiple of none of 8, 32, 128 (the kernels' row tiles)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_cache = {}


def _head(dev, C_, H, W, hidden=(256,) * 4, non_local=True, **kw):
    """(generator, feature [C,H,W], normalised LR [3,H,W]) of one seeded case, built once per module."""
    key = (C_, H, W, tuple(hidden), non_local, tuple(sorted(kw.items())))
    if key not in _cache:
        g = _my_generator(C_, hidden, seeded_head(C_, 3, hidden=hidden, head_gain=2.0, non_local=non_local), dev, eval_bsize=30000,
                          non_local_attn=non_local, **kw)
        _cache[key] = (g, randn((C_, H, W), 11).to(dev), randn((3, H, W), 12).to(dev) * 0.25)
    return _cache[key]


def _grid(H, W, s, dev):
    from ciaosr_amd import hip_ops
    ht, wt = round(H * s), round(W * s)
    return (ht, wt) + hip_ops.make_coord_cell(ht, wt, dev)


def _field(code, lo, bits):
    return (code >> lo) & ((1 << bits) - 1)


CASES = [(64, 24, 20, 'fp32'), (64, 24, 20, 'f16'),
         (64, 24, 24, 'fp32'), (64, 24, 24, 'f16'), (64, 24, 24, 'bf16'), (64, 24, 24, 'f16x3'),
         (64, 65, 64, 'fp32'), (64, 65, 64, 'f16'), (180, 16, 16, 'fp32'), (180, 16, 16, 'f16')]


@pytest.mark.parametrize('C_,H,W,precision', CASES)
def test_prepare_then_query_is_head_forward(dev, C_, H, W, precision):
    from ciaosr_amd import hip_ops
    g, feat, x = _head(dev, C_, H, W)
    opt = hip_ops.Options(precision)
    ht, wt, coord, cell = _grid(H, W, S, dev)
    Q = ht * wt
    code = g._head.route_code(H, W, Q, opt)
    if precision == 'fp32':         # the shapes are chosen for these routes: the fused kernels, and per map
        assert code & 1 == 1
        tables, logit = _field(code, 1, 2), _field(code, 3, 3)
        assert (tables, logit) == {(64, 24, 20): (1, 1),       # small layer-0 tables, GEMM logit table (HW < 512)
                                   (64, 24, 24): (1, 4),       # Winograd F(4x4) logit table
                                   (64, 65, 64): (2, 4),       # GEMM layer-0 tables (HW > 4096)
                                   (180, 16, 16): (tables, 1)}[(C_, H, W)], (tables, logit)
    want = g._head.forward(feat, x, coord, cell, 30000, options=opt)
    scene = g._head.prepare(feat, opt, Q)
    assert scene.desc.route == code and scene.desc.q_plan == Q and (scene.desc.H, scene.desc.W) == (H, W)
    assert scene.nbytes == scene.desc.total * 256 or scene.nbytes >= scene.desc.total * 256
    hip_ops.poison_workspaces()             # what the query reads from scratch instead of the scene is NaN now
    got = g._head.query(scene, x, coord, cell, 30000)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_staged_route_and_no_non_local_maps(dev):
    from ciaosr_amd import hip_ops
    for (C_, H, W, kw) in ((8, 10, 12, dict(hidden=(64, 32), local_size=3)), (64, 24, 20, dict(non_local=False))):
        g, feat, x = _head(dev, C_, H, W, **kw)
        ht, wt, coord, cell = _grid(H, W, S, dev)
        code = g._head.route_code(H, W, ht * wt)
        assert code & 1 == (0 if 'hidden' in kw else 1)
        want = g._head.forward(feat, x, coord, cell, 30000)
        scene = g._head.prepare(feat, None, ht * wt)
        assert scene.desc.Cn == (0 if kw.get('non_local') is False else C_)
        hip_ops.poison_workspaces()
        got = g._head.query(scene, x, coord, cell, 30000)
        assert torch.isfinite(want).all() and torch.equal(got, want)


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_window_alone_is_the_rows_of_the_full_render(dev, precision):
    from ciaosr_amd import hip_ops
    H = W = 24
    g, feat, x = _head(dev, 64, H, W)
    opt = hip_ops.Options(precision)
    ht, wt, coord, cell = _grid(H, W, S, dev)
    i0, j0, wh, ww = WINDOW
    assert wh * ww == 1961 and all(1961 % n for n in (8, 32, 128)) and i0 + wh <= ht and j0 + ww <= wt
    scene = g._head.prepare(feat, opt, ht * wt)
    full = g._head.query(scene, x, coord, cell, 30000)
    assert torch.equal(full, g._head.forward(feat, x, coord, cell, 30000, options=opt))
    wc, wl = hip_ops.make_coord_cell_window(ht, wt, i0, i0 + wh, j0, j0 + ww, dev)
    assert hip_ops.grid_width_of(wc) == ww
    hip_ops.poison_workspaces()
    part = g._head.query(scene, x, wc, wl, 30000)
    assert torch.equal(part, full.view(ht, wt, 3)[i0:i0 + wh, j0:j0 + ww].reshape(-1, 3))
    one = g._head.query(scene, x, wc[777:778].contiguous(), wl[777:778].contiguous(), 30000)      # Q = 1
    assert torch.equal(one, part[777:778])


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_renders_at_several_scales_from_one_scene(dev, precision):
    from ciaosr_amd import hip_ops
    H = W = 24
    g, feat, x = _head(dev, 64, H, W)
    opt = hip_ops.Options(precision)
    lo, hi = _grid(H, W, 2.7, dev), _grid(H, W, 3.3, dev)
    scene = g._head.prepare(feat, opt, hi[0] * hi[1])
    hip_ops.poison_workspaces()
    first = g._head.query(scene, x, lo[2], lo[3], 30000)
    second = g._head.query(scene, x, hi[2], hi[3], 30000)
    third = g._head.query(scene, x, lo[2], lo[3], 30000)
    assert torch.equal(first, third)
    assert torch.equal(second, g._head.forward(feat, x, hi[2], hi[3], 30000, options=opt))
    # both grids are on the same side of the logit-table threshold (and of u16_fits): one route, so the x2.7 render is head_forward's too
    assert g._head.route_code(H, W, lo[0] * lo[1], opt) == g._head.route_code(H, W, hi[0] * hi[1], opt) == scene.desc.route
    assert torch.equal(first, g._head.forward(feat, x, lo[2], lo[3], 30000, options=opt))


# ---- the window-coordinate kernel --------------------------------------------------------------------------------------------------------
def _spans(s0, s1):
    """Windows at both ends and in the middle of [s0, s1)."""
    m = (s0 + s1) // 2
    return sorted({(s0, min(s0 + 3, s1)), (max(s1 - 3, s0), s1), (m, min(m + 2, s1))})


@pytest.mark.parametrize('ny,nx', [(1, 7), (7, 158), (158, 4097), (4097, 1)])
def test_window_kernel_global_frame_is_make_coord(dev, ny, nx):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.coords import make_cell, make_coord
    grid = make_coord((ny, nx), flatten=False)
    cell = make_cell((ny, nx)).view(ny, nx, 2)
    for (i0, i1) in _spans(0, ny):
        for (j0, j1) in _spans(0, nx):
            c, l = hip_ops.make_coord_cell_window(ny, nx, i0, i1, j0, j1, dev)
            assert torch.equal(c.cpu(), grid[i0:i1, j0:j1].reshape(-1, 2)), (i0, i1, j0, j1)
            assert torch.equal(l.cpu(), cell[i0:i1, j0:j1].reshape(-1, 2))
    full_c, full_l = hip_ops.make_coord_cell(ny, nx, dev)                  # and the device's own full grid
    c, l = hip_ops.make_coord_cell_window(ny, nx, 0, ny, 0, nx, dev)
    assert torch.equal(c, full_c) and torch.equal(l, full_l)


@pytest.mark.parametrize('frame', [(40, 8, 32), (40, 0, 40), (40, 0, 32)])
@pytest.mark.parametrize('ny,nx', [(1, 7), (7, 158), (158, 4097), (4097, 1)])
def test_window_kernel_in_a_tile_frame_is_axis_local(dev, ny, nx, frame):
    from ciaosr_amd import hip_ops, tile_plan
    n_lr, y0, th = frame
    si0, si1, cy, celly = tile_plan.axis_local(y0, th, n_lr, ny)
    sj0, sj1, cx, cellx = tile_plan.axis_local(y0, th, n_lr, nx)
    assert si0 < si1 and sj0 < sj1
    for (i0, i1) in _spans(si0, si1):
        for (j0, j1) in _spans(sj0, sj1):
            c, l = hip_ops.make_coord_cell_window(ny, nx, i0, i1, j0, j1, dev, frame=frame + frame)
            want = torch.stack(torch.meshgrid(cy[i0 - si0:i1 - si0], cx[j0 - sj0:j1 - sj0], indexing='ij'), dim=-1).view(-1, 2)
            assert torch.equal(c.cpu(), want), (i0, i1, j0, j1, (c.cpu() - want).abs().max().item())
            wl = torch.empty_like(want)
            wl[:, 0], wl[:, 1] = float(celly), float(cellx)
            assert torch.equal(l.cpu(), wl)


def test_window_kernel_refuses_bad_windows(dev):
    from ciaosr_amd import hip_ops
    for args in ((7, 7, 3, 3, 0, 7), (7, 7, 0, 8, 0, 7), (7, 7, 0, 7, -1, 3)):
        with pytest.raises(ValueError):
            hip_ops.make_coord_cell_window(*args, dev)


# ---- refusals: argument checks, nothing launched -----------------------------------------------------------------------------------------
def test_query_refuses_a_descriptor_that_does_not_fit(dev):
    from ciaosr_amd import _lib, hip_ops
    from ciaosr_amd._lib import CiaoSRHipError
    H = W = 24
    g, feat, x = _head(dev, 64, H, W)
    ht, wt, coord, cell = _grid(H, W, S, dev)
    Q = ht * wt
    scene = g._head.prepare(feat, 'fp32', Q)
    lib = _lib.load()
    rgb = torch.full((Q, 3), 7.0, device=dev)
    ws = hip_ops.workspace(lib.ciaosr_head_workspace_bytes(H, W, C.byref(g._head.struct()), Q), dev)

    def run(entry, st, desc, scene_bytes, opt=None):
        return getattr(lib, entry)(hip_ops.ptr(scene.buf), scene_bytes, C.byref(desc), C.byref(st), hip_ops.ptr(x), hip_ops.ptr(coord),
                                   hip_ops.ptr(cell), Q, 30000, hip_ops.ptr(rgb), opt, hip_ops.ptr(ws), ws.numel(), hip_ops.stream_ptr())

    st32, st16 = g._head.struct(), g._head.struct('f16')
    assert run('ciaosr_head_query_f16', st16, scene.desc, scene.nbytes) == -1              # another precision
    other = _lib.HeadSceneT.from_buffer_copy(scene.desc)
    other.H = 25
    assert run('ciaosr_head_query_f32', st32, other, scene.nbytes) == -1                   # other dims
    assert run('ciaosr_head_query_f32', st32, scene.desc, scene.desc.total * 256 - 1) == -4    # a short buffer
    no_table = _lib.OptionsT()
    no_table.head_route = _lib.HEAD_NO_LOGIT_TABLE
    assert run('ciaosr_head_query_f32', st32, scene.desc, scene.nbytes, C.byref(no_table)) == -1   # a route-changing option bit
    torch.cuda.synchronize()
    assert bool((rgb == 7.0).all())                                                        # nothing ran
    assert run('ciaosr_head_query_f32', st32, scene.desc, scene.nbytes) == 0
    assert torch.equal(rgb, g._head.forward(feat, x, coord, cell, 30000))
    # a weight changed in place after prepare: the scene is stale
    g2 = _my_generator(64, (256,) * 4, seeded_head(64, 3, head_gain=2.0), dev, eval_bsize=30000)
    for param in (g2.imnet_v.layers[0].weight, g2.cs_attn.conv_assembly[0].weight):
        stale = g2._head.prepare(feat, 'fp32', Q)
        g2._head.query(stale, x, coord[:64].contiguous(), cell[:64].contiguous(), 30000)
        with torch.no_grad():
            param.mul_(1.0)
        with pytest.raises(CiaoSRHipError):
            g2._head.query(stale, x, coord[:64].contiguous(), cell[:64].contiguous(), 30000)
