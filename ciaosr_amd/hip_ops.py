"""Tensor-level wrappers over the C ABI: device pointers from `tensor.data_ptr()`, the stream
from `torch.cuda.current_stream()`.  PyTorch is used for device memory and streams only."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._lib import CiaoSRHipError

_workspaces = {}


def require_gpu(*tensors, allow_row_stride=False):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.is_cuda:
            # every launch goes to torch's current stream of the CURRENT device: a tensor living on another GPU would be
            # dereferenced from the wrong device (run the call under `torch.cuda.device(t.device)`)
            if dev is None:
                dev = torch.cuda.current_device()
            if t.device.index != dev:
                raise CiaoSRHipError(f'tensor on cuda:{t.device.index} but the current device is cuda:{dev}: '
                                     f'run the call under torch.cuda.device({t.device.index})')
        if not t.is_cuda:
            raise CiaoSRHipError('the LocalImplicitSR path runs on the MI355X only: got a CPU tensor '
                                 '(no CPU fallback; move the model and inputs to cuda)')
        if t.dtype not in (torch.float32, torch.int32):
            raise CiaoSRHipError(f'expected float32/int32 tensor, got {t.dtype}')
        if not t.is_contiguous() and not (allow_row_stride and t.dim() == 2 and t.stride(1) == 1):
            raise CiaoSRHipError('expected a contiguous tensor')


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on `device` (default: the current device, looked up per call so that a
    process driving several GPUs launches on the right one; the index is passed explicitly because the implicit
    lookup inside current_stream() costs ~0.2 ms per call on hosts with many cores)."""
    idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
    return C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


_coord_cache = {}


def make_coord_cell(ht, wt, device):
    """Device-side make_coord/make_cell of an ht x wt target grid, cached per shape."""
    key = (ht, wt, device.type, device.index)
    hit = _coord_cache.get(key)
    if hit is None:
        coord = torch.empty(ht * wt, 2, dtype=torch.float32, device=device)
        cell = torch.empty(ht * wt, 2, dtype=torch.float32, device=device)
        _lib.call('ciaosr_make_coord_cell_f32', ptr(coord), ptr(cell), ht, wt, stream_ptr())
        if len(_coord_cache) > 16:
            _coord_cache.clear()
            _grid_width.clear()
        hit = _coord_cache[key] = (coord, cell)
        _grid_width[(coord.data_ptr(), ht * wt)] = wt
    return hit


_grid_width = {}


_window_width = {}


def make_coord_cell_window(ht, wt, i0, i1, j0, j1, device, frame=None):
    """Rows [i0, i1) x columns [j0, j1) of the ht x wt target grid, made on the device: (coord, cell), each [(i1-i0)*(j1-j0), 2].
    frame = None: the `make_coord_cell` values at those rows and columns.  frame = (n_lr_y, y0, th, n_lr_x, x0, tw): the grid in the
    frame of that LR tile (tile_plan.axis_local's values).  Not cached -- windows do not repeat the way tile shapes do -- but the
    window's width is registered for `grid_width_of`."""
    n = (i1 - i0) * (j1 - j0)
    if not (0 <= i0 < i1 <= ht and 0 <= j0 < j1 <= wt):
        raise ValueError(f'window rows [{i0}, {i1}) x columns [{j0}, {j1}) outside the {ht} x {wt} grid (or empty)')
    coord = torch.empty(n, 2, dtype=torch.float32, device=device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=device)
    fr = (C.c_int * 6)(*[int(v) for v in frame]) if frame is not None else None
    _lib.call('ciaosr_make_coord_cell_window_f32', ptr(coord), ptr(cell), ht, wt, i0, i1, j0, j1, fr, stream_ptr())
    if len(_window_width) > 64:
        _window_width.clear()
    _window_width[(coord.data_ptr(), n)] = j1 - j0
    return coord, cell


def grid_width_of(coord):
    """Columns of the row-major target grid when `coord` [Q, 2] is (a view of) a tensor `make_coord_cell` or `make_coord_cell_window`
    produced, else 0: the traversal hint ciaosr_options_t.query_grid_w of the 16-bit fused head (results do not depend on it)."""
    key = (coord.data_ptr(), coord.shape[0])
    return _grid_width.get(key, 0) or _window_width.get(key, 0)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def workspace(nbytes, device, slot='head', exact=False):
    """Grow-only scratch buffer per (slot, device, stream): two streams or two devices never share scratch.  `exact`: grow to nbytes
    and no further (a caller that bounds its scratch on purpose: cs_attn under Options.csa_block_mb), else with 5 % of headroom."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (slot, device.type, idx, torch.cuda.current_stream(idx).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _workspaces[key] = None
        buf = torch.empty(int(nbytes) if exact else int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def take_workspaces(stream):
    """Remove and return the scratch buffers that were grown on `stream` (a torch.cuda.Stream): the caller becomes their owner
    (graphed_restore hands them to the captured graph's closure), and a later stream that happens to get the same raw handle
    starts with fresh scratch.  `release_workspaces()` = the same for every stream, dropping the buffers."""
    handle = stream.cuda_stream
    keys = [k for k in _workspaces if k[3] == handle and k[2] == stream.device_index]
    return {k: _workspaces.pop(k) for k in keys}


def poison_workspaces():
    """Test hook: fill every cached scratch buffer with 0xFF bytes (fp32 / bf16 / half NaN patterns).  A kernel that reads scratch
    it (or an earlier kernel of the call) did not write -- a ragged tile edge, a row past K -- then shows up as NaN in the result."""
    for buf in _workspaces.values():
        if buf is not None:
            buf.fill_(0xFF)


def release_workspaces():
    """Drop every cached scratch buffer (they are re-grown on demand)."""
    _workspaces.clear()


def gemm(a, b, bias=None, act=_lib.ACT_NONE, slope=0.0, alpha=1.0, b_is_kn=False, out=None):
    """out[M,N] = act((a[M,K] @ (b[N,K]^T | b[K,N]) + bias) * alpha) through ciaosr_gemm_f32."""
    require_gpu(a, b, bias, allow_row_stride=True)
    M, K = a.shape
    N = b.shape[1] if b_is_kn else b.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    _lib.call('ciaosr_gemm_f32', ptr(a), a.stride(0), ptr(b), b.stride(0), int(b_is_kn), ptr(out), out.stride(0),
              ptr(bias), M, N, K, float(alpha), int(act), float(slope), stream_ptr())
    return out


def nchw_to_hwc(x):
    require_gpu(x)
    Cc, H, W = x.shape
    out = torch.empty(H, W, Cc, dtype=torch.float32, device=x.device)
    _lib.call('ciaosr_nchw_to_hwc_f32', ptr(x), ptr(out), Cc, H, W, Cc, stream_ptr())
    return out


def hwc_to_nchw(x):
    require_gpu(x)
    H, W, Cc = x.shape
    out = torch.empty(Cc, H, W, dtype=torch.float32, device=x.device)
    _lib.call('ciaosr_hwc_to_nchw_f32', ptr(x), Cc, ptr(out), Cc, H, W, stream_ptr())
    return out


def head_indices(coord, cell, H, W, local_size=2, chunk=0, want_rel=True):
    require_gpu(coord, cell)
    Q = coord.shape[0]
    J = {1: 1, 2: 4, 3: 9}[local_size]
    q_idx = torch.empty(Q, dtype=torch.int32, device=coord.device)
    k_idx = torch.empty(Q, J, dtype=torch.int32, device=coord.device)
    rel = torch.empty(Q, J, 2, dtype=torch.float32, device=coord.device) if want_rel else None
    _lib.call('ciaosr_head_indices_f32', ptr(coord), ptr(cell), Q, chunk, H, W, local_size, ptr(q_idx), ptr(k_idx),
              ptr(rel), stream_ptr())
    return q_idx, k_idx, rel


def patch_rows(src_hwc, ksize, stride, pad, OH, OW, normalize=False, floor=0.0):
    require_gpu(src_hwc)
    Hs, Ws, Cs = src_hwc.shape
    out = torch.empty(OH * OW, ksize * ksize * Cs, dtype=torch.float32, device=src_hwc.device)
    _lib.call('ciaosr_patch_rows_f32', ptr(src_hwc), Cs, Hs, Ws, Cs, ksize, stride, pad, OH, OW, ptr(out),
              out.stride(0), int(normalize), float(floor), stream_ptr())
    return out


def local_attention(unfold, C_, Cn, q_idx, k_idx, wk, wv, softmax_scale=1.0):
    require_gpu(unfold, q_idx, k_idx, wk, wv)
    Q, J = k_idx.shape
    z = torch.empty(Q, 9 * C_ + Cn, dtype=torch.float32, device=unfold.device)
    _lib.call('ciaosr_local_attention_f32', ptr(unfold), unfold.stride(0), C_, Cn, ptr(q_idx), ptr(k_idx), ptr(wk),
              wk.stride(0), ptr(wv), wv.stride(0), ptr(z), z.stride(0), Q, J, float(softmax_scale), stream_ptr())
    return z


def local_attention_16(unfold, C_, Cn, q_idx, k_idx, wk16, wv16, softmax_scale=1.0):
    """K4 with wk / wv / z as torch.bfloat16 or torch.float16 tensors (ciaosr_local_attention_bf16 / _f16): half the HBM bytes per query."""
    require_gpu(unfold, q_idx, k_idx)
    if not (wk16.is_cuda and wv16.is_cuda and wk16.dtype == wv16.dtype and wk16.dtype in (torch.bfloat16, torch.float16)):
        raise CiaoSRHipError(f'local_attention_16: wk / wv must be bfloat16 or float16 tensors on the GPU, got {wk16.dtype} / {wv16.dtype}')
    Q, J = k_idx.shape
    z = torch.empty(Q, 9 * C_ + Cn, dtype=wk16.dtype, device=unfold.device)
    _lib.call('ciaosr_local_attention_' + ('bf16' if wk16.dtype == torch.bfloat16 else 'f16'), ptr(unfold), unfold.stride(0), C_, Cn,
              ptr(q_idx), ptr(k_idx), ptr(wk16), wk16.stride(0), ptr(wv16), wv16.stride(0), ptr(z), z.stride(0), Q, J, float(softmax_scale),
              stream_ptr())
    return z


def _f3(vals):
    return (C.c_float * 3)(*[float(v) for v in vals])


def normalize(lq_chw, mean, std):
    require_gpu(lq_chw)
    out = torch.empty_like(lq_chw)
    _, H, W = lq_chw.shape
    _lib.call('ciaosr_normalize_f32', ptr(lq_chw), ptr(out), H, W, _f3(mean), _f3(std), stream_ptr())
    return out


def denorm_clamp(pred_q3, H, W, mean, std):
    require_gpu(pred_q3)
    out = torch.empty(3, H, W, dtype=torch.float32, device=pred_q3.device)
    _lib.call('ciaosr_denorm_clamp_f32', ptr(pred_q3), ptr(out), H, W, _f3(mean), _f3(std), stream_ptr())
    return out


def tile_blend(E, Wt, tile_q3, y0, x0, th, tw):
    require_gpu(E, Wt, tile_q3)
    _, Himg, Wimg = E.shape
    _lib.call('ciaosr_tile_blend_f32', ptr(E), ptr(Wt), Himg, Wimg, ptr(tile_q3), y0, x0, th, tw, stream_ptr())


def tile_finalize(E, Wt):
    require_gpu(E, Wt)
    _, Himg, Wimg = E.shape
    out = torch.empty(Himg * Wimg, 3, dtype=torch.float32, device=E.device)
    _lib.call('ciaosr_tile_finalize_f32', ptr(E), ptr(Wt), ptr(out), Himg, Wimg, stream_ptr())
    return out


# ---- self-ensemble (include/ciaosr_hip.h, "self-ensemble"; ids and windows: scene.dihedral_ids / dihedral_window) ----------------------
def _planes(x, what):
    require_gpu(x)
    if x.dtype != torch.float32 or x.dim() < 2:
        raise CiaoSRHipError(f'{what}: expected a float32 tensor [..., h, w], got {x.dtype} {tuple(x.shape)}')
    planes = 1
    for n in x.shape[:-2]:
        planes *= int(n)
    return planes


def dihedral(x, k):
    """T_k of the last two axes of x [..., h, w]: k & 1 flips the columns, then k & 2 the rows, then k & 4 transposes -> a new tensor
    [..., h, w], or [..., w, h] when k & 4 (ciaosr_dihedral_f32)."""
    planes = _planes(x, 'dihedral')
    h, w = x.shape[-2:]
    k = int(k)
    out = torch.empty(*x.shape[:-2], *((w, h) if k & 4 else (h, w)), dtype=torch.float32, device=x.device)
    _lib.call('ciaosr_dihedral_f32', ptr(x), ptr(out), planes, h, w, k, stream_ptr())
    return out


def dihedral_accum(acc, src, k, first, divisor=0.0):
    """acc [..., h, w] = (0 if first else acc) + U_k(src), U_k the inverse of `dihedral`'s T_k (src [..., w, h] when k & 4); with
    divisor > 0 the sum is then divided by it.  In place; `first` never reads acc (ciaosr_dihedral_accum_f32)."""
    planes = _planes(acc, 'dihedral_accum')
    _planes(src, 'dihedral_accum')
    h, w = acc.shape[-2:]
    k = int(k)
    want = tuple(acc.shape[:-2]) + ((w, h) if k & 4 else (h, w))
    if tuple(src.shape) != want:
        raise ValueError(f'dihedral_accum: member {k} of an accumulator {tuple(acc.shape)} is {want}, got {tuple(src.shape)}')
    _lib.call('ciaosr_dihedral_accum_f32', ptr(acc), ptr(src), planes, h, w, k, int(bool(first)), float(divisor), stream_ptr())
    return acc


# ---- affine views of an encoded scene (include/ciaosr_hip.h, "views"; the definition and the host helpers: scene.py) -------------------
def _m6(m):
    m = [float(v) for v in m]
    if len(m) != 6:
        raise ValueError(f'a view matrix is (m_yy, m_yx, t_y, m_xy, m_xx, t_x), got {len(m)} numbers')
    return (C.c_double * 6)(*m)


def _i4(frame):
    return (C.c_int * 4)(*[int(v) for v in frame])


def view_block_queries():
    """Consecutive queries one workgroup of the count / select kernels owns."""
    return _lib.load().ciaosr_view_block_queries()


def make_coord_cell_view(m, hv, wv, frame, device):
    """(coord, cell), each [hv * wv, 2], of the whole hv x wv view under matrix `m` in the frame (y0, x0, th, tw), made on the device,
    members of the frame or not.  The grid's width is registered for `grid_width_of`: a view is walked as a row-major grid."""
    n = hv * wv
    coord = torch.empty(n, 2, dtype=torch.float32, device=device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=device)
    _lib.call('ciaosr_view_coord_cell_f32', ptr(coord), ptr(cell), _m6(m), hv, wv, _i4(frame), stream_ptr())
    if len(_window_width) > 64:
        _window_width.clear()
    _window_width[(coord.data_ptr(), n)] = wv
    return coord, cell


def view_count(m, hv, wv, tiles):
    """tiles [n_tiles, 4] int32 on the device, rows (y0, x0, th, tw) -> (counts [n_tiles] int32 on the device, ws): the members of every
    tile among the hv x wv queries, in one pass over the queries; `ws` is what `view_select` places a tile's members with."""
    require_gpu(tiles)
    n_tiles = tiles.shape[0]
    lib = _lib.load()
    ws = workspace(lib.ciaosr_view_workspace_bytes(hv, wv, n_tiles), tiles.device, slot='view')
    counts = torch.empty(n_tiles, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_view_count_i32', _m6(m), hv, wv, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws


def view_count_many(ms, sizes, tiles):
    """`view_count` for a list of views in one go: ms V x 6 numbers, sizes V x (hv, wv), tiles as there -> (counts [V, n_tiles] int32 on
    the device, ws, offsets).  `ws[offsets[v]:]` is view v's workspace for `view_select`; counts[v] and that workspace are bitwise what
    `view_count` gives for the view alone.  One launch pair per `ciaosr_view_count_many_max_views()` views, nothing synchronises."""
    require_gpu(tiles)
    n_tiles, n_views = tiles.shape[0], len(ms)
    if n_views < 1 or len(sizes) != n_views:
        raise ValueError(f'view_count_many: {n_views} matrices, {len(sizes)} sizes')
    lib = _lib.load()
    flat = [v for m in ms for v in _m6(m)]
    m_arr = (C.c_double * (6 * n_views))(*flat)
    s_arr = (C.c_int * (2 * n_views))(*[int(v) for s in sizes for v in (s[0], s[1])])
    ws = workspace(lib.ciaosr_view_many_workspace_bytes(s_arr, n_views, n_tiles), tiles.device, slot='view_many')
    offsets = [lib.ciaosr_view_many_workspace_offset(s_arr, n_views, n_tiles, v) for v in range(n_views)]
    counts = torch.empty(n_views, n_tiles, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_view_count_many_i32', m_arr, s_arr, n_views, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws, offsets


def view_select(m, hv, wv, frame, index, n_tiles, ws, n):
    """The `n` members (view_count's number) of tile `index` = `frame`, in increasing query index: (q_index [n] int32, coord [n, 2],
    cell [n, 2] in the tile's frame).  No grid hint is registered: the head sees a caller's own list of coordinates."""
    q_index = torch.empty(n, dtype=torch.int32, device=ws.device)
    coord = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    _window_width.pop((coord.data_ptr(), n), None)          # the allocator may hand out the address of a dead grid's coordinates
    _lib.call('ciaosr_view_select_f32', _m6(m), hv, wv, _i4(frame), index, n_tiles, ptr(ws), ws.numel(), n, ptr(q_index), ptr(coord),
              ptr(cell), stream_ptr())
    return q_index, coord, cell


def view_count_blocks(m, hv, wv, tiles):
    """`view_count` with the output grid cut into blocks 4 wide x 2 high (include/ciaosr_hip.h, "Members in blocks"): -> (counts
    [n_tiles, 2] int32 on the device, rows (members, live blocks), ws); `ws` is what `view_select_blocks` places a tile's blocks with."""
    require_gpu(tiles)
    n_tiles = tiles.shape[0]
    lib = _lib.load()
    ws = workspace(lib.ciaosr_view_blocks_workspace_bytes(hv, wv, n_tiles), tiles.device, slot='view_blocks')
    counts = torch.empty(n_tiles, 2, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_view_count_blocks_i32', _m6(m), hv, wv, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws


def view_count_blocks_many(ms, sizes, tiles):
    """`view_count_blocks` for a list of views, as `view_count_many`: -> (counts [V, n_tiles, 2] int32 on the device, ws, offsets);
    counts[v] and `ws[offsets[v]:]` are bitwise what `view_count_blocks` gives for the view alone."""
    require_gpu(tiles)
    n_tiles, n_views = tiles.shape[0], len(ms)
    if n_views < 1 or len(sizes) != n_views:
        raise ValueError(f'view_count_blocks_many: {n_views} matrices, {len(sizes)} sizes')
    lib = _lib.load()
    flat = [v for m in ms for v in _m6(m)]
    m_arr = (C.c_double * (6 * n_views))(*flat)
    s_arr = (C.c_int * (2 * n_views))(*[int(v) for s in sizes for v in (s[0], s[1])])
    ws = workspace(lib.ciaosr_view_blocks_many_workspace_bytes(s_arr, n_views, n_tiles), tiles.device, slot='view_blocks_many')
    offsets = [lib.ciaosr_view_blocks_many_workspace_offset(s_arr, n_views, n_tiles, v) for v in range(n_views)]
    counts = torch.empty(n_views, n_tiles, 2, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_view_count_blocks_many_i32', m_arr, s_arr, n_views, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws, offsets


def view_select_blocks(m, hv, wv, frame, index, n_tiles, ws, n_blocks):
    """The `n_blocks` live blocks (view_count_blocks' number) of tile `index` = `frame`, in increasing block index, eight entries each in
    the order the chained 16-bit head kernel walks a row tile: (q_index [8 n_blocks] int32, coord, cell [8 n_blocks, 2]).  A pad -- no
    member of the tile, or outside the grid -- has q_index -1 and the coordinate of its block's first member; `view_blend` skips it.
    No grid hint is registered: eight consecutive entries are one row tile."""
    n = 8 * n_blocks
    q_index = torch.empty(n, dtype=torch.int32, device=ws.device)
    coord = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    _window_width.pop((coord.data_ptr(), n), None)          # the allocator may hand out the address of a dead grid's coordinates
    _lib.call('ciaosr_view_select_blocks_f32', _m6(m), hv, wv, _i4(frame), index, n_tiles, ptr(ws), ws.numel(), n_blocks, ptr(q_index),
              ptr(coord), ptr(cell), stream_ptr())
    return q_index, coord, cell


def view_blend(E, Wt, q_index, rgb):
    """E[:, q_index[s]] += rgb[s], Wt[q_index[s]] += 1 (E [3, Q], Wt [Q], rgb [n, 3]); q_index None: s itself.  An index outside
    [0, Q) -- the -1 of a block list's pad -- is skipped."""
    require_gpu(E, Wt, q_index, rgb)
    if E.shape != (3, Wt.shape[0]) or rgb.dim() != 2 or rgb.shape[1] != 3 or (q_index is not None and q_index.shape != (rgb.shape[0],)):
        raise ValueError(f'view_blend: E {tuple(E.shape)}, Wt {tuple(Wt.shape)}, rgb {tuple(rgb.shape)} do not fit together')
    _lib.call('ciaosr_view_blend_f32', ptr(E), ptr(Wt), Wt.shape[0], ptr(q_index), ptr(rgb), rgb.shape[0], stream_ptr())


def view_finalize(E, Wt, fill, mean, std):
    """[Q, 3] for `denorm_clamp`: E / Wt where a tile claimed the query, elsewhere what `denorm_clamp` turns into `fill` (three floats in
    the output's [0, 1])."""
    require_gpu(E, Wt)
    out = torch.empty(Wt.shape[0], 3, dtype=torch.float32, device=E.device)
    _lib.call('ciaosr_view_finalize_f32', ptr(E), ptr(Wt), ptr(out), Wt.shape[0], _f3(fill), _f3(mean), _f3(std), stream_ptr())
    return out


# ---- warps of an encoded scene (include/ciaosr_hip.h, "warps"; the definition and the host helpers: scene.py) --------------------------
def _warp_source(h, map_, footprint, hv, wv):
    """The (h9, map, footprint) arguments of a warp entry: exactly one of `h` (nine numbers) and `map_` (a contiguous float64 device
    tensor [hv, wv, 2]) is given.  There is no CPU fallback: a host map is an error."""
    if (h is None) == (map_ is None):
        raise ValueError('a warp has exactly one point source: a homography or a map')
    fp = (C.c_double * 2)(*[float(v) for v in footprint])
    if h is not None:
        h = [float(v) for v in h]
        if len(h) != 9:
            raise ValueError(f'a homography is (h00, h01, h02, h10, h11, h12, h20, h21, h22), got {len(h)} numbers')
        return (C.c_double * 9)(*h), C.c_void_p(0), fp
    if not map_.is_cuda:
        raise CiaoSRHipError('a warp map lives on the MI355X: got a CPU tensor (no CPU fallback; move the map to cuda)')
    if map_.dtype != torch.float64 or tuple(map_.shape) != (hv, wv, 2) or not map_.is_contiguous():
        raise ValueError(f'a warp map is a contiguous float64 tensor [{hv}, {wv}, 2] of (y_lr, x_lr), got {map_.dtype} {tuple(map_.shape)}')
    return None, ptr(map_), fp


def make_coord_cell_warp(h, map_, footprint, hv, wv, frame, device):
    """(coord, cell), each [hv * wv, 2], of the whole hv x wv warp -- homography `h` or map `map_`, one of them None -- in the frame
    (y0, x0, th, tw), made on the device, members of the frame or not.  The grid's width is registered for `grid_width_of`, exactly as
    `make_coord_cell_view` does: a warp inside one frame is walked as a row-major grid."""
    h9, mp, fp = _warp_source(h, map_, footprint, hv, wv)
    n = hv * wv
    coord = torch.empty(n, 2, dtype=torch.float32, device=device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=device)
    _lib.call('ciaosr_warp_coord_cell_f32', ptr(coord), ptr(cell), h9, mp, fp, hv, wv, _i4(frame), stream_ptr())
    if len(_window_width) > 64:
        _window_width.clear()
    _window_width[(coord.data_ptr(), n)] = wv
    return coord, cell


def warp_workspace_bytes(hv, wv, n_tiles):
    return _lib.load().ciaosr_warp_workspace_bytes(hv, wv, n_tiles)


def warp_count(h, map_, footprint, hv, wv, tiles, ws=None):
    """`view_count` of a warp: tiles [n_tiles, 4] int32 on the device -> (counts [n_tiles] int32 on the device, ws), `ws` what
    `warp_select` places a tile's members with.  `ws`: the caller's own uint8 buffer of at least `warp_workspace_bytes` (several warps
    counted before one copy of their counts each need their own), default the cached 'warp' scratch.  Nothing synchronises."""
    require_gpu(tiles)
    h9, mp, fp = _warp_source(h, map_, footprint, hv, wv)
    n_tiles = tiles.shape[0]
    if ws is None:
        ws = workspace(warp_workspace_bytes(hv, wv, n_tiles), tiles.device, slot='warp')
    counts = torch.empty(n_tiles, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_warp_count_i32', h9, mp, fp, hv, wv, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws


def warp_select(h, map_, footprint, hv, wv, frame, index, n_tiles, ws, n):
    """The `n` members (warp_count's number) of tile `index` = `frame`, in increasing query index: (q_index [n] int32, coord [n, 2],
    cell [n, 2] in the tile's frame).  No grid hint is registered: the head sees a caller's own list of coordinates."""
    h9, mp, fp = _warp_source(h, map_, footprint, hv, wv)
    q_index = torch.empty(n, dtype=torch.int32, device=ws.device)
    coord = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    _window_width.pop((coord.data_ptr(), n), None)          # the allocator may hand out the address of a dead grid's coordinates
    _lib.call('ciaosr_warp_select_f32', h9, mp, fp, hv, wv, _i4(frame), index, n_tiles, ptr(ws), ws.numel(), n, ptr(q_index), ptr(coord),
              ptr(cell), stream_ptr())
    return q_index, coord, cell


# ---- per-pixel warps (include/ciaosr_hip.h, "per-pixel warps"): `spec` is a scene.PerPixel with a float64 contiguous device tensor -------
def _warp_pp_source(h, map_, spec, hv, wv):
    """The (h9, map, mode, range, tensor) arguments of a per-pixel warp entry."""
    h9, mp, _ = _warp_source(h, map_, (1.0, 1.0), hv, wv)
    tensor = C.c_void_p(0)
    if spec.tensor is not None:
        t = spec.tensor
        if not t.is_cuda:
            raise CiaoSRHipError('a footprint tensor lives on the MI355X: got a CPU tensor (no CPU fallback; move it to cuda)')
        if t.dtype != torch.float64 or tuple(t.shape) != (hv, wv, 2) or not t.is_contiguous():
            raise ValueError(f'a footprint tensor is a contiguous float64 tensor [{hv}, {wv}, 2] of (g_y, g_x), got {t.dtype} {tuple(t.shape)}')
        tensor = ptr(t)
    return h9, mp, int(spec.mode), (C.c_double * 2)(*[float(v) for v in spec.range]), tensor


def make_coord_cell_warp_pp(h, map_, spec, hv, wv, frame, device):
    """`make_coord_cell_warp` of a per-pixel warp: cell [hv * wv, 2] holds every query's own cell (NaN where the pixel has no footprint)."""
    src = _warp_pp_source(h, map_, spec, hv, wv)
    n = hv * wv
    coord = torch.empty(n, 2, dtype=torch.float32, device=device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=device)
    _lib.call('ciaosr_ppwarp_coord_cell_f32', ptr(coord), ptr(cell), *src, hv, wv, _i4(frame), stream_ptr())
    if len(_window_width) > 64:
        _window_width.clear()
    _window_width[(coord.data_ptr(), n)] = wv
    return coord, cell


def warp_pp_count(h, map_, spec, hv, wv, tiles, ws=None):
    """`warp_count` of a per-pixel warp: a pixel without a footprint is a member of no tile.  The workspace is `warp_count`'s."""
    require_gpu(tiles)
    src = _warp_pp_source(h, map_, spec, hv, wv)
    n_tiles = tiles.shape[0]
    if ws is None:
        ws = workspace(warp_workspace_bytes(hv, wv, n_tiles), tiles.device, slot='warp')
    counts = torch.empty(n_tiles, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_ppwarp_count_i32', *src, hv, wv, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws


def warp_pp_select(h, map_, spec, hv, wv, frame, index, n_tiles, ws, n):
    """`warp_select` of a per-pixel warp (`n`, `ws`: warp_pp_count's): cell [n, 2] holds each member's own cell in the tile's frame."""
    src = _warp_pp_source(h, map_, spec, hv, wv)
    q_index = torch.empty(n, dtype=torch.int32, device=ws.device)
    coord = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    _window_width.pop((coord.data_ptr(), n), None)          # the allocator may hand out the address of a dead grid's coordinates
    _lib.call('ciaosr_ppwarp_select_f32', *src, hv, wv, _i4(frame), index, n_tiles, ptr(ws), ws.numel(), n, ptr(q_index), ptr(coord),
              ptr(cell), stream_ptr())
    return q_index, coord, cell


def warp_footprints(h, map_, spec, hv, wv, device=None):
    """The clamped footprints (f_y, f_x) of the whole grid of a per-pixel warp, [hv, wv, 2] float64 on the device, NaN where the pixel has
    none: a warp's scale field, for inspection.  Nothing synchronises."""
    src = _warp_pp_source(h, map_, spec, hv, wv)
    if device is None:
        device = map_.device if map_ is not None else (spec.tensor.device if spec.tensor is not None else torch.device('cuda'))
    out = torch.empty(hv, wv, 2, dtype=torch.float64, device=device)
    _lib.call('ciaosr_ppwarp_footprints_f64', ptr(out), *src, hv, wv, stream_ptr())
    return out


# ---- area-sampled warps (include/ciaosr_hip.h, "area-sampled warps"): `spec` is a scene.PerPixel with `samples` = max_samples ---------------
def _warp_area_source(h, spec, hv, wv):
    """The (h9, mode, range, tensor, max_samples) arguments of the area entries that build the table: a homography only."""
    if h is None:
        raise ValueError('an area-sampled warp has a homography as its point source')
    h9, _, mode, rng, tensor = _warp_pp_source(h, None, spec, hv, wv)
    return h9, mode, rng, tensor, int(spec.samples)


def warp_area_workspace_bytes(hv, wv, n_tiles, max_samples):
    return _lib.load().ciaosr_areawarp_workspace_bytes(hv, wv, n_tiles, max_samples)


def _warp_area_ws(hv, wv, n_tiles, max_samples, device, ws):
    nbytes = warp_area_workspace_bytes(hv, wv, n_tiles, max_samples)
    if nbytes == 0:
        raise ValueError(f'no area-sampled warp of {hv} x {wv} pixels with max_samples {max_samples} over {n_tiles} tiles')
    return workspace(nbytes, device, slot='warp_area') if ws is None else ws


def warp_area_count(h, spec, hv, wv, tiles, ws=None):
    """The sample table of an area-sampled warp and its tile membership: tiles [n_tiles, 4] int32 on the device -> (counts [n_tiles + 2]
    int32 on the device: the samples in each tile, then S, the number of samples, then the number of pixels with exactly one sample;
    ws).  `ws` holds the table and the partial counts for `warp_area_select` / `warp_area_resolve`: the caller's own uint8 buffer of at
    least `warp_area_workspace_bytes`, default the cached 'warp_area' scratch.  Nothing synchronises."""
    require_gpu(tiles)
    src = _warp_area_source(h, spec, hv, wv)
    n_tiles = tiles.shape[0]
    ws = _warp_area_ws(hv, wv, n_tiles, src[-1], tiles.device, ws)
    counts = torch.empty(n_tiles + 2, dtype=torch.int32, device=tiles.device)
    _lib.call('ciaosr_areawarp_count_i32', *src, hv, wv, ptr(tiles), n_tiles, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    return counts, ws


def warp_area_select(h, max_samples, hv, wv, frame, index, n_tiles, ws, n_samples, n):
    """The `n` samples (warp_area_count's number) of tile `index` = `frame` among the `n_samples` of the warp, in increasing sample id:
    (s_index [n] int32, coord [n, 2], cell [n, 2] in the tile's frame)."""
    h9 = (C.c_double * 9)(*[float(v) for v in h])
    s_index = torch.empty(n, dtype=torch.int32, device=ws.device)
    coord = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    cell = torch.empty(n, 2, dtype=torch.float32, device=ws.device)
    _window_width.pop((coord.data_ptr(), n), None)          # the allocator may hand out the address of a dead grid's coordinates
    _lib.call('ciaosr_areawarp_select_f32', h9, int(max_samples), hv, wv, _i4(frame), index, n_tiles, ptr(ws), ws.numel(), n_samples, n,
              ptr(s_index), ptr(coord), ptr(cell), stream_ptr())
    return s_index, coord, cell


def warp_area_resolve(E, Wt, n_samples, max_samples, hv, wv, n_tiles, ws, fill, mean, std):
    """The finished image [3, hv, wv] of the sample accumulators E [3, S], Wt [S] (S = `n_samples`; tensors of one column where S is 0):
    per pixel the mean of its samples' values, each finished as `view_finalize` + `denorm_clamp` finish a query."""
    require_gpu(E, Wt)
    if E.shape != (3, Wt.shape[0]) or Wt.shape[0] != max(n_samples, 1):   # the channel stride of E is the number of samples
        raise ValueError(f'warp_area_resolve: E {tuple(E.shape)}, Wt {tuple(Wt.shape)} are not the accumulators of {n_samples} samples')
    out = torch.empty(3, hv, wv, dtype=torch.float32, device=E.device)
    _lib.call('ciaosr_areawarp_resolve_f32', ptr(E), ptr(Wt), ptr(out), n_samples, int(max_samples), hv, wv, n_tiles, ptr(ws), ws.numel(),
              _f3(fill), _f3(mean), _f3(std), stream_ptr())
    return out


def warp_area_table(h, spec, hv, wv, device=None):
    """The sample table of an area-sampled warp, for inspection and tests: (first [hv * wv + 1] int32, n [hv, wv, 2] int32 = (n_y, n_x),
    (0, 0) where the pixel has no samples), on the device; first[-1] is S.  Nothing synchronises."""
    src = _warp_area_source(h, spec, hv, wv)
    if device is None:
        device = spec.tensor.device if spec.tensor is not None else torch.device('cuda')
    ws = _warp_area_ws(hv, wv, 1, src[-1], device, None)
    first = torch.empty(hv * wv + 1, dtype=torch.int32, device=device)
    n = torch.empty(hv, wv, 2, dtype=torch.int32, device=device)
    _lib.call('ciaosr_areawarp_table_i32', ptr(first), ptr(n), *src, hv, wv, 1, ptr(ws), ws.numel(), stream_ptr())
    return first, n


class Mode(namedtuple('Mode', 'name precision f16_pairs bf16_single trunk head')):
    """One named arithmetic mode.  (precision, f16_pairs, bf16_single): the entry suffix and the canonical ciaosr_options_t fields
    (include/ciaosr_hip.h, "Precision modes").  trunk: element type of the RDN trunk's dense layers, None = the fp32 trunk.  head: the
    head weight form PackedHead packs, None = fp32 only, 'bf16' / 'f16' = hi + lo fragment pairs, 'bf16-single' = one
    error-feedback-rounded bf16 weight per product with calibrated biases."""
    __slots__ = ()


MODES = {m.name: m for m in (
    Mode('fp32', 'fp32', 0, 0, None, None),          # exact-fp32 MFMA, the contract precision
    Mode('bf16', 'bf16', 0, 0, 'bf16', 'bf16'),      # bf16 MFMA inputs, fp32 accumulation, weights as bf16 hi + lo pairs
    Mode('bf16-single', 'bf16', 0, 1, 'bf16', 'bf16-single'),   # ONE bf16 weight per product (head_hip.py: _build_single)
    Mode('bf16x3', 'bf16', 2, 0, None, 'bf16'),      # the head's weights AND activations as bf16 pairs (three MFMAs per product), fp32 trunk
    Mode('f16', 'f16', 0, 0, 'f16', 'f16'),          # IEEE half MFMA inputs, one MFMA per product, saturating at 65504
    Mode('f16-pairs', 'f16', 1, 0, 'f16', 'f16'),    # half activations, every weight as a half hi + lo pair
    Mode('f16x3', 'f16', 2, 0, None, 'f16'),         # the fp32-tolerance fast mode: 'bf16x3' in half
    Mode('f16x3-fast', 'f16', 3, 0, 'f16', 'f16'),   # the head of 'f16x3' on the trunk of 'f16-pairs'; PSNR-gated only
)}
PRECISIONS = tuple(MODES)       # what Options(precision) / test_cfg.precision accept
_ALIASES = {'f32': 'fp32', 'bf16_single': 'bf16-single', 'bf16-x3': 'bf16x3', 'fp16': 'f16', 'half': 'f16', 'f16_pairs': 'f16-pairs',
            'f16p': 'f16-pairs', 'f16-x3': 'f16x3'}


def resolve_mode(precision='fp32', f16_pairs=None, bf16_single=None):
    """The MODES row a call runs: the name (or alias) gives the defaults, explicit raw fields override them, and the result reads the
    way the C entry points read it -- the _f32 entries ignore both fields, the _bf16 entries ignore f16_pairs 1 and 3 and
    bf16_single under f16_pairs 2, the _f16 entries ignore bf16_single."""
    name = _ALIASES.get(precision, precision)
    if name not in MODES:
        raise ValueError(f'unknown precision {precision!r}: one of {PRECISIONS} (or an alias: {sorted(_ALIASES)})')
    m = MODES[name]
    pairs = m.f16_pairs if f16_pairs is None else int(f16_pairs)
    single = m.bf16_single if bf16_single is None else int(bf16_single)
    if pairs not in (0, 1, 2, 3) or single not in (0, 1):
        raise ValueError(f'f16_pairs must be 0..3 and bf16_single 0 or 1, got {pairs} / {single}')
    if m.precision == 'fp32':
        return m
    if m.precision == 'bf16':
        return MODES['bf16x3' if pairs == 2 else 'bf16-single' if single else 'bf16']
    return MODES[('f16', 'f16-pairs', 'f16x3', 'f16x3-fast')[pairs]]


class Options:
    """Per-call evaluation options, passed explicitly down the call chain (no process-global switches).

    precision  a name of PRECISIONS (or an alias), optionally refined by raw f16_pairs / bf16_single: resolved to ONE row of MODES,
               `opt.mode`; `precision`, `f16_pairs` and `bf16_single` then hold that row's canonical values ('fp32' | 'bf16' | 'f16':
               the _f32 / _bf16 / _f16 entry point).
    the rest   fields of ciaosr_options_t (include/ciaosr_hip.h): result-equivalent route choices; 0 = default.
    Immutable; `replace()` returns a modified copy."""
    _C_FIELDS = ('head_route', 'csa_composed_min', 'dense_min_tiles', 'scatter_small_max', 'kv_rows', 'decode_rows', 'bf16_single', 'dense_direct', 'csa_scores_gemm', 'csa_attn_tile128', 'query_grid_w', 'f16_pairs',
                 'csa_attn_v16', 'edsr_resident', 'swin_h16', 'csa_block_mb')
    _MODE_FIELDS = ('precision', 'f16_pairs', 'bf16_single')
    __slots__ = ('mode', 'precision') + _C_FIELDS + ('_c',)

    def __init__(self, precision='fp32', f16_pairs=None, bf16_single=None, **kw):
        mode = resolve_mode(precision, f16_pairs, bf16_single)
        object.__setattr__(self, 'mode', mode)
        for f in self._MODE_FIELDS:
            object.__setattr__(self, f, getattr(mode, f))
        for f in self._C_FIELDS:
            if f not in self._MODE_FIELDS:
                object.__setattr__(self, f, int(kw.pop(f, 0)))
        if kw:
            raise TypeError(f'unknown option(s): {sorted(kw)}')
        st = None
        if any(getattr(self, f) for f in self._C_FIELDS):
            st = _lib.OptionsT()
            for f in self._C_FIELDS:
                setattr(st, f, getattr(self, f))
        object.__setattr__(self, '_c', st)

    def __setattr__(self, k, v):
        raise AttributeError('Options is immutable; use replace()')

    def replace(self, **kw):
        """A copy with some fields changed; `precision` may name any mode (its f16_pairs / bf16_single unless given too)."""
        cur = {f: getattr(self, f) for f in self._C_FIELDS if f not in self._MODE_FIELDS}
        cur['precision'] = self.mode.name
        cur.update(kw)
        return Options(**cur)

    @property
    def bf16(self):
        return self.precision == 'bf16'

    @property
    def half(self):
        """None for the fp32 entries, else the 16-bit element type of the MFMA operands: 'bf16' | 'f16'."""
        return None if self.precision == 'fp32' else self.precision

    @property
    def suffix(self):
        """Entry-point suffix of the C ABI: 'f32' | 'bf16' | 'f16'."""
        return 'f32' if self.precision == 'fp32' else self.precision

    def c_arg(self):
        """ctypes argument for `const ciaosr_options_t* opt` (NULL when every field is default)."""
        return C.byref(self._c) if self._c is not None else None

    def __repr__(self):
        extra = ''.join(f', {f}={getattr(self, f)}' for f in self._C_FIELDS if getattr(self, f) and f not in self._MODE_FIELDS)
        return f'Options({self.mode.name!r}{extra})'


DEFAULT_OPTIONS = Options()


def as_options(options):
    """None -> defaults; 'fp32'/'bf16'/'f16' -> Options(precision); Options -> itself; dict -> Options(**dict)."""
    if options is None:
        return DEFAULT_OPTIONS
    if isinstance(options, Options):
        return options
    if isinstance(options, str):
        return Options(options)
    if isinstance(options, dict):
        return Options(**options)
    raise TypeError(f'options must be None, str, dict or hip_ops.Options, got {type(options)}')


def gather_rows(unfold, C_, Cn, coord, cell, H, W, local_size=2, chunk=0):
    """K1 as the reference assembles it: (q_rows [Q,9C], inp_k [Q*J,9C+4], inp_v [Q*J,9C+Cn+4], q_idx, k_idx)."""
    require_gpu(unfold, coord, cell)
    Q = coord.shape[0]
    J = {1: 1, 2: 4, 3: 9}[local_size]
    D, Dv = 9 * C_, 9 * C_ + Cn
    dev = unfold.device
    q_rows = torch.empty(Q, D, dtype=torch.float32, device=dev)
    inp_k = torch.empty(Q * J, D + 4, dtype=torch.float32, device=dev)
    inp_v = torch.empty(Q * J, Dv + 4, dtype=torch.float32, device=dev)
    q_idx = torch.empty(Q, dtype=torch.int32, device=dev)
    k_idx = torch.empty(Q, J, dtype=torch.int32, device=dev)
    _lib.call('ciaosr_gather_rows_f32', ptr(unfold), unfold.stride(0), C_, Cn, ptr(coord), ptr(cell), Q, int(chunk or 0),
              H, W, local_size, ptr(q_rows), D, ptr(inp_k), D + 4, ptr(inp_v), Dv + 4, ptr(q_idx), ptr(k_idx),
              stream_ptr())
    return q_rows, inp_k, inp_v, q_idx, k_idx


def mlp_forward(x, mlp_struct, n_run=0):
    """MLPRefiner.forward layer by layer (no hoist); n_run > 0 stops after that many layers (ReLU applied)."""
    require_gpu(x)
    rows = x.shape[0]
    n = n_run or mlp_struct.n_layers
    out = torch.empty(rows, mlp_struct.width[n - 1], dtype=torch.float32, device=x.device)
    nbytes = _lib.load().ciaosr_mlp_workspace_bytes(C.byref(mlp_struct), rows)
    ws = workspace(nbytes, x.device, slot='mlp')
    _lib.call('ciaosr_mlp_forward_f32', ptr(x), x.stride(0), C.byref(mlp_struct), int(n_run), rows, ptr(out),
              out.stride(0), ptr(ws), ws.numel(), stream_ptr())
    return out


def mlp_forward_16(x, mlp_struct, half='bf16'):
    """MLPRefiner.forward with every Linear on the 16-bit MFMA GEMM (ciaosr_mlp_forward_bf16 / _f16): fp32 in, fp32 out."""
    require_gpu(x)
    rows = x.shape[0]
    out = torch.empty(rows, mlp_struct.width[mlp_struct.n_layers - 1], dtype=torch.float32, device=x.device)
    nbytes = _lib.load().ciaosr_mlp_workspace_bytes_16(C.byref(mlp_struct), rows)
    ws = workspace(nbytes, x.device, slot='mlp16')
    _lib.call('ciaosr_mlp_forward_' + half, ptr(x), x.stride(0), C.byref(mlp_struct), rows, ptr(out), out.stride(0), ptr(ws), ws.numel(),
              stream_ptr())
    return out


def decode_residual(h, w_last, b_last, x_lr_chw, coord, H, W):
    require_gpu(h, w_last, b_last, x_lr_chw, coord)
    Q = h.shape[0]
    rgb = torch.empty(Q, 3, dtype=torch.float32, device=h.device)
    _lib.call('ciaosr_decode_residual_f32', ptr(h), h.stride(0), h.shape[1], ptr(w_last), w_last.stride(0), ptr(b_last),
              ptr(x_lr_chw), ptr(coord), Q, H, W, ptr(rgb), stream_ptr())
    return rgb


class profile:
    """Context manager around the library's per-kernel HIP-event timing."""

    def __init__(self, only=None):
        self.only = only

    def __enter__(self):
        lib = _lib.load()
        lib.ciaosr_prof_filter(self.only.encode() if self.only else None)
        lib.ciaosr_prof_reset()
        lib.ciaosr_prof_enable(1)
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        lib.ciaosr_prof_collect()
        lib.ciaosr_prof_enable(0)
        return False

    @staticmethod
    def results():
        lib = _lib.load()
        lib.ciaosr_prof_collect()
        buf = C.create_string_buffer(8192)
        lib.ciaosr_prof_names(buf, 8192)
        out = {}
        for name in [n for n in buf.value.decode().split(';') if n]:
            ms, n = C.c_double(0), C.c_long(0)
            lib.ciaosr_prof_get(name.encode(), C.byref(ms), C.byref(n))
            if n.value:
                out[name] = dict(total_ms=ms.value, launches=n.value, avg_ms=ms.value / n.value)
        return out
