"""The block-ordered member lists of an affine view (include/ciaosr_hip.h, "Members in blocks") restated in numpy float64 on top of
tests/view_reference.py (one rounded operation per numpy call): what tests/test_view_blocks_host.py and tests/test_view_blocks_gpu.py
hold `ciaosr_view_count_blocks_i32` / `ciaosr_view_select_blocks_f32` to, and the inputs those tests share."""
import numpy as np

from tests import view_reference as vr

# The view of the tests: 45 x 53 (odd height, width no multiple of 4) at zoom 3.3, turned by 30 degrees, centred at LR (4.0, 25.5) so
# that the image's upper border cuts it.  ONE: LR 32 x 40 as one frame.  TILED: LR 40 x 56 under tile 32 / overlap 8: 2 x 2 tiles.
SIZE, ARGS = (45, 53), ((4.0, 25.5), 3.3, 30)
ONE_LR, TILED_LR, TILE, OVERLAP = (32, 40), (40, 56), 32, 8


def block_pixels(hv, wv):
    """(q [n_blocks, 8] int64, -1 outside the grid): entry e of block b = by * ceil(wv / 4) + bx is output pixel
    (2 by + (e >> 2), 4 bx + (e & 3))."""
    nby, nbx = (hv + 1) // 2, (wv + 3) // 4
    b = np.arange(nby * nbx)
    e = np.arange(8)
    i = 2 * (b // nbx)[:, None] + (e >> 2)[None, :]
    j = 4 * (b % nbx)[:, None] + (e & 3)[None, :]
    return np.where((i < hv) & (j < wv), i * wv + j, -1)


def block_list(m, hv, wv, frame):
    """dict(members, blocks, q_index [8 blocks] int32, coord [8 blocks, 2] float32, cell [8 blocks, 2] float32, full: live blocks
    without a pad, padded: live blocks with one) of the frame's block list."""
    y, x = vr.lr_points(m, hv, wv)
    q = block_pixels(hv, wv)
    safe = np.maximum(q, 0)
    mem = (q >= 0) & vr.members(y, x, frame)[safe]
    live = mem.any(1)
    coord = vr.coord_in(y, x, frame)[safe]                              # [n_blocks, 8, 2]
    first = mem.argmax(1)                                               # the first member in entry order
    pad = coord[np.arange(q.shape[0]), first][:, None, :]
    coord = np.where(mem[:, :, None], coord, pad)
    n = int(live.sum())
    return dict(members=int(mem.sum()), blocks=n, q_index=np.where(mem, q, -1)[live].reshape(-1).astype(np.int32),
                coord=np.ascontiguousarray(coord[live].reshape(-1, 2)),
                cell=np.ascontiguousarray(np.broadcast_to(vr.cell_in(m, frame), (8 * n, 2))),
                full=int((mem.all(1)).sum()), padded=int((live & ~mem.all(1)).sum()))
