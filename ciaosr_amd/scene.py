"""Encode once, render any scale or window: the host side of the persistent head scene (include/ciaosr_hip.h, "a persistent head scene").

Pure Python, no GPU: the window planner (which LR tiles a window of the HR grid touches, and which part of each), the least-recently-used
cache that bounds the bytes of tile scenes kept alive, and the record `CiaoSR.encode` returns.  The device work is in
`PackedHead.prepare` / `query` (head_hip.py) and `hip_ops.make_coord_cell_window`.
"""
from collections import OrderedDict

from . import tile_plan


def target_size(h, w, size=None, scale=None):
    """(Ht, Wt) of a render: `size` as given, else round(h * s), round(w * s) -- the reference's rule (ciaosr.py:166-169)."""
    if (size is None) == (scale is None):
        raise ValueError('give exactly one of size=(Ht, Wt) and scale')
    if size is not None:
        ht, wt = int(size[0]), int(size[1])
    else:
        ht, wt = round(h * scale), round(w * scale)
    if ht < 1 or wt < 1:
        raise ValueError(f'empty target grid {ht} x {wt}')
    return ht, wt


def check_window(ht, wt, window=None):
    """(i0, j0, h, w) in HR pixels, the whole grid by default; ValueError when it is empty or leaves the ht x wt grid."""
    if window is None:
        return 0, 0, ht, wt
    i0, j0, hh, ww = (int(v) for v in window)
    if hh < 1 or ww < 1 or i0 < 0 or j0 < 0 or i0 + hh > ht or j0 + ww > wt:
        raise ValueError(f'window (i0, j0, h, w) = {(i0, j0, hh, ww)} is empty or outside the {ht} x {wt} grid')
    return i0, j0, hh, ww


def plan_window(h, w, tile, overlap, ht, wt, window=None, scale=None, any_scale=False):
    """The LR tiles of an h x w image (the reference's tiling, ciaosr.py:227-234, row-major: its blend order) that a window of the ht x wt
    target touches.  Per touched tile a dict:
        index            position in the full row-major tile list
        y0, x0, th, tw   the LR tile
        a0, a1, b0, b1   rows [a0, a1) x columns [b0, b1) of the HR grid: the tile's HR rectangle intersected with the window
        grid             (Ht, Wt, i0, i1, j0, j1, frame): the arguments of hip_ops.make_coord_cell_window for that part
    any_scale = False: `clip_test`'s meaning -- (ht, wt) must be (h * scale, w * scale) for the integer `scale` (ValueError otherwise:
    `restore` cannot produce that image either); a tile's queries are the tile-local make_coord grid of (th * scale, tw * scale).
    any_scale = True: `tile_plan`'s -- HR pixels by centre membership, the global grid seen in the tile's frame."""
    wi0, wj0, wh, ww = check_window(ht, wt, window)
    wi1, wj1 = wi0 + wh, wj0 + ww
    tile = min(int(tile), h, w)
    overlap = int(overlap or 0)
    if any_scale:
        overlap = min(overlap, tile - 1)
    else:
        if scale is None or int(scale) != scale or (ht, wt) != (h * int(scale), w * int(scale)):
            raise ValueError(f'tiled rendering without test_cfg.tile_any_scale makes the ({h} * s) x ({w} * s) image of the integer '
                             f'test_cfg.scale only (asked: {ht} x {wt}, scale {scale})')
        scale = int(scale)
    ys, xs = tile_plan.tile_starts(h, tile, overlap), tile_plan.tile_starts(w, tile, overlap)

    def span(p0, n_lr, n_hr):
        return tile_plan.hr_span(p0, tile, n_lr, n_hr) if any_scale else (p0 * scale, (p0 + tile) * scale)

    out = []
    for ny, y0 in enumerate(ys):
        i0, i1 = span(y0, h, ht)
        a0, a1 = max(i0, wi0), min(i1, wi1)
        if a0 >= a1:
            continue
        for nx, x0 in enumerate(xs):
            j0, j1 = span(x0, w, wt)
            b0, b1 = max(j0, wj0), min(j1, wj1)
            if b0 >= b1:
                continue
            if any_scale:
                grid = (ht, wt, a0, a1, b0, b1, (h, y0, tile, w, x0, tile))
            else:
                grid = (tile * scale, tile * scale, a0 - i0, a1 - i0, b0 - j0, b1 - j0, None)
            out.append(dict(index=ny * len(xs) + nx, y0=y0, x0=x0, th=tile, tw=tile, a0=a0, a1=a1, b0=b0, b1=b1, grid=grid))
    return out


class SceneCache:
    """Least-recently-used cache of built scenes under a byte budget.  `build(key)` returns an object with `.nbytes`.  The entry `get`
    returns is never evicted by that call, so the smallest budget still works, by rebuilding; `builds` counts every build, rebuilt
    entries included."""

    def __init__(self, budget_bytes, build):
        self.budget = int(budget_bytes)
        self.build = build
        self.entries = OrderedDict()
        self.nbytes = 0
        self.builds = 0
        self._last = 0                  # bytes of the last build: what the next one is expected to take (tiles are equally sized)

    def _evict(self, room, keep=None):
        for key in list(self.entries):
            if self.nbytes + room <= self.budget:
                break
            if key != keep:
                self.nbytes -= self.entries.pop(key).nbytes

    def get(self, key):
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit
        self._evict(self._last)          # before the build, so that the peak stays at the budget
        hit = self.build(key)
        self.builds += 1
        self._last = hit.nbytes
        self.entries[key] = hit
        self.nbytes += hit.nbytes
        self._evict(0, keep=key)
        return hit

    def clear(self):
        self.entries.clear()
        self.nbytes = 0


class EncodedImage:
    """What `CiaoSR.encode` returns: the normalised LR batch, the Options and max_scale its scenes are planned with, and the scenes -- the
    whole image's (no `test_cfg.tile`), or a SceneCache of one per (batch item, LR tile), built when a render first touches the tile."""

    def __init__(self, x, options, max_scale, budget_bytes, build):
        self.x = x
        self.options = options
        self.max_scale = max_scale
        self.cache = SceneCache(budget_bytes, build)

    @property
    def shape(self):
        return tuple(self.x.shape[-2:])

    @property
    def scene_bytes(self):
        return self.cache.nbytes
