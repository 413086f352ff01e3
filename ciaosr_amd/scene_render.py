"""The scene renderer behind CiaoSR.encode / render / render_view / render_warp / render_many / prefetch / render_pyramid (an extension,
absent from the reference): the device side of scene.py.  A target -- `scene.Grid`, `scene.View` or `scene.Warp`, resolved into a
`GridTarget`, a `ViewTarget` or a `WarpTarget` --
knows the tiles it touches, its accumulators, how to query one tile's scene into them and how to finish them; the single calls take the
scenes from the cache tile by tile, `render_many` and `prefetch` from one walk over the union of the tiles (`scene_walk`), whose missing
scenes are built from batched trunk calls on `CiaoSR.trunk_ahead`.  Every function takes the restorer first."""
import torch

from . import hip_ops
from . import scene as sc


def q_plan(ph, pw, s):
    """The query count a scene of a ph x pw LR map is planned for: its full grid at scale `s` (include/ciaosr_hip.h, q_plan)."""
    return max(1, round(ph * s) * round(pw * s))


def _crop(x, b, origin, t):
    """Item b of the normalised batch, or its t x t tile at `origin`."""
    return x[b:b + 1] if origin is None else x[b:b + 1, :, origin[0]:origin[0] + t, origin[1]:origin[1] + t]


def encode(r, lq, options=None, max_scale=None, self_ensemble=None, budget_bytes=None):
    """`self_ensemble` (None: `test_cfg.self_ensemble`): with members, the ensemble record of `encode_ensemble`.  `budget_bytes`: the
    scene budget of this encode (None: `test_cfg.scene_cache_mb`, default 4096 MiB)."""
    ids = r.ensemble_ids(self_ensemble)
    if ids is not None:
        return encode_ensemble(r, lq, ids, options, max_scale)
    opt = r.options(options)
    x = r.normalize(lq)
    gen = r.generator
    if max_scale is None:
        max_scale = r.test_cfg.get('scale', None)
    tile = r.test_cfg.get('tile', None)
    t = min(tile, *x.shape[-2:]) if tile else None

    def build(key):
        patch = _crop(x, *key, t).contiguous()
        return gen.encode(patch, opt, q_plan=q_plan(*patch.shape[-2:], enc.max_scale))

    if budget_bytes is None:
        budget_bytes = _scene_budget(r)
    enc = sc.EncodedImage(x, opt, max_scale, int(budget_bytes), build, tile=t)
    if not tile and max_scale is not None:
        for b in range(x.shape[0]):
            enc.cache.get((b, None))
    return enc


def _scene_budget(r):
    return int(r.test_cfg.get('scene_cache_mb', None) or 4096) << 20


def encode_rgba(r, lq4, options=None, max_scale=None, self_ensemble=None):
    """`encode` of the two-item batch of an RGBA image [1, 4, h, w]: item 0 the colour as stored (not premultiplied), item 1 the alpha
    plane in all three channels; `enc.alpha` marks it for the renders.  Not with `self_ensemble` (ValueError)."""
    if isinstance(lq4, torch.Tensor) and lq4.dim() == 4 and lq4.shape[1] == 2:
        raise ValueError(f'encode_rgba expects one RGBA image [1, 4, h, w], got {tuple(lq4.shape)}: there is no grey + alpha encode '
                         f'(PNG colour type 4); repeat the grey channel three times, or drop the alpha and use encode_grey')
    if not isinstance(lq4, torch.Tensor) or lq4.dim() != 4 or lq4.shape[0] != 1 or lq4.shape[1] != 4:
        shape = tuple(lq4.shape) if isinstance(lq4, torch.Tensor) else type(lq4).__name__
        raise ValueError(f'encode_rgba expects one RGBA image [1, 4, h, w], got {shape}')
    if r.ensemble_ids(self_ensemble) is not None:
        raise ValueError('encode_rgba has no self-ensemble: encode the colour image with self_ensemble, or turn the option off')
    enc = encode(r, torch.cat([lq4[:, :3], lq4[:, 3:4].expand(-1, 3, -1, -1)], 0), options, max_scale, self_ensemble=False)
    enc.alpha = True
    return enc


def encode_grey(r, lq1, options=None, max_scale=None, self_ensemble=None):
    """`encode` of the colour image (v, v, v) of a grey batch [B, 1, h, w]; `enc.grey` marks it for the renders, which quantise to one
    byte per pixel with `as_u8` (`metrics_hip.tensor2img_grey_u8`).  The record may be an ensemble's."""
    if not isinstance(lq1, torch.Tensor) or lq1.dim() != 4 or lq1.shape[1] != 1:
        shape = tuple(lq1.shape) if isinstance(lq1, torch.Tensor) else type(lq1).__name__
        raise ValueError(f'encode_grey expects grey images [B, 1, h, w], got {shape}')
    enc = encode(r, lq1.expand(-1, 3, -1, -1).contiguous(), options, max_scale, self_ensemble)
    enc.grey = True
    return enc


# -- self-ensemble: one plain encode per member, renders averaged back --------------------------------------------------------------------
def encode_ensemble(r, lq, ids, options=None, max_scale=None):
    """scene.EnsembleEncoded of the members `ids`: member k is the plain `encode` of T_k(lq) (hip_ops.dihedral), each under an even
    share of the scene budget."""
    lq = lq.contiguous().float()
    budget = _scene_budget(r) // len(ids)
    members = [encode(r, hip_ops.dihedral(lq, k), options, max_scale, self_ensemble=False, budget_bytes=budget) for k in ids]
    return sc.EnsembleEncoded(ids, members, lq.shape[-2:])


def is_ensemble(enc):
    return isinstance(enc, sc.EnsembleEncoded)


def refuse_ensemble(enc, what):
    """ValueError, before any device work, for the calls an ensemble record does not serve."""
    if is_ensemble(enc):
        raise ValueError(f'{what} is not defined for a self-ensemble encode (members {enc.ids}): render grids with render / render_many, '
                         f'or encode without self_ensemble')


def render_ensemble(r, enc, targets, as_u8=False, many=False, as_u16=False):
    """The `scene.Grid` targets of an ensemble record: member k renders the `scene.dihedral_window` of each target from its own scenes
    (`many`: all of them in one `render_many` per member, else the single call), and the results are averaged back in member order by
    `hip_ops.dihedral_accum` into one fp32 accumulator per target -- bitwise the window of `restore(..., self_ensemble=enc.ids)`.
    Quantised once, after the mean, with `as_u8` or `as_u16`.  A `scene.View` is a ValueError."""
    check_quant(enc, as_u8, as_u16)
    targets = list(targets)
    if not targets:
        raise ValueError('no targets: give a list of scene.Grid')
    for tg in targets:
        if isinstance(tg, sc.View):
            refuse_ensemble(enc, 'a view')
        if isinstance(tg, sc.Warp):
            refuse_ensemble(enc, 'a warp')
        if not isinstance(tg, sc.Grid):
            raise TypeError(f'a target is a scene.Grid or a scene.View, got {type(tg).__name__}')
    h, w = enc.shape
    resolved = [tg.resolve(h, w) for tg in targets]                   # render's ValueErrors, before any device work
    n = len(enc.ids)
    accs = [None] * len(targets)
    for i, (k, member) in enumerate(zip(enc.ids, enc.members)):
        grids = []
        for ht, wt, win in resolved:
            ht_k, wt_k, win_k = sc.dihedral_window(k, ht, wt, win)
            grids.append(sc.Grid(size=(ht_k, wt_k), window=win_k))
        outs = render_many(r, member, grids) if many else [render_one(r, member, tg) for tg in resolve(r, member, grids)]
        for j, out in enumerate(outs):
            if accs[j] is None:
                accs[j] = torch.empty(*out.shape[:2], *resolved[j][2][2:], dtype=torch.float32, device=out.device)
            hip_ops.dihedral_accum(accs[j], out, k, first=(i == 0), divisor=float(n) if i == n - 1 else 0.0)
        del outs
    if as_u8 or as_u16:
        return [_quantise(acc, grey=is_grey(enc), u16=as_u16) for acc in accs]
    return accs


ALPHA_FILL = (0.0, 0.0, 0.0)                  # outside a view the alpha item is 0: transparent


def is_alpha(enc):
    """Whether `enc` is an `encode_rgba` result (any other record, a test's stand-in included, is not)."""
    return bool(getattr(enc, 'alpha', False))


def is_grey(enc):
    """Whether `enc` is an `encode_grey` result."""
    return bool(getattr(enc, 'grey', False))


def check_quant(enc, as_u8, as_u16):
    """ValueError, before any device work, for the sample types a render cannot have: both at once, or 16 bits with alpha."""
    if as_u8 and as_u16:
        raise ValueError('as_u8 and as_u16 together: a render is quantised once, to 8 or to 16 bits per sample')
    if as_u16 and is_alpha(enc):
        raise ValueError('as_u16 on an encode_rgba record: there is no 16-bit alpha (PNG colour type 6 at depth 16 is not built); '
                         'render with as_u8, or encode the colour image alone')


def _quantise(out, alpha=False, grey=False, u16=False):
    """The ONE place a render becomes bytes, after everything fp32 (the tile blend, the view fill, the self-ensemble mean): BGR, BGRA
    of the (colour, alpha) pair of an RGBA encode, or one grey byte per pixel of a grey encode.  `u16`: uint16 samples, BGR or grey
    (`metrics_hip.tensor2img_u16` / `tensor2img_grey_u16`; `check_quant` has refused alpha)."""
    from . import metrics_hip
    if u16:
        return metrics_hip.tensor2img_grey_u16(out) if grey else metrics_hip.tensor2img_u16(out)
    if grey:
        return metrics_hip.tensor2img_grey_u8(out)
    return metrics_hip.tensor2img_bgra_u8(out) if alpha else metrics_hip.tensor2img_u8(out)


def _finish(tg, r, enc, b, acc):
    """`tg.finish` of batch item b: the alpha item of an RGBA encode ends a view with ALPHA_FILL instead of the caller's fill."""
    if is_alpha(enc) and b == 1 and isinstance(tg, ViewTarget):
        return tg.finish(r, acc, ALPHA_FILL)
    return tg.finish(r, acc)


# -- targets ----------------------------------------------------------------------------------------------------------------------------
class GridTarget:
    """A resolved scene.Grid: the window `win` of the ht x wt grid.  `tiles`: index -> `scene.plan_window`'s record of every LR tile the
    window touches; None without `test_cfg.tile`, where the whole image is the one frame and `render_whole` is the render."""

    def __init__(self, cfg, h, w, ht, wt, win):
        self.ht, self.wt, self.win, self.size = ht, wt, win, (win[2], win[3])
        self.max_scale = max(ht / h, wt / w)
        self.tiles = None
        if cfg.get('tile', None):
            self.tiles = {t['index']: t for t in sc.plan_window(
                h, w, cfg.get('tile'), cfg.get('tile_overlap', None), ht, wt, win, scale=cfg.get('scale', None),
                any_scale=bool(cfg.get('tile_any_scale', False)))}

    def touched(self):
        """{tile index: origin}, row-major: the reference's blend order."""
        return {0: None} if self.tiles is None else {k: (t['y0'], t['x0']) for k, t in self.tiles.items()}

    def render_whole(self, r, enc):
        """The render where `tiles` is None: a scene's prediction of the window's grid is the window, nothing is blended; the items of
        a batch share the coordinates."""
        wi0, wj0, wh, ww = self.win
        coord, cell = hip_ops.make_coord_cell_window(self.ht, self.wt, wi0, wi0 + wh, wj0, wj0 + ww, enc.x.device)
        return [hip_ops.denorm_clamp(r.generator.render(enc.cache.get((b, None)), coord, cell)[0].contiguous(), wh, ww, r.rgb_mean, r.rgb_std)
                for b in range(enc.x.shape[0])]

    def alloc(self, device):
        E = torch.zeros(3, *self.size, dtype=torch.float32, device=device)
        return E, torch.zeros_like(E)

    def query(self, gen, k, tile_scene, acc):
        """Tile k's part of the window from its scene, blended into `acc`.  Coordinates are made right before the query that reads them
        (the 16-bit head's grid-width hint is kept for the last 64 coordinate tensors only)."""
        t = self.tiles[k]
        gh, gw, r0, r1, c0, c1, frame = t['grid']
        coord, cell = hip_ops.make_coord_cell_window(gh, gw, r0, r1, c0, c1, tile_scene.x.device, frame)
        out = gen.render(tile_scene, coord, cell)[0]
        hip_ops.tile_blend(*acc, out, t['a0'] - self.win[0], t['b0'] - self.win[1], t['a1'] - t['a0'], t['b1'] - t['b0'])

    def finish(self, r, acc):
        return hip_ops.denorm_clamp(hip_ops.tile_finalize(*acc).contiguous(), *self.size, r.rgb_mean, r.rgb_std)


class ViewTarget:
    """A resolved scene.View: matrix `m`, output `size`, `fill`, and the frames (y0, x0, th, tw) its queries are sorted into.  `count`
    (or `count_views`, for many at once) gives it `counts`, the members per frame, `n_blocks` (the live 4 x 2 blocks per frame where
    the member lists are selected in blocks, `view_blocks`; else None) and `ws`, the count's workspace for the select."""

    def __init__(self, cfg, m, size, fill, frames):
        self.m, self.size, self.fill, self.frames = m, size, fill, frames
        self.max_scale = sc.view_max_scale(m)
        self.tiled = bool(cfg.get('tile', None))
        self.counts = self.n_blocks = self.ws = None

    def count(self, r, enc):
        """Count this view alone: the ONE device-to-host copy, and the only synchronisation, of a single view render of a batch item."""
        hv, wv = self.size
        if view_blocks(r, enc, self.m, self.frames):                    # per tile (members, live blocks of 4 x 2 output pixels)
            counts, self.ws = hip_ops.view_count_blocks(self.m, hv, wv, _view_tiles(enc, self.frames))
            both = counts.tolist()
            self.counts, self.n_blocks = [n for n, _ in both], [n_blk for _, n_blk in both]
        else:
            counts, self.ws = hip_ops.view_count(self.m, hv, wv, _view_tiles(enc, self.frames))
            self.counts = counts.tolist()

    def touched(self):
        """{frame index: origin} of the frames with a member, row-major: a frame without one is neither built nor queried."""
        return {k: ((f[0], f[1]) if self.tiled else None) for k, (f, n) in enumerate(zip(self.frames, self.counts)) if n}

    def alloc(self, device):
        n_q = self.size[0] * self.size[1]
        return torch.zeros(3, n_q, dtype=torch.float32, device=device), torch.zeros(n_q, dtype=torch.float32, device=device)

    def query(self, gen, k, tile_scene, acc):
        """Frame k's members from its scene, blended into `acc`."""
        (hv, wv), m, frame, n = self.size, self.m, self.frames[k], self.counts[k]
        if n == hv * wv:                                                # the tile owns the whole view: a grid, known to the head as one
            q_index = None
            coord, cell = hip_ops.make_coord_cell_view(m, hv, wv, frame, tile_scene.x.device)
        elif self.n_blocks is not None:                                 # row tiles of the chained 16-bit kernel, pads at q_index -1
            q_index, coord, cell = hip_ops.view_select_blocks(m, hv, wv, frame, k, len(self.frames), self.ws, self.n_blocks[k])
        else:
            q_index, coord, cell = hip_ops.view_select(m, hv, wv, frame, k, len(self.frames), self.ws, n)
        hip_ops.view_blend(*acc, q_index, gen.render(tile_scene, coord, cell)[0])

    def finish(self, r, acc, fill=None):
        """`fill`: the item's own (None: the view's)."""
        fill = self.fill if fill is None else fill
        return hip_ops.denorm_clamp(hip_ops.view_finalize(*acc, fill, r.rgb_mean, r.rgb_std), *self.size, r.rgb_mean, r.rgb_std)


class WarpTarget(ViewTarget):
    """A resolved scene.Warp: its point source -- the homography `h` (nine numbers) or the device map `map` [hv, wv, 2] float64, the other
    None --, the `footprint`, output `size`, `fill` and the frames.  Everything after the LR position is the view's: `touched`, `alloc` and
    `finish` are ViewTarget's own.  `test_cfg.view_blocks` is ignored: a cut warp's member lists stay in index order.  A per-pixel warp
    (`footprint` a `scene.PerPixel`, kept as `pp`) runs the per-pixel count / select / coordinate entries and queries the head with
    chunk = 1: the shift radius of a query comes from its own cell.  An area-sampled warp (`pp.samples` = max_samples, `area`) counts
    SAMPLES: the count's copy carries `n_samples` = S and the number of one-sample pixels beside the tiles' counts.  Where every pixel has
    exactly one sample (`supersampled` False) the samples are the pixels and it runs as the per-pixel warp it is; else its accumulators
    are S wide, every touched tile is answered as a list of samples, and `finish` is the resolve that averages them."""

    def __init__(self, cfg, h, map_, size, footprint, fill, frames):
        self.h, self.footprint, self.size, self.fill, self.frames = h, footprint, size, fill, frames
        # a float32 map is widened exactly; the kernels read one aligned 16-byte (y_lr, x_lr) pair per query
        self.map = None if map_ is None else map_.detach().to(torch.float64).contiguous()
        self.pp = None
        self.area = False
        if isinstance(footprint, sc.PerPixel):
            tensor = None if footprint.tensor is None else footprint.tensor.detach().to(torch.float64).contiguous()
            self.pp = sc.PerPixel(footprint.mode, footprint.range, tensor, footprint.samples)
            self.area = bool(footprint.samples)
            self.max_scale = 1.0 / footprint.range[0]
        else:
            self.max_scale = sc.warp_max_scale(footprint)
        self.tiled = bool(cfg.get('tile', None))
        self.counts = self.n_blocks = self.ws = None
        self.n_samples, self.supersampled = None, False

    def n_counts(self):
        """How many numbers the count of this warp adds to the copy."""
        return len(self.frames) + (2 if self.area else 0)

    def workspace_bytes(self):
        n_t = len(self.frames)
        if self.area:
            return hip_ops.warp_area_workspace_bytes(*self.size, n_t, self.pp.samples)
        return hip_ops.warp_workspace_bytes(*self.size, n_t)

    def take_counts(self, counts):
        """`counts`: the `n_counts()` numbers of this warp, on the host."""
        n_t = len(self.frames)
        self.counts = counts[:n_t]
        if self.area:
            self.n_samples = counts[n_t]
            self.supersampled = counts[n_t + 1] != self.size[0] * self.size[1]

    def count(self, r, enc):
        """Count this warp alone: the ONE device-to-host copy, and the only synchronisation, of a single warp render of a batch item."""
        self.take_counts(self.launch_count(enc).tolist())

    def launch_count(self, enc, ws=None):
        """The count launches without the copy: -> the counts on the device (`render_many` copies every target's at once)."""
        if self.area:
            counts, self.ws = hip_ops.warp_area_count(self.h, self.pp, *self.size, _view_tiles(enc, self.frames), ws)
            return counts
        if self.pp is not None:
            counts, self.ws = hip_ops.warp_pp_count(self.h, self.map, self.pp, *self.size, _view_tiles(enc, self.frames), ws)
        else:
            counts, self.ws = hip_ops.warp_count(self.h, self.map, self.footprint, *self.size, _view_tiles(enc, self.frames), ws)
        return counts

    def query(self, gen, k, tile_scene, acc):
        """Frame k's members from its scene, blended into `acc`."""
        (hv, wv), frame, n = self.size, self.frames[k], self.counts[k]
        if self.pp is not None:
            if n == hv * wv and not self.supersampled:                  # every query is a member, so every query has a footprint
                q_index = None
                coord, cell = hip_ops.make_coord_cell_warp_pp(self.h, self.map, self.pp, hv, wv, frame, tile_scene.x.device)
            elif self.area:                                             # samples in increasing id (the pixels' own where none is split)
                q_index, coord, cell = hip_ops.warp_area_select(self.h, self.pp.samples, hv, wv, frame, k, len(self.frames), self.ws,
                                                                self.n_samples, n)
            else:
                q_index, coord, cell = hip_ops.warp_pp_select(self.h, self.map, self.pp, hv, wv, frame, k, len(self.frames), self.ws, n)
            hip_ops.view_blend(*acc, q_index, gen.render(tile_scene, coord, cell, chunk=1)[0])
            return
        if n == hv * wv:                                                # the frame owns every query: a grid, known to the head as one
            q_index = None
            coord, cell = hip_ops.make_coord_cell_warp(self.h, self.map, self.footprint, hv, wv, frame, tile_scene.x.device)
        else:
            q_index, coord, cell = hip_ops.warp_select(self.h, self.map, self.footprint, hv, wv, frame, k, len(self.frames), self.ws, n)
        hip_ops.view_blend(*acc, q_index, gen.render(tile_scene, coord, cell)[0])

    def alloc(self, device):
        """One accumulator column per query; per SAMPLE where the warp is supersampled (one column where it has no sample at all)."""
        if not self.supersampled:
            return super().alloc(device)
        n_s = max(self.n_samples, 1)
        return torch.zeros(3, n_s, dtype=torch.float32, device=device), torch.zeros(n_s, dtype=torch.float32, device=device)

    def finish(self, r, acc, fill=None):
        if not self.supersampled:
            return super().finish(r, acc, fill)
        fill = self.fill if fill is None else fill
        return hip_ops.warp_area_resolve(*acc, self.n_samples, self.pp.samples, *self.size, len(self.frames), self.ws, fill,
                                         r.rgb_mean, r.rgb_std)


def view_blocks(r, enc, m, frames):
    """Whether the partial member lists of view `m` are selected in 4 x 2 blocks (`hip_ops.view_select_blocks`): `test_cfg.view_blocks`
    is on, `scene.view_blocks_fit(m)` holds, and the route the tile scenes are planned under runs the chained 16-bit kv kernel --
    the one kernel that walks 8 consecutive list entries as a row tile.  Elsewhere (fp32, f16x3, bf16x3, `head_route` bits that
    disable the chain) the pads would only cost queries and the index-order list stays.  Pure host work; needs `enc.max_scale`."""
    if not r.test_cfg.get('view_blocks', False) or not sc.view_blocks_fit(m):
        return False
    th, tw = frames[0][2], frames[0][3]                                 # every frame has the first one's size
    return r.generator.scene_chained(th, tw, q_plan(th, tw, enc.max_scale), enc.options)


def _view_tiles(enc, frames):
    if enc.view_tiles is None:                                          # uploaded once per encoded image, not per view
        enc.view_tiles = torch.tensor(frames, dtype=torch.int32).to(enc.x.device)
    return enc.view_tiles


def count_views(r, enc, views, warps=()):
    """`ViewTarget.count` for ALL views of a `render_many` / `prefetch` in one `view_count_many` (and one `view_count_blocks_many` for
    those selected in blocks) and one device-to-host copy -- per call, not per batch item: the counts do not depend on the item.
    `warps`: each is counted by its own launches, into its own part of one workspace, and its counts ride in the same copy -- behind
    them, for an area-sampled warp, its number of samples S and of one-sample pixels (`WarpTarget.take_counts`)."""
    frames = (list(views) + list(warps))[0].frames                      # the image's: the same for every view and warp
    n_t = len(frames)
    plain, blk = [], []
    for v in views:
        (blk if view_blocks(r, enc, v.m, frames) else plain).append(v)
    flat = []
    for group, count in ((plain, hip_ops.view_count_many), (blk, hip_ops.view_count_blocks_many)):
        if group:
            counts, ws, offsets = count([v.m for v in group], [v.size for v in group], _view_tiles(enc, frames))
            flat.append(counts.flatten())
            for v, off in zip(group, offsets):
                v.ws = ws[off:]
    if warps:
        sizes = [(wp.workspace_bytes() + 255) & ~255 for wp in warps]
        ws = hip_ops.workspace(sum(sizes), enc.x.device, slot='warp_many')
        off = 0
        for wp, nbytes in zip(warps, sizes):
            flat.append(wp.launch_count(enc, ws[off:off + nbytes]))
            off += nbytes
    flat = (flat[0] if len(flat) == 1 else torch.cat(flat)).tolist()    # the one synchronisation of the call
    for i, v in enumerate(plain):
        v.counts = flat[i * n_t:(i + 1) * n_t]
    base = len(plain) * n_t
    for i, v in enumerate(blk):                                         # per tile (members, live blocks of 4 x 2 output pixels)
        both = flat[base + 2 * i * n_t:base + 2 * (i + 1) * n_t]
        v.counts, v.n_blocks = both[0::2], both[1::2]
    base += 2 * len(blk) * n_t
    for wp in warps:                                                    # an area-sampled warp's S rides behind its tiles' counts
        wp.take_counts(flat[base:base + wp.n_counts()])
        base += wp.n_counts()


def resolve(r, enc, targets):
    """`scene.Grid` / `scene.View` records -> GridTarget / ViewTarget, with the single calls' ValueErrors, before any device work; sets
    `enc.max_scale` where it is open: the largest any target needs."""
    cfg = r.test_cfg
    h, w = enc.x.shape[-2:]
    tile, overlap, any_scale = cfg.get('tile', None), cfg.get('tile_overlap', None), bool(cfg.get('tile_any_scale', False))
    targets = list(targets)
    if not targets:
        raise ValueError('no targets: give a list of scene.Grid / scene.View')
    out = []
    for tg in targets:
        if isinstance(tg, sc.Grid):
            out.append(GridTarget(cfg, h, w, *tg.resolve(h, w)))
        elif isinstance(tg, sc.View):
            out.append(ViewTarget(cfg, *tg.resolve(h, w, tile, overlap, any_scale)))
        elif isinstance(tg, sc.Warp):
            default = enc.max_scale if enc.max_scale is not None else cfg.get('scale', None)    # what `encode` would default it to
            out.append(WarpTarget(cfg, *tg.resolve(h, w, tile, overlap, any_scale, max_scale=default)))
        else:
            raise TypeError(f'a target is a scene.Grid, a scene.View or a scene.Warp, got {type(tg).__name__}')
    if enc.max_scale is None:
        enc.max_scale = max(tg.max_scale for tg in out)
    return out


def _stacked(outs, as_u8, alpha=False, grey=False, as_u16=False):
    """The items' outputs as one tensor; with `as_u8` the 8-bit image, with `as_u16` the 16-bit one (`_quantise`)."""
    out = torch.stack(outs)
    return _quantise(out, alpha, grey, bool(as_u16)) if (as_u8 or as_u16) else out


# -- one target: scenes from the cache, tile by tile ------------------------------------------------------------------------------------
def render_one(r, enc, tg, as_u8=False, as_u16=False):
    """The single calls `render` / `render_view`, of a resolved target: per batch item, every scene taken with `enc.cache.get` when its
    tile's turn comes -- no walk, no batched trunk, no side stream."""
    if isinstance(tg, GridTarget) and tg.tiles is None:
        return _stacked(tg.render_whole(r, enc), as_u8, is_alpha(enc), is_grey(enc), as_u16)
    outs = []
    for b in range(enc.x.shape[0]):
        if isinstance(tg, ViewTarget):
            tg.count(r, enc)
        acc = tg.alloc(enc.x.device)
        for k, origin in tg.touched().items():
            tg.query(r.generator, k, enc.cache.get((b, origin)), acc)
        outs.append(_finish(tg, r, enc, b, acc))
    return _stacked(outs, as_u8, is_alpha(enc), is_grey(enc), as_u16)


# -- many targets from one walk over the tile scenes ------------------------------------------------------------------------------------
def plan_many(r, enc, targets):
    """Everything `render_many` / `prefetch` know before a scene is touched: -> (the resolved targets, walk, users).  walk: the union
    of the tiles the targets touch as [(tile index, origin)], row-major; users[tile index]: the targets that touch it, in list order."""
    tgs = resolve(r, enc, targets)
    warps = [tg for tg in tgs if isinstance(tg, WarpTarget)]
    views = [tg for tg in tgs if isinstance(tg, ViewTarget) and not isinstance(tg, WarpTarget)]
    if views or warps:
        count_views(r, enc, views, warps)
    origins = {}
    for tg in tgs:
        origins.update(tg.touched())
    union, users = sc.plan_union([list(tg.touched()) for tg in tgs])
    return tgs, [(k, origins[k]) for k in union], users


def scene_walk(r, enc, b, tiles):
    """Yield (tile index, scene) for `tiles`, a list of (tile index, origin), of batch item b, in order, each scene taken from the cache
    once.  The tiles missing from the cache are encoded in groups: `tile_batch()` tiles per trunk call (`encode_trunk` on the stacked
    patches) where the tile loops feed this trunk batches, else one; with `test_cfg.encoder_ahead` (default on) the next group's trunk
    runs on the side stream under the current group's prepares and queries (`CiaoSR.trunk_ahead`).  A scene is prepared from its
    feature map right before it is yielded; only a group's feature maps are held, never its scenes."""
    from .restorer import effective_options, trunk_batches           # (restorer.py imports this module)
    gen, cache, x, opt = r.generator, enc.cache, enc.x, enc.options
    batches = bool(enc.tile and trunk_batches(gen, opt))
    origin_of = dict(tiles)
    order = [k for k, _ in tiles]
    key_of = {k: (b, origin_of[k]) for k in order}
    groups = sc.group_missing(order, {k for k in order if key_of[k] in cache.entries}, r.tile_batch(opt) if batches else 1)
    where = {k: (g, j) for g, group in enumerate(groups) for j, k in enumerate(group)}
    eff = effective_options(gen, opt)
    ahead = bool(r.test_cfg.get('encoder_ahead', True) and len(groups) > 1 and x.is_cuda and batches)
    trunks = r.trunk_ahead(groups, lambda group: gen.encode_trunk(
        torch.cat([_crop(x, b, origin_of[k], enc.tile) for k in group], 0).contiguous(), opt)[:2], ahead, opt, x.device)
    g_ready, ready = -1, None                     # the group in use and its (patches, feats)
    cache.hold = set(key_of.values())
    try:
        for k in order:
            key = key_of[k]
            cache.hold.discard(key)
            if k not in where or key in cache.entries:
                yield k, cache.get(key)           # cached (a held entry the budget pushed out all the same is rebuilt on its own)
                continue
            g, j = where[k]
            if g != g_ready:
                ready = None                      # the group before is done: its feature maps go before the next trunk is launched
                g_ready, ready = g, next(trunks)
            cache.make_room()                 # (`ready` alone names the group's patches and feature maps: they go with it)
            scene = gen.encode_scenes(ready[0][j:j + 1], [ready[1][j]], eff, q_plan=q_plan(*ready[0].shape[-2:], enc.max_scale))
            yield k, cache.put(key, scene)
    finally:
        cache.hold = set()
        trunks.close()


def render_many(r, enc, targets, as_u8=False, as_u16=False):
    check_quant(enc, as_u8, as_u16)
    if is_ensemble(enc):
        return render_ensemble(r, enc, targets, as_u8, many=True, as_u16=as_u16)
    x = enc.x
    if not enc.tile or tuple(x.shape[-2:]) == (enc.tile, enc.tile):     # one frame: no schedule to make
        return [render_one(r, enc, tg, as_u8, as_u16) for tg in resolve(r, enc, targets)]
    tgs, walk, users = plan_many(r, enc, targets)
    outs = [[] for _ in tgs]
    for b in range(x.shape[0]):
        acc = [tg.alloc(x.device) for tg in tgs]
        for k, tile_scene in scene_walk(r, enc, b, walk):
            for i in users[k]:
                tgs[i].query(r.generator, k, tile_scene, acc[i])
        for i, tg in enumerate(tgs):
            outs[i].append(_finish(tg, r, enc, b, acc[i]))
    return [_stacked(o, as_u8, is_alpha(enc), is_grey(enc), as_u16) for o in outs]


def prefetch(r, enc, targets):
    refuse_ensemble(enc, 'prefetch')
    _, walk, _ = plan_many(r, enc, targets)
    cache = enc.cache
    built = 0
    for b in range(enc.x.shape[0]):
        missing = [(k, origin) for k, origin in walk if (b, origin) not in cache.entries]
        if missing and cache.room() is None:                            # the size of a scene is not known yet: the first one tells
            built += sum(1 for _ in scene_walk(r, enc, b, missing[:1]))
            missing = missing[1:]
        built += sum(1 for _ in scene_walk(r, enc, b, missing[:cache.room() or 0]))
        if cache.room() == 0:
            break
    return built


# -- every level of a tile pyramid (pyramid.py) -----------------------------------------------------------------------------------------
def plan_pyramid(r, enc, size=None, scale=None):
    """The level sizes of `render_pyramid` and the index of the smallest model level; its ValueErrors.  Pure host work."""
    from . import pyramid
    refuse_ensemble(enc, 'render_pyramid')
    nb, _, h, w = enc.x.shape
    if nb != (2 if is_alpha(enc) else 1):
        raise ValueError(f'render_pyramid takes one image, got a batch of {nb}')
    ht, wt = sc.target_size(h, w, size, scale)
    if ht < h or wt < w:
        raise ValueError(f'the top level {ht} x {wt} is smaller than the LR image {h} x {w}: the model renders no scale below 1')
    if r.test_cfg.get('tile', None) and not r.test_cfg.get('tile_any_scale', False):
        raise ValueError('render_pyramid with test_cfg.tile needs test_cfg.tile_any_scale: the levels are not the integer-scale '
                         'rectangles of clip_test')
    sizes = pyramid.level_sizes(ht, wt)
    return sizes, min(k for k, (hl, wl) in enumerate(sizes) if hl >= h and wl >= w)


def render_pyramid(r, enc, size=None, scale=None, as_u16=False):
    from . import degrade
    if as_u16:
        return render_pyramid_u16(r, enc, size, scale)
    sizes, first = plan_pyramid(r, enc, size, scale)
    model_levels = render_many(r, enc, [sc.Grid(size=s) for s in sizes[first:]], as_u8=True)
    base = model_levels[0]
    if is_grey(enc):
        # Pillow's resize of an L image is every channel of its resize of (v, v, v): the three-channel resampler on the replicated
        # level, reduced back (a neutral pixel's grey byte is its value)
        from . import metrics_hip
        wide = base.unsqueeze(2).expand(-1, -1, 3).contiguous()
        return [metrics_hip.grey_from_bgr_u8(degrade.resize_bicubic_u8(wide, (wl, hl))) for hl, wl in sizes[:first]] + list(model_levels)
    if not is_alpha(enc):
        return [degrade.resize_bicubic_u8(base, (wl, hl)) for hl, wl in sizes[:first]] + list(model_levels)
    # RGBA: colour and alpha are resized on their own (Pillow's resize of the RGB image and of the A band, NOT its premultiplied
    # resize of an RGBA image), then packed
    from . import metrics_hip
    colour, grey = base[:, :, :3].contiguous(), base[:, :, 3:4].expand(-1, -1, 3).contiguous()
    small = [metrics_hip.pack_bgra_u8(degrade.resize_bicubic_u8(colour, (wl, hl)), degrade.resize_bicubic_u8(grey, (wl, hl)))
             for hl, wl in sizes[:first]]
    return small + list(model_levels)



def render_pyramid_u16(r, enc, size=None, scale=None):
    """`render_pyramid` with 16-bit samples: the model levels are the `as_u16` targets of the one `render_many`; below the LR size every
    level is the integer box halving (`tiff_hip.halve_box_u16`) of the level above, a chain that starts at the smallest model level."""
    from . import tiff_hip
    check_quant(enc, False, True)                                       # an RGBA record: no 16-bit alpha, before any device work
    sizes, first = plan_pyramid(r, enc, size, scale)
    model_levels = list(render_many(r, enc, [sc.Grid(size=s) for s in sizes[first:]], as_u16=True))
    small = []
    for _ in sizes[:first]:
        small.append(tiff_hip.halve_box_u16(small[-1] if small else model_levels[0]))
    return small[::-1] + model_levels
