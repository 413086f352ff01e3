"""Deep Zoom tile pyramids (`<name>.dzi` + `<name>_files/<level>/<col>_<row>.png`, as OpenSeadragon and libvips read them) of an encoded
scene.  The plan and the manifest are pure host code; `write_dzi` renders every level with `CiaoSR.render_pyramid` -- the levels at or
above the LR size are the model's own answer at that size, all from one walk over the tile scenes -- and codes each level's tiles with
ONE `png_hip.encode_png_tiles` call: two synchronising copies per level, whatever its number of tiles.  `fmt='jpg'` writes
`<col>_<row>.jpg` tiles through one `jpeg_hip.encode_jpeg_tiles` call per level instead, and `Format="jpg"` in the manifest.  The levels
of an RGBA encode (`CiaoSR.encode_rgba`) are uint8 [H_l, W_l, 4] images and become RGBA PNG tiles under the same manifest; JPEG has no
alpha, so `fmt='jpg'` refuses them.  The levels of a grey encode (`CiaoSR.encode_grey`) are uint8 [H_l, W_l] images and become grey
PNG tiles (colour type 0) or one-component JPEG tiles -- not progressive ones -- under the same manifest.

Deep Zoom's rules: Lmax = ceil(log2(max(W, H))), levels 0..Lmax; level L is max(1, ceil(W / 2^(Lmax - L))) wide and as high by the same
rule; on a level, column c spans [c T - (O if c > 0 else 0), min((c + 1) T + O, Wl)) for the tile size T and the overlap O, rows alike,
ceil(Wl / T) columns.

`write_tiff` writes the same render as ONE pyramidal tiled TIFF instead (tiff_hip.py: an image file directory per level, deflate tiles
with the horizontal predictor, 8 or 16 bits per sample); `write_dzi`, `write_levels` and `FORMATS` do not know of it.
"""
import os
import time

DZI_NS = 'http://schemas.microsoft.com/deepzoom/2008'


def level_sizes(height, width):
    """[(H_l, W_l)] of the levels 0..Lmax of a height x width image."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f'empty image {height} x {width}')
    lmax = (max(width, height) - 1).bit_length()                # ceil(log2(.)), exact in integers
    return [(max(1, (height + (1 << k) - 1) >> k), max(1, (width + (1 << k) - 1) >> k)) for k in range(lmax, -1, -1)]


def _check_tiling(tile_size, overlap):
    if int(tile_size) != tile_size or int(overlap) != overlap:
        raise ValueError(f'tile_size={tile_size!r} and overlap={overlap!r} are whole pixels')
    tile_size, overlap = int(tile_size), int(overlap)
    if tile_size < 1 or overlap < 0 or overlap >= tile_size:
        raise ValueError(f'tile_size={tile_size}, overlap={overlap}: need tile_size >= 1 and 0 <= overlap < tile_size')
    return tile_size, overlap


def spans(n, tile_size, overlap):
    """[(start, length)] of the columns (or rows) of a level n pixels wide (high)."""
    return [(c * tile_size - (overlap if c > 0 else 0),
             min((c + 1) * tile_size + overlap, n) - (c * tile_size - (overlap if c > 0 else 0)))
            for c in range(-(-n // tile_size))]


def dzi_plan(height, width, tile_size=254, overlap=1):
    """The levels of a height x width image, level 0 (1 x 1) first: [dict(level, height, width, tiles)], tiles = [(col, row, y0, x0, h, w)]
    row-major."""
    tile_size, overlap = _check_tiling(tile_size, overlap)
    plan = []
    for level, (hl, wl) in enumerate(level_sizes(height, width)):
        cols, rows = spans(wl, tile_size, overlap), spans(hl, tile_size, overlap)
        tiles = [(c, r, y0, x0, h, w) for r, (y0, h) in enumerate(rows) for c, (x0, w) in enumerate(cols)]
        plan.append(dict(level=level, height=hl, width=wl, tiles=tiles))
    return plan


FORMATS = ('png', 'jpg')


def _check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be 'png' or 'jpg', got {fmt!r}")
    return fmt


def _check_matches(matches, fmt):
    if not isinstance(matches, bool):
        raise ValueError(f'matches must be True or False, got {matches!r}')
    if matches and _check_format(fmt) == 'jpg':
        raise ValueError("matches=True is the PNG coder's option: not with fmt='jpg'")
    return matches


def dzi_manifest(height, width, tile_size=254, overlap=1, fmt='png'):
    """The `.dzi` file's XML for a height x width top level whose tiles are `fmt` files."""
    tile_size, overlap = _check_tiling(tile_size, overlap)
    _check_format(fmt)
    if int(height) < 1 or int(width) < 1:
        raise ValueError(f'empty image {height} x {width}')
    return (f'<?xml version="1.0" encoding="UTF-8"?><Image xmlns="{DZI_NS}" Format="{fmt}" Overlap="{overlap}" TileSize="{tile_size}">'
            f'<Size Width="{int(width)}" Height="{int(height)}"/></Image>')


def write_levels(levels, out_dir, name, tile_size=254, overlap=1, order='bgr', fmt='png', quality=90, subsampling='444', optimize=False,
                 progressive=False, matches=False):
    """Write the pyramid whose levels are the uint8 [H_l, W_l, 3] device images `levels` (level 0 first, as `CiaoSR.render_pyramid`
    returns them): one `encode_png_tiles` call per level, or for `fmt='jpg'` one `encode_jpeg_tiles` call with `quality` and
    `subsampling` (`optimize=True`: every tile with Huffman tables of its own; `progressive=True`: every tile a progressive file).
    Two-dimensional levels ([H_l, W_l], grey) are written as grey PNG tiles (`matches` too) or, with `fmt='jpg'`, as one-component
    JPEG tiles (`optimize` too; `progressive=True` or a `subsampling` other than '444' is a ValueError before any device work).
    Four-channel levels ([H_l, W_l, 4], bytes B G R A for `order` 'bgr' / 'bgra', R G B A for 'rgb' / 'rgba') are written as RGBA PNG
    tiles; with `fmt='jpg'` they are a ValueError before any device work.  `matches=True` (only `fmt='png'`, else a ValueError): the
    tiles are coded with `encode_png_tiles(..., matches=True)` -- flat and transparent tiles get far smaller, none gets larger.
    -> dict(files, bytes, encode_s, write_s); the manifest counts as a file."""
    _check_matches(matches, fmt)
    rgba = any(getattr(im, 'dim', lambda: 0)() == 3 and im.shape[2] == 4 for im in levels)
    if rgba:
        if _check_format(fmt) == 'jpg':
            raise ValueError("fmt='jpg' cannot hold the alpha channel of four-channel levels: write them with fmt='png'")
        order = {'bgr': 'bgra', 'rgb': 'rgba'}.get(order, order)
    grey = any(getattr(im, 'dim', lambda: 0)() == 2 for im in levels)
    if grey:
        if not all(getattr(im, 'dim', lambda: 0)() == 2 for im in levels):
            raise ValueError('grey [H_l, W_l] levels and colour levels do not mix in one pyramid')
        if order not in ('bgr', 'grey'):
            raise ValueError(f"order of grey [H_l, W_l] levels stays at its default or is 'grey', got {order!r}")
        order = 'grey'
    if _check_format(fmt) == 'jpg':
        from .jpeg_hip import check_optimize, check_params, check_progressive, encode_jpeg_tiles
        check_params(quality, subsampling)
        coding = dict(optimize=True) if check_optimize(optimize) else {}       # without it encode_jpeg_tiles is called as before
        if check_progressive(progressive):
            coding['progressive'] = True
        if grey and (progressive or subsampling != '444'):
            raise ValueError("grey levels have no progressive JPEG form and no subsampling: progressive=False, subsampling='444'")

        def encode(img, rects):
            return encode_jpeg_tiles(img, rects, quality=quality, subsampling=subsampling, order=order, **coding)
    else:
        from .png_hip import encode_png_tiles
        lz = dict(matches=True) if matches else {}                             # without it encode_png_tiles is called as before

        def encode(img, rects):
            return encode_png_tiles(img, rects, order=order, **lz)
    top = levels[-1]
    plan = dzi_plan(top.shape[0], top.shape[1], tile_size, overlap)
    if [(lv['height'], lv['width']) for lv in plan] != [(im.shape[0], im.shape[1]) for im in levels]:
        raise ValueError(f'the images are not the levels of a {top.shape[0]} x {top.shape[1]} pyramid')
    manifest = dzi_manifest(top.shape[0], top.shape[1], tile_size, overlap, fmt).encode()
    os.makedirs(out_dir, exist_ok=True)
    files, nbytes, t_enc, t_write = 1, len(manifest), 0.0, 0.0
    with open(os.path.join(out_dir, f'{name}.dzi'), 'wb') as f:
        f.write(manifest)
    for lv, img in zip(plan, levels):
        t0 = time.perf_counter()
        pngs = encode(img, [t[2:] for t in lv['tiles']])
        t1 = time.perf_counter()
        folder = os.path.join(out_dir, f'{name}_files', str(lv['level']))
        os.makedirs(folder, exist_ok=True)
        for (col, row, *_), data in zip(lv['tiles'], pngs):
            with open(os.path.join(folder, f'{col}_{row}.{fmt}'), 'wb') as f:
                f.write(data)
            nbytes += len(data)
        files += len(pngs)
        t_enc += t1 - t0
        t_write += time.perf_counter() - t1
    return dict(files=files, bytes=nbytes, encode_s=t_enc, write_s=t_write)


def write_dzi(model, enc, out_dir, name, scale=None, size=None, tile_size=254, overlap=1, order='bgr', fmt='png', quality=90,
              subsampling='444', optimize=False, progressive=False, matches=False):
    """`<out_dir>/<name>.dzi` and `<out_dir>/<name>_files/<level>/<col>_<row>.png` of the `size` / `scale` render of `enc` (an
    `encode` result of `model`).  `order`: the byte order of the rendered images, 'bgr' as `render_pyramid` makes them.  `fmt='jpg'`:
    `.jpg` tiles at `quality` (1..100) and `subsampling` ('444' or '420'), byte for byte Pillow's files of the same pixels; with
    `optimize=True` Pillow's `optimize=True` files (per-tile Huffman tables; the manifest is the same), with `progressive=True` Pillow's
    `progressive=True` files (the manifest is the same).  `matches=True` (only `fmt='png'`): the match coder of png_hip for every tile.
    -> dict: levels [(H_l, W_l)], model_levels (the levels rendered by the model; the ones below are Pillow-exact bicubic resizes of
    the smallest of them), files, bytes, and the seconds spent in render_s (to the last launch, not synchronised), encode_s, write_s."""
    _check_tiling(tile_size, overlap)
    _check_matches(matches, fmt)
    if _check_format(fmt) == 'jpg' and getattr(enc, 'alpha', False):
        raise ValueError("fmt='jpg' cannot hold the alpha channel of an RGBA encode: write the pyramid with fmt='png'")
    if _check_format(fmt) == 'jpg':
        from .jpeg_hip import check_optimize, check_params, check_progressive
        check_params(quality, subsampling)
        check_optimize(optimize)
        check_progressive(progressive)
        if getattr(enc, 'grey', False) and (progressive or subsampling != '444'):
            raise ValueError("a grey encode has no progressive JPEG form and no subsampling: progressive=False, subsampling='444'")
    t0 = time.perf_counter()
    levels = model.render_pyramid(enc, size=size, scale=scale)
    render_s = time.perf_counter() - t0
    h, w = enc.x.shape[-2:]
    sizes = [(im.shape[0], im.shape[1]) for im in levels]
    coding = dict(progressive=True) if progressive else {}                     # without it write_levels is called as before
    if matches:
        coding['matches'] = True
    res = write_levels(levels, out_dir, name, tile_size, overlap, order, fmt, quality, subsampling, optimize, **coding)
    res.update(levels=sizes, model_levels=[k for k, (hl, wl) in enumerate(sizes) if hl >= h and wl >= w], render_s=render_s)
    return res


def check_tiff(enc, tile=256, depth=8, matches=False):
    """The ValueErrors of `write_tiff`, before any device work: the tile rule, a depth other than 8 or 16, 16 bits on an
    `encode_rgba` record, a record that is grey AND alpha, a non-bool `matches`, an ensemble record."""
    from . import tiff_hip
    tiff_hip.check_tile(tile)
    if isinstance(depth, bool) or depth not in (8, 16):
        raise ValueError(f'depth={depth!r}: 8 or 16')
    if not isinstance(matches, bool):
        raise ValueError(f'matches must be True or False, got {matches!r}')
    alpha, grey = bool(getattr(enc, 'alpha', False)), bool(getattr(enc, 'grey', False))
    if depth == 16 and alpha:
        raise ValueError('depth=16 on an encode_rgba record: there is no 16-bit alpha; write the file with depth=8')
    if grey and alpha:
        raise ValueError('a grey + alpha record has no TIFF form here (nor a PNG one)')
    from .scene_render import refuse_ensemble
    refuse_ensemble(enc, 'write_tiff')


def write_tiff(model, enc, path, scale=None, size=None, tile=256, depth=8, order='bgr', matches=False):
    """The pyramidal tiled TIFF `path` (tiff_hip.py: one IFD per level, deflate tiles of `tile` x `tile` with the horizontal predictor)
    of the `size` / `scale` render of `enc`.  The levels are `model.render_pyramid`'s -- with `depth=16` its `as_u16` ones -- from the top
    down to the first that fits one tile (`tiff_hip.tiff_level_sizes`): a level at or above the LR size is the model's own answer,
    the ones below are Pillow-exact bicubic resizes of the smallest model level at 8 bits and a chain of box halvings at 16.  Each
    level's tiles are coded in one set of launches and read in two synchronising copies.  `order`: the byte order of the rendered
    images, 'bgr' as `render_pyramid` makes them.  `matches=True`: the match coder for every tile (edge padding then costs next to
    nothing).  -> dict: levels [(H_l, W_l)] top first, model_levels, tiles, bytes, and the seconds render_s (to the last launch, not
    synchronised), encode_s, write_s."""
    from . import tiff_hip
    check_tiff(enc, tile, depth, matches)
    t0 = time.perf_counter()
    levels = model.render_pyramid(enc, size=size, scale=scale, **(dict(as_u16=True) if depth == 16 else {}))
    render_s = time.perf_counter() - t0
    top = levels[-1]
    sizes = tiff_hip.tiff_level_sizes(top.shape[0], top.shape[1], tile)
    levels = levels[::-1][:len(sizes)]                                         # render_pyramid lists the 1 x 1 level first
    if [(im.shape[0], im.shape[1]) for im in levels] != sizes:
        raise ValueError(f'the rendered levels are not those of a {top.shape[0]} x {top.shape[1]} pyramid')
    t1 = time.perf_counter()
    plan, coded = tiff_hip._encode_file(levels, tile, order, 0, matches)
    t2 = time.perf_counter()
    os.makedirs(os.path.dirname(os.path.abspath(path)) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        for piece in tiff_hip._pieces(plan, coded):
            f.write(piece)
    h, w = enc.x.shape[-2:]
    return dict(levels=sizes, model_levels=[k for k, (hl, wl) in enumerate(sizes) if hl >= h and wl >= w],
                tiles=sum(len(o) - 1 for _, o in coded), bytes=plan['total'], render_s=render_s, encode_s=t2 - t1,
                write_s=time.perf_counter() - t2)
