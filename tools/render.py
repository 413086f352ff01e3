#!/usr/bin/env python
"""Render one image at several scales (or one window of each), and rotated / panned / zoomed views of it, from ONE encode:

    python tools/render.py CONFIG CHECKPOINT IMAGE --scale S [S ...] [--window I0 J0 H W] [--precision P] --out DIR
    python tools/render.py CONFIG CHECKPOINT IMAGE [--scale ...] --view CY CX ZOOM ANGLE --size H W [--view ... --size ...] --out DIR
    python tools/render.py CONFIG CHECKPOINT IMAGE [--scale ...] --homography H00 H01 H02 H10 H11 H12 H20 H21 H22 --size H W --out DIR

Config and checkpoint as for tools/test.py.  The trunk, cs_attn and the head's per-image tables run once (CiaoSR.encode); every
scale and view is a target of ONE CiaoSR.render_many -- a single walk over the tile scenes, each built once however many outputs touch
it -- and is bitwise the image CiaoSR.render / render_view give for it.  A scale is written to DIR/<image name>_x<S>.png, the image
`restore` gives for that target under the same test_cfg.  The configs tile integer scales only (`clip_test`), so this tool turns on
`test_cfg.tile_any_scale` where the config sets `tile`: an image no larger than the tile is then the whole-image path, a larger
one is tiled by tile_plan.  `--window` is in HR pixels of each scale's own grid; `--max-scale` sizes the scenes' plan (default: the
largest --scale; without --scale the largest view ZOOM).  Every `--view` (repeatable; alone or alongside --scale) is a CiaoSR.render_view of
ciaosr_amd.scene.view_matrix((CY, CX), ZOOM, ANGLE, (H, W)): an H x W picture whose centre looks at LR position (CY, CX) with ZOOM output
pixels per LR pixel, turned by ANGLE degrees (positive: the picture turns clockwise), written to DIR/<image name>_view<k>.png, k = 0,
1, ... in command-line order; one `--size` per `--view`, or a single one for all of them.  Pixels outside the image are black.
Every `--homography` (repeatable; alone or alongside --scale and --view) is a CiaoSR.render_warp: an H x W picture whose pixel centre
(v, u) = (i + 0.5, j + 0.5) looks at the LR position y = (H00 v + H01 u + H02) / D, x = (H10 v + H11 u + H12) / D, D = H20 v + H21 u + H22
(ciaosr_amd.scene: keystone and perspective correction; `homography_from_points` makes one from four point pairs), written to DIR/<image
name>_warp<k>.png in command-line order.  `--size` follows the rule of `--view`: one per --view and --homography, the views first, or a
single one for all of them.  D must be positive on the whole output; the model sees ONE footprint per warp, the Jacobian at the output
centre, unless `--footprint per-pixel` gives every output pixel of every --homography its own (the Jacobian at the pixel, clamped to
`--footprint-range LO HI`, default 1 / max scale and 1.0; the file names do not change): the choice under strong perspective.
`--footprint-range` without `--footprint per-pixel` is an argparse error.  `--minify area [--max-samples N]` with it supersamples the
pixels whose footprint exceeds HI -- up to N x N samples, N in 1, 2, 4, 8 (default 4), averaged -- instead of clamping them to one
aliasing point query; `--minify` without `--footprint per-pixel` is an argparse error too.  Not with --self-ensemble or --tiff (an argparse error).
`--gpu-png` sets `test_cfg.gpu_png`: every output is rendered as a uint8 image on the device and PNG-encoded there (ciaosr_amd/png_hip.py);
the files decode to the pixels of the default run.
`--view-blocks` sets `test_cfg.view_blocks` (CiaoSR.render_view): in f16 / bf16 a view that the tile seams or the image border cut is
queried in 4 x 2 blocks of output pixels, which keeps the head on its chained kernel; other precisions are unaffected.
`--dzi SCALE [--dzi-tile 254] [--dzi-overlap 1]` also writes the Deep Zoom pyramid of the SCALE render (ciaosr_amd/pyramid.py): DIR/<image
name>.dzi and DIR/<image name>_files/<level>/<col>_<row>.png, every level at or above the LR size rendered by the model from the same
encode, each level's tiles PNG-encoded on the device in one call (always the device encoder, with or without `--gpu-png`); alone or next
to --scale / --view outputs, which it does not change.  `--max-scale` then defaults to cover SCALE as well.
`--jpeg Q [--jpeg-subsampling 444|420]` writes baseline JPEG files of quality Q instead: DIR/<image name>_x<S>.jpg, _view<k>.jpg and, with
--dzi, `<col>_<row>.jpg` tiles under a manifest that says Format="jpg".  Every output is rendered as a uint8 image on the device (as for
`--gpu-png`) and coded there (ciaosr_amd/jpeg_hip.py); the files are byte for byte what Pillow saves for the same pixels.
`--jpeg-optimize` (only with --jpeg) gives every .jpg of the run Huffman tables of its own, made on the device: Pillow's `optimize=True`
files, smaller, the same pixels; the manifest does not change.
`--jpeg-progressive` (only with --jpeg) writes every .jpg of the run as a progressive file, coded on the device: Pillow's
`progressive=True` files, the same pixels in ten scans from coarse to fine; the manifest does not change.
`--niqe PARAMS` scores every --scale and --view output with NIQE under the pristine model PARAMS (the reference's niqe_pris_params.npz;
ciaosr_amd/niqe_hip.py): computed on the device from the 8-bit image, before any encoding, Y channel, no border cropped.  The values are
printed and written to DIR/niqe.json as {file name: value}; an output too small for two 96x96 blocks gets null.  Pyramid tiles are not
scored, and no output changes.
`--alpha` keeps the file's transparency: the image is read as RGBA (RGBA, LA and palette files with a tRNS chunk), encoded as a batch of
two -- the colour as stored and the alpha plane as a grey image, both through the same model (CiaoSR.encode_rgba) -- and every --scale,
--view and --dzi output is rendered as a uint8 B G R A image on the device and written as an RGBA PNG by the device coder (as --jpeg
forces the device path, with or without --gpu-png).  The colour bytes are those of the run without the flag on the colour image; alpha is
the integer luma of the rendered alpha image; outside a view the pixels are transparent (A = 0).  `--niqe` scores the colour part.  A
file without a transparent pixel is reported in one line and takes the plain path: its outputs are byte for byte those of the run
without the flag.  Not with --jpeg: JPEG files have no alpha.
`--self-ensemble` makes every --scale output (with or without --window) the geometric self-ensemble: the image is encoded once per flip /
transpose (8 members, `CiaoSR.encode(..., self_ensemble=True)`), every member renders its own transformed window and the results are mapped
back and averaged on the device in fp32 -- the image `CiaoSR.restore(..., self_ensemble=True)` gives, quantised once after the mean.  Eight
times the work and scene memory of the plain run.  Not with --view, --dzi or --alpha (an argparse error).
`--grey` treats the input as a single-channel image: it is read through Pillow's convert('L') (a file that was not grey is reported in
one line), encoded as the colour image (v, v, v) (CiaoSR.encode_grey), and every --scale, --view and --dzi output is rendered as a uint8
[H, W] image on the device -- the integer luma of the render's bytes, Pillow's convert('L'), so the answer is grey -- and coded there as
a grey .png (colour type 0), or with --jpeg Q [--jpeg-optimize] as a one-component .jpg, byte for byte Pillow's mode-L file.
--png-matches, --niqe and --self-ensemble work as for colour.  Not with --alpha (no grey + alpha files), --jpeg-progressive (no grey
progressive files) or --jpeg-subsampling 420.
`--png-matches` (only with --gpu-png, --alpha or --grey, never with --jpeg) lets the device PNG coder use LZ77 matches for every .png of the run,
pyramid tiles included: transparent and filled regions then cost next to nothing, and no file gets larger (png_hip `matches=True`).
`--depth16` keeps 16 bits per sample: the input is read with the 16-bit readers (ciaosr_amd.imageio.imread16_rgb01, or imread16_grey01
with --grey: depth-16 PNG files and 16-bit grey TIFF as sample / 65535, any other file as without the flag) and its bit depth is
printed; every --scale, --window and --view output is rendered as a torch.uint16 image on the device (`as_u16`: each sample
rint(clamp(v, 0, 1) * 65535), quantised once) and written as a PNG of bit depth 16 by the device coder, colour type 2, or 0 with
--grey.  An 8-bit input is allowed: the output then keeps the model's precision.  --png-matches and --self-ensemble work with it.
Not with --jpeg, --alpha, --dzi or --niqe (an argparse error): those stay 8-bit.
`--tiff [--tiff-tile 256]` writes every --scale output as ONE pyramidal tiled TIFF, DIR/<image name>_x<S>.tif, instead of a .png
(ciaosr_amd/tiff_hip.py, pyramid.write_tiff): one image file directory per level from the full render down to the first level that
fits one tile, each level halving the one above; deflate tiles (Compression 8, Predictor 2) of --tiff-tile pixels a side (a multiple
of 16 in 16..4096), coded on the device -- what OpenSlide, QuPath / Bio-Formats, libvips, GDAL and Pillow open.  Levels at or above
the LR size are the model's own renders from the same encode.  With --depth16 the file holds 16-bit samples (the levels below the LR
size are box halvings there, Pillow-exact bicubic resizes at 8 bits), with --grey one sample per pixel, with --alpha RGBA with
unassociated alpha, with --png-matches the tiles may use LZ77 matches.  Not with --jpeg, --view, --window, --dzi, --niqe or
--self-ensemble (an argparse error); --alpha with --depth16 and --grey with --alpha stay refused.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='ciaosr_amd multi-scale renderer')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help='checkpoint file ("None" = cfg.test_checkpoint_path)')
    p.add_argument('image', help='LR image file')
    p.add_argument('--scale', type=float, nargs='+', default=[], help='one output per scale: round(h * s) x round(w * s)')
    p.add_argument('--view', type=float, nargs=4, action='append', default=[], metavar=('CY', 'CX', 'ZOOM', 'ANGLE'),
                   help='one output per view: centre in LR pixels, output pixels per LR pixel, degrees (repeatable)')
    p.add_argument('--homography', type=float, nargs=9, action='append', default=[],
                   metavar=('H00', 'H01', 'H02', 'H10', 'H11', 'H12', 'H20', 'H21', 'H22'),
                   help='one output per homography: output pixel centres (v, u) to LR positions (y, x), y first (repeatable)')
    p.add_argument('--size', type=int, nargs=2, action='append', default=[], metavar=('H', 'W'),
                   help='output size of each --view and --homography')
    p.add_argument('--footprint', choices=['per-pixel'], default=None,
                   help='every --homography gives each output pixel its own footprint, its Jacobian there (default: one per warp)')
    p.add_argument('--footprint-range', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                   help='with --footprint per-pixel: clamp the footprints to [LO, HI] LR pixels (default: 1 / max scale, 1.0)')
    p.add_argument('--minify', choices=['clamp', 'area'], default=None,
                   help='with --footprint per-pixel: area supersamples the pixels whose footprint exceeds HI and averages (default: clamp)')
    p.add_argument('--max-samples', type=int, choices=[1, 2, 4, 8], default=None,
                   help='with --minify area: samples per axis and pixel at the most (default 4)')
    p.add_argument('--window', type=int, nargs=4, default=None, metavar=('I0', 'J0', 'H', 'W'), help='HR pixels; default: the whole grid')
    p.add_argument('--precision', default=None, help='test_cfg.precision (default: the config\'s, else fp32)')
    p.add_argument('--view-blocks', action='store_true',
                   help='test_cfg.view_blocks: the 16-bit modes select a cut view\'s members in 4 x 2 blocks of output pixels (default off)')
    p.add_argument('--gpu-png', action='store_true',
                   help='test_cfg.gpu_png: outputs are quantised and PNG-encoded on the GPU; no fp32 image crosses to the host (default off)')
    p.add_argument('--png-matches', action='store_true',
                   help='with --gpu-png or --alpha: the device PNG coder may use LZ77 matches, for every .png of the run (default off)')
    p.add_argument('--jpeg', type=int, default=None, metavar='Q',
                   help='write JPEG files of quality Q (1..100), coded on the GPU, instead of PNG files (default: PNG)')
    p.add_argument('--jpeg-subsampling', choices=['444', '420'], default='444', help='chroma subsampling of --jpeg (default 444)')
    p.add_argument('--jpeg-optimize', action='store_true',
                   help='with --jpeg: per-file Huffman tables made on the GPU, the files of Pillow\'s optimize=True (default off)')
    p.add_argument('--jpeg-progressive', action='store_true',
                   help='with --jpeg: progressive files coded on the GPU, the files of Pillow\'s progressive=True (default off)')
    p.add_argument('--alpha', action='store_true',
                   help='keep the transparency of the input: alpha goes through the model as a grey image, outputs are RGBA PNG files (default off)')
    p.add_argument('--grey', action='store_true',
                   help='the input is a single-channel image: outputs are grey .png (or one-component .jpg) files coded on the GPU (default off)')
    p.add_argument('--depth16', action='store_true',
                   help='16 bits per sample: read the input at full precision, write uint16 renders as PNG files of bit depth 16 coded on '
                        'the GPU (not with --jpeg, --alpha, --dzi or --niqe; default off)')
    p.add_argument('--dzi', type=float, default=None, metavar='SCALE', help='also write the Deep Zoom pyramid of the SCALE render: <name>.dzi, <name>_files/')
    p.add_argument('--dzi-tile', type=int, default=254, help='Deep Zoom tile size (default 254)')
    p.add_argument('--dzi-overlap', type=int, default=1, help='Deep Zoom overlap (default 1)')
    p.add_argument('--tiff', action='store_true',
                   help='write every --scale output as a pyramidal tiled TIFF (.tif) coded on the GPU (with --depth16, --grey, --alpha, '
                        '--png-matches; not with --jpeg, --view, --window, --dzi, --niqe or --self-ensemble; default off)')
    p.add_argument('--tiff-tile', type=int, default=256, help='TIFF tile side: a multiple of 16 in 16..4096 (default 256)')
    p.add_argument('--niqe', default=None, metavar='PARAMS',
                   help='score every --scale / --view output with NIQE on the GPU under the pristine model PARAMS (.npz); writes niqe.json')
    p.add_argument('--self-ensemble', action='store_true',
                   help='every --scale output is the mean over the 8 flips and transposes of the input, mapped back (8 encodes; not with '
                        '--view, --dzi or --alpha; default off)')
    p.add_argument('--max-scale', type=float, default=None,
                   help='the scale the scenes are planned for (default: the largest --scale, else the largest ZOOM; with --dzi at least its SCALE)')
    p.add_argument('--out', required=True, help='output directory')
    args = p.parse_args(argv)
    if not args.scale and not args.view and not args.homography and args.dzi is None:
        p.error('give --scale, --view, --dzi or several of them')
    if args.view and not args.homography and len(args.size) not in (1, len(args.view)):
        p.error('give one --size H W per --view, or a single one for all views')
    if args.homography and len(args.size) not in (1, len(args.view) + len(args.homography)):
        p.error('give one --size H W per --view and --homography (the views first), or a single one for all of them')
    if args.size and not args.view and not args.homography:
        p.error('--size belongs to --view')
    if args.footprint and not args.homography:
        p.error('--footprint per-pixel applies to --homography outputs')
    if args.footprint_range and not args.footprint:
        p.error('--footprint-range clamps per-pixel footprints: give --footprint per-pixel with it')
    if args.minify and not args.footprint:
        p.error('--minify chooses what a per-pixel footprint above the range does: give --footprint per-pixel with it')
    if args.max_samples and args.minify != 'area':
        p.error('--max-samples bounds the samples of --minify area: give --minify area with it')
    if args.footprint_range and not 0.0 < args.footprint_range[0] <= args.footprint_range[1] < float('inf'):
        p.error('--footprint-range takes 0 < LO <= HI')
    if args.jpeg is not None and not 1 <= args.jpeg <= 100:
        p.error('--jpeg takes a quality in 1..100')
    if args.alpha and args.jpeg is not None:
        p.error('--alpha writes RGBA PNG files: JPEG has no alpha channel, drop --jpeg')
    if args.png_matches and args.jpeg is not None:
        p.error('--png-matches is the PNG coder\'s option: drop --jpeg')
    if args.grey and args.alpha:
        p.error('--grey with --alpha: there are no grey + alpha files (PNG colour type 4) here, drop one of them')
    if args.grey and args.jpeg_progressive:
        p.error('--grey with --jpeg-progressive: there are no one-component progressive files here, drop --jpeg-progressive')
    if args.grey and args.jpeg is not None and args.jpeg_subsampling != '444':
        p.error('--grey has no chroma to subsample: drop --jpeg-subsampling')
    if args.depth16:
        for flag, given in (('--jpeg', args.jpeg is not None), ('--alpha', args.alpha), ('--dzi', args.dzi is not None),
                            ('--niqe', args.niqe is not None)):
            if given:
                p.error(f'--depth16 with {flag}: JPEG, alpha, pyramids and NIQE stay 8-bit here, drop one of the two')
    if args.tiff:
        if not args.scale:
            p.error('--tiff writes the --scale outputs: give --scale')
        for flag, given in (('--jpeg', args.jpeg is not None), ('--view', bool(args.view)), ('--window', args.window is not None),
                            ('--niqe', args.niqe is not None), ('--self-ensemble', args.self_ensemble), ('--dzi', args.dzi is not None)):
            if given:
                p.error(f'--tiff with {flag}: a pyramidal TIFF is the whole render of a plain encode in deflate tiles, drop one of the two')
        if args.homography:
            p.error('--tiff with --homography: a pyramidal TIFF is the whole render of a plain encode in deflate tiles, drop one of the two')
        if args.tiff_tile < 16 or args.tiff_tile > 4096 or args.tiff_tile % 16:
            p.error('--tiff-tile is a multiple of 16 in 16..4096')
    if args.png_matches and not (args.gpu_png or args.alpha or args.grey or args.depth16 or args.tiff):
        p.error('--png-matches belongs to --gpu-png, --alpha, --grey or --depth16, whose files the device codes')
    if args.jpeg_optimize and args.jpeg is None:
        p.error('--jpeg-optimize belongs to --jpeg')
    if args.jpeg_progressive and args.jpeg is None:
        p.error('--jpeg-progressive belongs to --jpeg')
    if args.self_ensemble and (args.view or args.dzi is not None or args.alpha):
        p.error('--self-ensemble applies to --scale and --window outputs: views, pyramids and RGBA encodes have no ensemble, drop '
                '--view / --dzi / --alpha')
    if args.self_ensemble and args.homography:
        p.error('--self-ensemble applies to --scale and --window outputs: warps have no ensemble, drop --homography')
    return args


def output_format(args):
    """What the flags ask the writers for: dict(fmt, ext) and, for JPEG, quality and subsampling, with --jpeg-optimize also optimize=True, with
    --jpeg-progressive also progressive=True."""
    if args.jpeg is None:
        return dict(fmt='png', ext='.png')
    form = dict(fmt='jpg', ext='.jpg', quality=args.jpeg, subsampling=args.jpeg_subsampling)
    if args.jpeg_optimize:
        form['optimize'] = True
    if args.jpeg_progressive:
        form['progressive'] = True
    return form


def scale_tag(s):
    return f'{s:g}'.replace('.', 'p')


def main(argv=None):
    args = parse_args(argv)
    import ciaosr_amd
    from ciaosr_amd import metrics
    from ciaosr_amd.checkpoint import load_checkpoint
    from ciaosr_amd.config import Config
    from ciaosr_amd.imageio import imread16_grey01, imread16_rgb01, imread_grey01, imread_rgb01, imread_rgba01, imwrite

    cfg = Config.fromfile(args.config)
    if args.checkpoint in (None, 'None'):
        args.checkpoint = cfg.get('test_checkpoint_path')
    if args.precision:
        cfg.test_cfg['precision'] = args.precision
    if args.view_blocks:
        cfg.test_cfg['view_blocks'] = True
    if args.gpu_png:
        cfg.test_cfg['gpu_png'] = True
    if cfg.test_cfg.get('tile', None):
        cfg.test_cfg['tile_any_scale'] = True
    dev = torch.device('cuda', torch.cuda.current_device())
    model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if args.checkpoint:
        load_checkpoint(model, args.checkpoint, map_location='cpu')
    model = model.to(dev).eval()

    alpha = False
    if args.alpha:
        lq4, opaque = imread_rgba01(args.image)
        if opaque:
            print(f'{args.image}: no transparent pixel, --alpha changes nothing')
        alpha = not opaque
    wanted = args.scale or [v[2] for v in args.view]
    sizes = [args.size[k if len(args.size) > 1 else 0] for k in range(len(args.view) + len(args.homography))]
    if args.homography and not args.scale:                                           # without --homography `wanted` is what it was
        from ciaosr_amd.scene import warp_footprint, warp_max_scale
        wanted = wanted + [warp_max_scale(warp_footprint(h, size)) for h, size in zip(args.homography, sizes[len(args.view):])]
        if args.footprint_range:                                                     # a per-pixel warp plans for 1 / lo
            wanted = wanted + [1.0 / args.footprint_range[0]]
    if args.dzi is not None:
        wanted = wanted + [args.dzi]
    if alpha:
        enc = model.encode_rgba(lq4.unsqueeze(0).to(dev), max_scale=args.max_scale or max(wanted))
    elif args.grey:
        if args.depth16:
            lq1, was_grey, bits = imread16_grey01(args.image)
            print(f'{args.image}: {bits} bits per sample')
        else:
            lq1, was_grey = imread_grey01(args.image)
        if not was_grey:
            print(f'{args.image}: not a grey image, --grey keeps its luma (convert("L")) only')
        ens = dict(self_ensemble=True) if args.self_ensemble else {}
        enc = model.encode_grey(lq1.unsqueeze(0).to(dev), max_scale=args.max_scale or max(wanted), **ens)
    else:
        if args.depth16:
            lq, bits = imread16_rgb01(args.image)
            print(f'{args.image}: {bits} bits per sample')
            lq = lq.unsqueeze(0).to(dev)
        else:
            lq = imread_rgb01(args.image).unsqueeze(0).to(dev)
        ens = dict(self_ensemble=True) if args.self_ensemble else {}                 # without --self-ensemble encode is called as before
        enc = model.encode(lq, max_scale=args.max_scale or max(wanted), **ens)
    name = os.path.splitext(os.path.basename(args.image))[0]
    from ciaosr_amd.scene import Grid, View, Warp, view_matrix
    form = output_format(args)
    coding = {k: form[k] for k in ('quality', 'subsampling', 'optimize', 'progressive') if k in form}
    dzi_format = dict(fmt='jpg', **coding) if form['fmt'] == 'jpg' else {}           # without --jpeg write_dzi is called as before
    lz = dict(matches=True) if args.png_matches else {}                              # without --png-matches every writer is called as before
    dzi_format.update(lz)
    if args.tiff:                                                                    # every scale is a file of its own pyramid
        from ciaosr_amd.pyramid import write_tiff
        paths = [os.path.join(args.out, f'{name}_x{scale_tag(s)}.tif') for s in args.scale]
        for s, path in zip(args.scale, paths):
            res = write_tiff(model, enc, path, scale=s, tile=args.tiff_tile, depth=16 if args.depth16 else 8, **lz)
            top = res['levels'][0]
            print(f"{path}: {top[0]} x {top[1]}, {len(res['levels'])} levels ({len(res['model_levels'])} from the model), "
                  f"{res['tiles']} tiles, {res['bytes']} bytes, {16 if args.depth16 else 8} bits per sample")
        return paths
    targets = [Grid(scale=s, window=args.window) for s in args.scale]
    paths = [os.path.join(args.out, f'{name}_x{scale_tag(s)}{form["ext"]}') for s in args.scale]
    for k, (cy, cx, zoom, angle) in enumerate(args.view):
        size = args.size[k if len(args.size) > 1 else 0]
        targets.append(View(view_matrix((cy, cx), zoom, angle, size), size))
        paths.append(os.path.join(args.out, f'{name}_view{k}{form["ext"]}'))
    for k, h in enumerate(args.homography):
        per_pixel = dict(footprint=args.footprint, footprint_range=args.footprint_range) if args.footprint else {}
        if args.minify:
            per_pixel.update(minify=args.minify, max_samples=args.max_samples or 4)
        targets.append(Warp(homography=h, size=sizes[len(args.view) + k], **per_pixel))
        paths.append(os.path.join(args.out, f'{name}_warp{k}{form["ext"]}'))
    gpu_png = model.gpu_png()
    as_u8 = (gpu_png or form['fmt'] == 'jpg' or alpha or args.grey) and not args.depth16
    quant = dict(as_u16=True) if args.depth16 else dict(as_u8=as_u8)                 # without --depth16 render_many is called as before
    outs = model.render_many(enc, targets, **quant) if targets else []               # one walk over the tile scenes for every output
    scores = {}
    if args.niqe and targets:
        from ciaosr_amd import niqe_hip
        from ciaosr_amd.metrics_hip import tensor2img_u8
        params = niqe_hip.load_params(args.niqe)
    for path, out in zip(paths, outs):
        if args.niqe:
            img = out if as_u8 else tensor2img_u8(out)                 # the bytes the file holds (bitwise metrics.tensor2img)
            if alpha:
                img = img[:, :, :3].contiguous()                       # the colour part: tensor2img_u8 of item 0
            try:
                niqe_hip.geometry(img.shape[0], img.shape[1])
                scores[os.path.basename(path)] = niqe_hip.niqe_u8(img, params)
            except ValueError:                                         # fewer than two blocks (or fewer than two without a NaN)
                scores[os.path.basename(path)] = None
            print(f'{path}: NIQE {scores[os.path.basename(path)]}')
        if args.depth16:
            from ciaosr_amd.png_hip import imwrite_gpu
            imwrite_gpu(out, path, **lz)                               # uint16 [H, W, 3] BGR (--grey: [H, W]) on the device
            print(f'{path}: {out.shape[0]} x {out.shape[1]}{" grey" if args.grey else ""}, 16 bits per sample')
        elif form['fmt'] == 'jpg':
            from ciaosr_amd.jpeg_hip import imwrite_gpu_jpeg
            imwrite_gpu_jpeg(out, path, **coding)                      # uint8 [H, W, 3] BGR (--grey: [H, W]) on the device
            print(f'{path}: {out.shape[0]} x {out.shape[1]}')
        elif args.grey:
            from ciaosr_amd.png_hip import imwrite_gpu
            imwrite_gpu(out, path, **lz)                               # uint8 [H, W] on the device
            print(f'{path}: {out.shape[0]} x {out.shape[1]} grey')
        elif alpha:
            from ciaosr_amd.png_hip import imwrite_gpu
            imwrite_gpu(out, path, order='bgra', **lz)                 # uint8 [H, W, 4] B G R A on the device
            print(f'{path}: {out.shape[0]} x {out.shape[1]} RGBA')
        elif gpu_png:
            from ciaosr_amd.png_hip import imwrite_gpu
            imwrite_gpu(out, path, **lz)                               # uint8 [H, W, 3] BGR on the device
            print(f'{path}: {out.shape[0]} x {out.shape[1]}')
        else:
            imwrite(metrics.tensor2img(out), path)
            print(f'{path}: {out.shape[-2]} x {out.shape[-1]}')
    if args.niqe and targets:
        import json
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'niqe.json'), 'w') as f:
            json.dump(scores, f, indent=1)
    if args.dzi is not None:
        from ciaosr_amd.pyramid import write_dzi
        res = write_dzi(model, enc, args.out, name, scale=args.dzi, tile_size=args.dzi_tile, overlap=args.dzi_overlap, **dzi_format)
        top = res['levels'][-1]
        print(f"{os.path.join(args.out, name + '.dzi')}: {top[0]} x {top[1]}, {len(res['levels'])} levels ({len(res['model_levels'])} from the "
              f"model), {res['files']} files, {res['bytes']} bytes")
    return paths


if __name__ == '__main__':
    main()
