#!/usr/bin/env python
"""Times the two PNG writers of the --save-path / --out path on uint8 device images and writes profiles/png_gpu.txt:

    python tools/png_probe.py [--sizes 5424x8160 768x768] [--contents smooth noisy] [--warmup 2] [--rounds 5] [--out FILE] [--append]

host leg:   what the default path does with a quantised device image: `imageio.imwrite(img.cpu().numpy(), path)` (PIL at its default level);
device leg: `png_hip.imwrite_gpu(img, path)` (csrc/png_u8.hip + the container on the host).
Images: `init_utils.synthetic_gt` quantised by `tensor2img_u8`, as is ('smooth') and with 2 grey levels of noise ('noisy').  The legs
alternate in one process; wall time runs from the device image (after a synchronize) to the closed file.  Device time per kernel comes
from `hip_ops.profile` in a round of its own.  The files of both writers are decoded and compared, and their sizes recorded.

    python tools/png_probe.py --leg tiles [--parent-root DIR] [--dzi] [--sizes 5424x8160] [--tile 254] [--overlap 1] [--out FILE]

times the tiles of a pyramid's top level (ciaosr_amd/pyramid.py) and writes profiles/png_tiles.txt:
(a) one `encode_png` per tile on the pitched crops -- with `--parent-root DIR` (a built checkout of the parent commit) from that tree's
    library, in a child process that stays up for the whole run and takes its turn in every round; otherwise in this process;
(b) one `encode_png_tiles` call;  (c) the whole image in one `encode_png`, for scale.
Wall time runs from the device image (after a synchronize) to the bytes on the host; the legs alternate; kernel time is the sum over
`hip_ops.profile` of a round of its own.  The files of (a) and (b) are compared byte for byte.  `--dzi` adds one full pyramid of the
bench output (config 001, LR 1356 x 2040, x4) from a ready encode, split into render, encode and file writing.

    python tools/png_probe.py --leg jpeg [--sizes 5424x8160 768x768] [--quality 90] [--tile 254] [--overlap 1] [--out FILE]

times the JPEG encoder (ciaosr_amd/jpeg_hip.py) and writes profiles/jpeg_gpu.txt.  Per image and subsampling ('444', '420'):
(a) `encode_jpeg` on the device;  (b) the device-to-host copy followed by `PIL.Image.save` as JPEG into memory;  (c) `encode_png` on the
device.  For images larger than one tile also the top-level tiles: (d) one `encode_jpeg_tiles` call against (e) one `encode_jpeg` per
tile.  Wall time runs from the device image (after a synchronize) to the bytes on the host; the legs alternate in one process; kernel
time by tag comes from `hip_ops.profile` in a round of its own.  The files of (a) and (b), and of (d) and (e), are compared byte for
byte, and the sizes of the JPEG, device PNG and Pillow PNG files are recorded.

    python tools/png_probe.py --leg jpeg-opt [--sizes 5424x8160 768x768] [--quality 90] [--tile 254] [--overlap 1] [--out FILE]

times JPEG files with optimised Huffman tables (`optimize=True`) on the 'noisy' images and writes profiles/jpeg_opt.txt.  Per image and
subsampling: (a) `encode_jpeg(optimize=True)`;  (b) the same call with `optimize=False`;  (c) the device-to-host copy followed by
`PIL.Image.save(optimize=True)` into memory.  For images larger than one tile also the top-level tiles: (d) one
`encode_jpeg_tiles(optimize=True)` call, (e) the same with `optimize=False`, (f) the copy followed by one optimised Pillow file per tile.
Timing as for `--leg jpeg`, and the device legs once more alternating without the Pillow leg; the files of (a) and (c), and of (d) and (f), are compared byte for byte; the sizes of both modes and the
kernel times by tag (jpeg_hist and jpeg_tables among them) are recorded.

    python tools/png_probe.py --leg jpeg-prog [--sizes 5424x8160 768x768] [--quality 90] [--tile 254] [--overlap 1] [--out FILE]

times progressive JPEG files (`progressive=True`) and writes profiles/jpeg_prog.txt.  Per image -- the 'noisy' image of every size and,
for sizes larger than one tile, a flat image of the same size, whose every AC scan is ONE chain of EOB runs that a single lane walks
(the worst case of prog_runs) -- and subsampling: (a) `encode_jpeg(progressive=True)`;  (b) `encode_jpeg(optimize=True)`;  (c) the
device-to-host copy followed by `PIL.Image.save(progressive=True)` into memory.  For the noisy image also the top-level tiles as one
call: (d) `encode_jpeg_tiles(progressive=True)`, (e) `encode_jpeg_tiles(optimize=True)`, (f) the copy followed by one progressive Pillow
file per tile.  Protocol as for `--leg jpeg-opt`; the files of (a) and (c), and of (d) and (f), are compared byte for byte; the sizes of
the progressive and the optimised baseline files and the kernel times by tag (prog_runs among them) are recorded.

    python tools/png_probe.py --leg rgba [--sizes 768x768 5424x8160] [--out FILE]

RGBA files (colour type 6) from uint8 [H, W, 4] B G R A device images: (a) `png_hip.encode_png(img, 'bgra')` against (b) the copy to the
host + `PIL.Image.save` of the same RGBA pixels.  Cases: the first size as a 'view' (noisy colour, alpha 255 inside a rectangle turned by
30 degrees and 0 in the corners outside it), every other size with a 'noisy' alpha (uniform random bytes) and with a 'sprite' alpha (an
ellipse with soft edges: about 70 % of the pixels fully transparent; the colour under them stays, as a render leaves it; 'sprite0' is
the same image with that colour set to 0, as many files store it: the case the literal-only coder is worst at).  Wall time
runs from the device image (after a synchronize) to the file's bytes on the host; the legs alternate; the file sizes of both and the
kernel times of (a) are recorded.  Default --out: profiles/png_rgba.txt.

    python tools/png_probe.py --leg matches [--sizes 768x768 5424x8160] [--out FILE]

The opt-in match coder: (a) `encode_png(img, order)`, the literal coder;  (b) `encode_png(img, order, matches=True)`;  (c) the copy to the
host + `PIL.Image.save`.  Inputs: the first size as the RGBA 'view' with the fill 0 outside it, as a render leaves it; every later size
as that view, the three other `--rgba-cases` and the smooth and noisy RGB images.  Legs alternating in one process, 2 warm-up + 5
timed rounds; the file bytes of all three and both device coders' kernel times (a profiled call of their own) are recorded.  Default
--out: profiles/png_matches.txt.

    python tools/png_probe.py --leg grey [--sizes 5424x8160 768x768] [--quality 90] [--out FILE]

Grey files from uint8 [H, W] device images (the integer luma of the smooth and the noisy image), in four formats: PNG, PNG with
matches, JPEG of --quality plain and optimised.  Per image and format (a) the grey device call, against two baselines: (b) the
three-channel device call on the (v, v, v) image of the same run, (c) the copy to the host + `PIL.Image.save` of the `L` image.  Legs
alternating in one process, 2 warm-up + 5 timed rounds; wall times, the kernel times of (a) and (b) (a profiled call of their own) and the
file bytes of all three are recorded; the PNG pixels of (a) and (c) and the JPEG bytes of (a) and (c) are compared.  Default --out:
profiles/grey_codecs.txt.

    python tools/png_probe.py --leg depth16 [--sizes 5424x8160 768x768] [--out FILE]

Depth-16 PNG files from torch.uint16 device images: `tensor2img_u16` (RGB16) and `tensor2img_grey_u16` (grey16) of the fp32 synthetic
image, as is ('smooth') and with Gaussian noise of two 8-bit levels ('noisy'), with `matches` off and on.  (a) the 16-bit device call;
(b) the 8-bit device call on the `tensor2img_u8` / `tensor2img_grey_u8` image of the same fp32 data; (c) for grey only, the copy to
the host + `PIL.Image.save` of the `I;16` image (Pillow has no 16-bit RGB writer, so RGB has no host leg).  Legs alternating in one
process, 2 warm-up + 5 timed rounds, wall time from the device image to the file's bytes; the kernel times of (a) and (b) come from a
profiled call of their own; the file bytes are held against the raw 2 C H W and, for grey, against Pillow's, whose decoded samples are
compared.  Default --out: profiles/png_depth16.txt.

    python tools/png_probe.py --leg tiff [--sizes 5424x8160 768x768] [--tiff-tile 256] [--out FILE]

Pyramidal tiled TIFF files (ciaosr_amd/tiff_hip.py) of the synthetic image as RGB8 (`tensor2img_u8`), RGB16 (`tensor2img_u16`) and
grey16 (`tensor2img_grey_u16`).  The levels are made before the clock starts: Pillow-exact bicubic resizes of the top at 8 bits, the
box-halving chain at 16.  (a) `encode_tiff` of all levels, `matches` off; (b) the same with `matches=True`; (c) the copy of the TOP
level to the host + `PIL.Image.save(format='TIFF', compression='tiff_adobe_deflate')` -- Pillow writes strips and no pyramid, so (c)
codes about three quarters of the samples of (a) and (b); it has no 16-bit RGB writer, so RGB16 has no host leg.  Legs alternating in
one process, 2 warm-up + 5 timed rounds, wall time from the device images to the file's bytes; kernel times from a profiled call of
their own; the file bytes are held against the raw bytes of all levels and against Pillow's, and the top page is read back through
Pillow and compared.  Default --out: profiles/tiff_gpu.txt.
"""
import json
import subprocess
import argparse
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_image(h, w, content, dev):
    from ciaosr_amd.init_utils import synthetic_gt
    from ciaosr_amd.metrics_hip import tensor2img_u8
    img = tensor2img_u8(synthetic_gt(h, w).to(dev))
    if content == 'noisy':
        g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
        noise = torch.randint(-2, 3, (h, w, 3), generator=g, dtype=torch.int16).to(dev)
        img = (img.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    return img.contiguous()


def top_rects(h, w, tile, overlap):
    """(y0, x0, h, w) of the tiles of a pyramid's top level (pyramid.dzi_plan's rule, restated: the parent tree has no pyramid.py)."""
    def spans(n):
        return [(c * tile - (overlap if c else 0), min((c + 1) * tile + overlap, n) - (c * tile - (overlap if c else 0)))
                for c in range(-(-n // tile))]
    return [(y0, x0, hh, ww) for y0, hh in spans(h) for x0, ww in spans(w)]


class PerTile:
    """Leg (a): one `encode_png` per rect, on the tree this process imports."""

    def __init__(self):
        self.img, self.rects = None, None

    def setup(self, h, w, content, rects):
        self.img = make_image(h, w, content, torch.device('cuda', torch.cuda.current_device()))
        self.rects = [tuple(r) for r in rects]
        torch.cuda.synchronize()
        return True

    def files(self):
        from ciaosr_amd.png_hip import encode_png
        return [encode_png(self.img[y0:y0 + h, x0:x0 + w]) for y0, x0, h, w in self.rects]

    def round(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.files()
        return time.perf_counter() - t0

    def kernels(self):
        from ciaosr_amd import hip_ops
        with hip_ops.profile():
            self.files()
        prof = hip_ops.profile.results()
        return dict(ms=sum(v['total_ms'] for v in prof.values()), launches=sum(v['launches'] for v in prof.values()))

    def digest(self):
        import hashlib
        return hashlib.sha256(b''.join(self.files())).hexdigest()

    def header(self):
        from ciaosr_amd import _lib
        return dict(version=_lib.load().ciaosr_version(), tiles_entry_point=hasattr(_lib.load(), 'ciaosr_png_encode_tiles_u8'))


def serve():
    """The parent-tree child: one JSON line per command line {cmd, args}; EOF ends it."""
    leg = PerTile()
    for line in sys.stdin:
        req = json.loads(line)
        print(json.dumps(getattr(leg, req['cmd'])(*req.get('args', []))), flush=True)
    return 0


class Child:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--root', os.path.abspath(root)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)

    def __getattr__(self, cmd):
        def ask(*args):
            self.p.stdin.write(json.dumps(dict(cmd=cmd, args=list(args))) + '\n')
            self.p.stdin.flush()
            line = self.p.stdout.readline()
            if not line:
                raise SystemExit(f'parent-tree child ended (exit status {self.p.wait()}) at {cmd!r}')
            return json.loads(line)
        return ask

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def stats(t):
    return f'mean {statistics.mean(t):.4f}, min {min(t):.4f}, max {max(t):.4f}  [{" ".join(f"{v:.4f}" for v in t)}]'


def tiles_leg(args, say):
    import hashlib
    from ciaosr_amd import hip_ops
    from ciaosr_amd.png_hip import encode_png, encode_png_tiles
    dev = torch.device('cuda', torch.cuda.current_device())
    a = Child(args.parent_root) if args.parent_root else PerTile()
    where = 'parent commit, child process' if args.parent_root else 'this tree, this process'
    if args.parent_root:
        say(f'leg (a) runs the parent tree\'s library: {a.header()}')
    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        rects = top_rects(h, w, args.tile, args.overlap)
        for content in args.contents:
            img = make_image(h, w, content, dev)
            a.setup(h, w, content, rects)
            torch.cuda.synchronize()
            legs = {'b': lambda: encode_png_tiles(img, rects), 'c': lambda: encode_png(img)}
            times = dict(a=[], b=[], c=[])
            for r in range(args.warmup + args.rounds):
                took = dict(a=a.round())
                for name in ('b', 'c'):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    legs[name]()
                    took[name] = time.perf_counter() - t0
                if r >= args.warmup:
                    for k, v in took.items():
                        times[k].append(v)
                print(f'  {size} {content} round {r}: ' + ', '.join(f'({k}) {v:.4f} s' for k, v in took.items()), flush=True)
            kern = dict(a=a.kernels())
            for name in ('b', 'c'):
                with hip_ops.profile():
                    out = legs[name]()
                prof = hip_ops.profile.results()
                kern[name] = dict(ms=sum(v['total_ms'] for v in prof.values()), launches=sum(v['launches'] for v in prof.values()))
                if name == 'b':
                    same = hashlib.sha256(b''.join(out)).hexdigest() == a.digest()
                    nbytes = sum(len(f) for f in out)
                    detail = ', '.join(f'{k} {v["total_ms"]:.3f}' for k, v in sorted(prof.items()))
            say(f'{h} x {w} {content}, top level at {args.tile}+{args.overlap}: {len(rects)} tiles, {nbytes} bytes of files; '
                f'(a) and (b) byte for byte identical: {same}')
            say(f'  (a) encode_png per tile ({where}) wall s: {stats(times["a"])}; kernels {kern["a"]["ms"]:.3f} ms in {kern["a"]["launches"]} launches')
            say(f'  (b) encode_png_tiles, one call wall s: {stats(times["b"])}; kernels {kern["b"]["ms"]:.3f} ms in {kern["b"]["launches"]} launches')
            say(f'  (c) encode_png, whole image   wall s: {stats(times["c"])}; kernels {kern["c"]["ms"]:.3f} ms in {kern["c"]["launches"]} launches')
            gap = statistics.mean(times['a']) - statistics.mean(times['b'])
            spread = max(max(times[k]) - min(times[k]) for k in ('a', 'b'))
            say(f'  (a) - (b) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                f'{"one call faster beyond the spread" if gap > spread else "NOT separated"}; '
                f'ratio {statistics.mean(times["a"]) / statistics.mean(times["b"]):.1f}x')
            say(f'  (b) kernels, ms: {detail}')
            del img
    if args.parent_root:
        a.close()
    if args.dzi:
        dzi_leg(args, say)


def dzi_leg(args, say):
    """One full pyramid of the bench output from a ready encode: render (synchronised), encode, file writing."""
    import ciaosr_amd
    from ciaosr_amd.config import Config
    from ciaosr_amd.init_utils import seeded_init_, synthetic_pair
    from ciaosr_amd.pyramid import write_levels
    dev = torch.device('cuda', torch.cuda.current_device())
    cfg = Config.fromfile(os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py'))
    cfg.test_cfg['tile_any_scale'] = True
    model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    seeded_init_(model, seed=0, gain=1.25, head_gain=6 ** 0.5)
    model = model.to(dev).eval()
    lq = synthetic_pair(1356, 2040, 4)[0].to(dev)
    enc = model.encode(lq, max_scale=4)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        levels = model.render_pyramid(enc, scale=4)
        torch.cuda.synchronize()
        render_s = time.perf_counter() - t0
        res = write_levels(levels, tmp, 'bench', args.tile, args.overlap)
    h, w = lq.shape[-2:]
    n_model = sum(1 for im in levels if im.shape[0] >= h and im.shape[1] >= w)
    say(f'write_dzi of the bench output (LR {h} x {w}, x4, {args.tile}+{args.overlap}; fp32, tile 192 / 32 with tile_any_scale; one run, scenes built '
        f'during the render): {len(levels)} levels, {n_model} from the model, {res["files"]} files, {res["bytes"]} bytes; render {render_s:.3f} s '
        f'({enc.cache.builds} scene builds), encode {res["encode_s"]:.3f} s, file writing {res["write_s"]:.3f} s')


def pil_file(img, fmt, **kw):
    """The Pillow file (bytes) of a uint8 [H, W, 3] BGR device image: the copy to the host, then the encoder."""
    import io
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img.cpu().numpy()[:, :, ::-1])).save(bio, format=fmt, **kw)
    return bio.getvalue()


def kernels(fn):
    """One profiled call of fn: total kernel time, launches, and the time of every tag."""
    from ciaosr_amd import hip_ops
    with hip_ops.profile():
        fn()
    prof = hip_ops.profile.results()
    return (f'{sum(v["total_ms"] for v in prof.values()):.3f} ms in {sum(v["launches"] for v in prof.values())} launches: '
            + ', '.join(f'{k} {v["total_ms"]:.3f}' for k, v in sorted(prof.items())))


def run_legs(args, legs):
    """{name: wall seconds of the timed rounds}; the legs alternate within every round."""
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    return times


def rgba_cases(h, w, first, dev):
    """[(name, uint8 [h, w, 4] B G R A device image)]: 'view' for the first size, else 'noisy' and 'sprite' alphas over the noisy colour."""
    from ciaosr_amd.metrics_hip import pack_bgra_u8
    colour = make_image(h, w, 'noisy', dev)
    y = (torch.arange(h, dtype=torch.float32, device=dev) + 0.5 - h / 2)[:, None]
    x = (torch.arange(w, dtype=torch.float32, device=dev) + 0.5 - w / 2)[None, :]

    def with_alpha(a):
        return pack_bgra_u8(colour, a.to(torch.uint8)[:, :, None].expand(-1, -1, 3).contiguous())
    if first:
        c, s_ = 0.8660254, 0.5                                          # a rectangle of 0.7 h x 0.7 w turned by 30 degrees
        u, v = c * y + s_ * x, -s_ * y + c * x
        return [('view', with_alpha(((u.abs() < 0.35 * h) & (v.abs() < 0.35 * w)) * 255))]
    g = torch.Generator(device='cpu').manual_seed(h * 11 + w)
    noisy = torch.randint(0, 256, (h, w), generator=g, dtype=torch.int16).to(dev)
    r = ((y / (0.309 * h)) ** 2 + (x / (0.309 * w)) ** 2).sqrt()       # pi * 0.309^2 = 0.30 of the pixels lie inside
    sprite = ((1.0 - r) * (0.309 * min(h, w)) / 8.0 + 0.5).clamp(0, 1).mul(255).round()      # an edge eight pixels wide
    cleared = with_alpha(sprite)
    cleared[:, :, :3] *= (cleared[:, :, 3:4] != 0)                      # the colour under fully transparent pixels set to 0, as many files store it
    return [('noisy', with_alpha(noisy)), ('sprite', with_alpha(sprite)), ('sprite0', cleared)]


def rgba_leg(args, say):
    import io
    from PIL import Image
    from ciaosr_amd.png_hip import encode_png
    dev = torch.device('cuda', torch.cuda.current_device())

    def pil_rgba(img):
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img.cpu().numpy()[:, :, [2, 1, 0, 3]]), 'RGBA').save(bio, format='PNG')
        return bio.getvalue()

    for k, size in enumerate(args.sizes):
        h, w = (int(v) for v in size.split('x'))
        for name, img in rgba_cases(h, w, k == 0 and 'view' in args.rgba_cases, dev):
            if name not in args.rgba_cases:
                continue
            torch.cuda.synchronize()
            legs = {'a': lambda: encode_png(img, 'bgra'), 'b': lambda: pil_rgba(img)}
            times = run_legs(args, legs)
            mine, pil = legs['a'](), legs['b']()
            same = np.array_equal(np.asarray(Image.open(io.BytesIO(mine))), np.asarray(Image.open(io.BytesIO(pil))))
            a = img[:, :, 3]
            say(f'{h} x {w} {name}: alpha 0 on {(a == 0).float().mean().item():.3f}, 255 on {(a == 255).float().mean().item():.3f} of the pixels; '
                f'decoded pixels identical: {same}; file bytes device {len(mine)}, Pillow {len(pil)} ({len(mine) / len(pil):.4f})')
            say(f'  (a) encode_png(bgra) on the device  wall s: {stats(times["a"])}')
            say(f'  (b) copy to the host + PIL save     wall s: {stats(times["b"])}')
            gap = statistics.mean(times['b']) - statistics.mean(times['a'])
            spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', 'b'))
            say(f'  (b) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                f'{"device encoder faster beyond the spread" if gap > spread else ("host encoder faster beyond the spread" if -gap > spread else "NOT separated")}; '
                f'ratio (b) / (a) {statistics.mean(times["b"]) / statistics.mean(times["a"]):.2f}x')
            say(f'  (a) kernels: {kernels(legs["a"])}')
            del img


def matches_leg(args, say):
    """The literal coder, the match coder (`matches=True`) and copy + PIL save, alternating in one process: file bytes of all three,
    wall times, and both device coders' kernel times from a profiled call of their own.  Inputs: the RGBA view at the first size, the
    four RGBA cases and the smooth and noisy RGB images at every later size."""
    import io
    from PIL import Image
    from ciaosr_amd.png_hip import encode_png
    dev = torch.device('cuda', torch.cuda.current_device())

    def pil_rgba(img):
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img.cpu().numpy()[:, :, [2, 1, 0, 3]]), 'RGBA').save(bio, format='PNG')
        return bio.getvalue()

    def view(h, w):
        img = rgba_cases(h, w, True, dev)[0][1]
        img[:, :, :3] *= (img[:, :, 3:4] != 0)                             # outside a view a render holds the fill, 0
        return img

    def cases(k, h, w):
        if 'view' in args.rgba_cases:
            yield 'view, fill 0', 'bgra', view(h, w)
        if k == 0:
            return
        for name in ('noisy', 'sprite', 'sprite0'):
            if name in args.rgba_cases:
                yield (name, 'bgra', dict(rgba_cases(h, w, False, dev))[name])
        for content in args.contents:
            yield ('RGB ' + content, 'bgr', make_image(h, w, content, dev))

    for k, size in enumerate(args.sizes):
        h, w = (int(v) for v in size.split('x'))
        for name, order, img in cases(k, h, w):
            torch.cuda.synchronize()
            legs = {'a': lambda: encode_png(img, order), 'b': lambda: encode_png(img, order, matches=True),
                    'c': (lambda: pil_rgba(img)) if order == 'bgra' else (lambda: pil_file(img, 'PNG'))}
            times = run_legs(args, legs)
            lit, lz, pil = legs['a'](), legs['b'](), legs['c']()
            same = np.array_equal(np.asarray(Image.open(io.BytesIO(lz))), np.asarray(Image.open(io.BytesIO(pil))))
            say(f'{h} x {w} {name}: decoded pixels identical: {same}; file bytes literals {len(lit)}, matches {len(lz)}, Pillow {len(pil)}; '
                f'matches / literals {len(lz) / len(lit):.4f}, matches / Pillow {len(lz) / len(pil):.4f}, literals / Pillow {len(lit) / len(pil):.4f}')
            say(f'  (a) encode_png on the device            wall s: {stats(times["a"])}')
            say(f'  (b) encode_png(matches=True)            wall s: {stats(times["b"])}')
            say(f'  (c) copy to the host + PIL save         wall s: {stats(times["c"])}')
            gap = statistics.mean(times['b']) - statistics.mean(times['a'])
            spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', 'b'))
            say(f'  (b) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                f'{"matches slower beyond the spread" if gap > spread else ("matches faster beyond the spread" if -gap > spread else "NOT separated")}; '
                f'ratio (b) / (a) {statistics.mean(times["b"]) / statistics.mean(times["a"]):.2f}x, '
                f'(c) / (b) {statistics.mean(times["c"]) / statistics.mean(times["b"]):.1f}x')
            say(f'  (a) kernels: {kernels(legs["a"])}')
            say(f'  (b) kernels: {kernels(legs["b"])}')
            del img


def grey_leg(args, say):
    """The grey device calls against the three-channel device calls on (v, v, v) and against copy + PIL save of the L image."""
    import io
    from PIL import Image
    from ciaosr_amd.jpeg_hip import encode_jpeg
    from ciaosr_amd.metrics_hip import grey_from_bgr_u8
    from ciaosr_amd.png_hip import encode_png
    dev = torch.device('cuda', torch.cuda.current_device())

    def pil_l(img, fmt, **kw):
        bio = io.BytesIO()
        Image.fromarray(img.cpu().numpy(), 'L').save(bio, format=fmt, **kw)
        return bio.getvalue()

    formats = [('PNG', lambda im: encode_png(im), lambda im: pil_l(im, 'PNG')),
               ('PNG, matches=True', lambda im: encode_png(im, matches=True), lambda im: pil_l(im, 'PNG')),
               (f'JPEG q{args.quality}', lambda im: encode_jpeg(im, quality=args.quality), lambda im: pil_l(im, 'JPEG', quality=args.quality)),
               (f'JPEG q{args.quality}, optimize=True', lambda im: encode_jpeg(im, quality=args.quality, optimize=True),
                lambda im: pil_l(im, 'JPEG', quality=args.quality, optimize=True))]
    import PIL.ImageFile
    PIL.ImageFile.MAXBLOCK = max(PIL.ImageFile.MAXBLOCK, 1 << 28)      # Pillow codes an optimised file into one buffer
    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        for content in args.contents:
            grey = grey_from_bgr_u8(make_image(h, w, content, dev))
            wide = grey.unsqueeze(2).expand(-1, -1, 3).contiguous()
            torch.cuda.synchronize()
            for name, device_call, pil_call in formats:
                legs = {'a': lambda: device_call(grey), 'b': lambda: device_call(wide), 'c': lambda: pil_call(grey)}
                times = run_legs(args, legs)
                mine, three, pil = legs['a'](), legs['b'](), legs['c']()
                if name.startswith('PNG'):
                    im = Image.open(io.BytesIO(mine))
                    same = f'mode {im.mode}, decoded pixels identical to Pillow\'s: {np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(pil))))}'
                else:
                    same = f'bytes identical to Pillow\'s: {mine == pil}'
                say(f'{h} x {w} {content}, {name}: {same}; file bytes grey {len(mine)}, three-channel {len(three)}, Pillow L {len(pil)}; '
                    f'grey / three-channel {len(mine) / len(three):.4f}, grey / Pillow {len(mine) / len(pil):.4f}')
                say(f'  (a) grey device call                    wall s: {stats(times["a"])}')
                say(f'  (b) three-channel device call, (v,v,v)  wall s: {stats(times["b"])}')
                say(f'  (c) copy to the host + PIL save of L    wall s: {stats(times["c"])}')
                for other, what in (('b', 'three-channel'), ('c', 'host')):
                    gap = statistics.mean(times[other]) - statistics.mean(times['a'])
                    spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', other))
                    say(f'  ({other}) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                        f'{"grey call faster beyond the spread" if gap > spread else (what + " call faster beyond the spread" if -gap > spread else "NOT separated")}; '
                        f'ratio ({other}) / (a) {statistics.mean(times[other]) / statistics.mean(times["a"]):.2f}x')
                say(f'  (a) kernels: {kernels(legs["a"])}')
                say(f'  (b) kernels: {kernels(legs["b"])}')
            del grey, wide


def depth16_leg(args, say):
    """The 16-bit device calls against the 8-bit device calls on the same fp32 data and, for grey, copy + PIL save of the I;16 image."""
    import io
    from PIL import Image
    from ciaosr_amd.init_utils import synthetic_gt
    from ciaosr_amd.metrics_hip import tensor2img_grey_u16, tensor2img_grey_u8, tensor2img_u16, tensor2img_u8
    from ciaosr_amd.png_hip import encode_png
    dev = torch.device('cuda', torch.cuda.current_device())

    def pil_i16(img):
        bio = io.BytesIO()
        Image.fromarray(img.cpu().numpy()).save(bio, format='PNG')                 # uint16 [H, W]: mode I;16
        return bio.getvalue()

    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        for content in args.contents:
            fp = synthetic_gt(h, w).to(dev)
            if content == 'noisy':
                g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
                for ch in range(3):                                                    # plane by plane: the host noise of one plane at a time
                    fp[..., ch, :, :] += (torch.randn(h, w, generator=g) * (2.0 / 255.0)).to(dev)
            images = {'grey16': (tensor2img_grey_u16(fp), tensor2img_grey_u8(fp)), 'RGB16': (tensor2img_u16(fp), tensor2img_u8(fp))}
            del fp
            torch.cuda.synchronize()
            for kind, (im16, im8) in images.items():
                raw = im16.numel() * 2
                for lz in (False, True):
                    legs = {'a': lambda: encode_png(im16, matches=lz), 'b': lambda: encode_png(im8, matches=lz)}
                    if kind == 'grey16':
                        legs['c'] = lambda: pil_i16(im16)
                    times = run_legs(args, legs)
                    mine, eight = legs['a'](), legs['b']()
                    line = (f'{h} x {w} {content}, {kind}, matches={lz}: file bytes 16-bit {len(mine)}, raw 2 C H W {raw}, 16-bit / raw '
                            f'{len(mine) / raw:.4f}; 8-bit file {len(eight)}, 16-bit / 8-bit {len(mine) / len(eight):.4f}')
                    if 'c' in legs:
                        pil = legs['c']()
                        same = np.array_equal(np.asarray(Image.open(io.BytesIO(mine))), np.asarray(Image.open(io.BytesIO(pil))))
                        line += f'; Pillow I;16 {len(pil)}, 16-bit / Pillow {len(mine) / len(pil):.4f}, decoded samples identical to Pillow\'s: {same}'
                    say(line)
                    say(f'  (a) 16-bit device call                    wall s: {stats(times["a"])}')
                    say(f'  (b) 8-bit device call, same fp32 data     wall s: {stats(times["b"])}')
                    if 'c' in legs:
                        say(f'  (c) copy to the host + PIL save of I;16   wall s: {stats(times["c"])}')
                    for other, what in (('b', '8-bit'), ('c', 'host')):
                        if other not in legs:
                            continue
                        gap = statistics.mean(times[other]) - statistics.mean(times['a'])
                        spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', other))
                        say(f'  ({other}) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                            f'{"16-bit call faster beyond the spread" if gap > spread else (what + " call faster beyond the spread" if -gap > spread else "NOT separated")}; '
                            f'ratio ({other}) / (a) {statistics.mean(times[other]) / statistics.mean(times["a"]):.2f}x')
                    say(f'  (a) kernels: {kernels(legs["a"])}')
                    say(f'  (b) kernels: {kernels(legs["b"])}')
            del images, im16, im8


def tiff_leg(args, say):
    """The device pyramid with and without matches against copy + PIL save of the top level as a deflate TIFF (strips, no pyramid)."""
    import io
    from PIL import Image
    from ciaosr_amd import degrade, tiff_hip
    from ciaosr_amd.init_utils import synthetic_gt
    from ciaosr_amd.metrics_hip import tensor2img_grey_u16, tensor2img_u16, tensor2img_u8
    dev = torch.device('cuda', torch.cuda.current_device())
    tile = args.tiff_tile

    def pil_tiff(top):
        arr = top.cpu().numpy()
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(arr[:, :, ::-1]) if arr.ndim == 3 else arr).save(bio, format='TIFF', compression='tiff_adobe_deflate')
        return bio.getvalue()

    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        sizes = tiff_hip.tiff_level_sizes(h, w, tile)
        for content in args.contents:
            fp = synthetic_gt(h, w).to(dev)
            if content == 'noisy':
                g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
                for ch in range(3):
                    fp[..., ch, :, :] += (torch.randn(h, w, generator=g) * (2.0 / 255.0)).to(dev)
            tops = {'RGB8': tensor2img_u8(fp), 'RGB16': tensor2img_u16(fp), 'grey16': tensor2img_grey_u16(fp)}
            del fp
            for kind, top in tops.items():
                levels = [top]
                for hl, wl in sizes[1:]:
                    levels.append(degrade.resize_bicubic_u8(top, (wl, hl)) if kind == 'RGB8' else tiff_hip.halve_box_u16(levels[-1]))
                torch.cuda.synchronize()
                raw = sum(lv.numel() * lv.element_size() for lv in levels)
                legs = {'a': lambda: tiff_hip.encode_tiff(levels, tile), 'b': lambda: tiff_hip.encode_tiff(levels, tile, matches=True)}
                if kind != 'RGB16':
                    legs['c'] = lambda: pil_tiff(top)
                times = run_legs(args, legs)
                lit, lz = legs['a'](), legs['b']()
                tiles = sum(-(-a // tile) * -(-b // tile) for a, b in sizes)
                line = (f'{h} x {w} {content}, {kind}, tile {tile}: {len(sizes)} levels, {tiles} tiles; file bytes literal {len(lit)}, matches '
                        f'{len(lz)} ({len(lz) / len(lit):.4f}), raw bytes of all levels {raw}, literal / raw {len(lit) / raw:.4f}')
                if 'c' in legs:
                    pil = legs['c']()
                    page = np.asarray(Image.open(io.BytesIO(lit)))
                    want = top.cpu().numpy()
                    same = np.array_equal(page, want[:, :, ::-1] if want.ndim == 3 else want)
                    line += (f'; Pillow (top level only, strips) {len(pil)}, literal / Pillow {len(lit) / len(pil):.4f}; top page read back by '
                             f'Pillow identical: {same}')
                say(line)
                say(f'  (a) device pyramid, matches off           wall s: {stats(times["a"])}')
                say(f'  (b) device pyramid, matches on            wall s: {stats(times["b"])}')
                if 'c' in legs:
                    say(f'  (c) copy + PIL save, top level, strips    wall s: {stats(times["c"])}')
                    gap = statistics.mean(times['c']) - statistics.mean(times['a'])
                    spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', 'c'))
                    say(f'  (c) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                        f'{"device pyramid faster beyond the spread" if gap > spread else ("host call faster beyond the spread" if -gap > spread else "NOT separated")}; '
                        f'ratio (c) / (a) {statistics.mean(times["c"]) / statistics.mean(times["a"]):.2f}x')
                gap = statistics.mean(times['b']) - statistics.mean(times['a'])
                spread = max(max(times[k_]) - min(times[k_]) for k_ in ('a', 'b'))
                say(f'  (b) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                    f'{"matches cost time beyond the spread" if gap > spread else ("matches faster beyond the spread" if -gap > spread else "NOT separated")}')
                say(f'  (a) kernels: {kernels(legs["a"])}')
                say(f'  (b) kernels: {kernels(legs["b"])}')
                del levels
            del tops, top


def jpeg_leg(args, say):
    from ciaosr_amd.jpeg_hip import SUBSAMPLINGS, encode_jpeg, encode_jpeg_tiles
    from ciaosr_amd.png_hip import encode_png
    dev = torch.device('cuda', torch.cuda.current_device())

    def run(legs):
        return run_legs(args, legs)

    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        rects = top_rects(h, w, args.tile, args.overlap)
        for content in args.contents:
            img = make_image(h, w, content, dev)
            torch.cuda.synchronize()
            png_dev, png_pil = len(encode_png(img)), len(pil_file(img, 'PNG'))
            for sub in ('444', '420'):
                legs = {'a': lambda: encode_jpeg(img, args.quality, sub), 'b': lambda: pil_file(img, 'JPEG', quality=args.quality, subsampling=SUBSAMPLINGS[sub]),
                        'c': lambda: encode_png(img)}
                times = run(legs)
                mine, pil = legs['a'](), legs['b']()
                say(f'{h} x {w} {content}, quality {args.quality}, {sub}: device file is Pillow\'s byte for byte: {mine == pil}; bytes JPEG {len(mine)}, '
                    f'device PNG {png_dev}, Pillow PNG {png_pil}')
                say(f'  (a) encode_jpeg on the device      wall s: {stats(times["a"])}')
                say(f'  (b) copy to the host + PIL JPEG    wall s: {stats(times["b"])}')
                say(f'  (c) encode_png on the device       wall s: {stats(times["c"])}')
                gap = statistics.mean(times['b']) - statistics.mean(times['a'])
                spread = max(max(times[k]) - min(times[k]) for k in ('a', 'b'))
                say(f'  (b) - (a) = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                    f'{"device encoder faster beyond the spread" if gap > spread else ("host encoder faster beyond the spread" if -gap > spread else "NOT separated")}; '
                    f'ratio (b) / (a) {statistics.mean(times["b"]) / statistics.mean(times["a"]):.2f}x')
                say(f'  (a) kernels: {kernels(legs["a"])}')
                say(f'  (c) kernels: {kernels(legs["c"])}')
                if len(rects) > 1:
                    legs = {'d': lambda: encode_jpeg_tiles(img, rects, args.quality, sub),
                            'e': lambda: [encode_jpeg(img[y0:y0 + hh, x0:x0 + ww], args.quality, sub) for y0, x0, hh, ww in rects]}
                    times = run(legs)
                    one, each = legs['d'](), legs['e']()
                    say(f'  top level at {args.tile}+{args.overlap}: {len(rects)} tiles, {sum(len(f) for f in one)} bytes of files; (d) and (e) byte for byte '
                        f'identical: {one == each}')
                    say(f'  (d) encode_jpeg_tiles, one call    wall s: {stats(times["d"])}')
                    say(f'  (e) encode_jpeg per tile           wall s: {stats(times["e"])}')
                    say(f'  ratio (e) / (d) {statistics.mean(times["e"]) / statistics.mean(times["d"]):.1f}x')
                    say(f'  (d) kernels: {kernels(legs["d"])}')
            del img


def jpeg_opt_leg(args, say):
    import io
    import PIL.ImageFile
    from PIL import Image
    from ciaosr_amd.jpeg_hip import SUBSAMPLINGS, encode_jpeg, encode_jpeg_tiles
    dev = torch.device('cuda', torch.cuda.current_device())
    PIL.ImageFile.MAXBLOCK = 1 << 26          # Pillow codes an optimised file into one buffer and refuses what does not fit its default

    def pil_tiles(img, rects, sub):
        host = np.ascontiguousarray(img.cpu().numpy()[:, :, ::-1])
        files = []
        for y0, x0, hh, ww in rects:
            bio = io.BytesIO()
            Image.fromarray(host[y0:y0 + hh, x0:x0 + ww]).save(bio, format='JPEG', quality=args.quality, subsampling=SUBSAMPLINGS[sub], optimize=True)
            files.append(bio.getvalue())
        return files

    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        rects = top_rects(h, w, args.tile, args.overlap)
        img = make_image(h, w, 'noisy', dev)
        torch.cuda.synchronize()
        for sub in ('444', '420'):
            legs = {'a': lambda: encode_jpeg(img, args.quality, sub, optimize=True), 'b': lambda: encode_jpeg(img, args.quality, sub),
                    'c': lambda: pil_file(img, 'JPEG', quality=args.quality, subsampling=SUBSAMPLINGS[sub], optimize=True)}
            times = run_legs(args, legs)
            mine, plain, pil = legs['a'](), legs['b'](), legs['c']()
            say(f'{h} x {w} noisy, quality {args.quality}, {sub}: optimised device file is Pillow\'s optimize=True file byte for byte: {mine == pil}; '
                f'bytes optimised {len(mine)}, Annex K tables {len(plain)}, ratio {len(mine) / len(plain):.4f}')
            say(f'  (a) encode_jpeg(optimize=True)         wall s: {stats(times["a"])}')
            say(f'  (b) encode_jpeg(optimize=False)        wall s: {stats(times["b"])}')
            say(f'  (c) copy to the host + PIL optimize    wall s: {stats(times["c"])}')
            say(f'  ratios of the means: (a) / (b) {statistics.mean(times["a"]) / statistics.mean(times["b"]):.2f}x, '
                f'(c) / (a) {statistics.mean(times["c"]) / statistics.mean(times["a"]):.2f}x')
            # in the rotation above (a) runs right after the Pillow leg and its host buffers: the two device legs once more, by themselves
            pair = run_legs(args, {k: legs[k] for k in ('a', 'b')})
            say(f'  (a), (b) alternating without (c)       wall s: (a) {stats(pair["a"])}')
            say(f'                                                 (b) {stats(pair["b"])}')
            say(f'  (a) kernels: {kernels(legs["a"])}')
            say(f'  (b) kernels: {kernels(legs["b"])}')
            if len(rects) > 1:
                legs = {'d': lambda: encode_jpeg_tiles(img, rects, args.quality, sub, optimize=True),
                        'e': lambda: encode_jpeg_tiles(img, rects, args.quality, sub), 'f': lambda: pil_tiles(img, rects, sub)}
                times = run_legs(args, legs)
                one, plain, pil = legs['d'](), legs['e'](), legs['f']()
                say(f'  top level at {args.tile}+{args.overlap}: {len(rects)} tiles; (d) and (f) byte for byte identical: {one == pil}; bytes of files '
                    f'optimised {sum(len(f) for f in one)}, Annex K tables {sum(len(f) for f in plain)}, '
                    f'ratio {sum(len(f) for f in one) / sum(len(f) for f in plain):.4f}')
                say(f'  (d) encode_jpeg_tiles(optimize=True)   wall s: {stats(times["d"])}')
                say(f'  (e) encode_jpeg_tiles(optimize=False)  wall s: {stats(times["e"])}')
                say(f'  (f) copy + PIL optimize per tile       wall s: {stats(times["f"])}')
                say(f'  ratios of the means: (d) / (e) {statistics.mean(times["d"]) / statistics.mean(times["e"]):.2f}x, '
                    f'(f) / (d) {statistics.mean(times["f"]) / statistics.mean(times["d"]):.2f}x')
                pair = run_legs(args, {k: legs[k] for k in ('d', 'e')})
                say(f'  (d), (e) alternating without (f)       wall s: (d) {stats(pair["d"])}')
                say(f'                                                 (e) {stats(pair["e"])}')
                say(f'  (d) kernels: {kernels(legs["d"])}')
                say(f'  (e) kernels: {kernels(legs["e"])}')
        del img


def jpeg_prog_leg(args, say):
    import io
    import PIL.ImageFile
    from PIL import Image
    from ciaosr_amd.jpeg_hip import SUBSAMPLINGS, encode_jpeg, encode_jpeg_tiles
    dev = torch.device('cuda', torch.cuda.current_device())
    PIL.ImageFile.MAXBLOCK = 1 << 26          # Pillow codes a progressive file into one buffer and refuses what does not fit its default

    def pil_tiles(img, rects, sub):
        host = np.ascontiguousarray(img.cpu().numpy()[:, :, ::-1])
        files = []
        for y0, x0, hh, ww in rects:
            bio = io.BytesIO()
            Image.fromarray(host[y0:y0 + hh, x0:x0 + ww]).save(bio, format='JPEG', quality=args.quality, subsampling=SUBSAMPLINGS[sub], progressive=True)
            files.append(bio.getvalue())
        return files

    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        rects = top_rects(h, w, args.tile, args.overlap)
        for content in (['noisy', 'flat'] if len(rects) > 1 else ['noisy']):
            img = torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev) if content == 'flat' else make_image(h, w, 'noisy', dev)
            torch.cuda.synchronize()
            for sub in ('444', '420'):
                legs = {'a': lambda: encode_jpeg(img, args.quality, sub, progressive=True), 'b': lambda: encode_jpeg(img, args.quality, sub, optimize=True),
                        'c': lambda: pil_file(img, 'JPEG', quality=args.quality, subsampling=SUBSAMPLINGS[sub], progressive=True)}
                times = run_legs(args, legs)
                mine, base, pil = legs['a'](), legs['b'](), legs['c']()
                say(f'{h} x {w} {content}, quality {args.quality}, {sub}: progressive device file is Pillow\'s progressive=True file byte for byte: '
                    f'{mine == pil}; bytes progressive {len(mine)}, optimised baseline {len(base)}, ratio {len(mine) / len(base):.4f}')
                say(f'  (a) encode_jpeg(progressive=True)      wall s: {stats(times["a"])}')
                say(f'  (b) encode_jpeg(optimize=True)         wall s: {stats(times["b"])}')
                say(f'  (c) copy to the host + PIL progressive wall s: {stats(times["c"])}')
                say(f'  ratios of the means: (a) / (b) {statistics.mean(times["a"]) / statistics.mean(times["b"]):.2f}x, '
                    f'(c) / (a) {statistics.mean(times["c"]) / statistics.mean(times["a"]):.2f}x')
                pair = run_legs(args, {k: legs[k] for k in ('a', 'b')})
                say(f'  (a), (b) alternating without (c)       wall s: (a) {stats(pair["a"])}')
                say(f'                                                 (b) {stats(pair["b"])}')
                say(f'  (a) kernels: {kernels(legs["a"])}')
                say(f'  (b) kernels: {kernels(legs["b"])}')
                if len(rects) > 1 and content == 'noisy':
                    legs = {'d': lambda: encode_jpeg_tiles(img, rects, args.quality, sub, progressive=True),
                            'e': lambda: encode_jpeg_tiles(img, rects, args.quality, sub, optimize=True), 'f': lambda: pil_tiles(img, rects, sub)}
                    times = run_legs(args, legs)
                    one, base, pil = legs['d'](), legs['e'](), legs['f']()
                    say(f'  top level at {args.tile}+{args.overlap}: {len(rects)} tiles; (d) and (f) byte for byte identical: {one == pil}; bytes of files '
                        f'progressive {sum(len(f) for f in one)}, optimised baseline {sum(len(f) for f in base)}, '
                        f'ratio {sum(len(f) for f in one) / sum(len(f) for f in base):.4f}')
                    say(f'  (d) encode_jpeg_tiles(progressive=True) wall s: {stats(times["d"])}')
                    say(f'  (e) encode_jpeg_tiles(optimize=True)    wall s: {stats(times["e"])}')
                    say(f'  (f) copy + PIL progressive per tile     wall s: {stats(times["f"])}')
                    say(f'  ratios of the means: (d) / (e) {statistics.mean(times["d"]) / statistics.mean(times["e"]):.2f}x, '
                        f'(f) / (d) {statistics.mean(times["f"]) / statistics.mean(times["d"]):.2f}x')
                    say(f'  (d) kernels: {kernels(legs["d"])}')
                    say(f'  (e) kernels: {kernels(legs["e"])}')
            del img


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--leg', default='files', choices=['files', 'tiles', 'jpeg', 'jpeg-opt', 'jpeg-prog', 'rgba', 'matches', 'grey', 'depth16', 'tiff'])
    p.add_argument('--parent-root', default=None, help='tiles: a built checkout of the parent commit for leg (a)')
    p.add_argument('--root', default=None, help='the tree whose package and library run (the parent-tree child)')
    p.add_argument('--worker', action='store_true', help='serve leg (a) on stdin / stdout (the parent-tree child)')
    p.add_argument('--dzi', action='store_true', help='tiles: also one full write_dzi of the bench output')
    p.add_argument('--tile', type=int, default=254)
    p.add_argument('--overlap', type=int, default=1)
    p.add_argument('--tiff-tile', type=int, default=256, help='tiff: the tile side')
    p.add_argument('--quality', type=int, default=90, help='jpeg: the quality of every JPEG file')
    p.add_argument('--sizes', nargs='+', default=None)
    p.add_argument('--contents', nargs='+', default=['smooth', 'noisy'], choices=['smooth', 'noisy'])
    p.add_argument('--rgba-cases', nargs='+', default=['view', 'noisy', 'sprite', 'sprite0'], choices=['view', 'noisy', 'sprite', 'sprite0'],
                   help='rgba: the cases to run (view on the first size, the others on every later size)')
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--out', default=None)
    p.add_argument('--append', action='store_true', help='add to --out instead of replacing it (a run split over several calls)')
    args = p.parse_args(argv)
    if args.root:
        sys.path.insert(0, args.root)
    if args.worker:
        return serve()
    tiles = args.leg == 'tiles'
    jpeg = args.leg in ('jpeg', 'jpeg-opt', 'jpeg-prog')
    if args.leg in ('jpeg-opt', 'jpeg-prog'):
        args.contents = ['noisy']
    rgba = args.leg in ('rgba', 'matches')
    grey = args.leg == 'grey'
    if grey:                                                 # sizes and file of its own; the shared tail below is the jpeg legs'
        args.sizes = args.sizes or ['5424x8160', '768x768']
        args.out = args.out or os.path.join(REPO, 'profiles', 'grey_codecs.txt')
        jpeg = True
    if args.leg == 'depth16':                                # likewise
        args.sizes = args.sizes or ['5424x8160', '768x768']
        args.out = args.out or os.path.join(REPO, 'profiles', 'png_depth16.txt')
        jpeg = True
    if args.leg == 'tiff':                                   # likewise
        args.sizes = args.sizes or ['5424x8160', '768x768']
        args.out = args.out or os.path.join(REPO, 'profiles', 'tiff_gpu.txt')
        jpeg = True
    args.sizes = args.sizes or (['5424x8160'] if tiles else ['768x768', '5424x8160'] if rgba else ['5424x8160', '768x768'])
    args.out = args.out or os.path.join(REPO, 'profiles', 'png_tiles.txt' if tiles else 'png_matches.txt' if args.leg == 'matches' else 'png_rgba.txt' if rgba else ('jpeg_opt.txt' if args.leg == 'jpeg-opt' else 'jpeg_prog.txt' if args.leg == 'jpeg-prog' else 'jpeg_gpu.txt' if jpeg else 'png_gpu.txt'))
    from ciaosr_amd import _lib, hip_ops
    from ciaosr_amd.imageio import imread_u8, imwrite
    from ciaosr_amd.png_hip import imwrite_gpu
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/png_probe.py{" --leg " + args.leg if tiles or jpeg or rgba else ""} --sizes {" ".join(args.sizes)} --contents {" ".join(args.contents)} --warmup {args.warmup} --rounds {args.rounds}: '
        f'library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}, {os.cpu_count()} host CPUs visible')
    if tiles:
        tiles_leg(args, say)
    if args.leg == 'rgba':
        rgba_leg(args, say)
    if args.leg == 'matches':
        matches_leg(args, say)
    if args.leg == 'jpeg':
        jpeg_leg(args, say)
    if args.leg == 'jpeg-opt':
        jpeg_opt_leg(args, say)
    if args.leg == 'jpeg-prog':
        jpeg_prog_leg(args, say)
    if grey:
        grey_leg(args, say)
    if args.leg == 'depth16':
        depth16_leg(args, say)
    if args.leg == 'tiff':
        tiff_leg(args, say)
    with tempfile.TemporaryDirectory() as tmp:
        for size in ([] if tiles or jpeg or rgba else args.sizes):
            h, w = (int(v) for v in size.split('x'))
            for content in args.contents:
                img = make_image(h, w, content, dev)
                torch.cuda.synchronize()
                paths = dict(host=os.path.join(tmp, 'host.png'), device=os.path.join(tmp, 'device.png'))
                legs = dict(host=lambda: imwrite(img.cpu().numpy(), paths['host']), device=lambda: imwrite_gpu(img, paths['device']))
                times = dict(host=[], device=[])
                for r in range(args.warmup + args.rounds):
                    took = {}
                    for name in ('host', 'device'):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        legs[name]()
                        took[name] = time.perf_counter() - t0
                        if r >= args.warmup:
                            times[name].append(took[name])
                    print(f'  {size} {content} round {r} ({"timed" if r >= args.warmup else "warm-up"}): host {took["host"]:.4f} s, '
                          f'device {took["device"]:.4f} s', flush=True)
                same = np.array_equal(imread_u8(paths['host']), imread_u8(paths['device']))
                sizes = {k: os.path.getsize(v) for k, v in paths.items()}
                with hip_ops.profile():
                    imwrite_gpu(img, paths['device'])
                prof = hip_ops.profile.results()
                say(f'{h} x {w} {content}: decoded pixels identical: {same}; file bytes host {sizes["host"]}, device {sizes["device"]} '
                    f'({sizes["device"] / sizes["host"]:.4f})')
                for name in ('host', 'device'):
                    t = times[name]
                    say(f'  {name:6s} wall s: mean {statistics.mean(t):.4f}, min {min(t):.4f}, max {max(t):.4f}, spread {max(t) - min(t):.4f}  '
                        f'[{" ".join(f"{v:.4f}" for v in t)}]')
                gap = statistics.mean(times['host']) - statistics.mean(times['device'])
                spread = max(max(t) - min(t) for t in times.values())
                say(f'  host - device = {gap:.4f} s, larger round-to-round spread {spread:.4f} s: '
                    f'{"device writer faster beyond the spread" if gap > spread else "NOT separated"}; '
                    f'speed-up {statistics.mean(times["host"]) / statistics.mean(times["device"]):.1f}x')
                say('  device kernels, one call, ms: ' + ', '.join(f'{k} {v["total_ms"]:.3f}' for k, v in sorted(prof.items())))
                del img
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
