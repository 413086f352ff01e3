"""Encode once, render many: wall times of CiaoSR.encode / render against CiaoSR.restore on the C3 tile (RDN-CiaoSR, one 192 x 192 LR
image) and the C2 image (48 x 48), fp32 and f16, whole-image test_cfg, one process on one GPU (profiles/scene_render.txt).

Per size and precision, after two warm-up passes of every call: `--reps` rounds in which the calls alternate (restore x4, render x4,
restore x2, render x2, ..., encode), each call between two device synchronisations.  Reported per call: mean, min and max in ms; per
scale the ratio render / restore of the means and of the minima.  `restore` is the path of every earlier version; a full-grid render
from a ready scene runs a strict subset of its launches (no trunk, cs_attn or tables), so it must not come out slower beyond the
min-max spread shown.  Also: the scene's bytes and the peak allocated memory of a render-only loop against a restore-only loop.

`--legs view` (profiles/view_render.txt) instead times CiaoSR.render_view on the first of `--sizes` (the C3 tile: one 192 x 192 LR image,
whole-image test_cfg, scene planned for x4), per precision, three legs alternating in one process, each call between two device
synchronisations: an angle-0 view and a 30-degree view of `--view-size` (768) squared about the image centre at zoom x4, and the window
render of that size from the same scene.  Per leg: wall time (mean, min, max over `--reps` rounds after two warm-up rounds, profiler
off), and from one more round under hip_ops.profile the device time of the view kernels (count + select + blend + finalize), of the
coordinate kernels and of the head query (every other launch of the call but denorm_clamp).  Two more legs alternate with these: the
30-degree view with `test_cfg.view_blocks` off (the leg above, named again) and on.  For them a second table (with `--out` also written
to that file: profiles/view_blocks.txt) holds per precision and leg the wall time, the head query's device time, the pad share
8 * blocks / members - 1 of the block list, and the flag of the leg's head query (`PackedHead.query(..., return_flag=True)` on the
list the leg selects: 1 = the chained 16-bit kernel gave the launch up to the gated 128-row kernel; n/a where no chained kernel runs).

`--legs warp` (profiles/warp_render.txt, with `--out`): the affine-degenerate homography, the same points as a map, and `render_view` of
that matrix, alternating, by the protocol of the view legs (`warp_legs`).
`--legs warp-pp` (profiles/warp_pp.txt, with `--out`): a projective homography with its centre footprint, with a footprint per output
pixel, and as a map with differences, alternating, by the same protocol (`warp_pp_legs`).
`--legs warp-area` (profiles/warp_area.txt, with `--out`): a homography that minifies its far side as a per-pixel warp with
`minify='clamp'`, with `minify='area'`, and as the 4 x 4 times finer single-footprint warp box-averaged with torch (`warp_area_legs`).

`--legs many` (profiles/render_many.txt, with `--out`) is the tiled image of bench.py -- LR 1356 x 2040, tile 192 / overlap 32,
`tile_any_scale`: 9 x 13 = 117 tiles -- rendered at x2, x3.3 and x4 (full grids) from one encode, per precision and for two scene caches
(the default `scene_cache_mb`, and one that holds every scene):
  (a) three `render` calls in a row with the PARENT commit's package and library: a child process of this job on `--parent-root DIR`
      (a built checkout of the parent commit), kept alive and told when to run a round, so that its rounds alternate with (b) and (c)
  (b) one `render_many` of the three targets (this tree)
  (c) `restore` at x4 (this tree), for scale
One warm-up round of every leg, then `--reps` rounds in which the legs alternate; every round starts from a fresh `encode`, is timed
between two device synchronisations, and reports `cache.builds`.  Without `--parent-root`, leg (a) runs this tree's `render` in the
same process.  A second table: 16 views of `--view-size` squared along a pan across the image at x4, as 16 `render_view` calls and as
one `render_many`: wall time and the number of synchronising device-to-host copies (counted around Tensor.tolist)."""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='192,48')
ap.add_argument('--precisions', default='fp32,f16')
ap.add_argument('--scales', default='4,2,3.3')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--legs', default='scene', choices=('scene', 'view', 'many', 'warp', 'warp-pp', 'warp-area'))
ap.add_argument('--view-size', type=int, default=768)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='tree whose package and library run')
ap.add_argument('--parent-root', default=None, help='--legs many: a built checkout of the parent commit for leg (a)')
ap.add_argument('--worker', action='store_true', help='--legs many: serve leg (a) rounds on stdin / stdout (the parent-tree child)')
ap.add_argument('--out', default=None, help='--legs many: also write the report to this file; --legs view: the view_blocks table')
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import ciaosr_amd  # noqa: E402
from ciaosr_amd import _lib, hip_ops  # noqa: E402
from ciaosr_amd.config import Config  # noqa: E402
from ciaosr_amd.init_utils import seeded_init_, synthetic_pair  # noqa: E402

dev = torch.device('cuda:0')
cfg = Config.fromfile(os.path.join(os.path.abspath(args.root), 'configs',
                                   '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py'))
model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=dict(scale=4))
seeded_init_(model, seed=0, gain=1.0)
model = model.to(dev).eval()
if not args.worker:
    print(f'library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}, reps {args.reps}')


def timed(fn):
    gc.collect()                # an encode result is a reference cycle: a dropped round's scenes go now, not at the collector's next full pass
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def peak_of(fn, n=2):
    hip_ops.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(n):
        fn()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def view_query_flag(enc, m, n, size, blocks):
    """(flag, members, list length) of the head query a 30-degree leg makes: its member list of the one frame, selected as the leg does."""
    frame = (0, 0, size, size)
    tiles = torch.tensor([frame], dtype=torch.int32).to(dev)
    scene = enc.cache.get((0, None))
    if blocks:
        counts, ws = hip_ops.view_count_blocks(m, n, n, tiles)
        members, n_blk = counts.tolist()[0]
        _, coord, cell = hip_ops.view_select_blocks(m, n, n, frame, 0, 1, ws, n_blk)
    else:
        counts, ws = hip_ops.view_count(m, n, n, tiles)
        members = counts.tolist()[0]
        _, coord, cell = hip_ops.view_select(m, n, n, frame, 0, 1, ws, members)
    flag = 'n/a'
    if scene.scenes[0].chained:
        flag = str(int(model.generator.render(scene, coord, cell, return_flags=True)[1][0]))
    return flag, members, coord.shape[0]


def view_legs():
    from ciaosr_amd.scene import view_blocks_fit, view_matrix
    report = [f'tools/scene_probe.py --legs view --reps {args.reps}: library version {_lib.load().ciaosr_version()}, '
              f'{torch.cuda.get_device_name(0)}; the 30-degree view with test_cfg.view_blocks off and on, alternating with the other legs '
              f'in one process (2 warm-up rounds, {args.reps} timed rounds)']
    size, n = int(args.sizes.split(',')[0]), args.view_size
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    groups = (('view kernels', lambda k: k.startswith('view_') and k != 'view_coord_cell'),
              ('coordinates', lambda k: k in ('view_coord_cell', 'make_coord_cell_window', 'make_coord_cell')),
              ('head query', lambda k: not k.startswith(('view_', 'make_coord_cell')) and k != 'denorm_clamp'))
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        enc = model.encode(lq)
        off = (size * 4 - n) // 2
        m30 = view_matrix((size / 2, size / 2), 4.0, 30, (n, n))

        def with_blocks():
            model.test_cfg['view_blocks'] = True
            try:
                return model.render_view(enc, m30, (n, n))
            finally:
                model.test_cfg['view_blocks'] = False

        calls = {'view   0 deg': lambda: model.render_view(enc, view_matrix((size / 2, size / 2), 4.0, 0, (n, n)), (n, n)),
                 'view  30 deg': lambda: model.render_view(enc, m30, (n, n)),
                 'view  30 blk': with_blocks,
                 'window render': lambda: model.render(enc, size=(size * 4, size * 4), window=(off, off, n, n))}
        a, b = calls['view   0 deg'](), calls['window render']()
        print(f'\n{size}x{size} LR, {precision}, {n} x {n} output at x4: angle-0 view against the window render: max |diff| = '
              f'{(a - b).abs().max().item():.3e}; 30-degree view: {(calls["view  30 deg"]().sum(1) == 0).float().mean().item():.1%} of the pixels outside')
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn)[0])
        for k, fn in calls.items():
            with hip_ops.profile():
                fn()
            prof = hip_ops.profile.results()
            v = times[k]
            parts = ', '.join(f'{name} {sum(r["total_ms"] for kk, r in prof.items() if pick(kk)):8.3f} ms '
                              f'({sum(r["launches"] for kk, r in prof.items() if pick(kk))} launches)' for name, pick in groups)
            print(f'    {k:14s} wall mean {sum(v) / len(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f} | device: {parts}')
            if k in ('view  30 deg', 'view  30 blk'):
                blocks = k == 'view  30 blk' and view_blocks_fit(m30) and enc.cache.get((0, None)).scenes[0].chained
                flag, members, length = view_query_flag(enc, m30, n, size, blocks)
                head_ms = sum(r['total_ms'] for kk, r in prof.items() if groups[2][1](kk))
                report.append(f'    {size}x{size} LR {precision:5s} {n} x {n} at x4, 30 deg, view_blocks {"on " if k.endswith("blk") else "off"}: '
                              f'wall mean {sum(v) / len(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f} | head query {head_ms:8.3f} ms | '
                              f'members {members}, list {length} ({"blocks" if blocks else "index order"}), pad share '
                              f'{length / members - 1:.4f} | flag {flag}')
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
    print()
    print('\n'.join(report))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(report) + '\n')


def warp_legs():
    """`--legs warp`: per precision three legs alternating in one process on the first of `--sizes` (the C3 tile, whole-image test_cfg,
    scene planned for x4), `--view-size` squared at zoom x4 turned by 30 degrees: the affine-degenerate homography, the same points as
    a map, and `render_view` of that matrix -- all three the same picture, bit for bit.  2 warm-up rounds, `--reps` timed rounds, wall
    time between device synchronisations; one more round under hip_ops.profile gives the device time of the warp / view kernels, of the
    coordinate kernels and of the head query.  With `--out` the report is also written to that file (profiles/warp_render.txt)."""
    from ciaosr_amd.scene import homography_of_view, view_matrix, warp_footprint
    size, n = int(args.sizes.split(',')[0]), args.view_size
    report = [f'tools/scene_probe.py --legs warp --reps {args.reps}: library version {_lib.load().ciaosr_version()}, '
              f'{torch.cuda.get_device_name(0)}; {size}x{size} LR, {n} x {n} output at x4 turned by 30 degrees, three legs alternating in one '
              f'process (2 warm-up rounds, {args.reps} timed rounds)']
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    groups = (('warp / view kernels', lambda k: k.startswith(('view_', 'warp_')) and k not in ('view_coord_cell', 'warp_coord_cell')),
              ('coordinates', lambda k: k in ('view_coord_cell', 'warp_coord_cell')),
              ('head query', lambda k: not k.startswith(('view_', 'warp_', 'make_coord_cell')) and k != 'denorm_clamp'))
    m = view_matrix((size / 2, size / 2), 4.0, 30, (n, n))
    h = homography_of_view(m)
    fp = warp_footprint(h, (n, n))
    v = (torch.arange(n, dtype=torch.float64, device=dev) + 0.5).view(n, 1)
    u = (torch.arange(n, dtype=torch.float64, device=dev) + 0.5).view(1, n)
    points = torch.stack([(m[0] * v + m[1] * u) + m[2], (m[3] * v + m[4] * u) + m[5]], -1).contiguous()
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        enc = model.encode(lq)
        calls = {'homography': lambda: model.render_warp(enc, homography=h, size=(n, n)),
                 'map': lambda: model.render_warp(enc, map=points, footprint=fp),
                 'render_view': lambda: model.render_view(enc, m, (n, n))}
        outs = {k: fn() for k, fn in calls.items()}
        same = all(torch.equal(outs[k], outs['render_view']) for k in ('homography', 'map'))
        report.append(f'  {precision}: both warps bitwise render_view: {same}; {(outs["render_view"].sum(1) == 0).float().mean().item():.1%} of '
                      f'the pixels outside')
        del outs
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn)[0])
        for k, fn in calls.items():
            with hip_ops.profile():
                fn()
            prof = hip_ops.profile.results()
            t = times[k]
            parts = ', '.join(f'{name} {sum(r["total_ms"] for kk, r in prof.items() if pick(kk)):8.3f} ms '
                              f'({sum(r["launches"] for kk, r in prof.items() if pick(kk))} launches)' for name, pick in groups)
            report.append(f'    {k:12s} wall mean {sum(t) / len(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f} | device: {parts}')
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
    print('\n'.join(report))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(report) + '\n')


def warp_pp_legs():
    """`--legs warp-pp`: the warp legs' protocol (the C3 tile, whole-image test_cfg, scene planned for x4, `--view-size` squared, 2
    warm-up + `--reps` timed rounds, legs alternating in one process, one profiled round per leg) on a projective homography -- zoom
    x3 turned by 30 degrees with the last row of the test warps scaled to the output, so that most footprints lie above the default
    lower clamp 1 / 4 of the x4 plan -- with its centre footprint, with
    `footprint='per-pixel'`, and as a map with differences.  The comparison is against the single-footprint leg of the same run.  With
    `--out` the report is also written to that file (profiles/warp_pp.txt)."""
    from ciaosr_amd.scene import FP_JACOBIAN, PerPixel, view_matrix, warp_footprint
    size, n = int(args.sizes.split(',')[0]), args.view_size
    report = [f'tools/scene_probe.py --legs warp-pp --reps {args.reps}: library version {_lib.load().ciaosr_version()}, '
              f'{torch.cuda.get_device_name(0)}; {size}x{size} LR, {n} x {n} output, three legs alternating in one process (2 warm-up '
              f'rounds, {args.reps} timed rounds)']
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    coords = ('view_coord_cell', 'warp_coord_cell', 'warp_pp_coord_cell')
    groups = (('warp kernels', lambda k: k.startswith(('view_', 'warp_')) and k not in coords),
              ('coordinates', lambda k: k in coords),
              ('head query', lambda k: not k.startswith(('view_', 'warp_', 'make_coord_cell')) and k != 'denorm_clamp'))
    h = (*view_matrix((size / 2, size / 2), 3.0, 30, (n, n)), 0.0025 * 61 / n, -0.002 * 83 / n, 1.0)
    v = (torch.arange(n, dtype=torch.float64, device=dev) + 0.5).view(n, 1)
    u = (torch.arange(n, dtype=torch.float64, device=dev) + 0.5).view(1, n)
    d = (h[6] * v + h[7] * u) + h[8]
    points = torch.stack([((h[0] * v + h[1] * u) + h[2]) / d, ((h[3] * v + h[4] * u) + h[5]) / d], -1).contiguous()
    raw = hip_ops.warp_footprints(h, None, PerPixel(FP_JACOBIAN, (1e-6, 1e6)), n, n, dev)
    fp = warp_footprint(h, (n, n))
    report.append(f'  footprints: centre {fp[0]:.4f} x {fp[1]:.4f}, per pixel {raw.min().item():.4f} .. {raw.max().item():.4f}; the default range '
                  f'(0.25, 1.0) clamps {(raw < 0.25).any(-1).float().mean().item():.1%} of the pixels at lo')
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        enc = model.encode(lq)
        calls = {'centre': lambda: model.render_warp(enc, homography=h, size=(n, n)),
                 'per-pixel': lambda: model.render_warp(enc, homography=h, size=(n, n), footprint='per-pixel'),
                 'map, differences': lambda: model.render_warp(enc, map=points, footprint='per-pixel')}
        outs = {k: fn() for k, fn in calls.items()}
        report.append(f'  {precision}: max |per-pixel - centre| = {(outs["per-pixel"] - outs["centre"]).abs().max().item():.3e}, max |map - '
                      f'per-pixel| = {(outs["map, differences"] - outs["per-pixel"]).abs().max().item():.3e}; '
                      f'{(outs["centre"].sum(1) == 0).float().mean().item():.1%} of the pixels outside')
        del outs
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn)[0])
        for k, fn in calls.items():
            with hip_ops.profile():
                fn()
            prof = hip_ops.profile.results()
            t = times[k]
            parts = ', '.join(f'{name} {sum(r["total_ms"] for kk, r in prof.items() if pick(kk)):8.3f} ms '
                              f'({sum(r["launches"] for kk, r in prof.items() if pick(kk))} launches)' for name, pick in groups)
            report.append(f'    {k:16s} wall mean {sum(t) / len(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f} | device: {parts}')
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
    print('\n'.join(report))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(report) + '\n')


def warp_area_legs():
    """`--legs warp-area`: the warp legs' protocol (the C3 tile, whole-image test_cfg, scene planned for x4, `--view-size` squared, 2
    warm-up + `--reps` timed rounds, legs alternating in one process, one profiled round per leg) on a projective homography that looks
    along the image like a floor -- x2 at the near edge, its far side minified -- as a per-pixel warp with `minify='clamp'`, with
    `minify='area'` (max_samples 4), and as the caller's alternative: the single-footprint warp of the 4 x 4 times finer grid, box-averaged
    with torch.  Reports the histogram of the samples per axis, S, and the inside samples each leg asks of the head.  With `--out` the
    report is also written to that file (profiles/warp_area.txt)."""
    from ciaosr_amd.scene import FP_JACOBIAN, PerPixel, view_matrix, warp_footprint
    size, n, n_max = int(args.sizes.split(',')[0]), args.view_size, 4
    report = [f'tools/scene_probe.py --legs warp-area --reps {args.reps}: library version {_lib.load().ciaosr_version()}, '
              f'{torch.cuda.get_device_name(0)}; {size}x{size} LR, {n} x {n} output, three legs alternating in one process (2 warm-up '
              f'rounds, {args.reps} timed rounds)']
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    rng = (0.25, 1.0)
    h = (*view_matrix((size / 2, size / 2), 2.0, 0, (n, n)), -0.7 / n, -0.15 / n, 1.0)      # D = 0.15 at the far corner: no horizon
    fine_h = tuple(c / n_max if k % 3 < 2 else c for k, c in enumerate(h))
    fine_fp = tuple(min(max(f, rng[0]), rng[1]) for f in warp_footprint(fine_h, (n_max * n, n_max * n)))
    spec = PerPixel(FP_JACOBIAN, rng, None, n_max)
    tiles = torch.tensor([(0, 0, size, size)], dtype=torch.int32).to(dev)
    first, n_yx = hip_ops.warp_area_table(h, spec, n, n, dev)
    counts, _ = hip_ops.warp_area_count(h, spec, n, n, tiles)
    inside_samples, n_samples, _ = counts.tolist()
    inside_px = hip_ops.warp_pp_count(h, None, PerPixel(FP_JACOBIAN, rng), n, n, tiles)[0].tolist()[0]
    inside_fine = hip_ops.warp_count(fine_h, None, fine_fp, n_max * n, n_max * n, tiles)[0].tolist()[0]
    hist = ', '.join(f'n_{ax} ' + ' / '.join(str(int((n_yx[..., k] == v).sum())) for v in (1, 2, 4)) for k, ax in enumerate('yx'))
    report.append(f'  samples per axis over 1 / 2 / 4: {hist}; S = {n_samples} samples for {n * n} pixels; the head answers {inside_px} '
                  f'queries (clamp), {inside_samples} (area), {inside_fine} (the {n_max * n} x {n_max * n} grid)')
    chunk = _lib.load().ciaosr_view_block_queries()
    report.append(f'  the count launches {-(-n * n * n_max * n_max // chunk)} workgroups of {chunk} sample ids, the blocks of the largest S; '
                  f'{-(-n_samples // chunk)} hold a sample; workspace {hip_ops.warp_area_workspace_bytes(n, n, 1, n_max) / 2 ** 20:.1f} MiB')
    groups = (('count (table included)', lambda k: k in ('warp_area_count', 'warp_pp_count', 'warp_count')),
              ('count + select + blend + resolve', lambda k: k.startswith(('view_', 'warp_')) or k == 'denorm_clamp'),
              ('head query', lambda k: not k.startswith(('view_', 'warp_', 'make_coord_cell')) and k != 'denorm_clamp'))
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        enc = model.encode(lq)
        pp = dict(homography=h, size=(n, n), footprint='per-pixel', footprint_range=rng)

        def alternative():
            fine = model.render_warp(enc, homography=fine_h, size=(n_max * n, n_max * n), footprint=fine_fp)
            return fine.view(1, 3, n, n_max, n, n_max).mean((3, 5))

        calls = {'clamp': lambda: model.render_warp(enc, **pp), 'area': lambda: model.render_warp(enc, minify='area', max_samples=n_max, **pp),
                 'fine grid + box': alternative}
        outs = {k: fn() for k, fn in calls.items()}
        report.append(f'  {precision}: max |area - clamp| = {(outs["area"] - outs["clamp"]).abs().max().item():.3e}, max |area - fine grid| = '
                      f'{(outs["area"] - outs["fine grid + box"]).abs().max().item():.3e}')
        del outs
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn)[0])
        for k, fn in calls.items():
            with hip_ops.profile():
                fn()
            prof = hip_ops.profile.results()
            t = times[k]
            parts = ', '.join(f'{name} {sum(r["total_ms"] for kk, r in prof.items() if pick(kk)):8.3f} ms '
                              f'({sum(r["launches"] for kk, r in prof.items() if pick(kk))} launches)' for name, pick in groups)
            report.append(f'    {k:16s} wall mean {sum(t) / len(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f} | device: {parts}')
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
    print('\n'.join(report))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(report) + '\n')


MANY_LR, MANY_SCALES = (1356, 2040), (2.0, 3.3, 4.0)


def many_cfg(precision, cache_mb):
    cfg = dict(scale=4, tile=192, tile_overlap=32, tile_any_scale=True, precision=precision)
    if cache_mb:
        cfg['scene_cache_mb'] = int(cache_mb)
    return cfg


def three_renders(lq):
    """Leg (a): encode, then one `render` per scale.  -> (wall ms, scene builds)"""
    def run():
        enc = model.encode(lq, max_scale=4)
        for s in MANY_SCALES:
            model.render(enc, scale=s)
        return enc.cache.builds
    return timed(run)


def many_worker():
    """The parent-tree child: `cfg <precision> <cache_mb or 0>` sets the test_cfg, `round` runs leg (a) once and answers one JSON line."""
    lq = synthetic_pair(*MANY_LR, 4)[0].to(dev)
    print(json.dumps(dict(version=_lib.load().ciaosr_version())), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == 'quit':
            break
        if cmd[0] == 'cfg':
            model.test_cfg = many_cfg(cmd[1], int(cmd[2]))
            hip_ops.release_workspaces()
            torch.cuda.empty_cache()
            print(json.dumps(dict(ok=True)), flush=True)
        elif cmd[0] == 'round':
            ms, builds = three_renders(lq)
            print(json.dumps(dict(ms=ms, builds=builds)), flush=True)


def many_legs():
    from ciaosr_amd.scene import Grid, View, view_matrix
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    child = None
    if args.parent_root:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--legs', 'many', '--worker', '--root', args.parent_root],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def ask(cmd):
            child.stdin.write(cmd + '\n')
            child.stdin.flush()
            answer = child.stdout.readline()
            if not answer:
                raise SystemExit(f'the parent-tree child ended (exit status {child.wait()})')
            return json.loads(answer)
        parent_version = json.loads(child.stdout.readline())['version']
    lq = synthetic_pair(*MANY_LR, 4)[0].to(dev)
    h, w = MANY_LR
    n_tiles = len(ciaosr_amd.scene.plan_view(h, w, 192, 32, any_scale=True))
    say(f'tools/scene_probe.py --legs many --reps {args.reps}: library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}; '
        f'LR {h} x {w}, tile 192 / overlap 32 ({n_tiles} tiles), targets x2, x3.3, x4 full grids')
    say('leg (a): ' + (f'three render calls, parent commit (library version {parent_version}) in a child process' if child else
                      'three render calls, THIS tree in this process (no --parent-root given)'))
    targets = [Grid(scale=s) for s in MANY_SCALES]

    def leg_b():
        def run():
            enc = model.encode(lq, max_scale=4)
            model.render_many(enc, targets)
            return enc.cache.builds
        return timed(run)

    def leg_c():
        return timed(lambda: model.restore(lq))[0], 0

    def leg_a():
        if child:
            r = ask('round')
            return r['ms'], r['builds']
        return three_renders(lq)

    legs = (('(a) 3 x render', leg_a), ('(b) render_many', leg_b), ('(c) restore x4', leg_c))
    everything = 117 * 520                       # MiB: above 117 fp32 tile scenes of 491 MiB
    for precision in args.precisions.split(','):
        for cache_mb, label in ((0, 'default cache (4096 MiB)'), (everything, f'cache that holds everything ({everything} MiB)')):
            model.test_cfg = many_cfg(precision, cache_mb)
            if child:
                ask(f'cfg {precision} {cache_mb}')
            hip_ops.release_workspaces()
            torch.cuda.empty_cache()
            for _, fn in legs:                   # warm-up
                fn()
            times = {name: [] for name, _ in legs}
            builds = {name: [] for name, _ in legs}
            for _ in range(args.reps):
                for name, fn in legs:
                    ms, n = fn()
                    times[name].append(ms)
                    builds[name].append(n)
            say(f'\n{precision}, {label}:')
            for name, _ in legs:
                v = times[name]
                say(f'    {name:16s} wall mean {sum(v) / len(v):10.1f} ms  min {min(v):10.1f}  max {max(v):10.1f}   scene builds per round {sorted(set(builds[name]))}')
            a, b = times['(a) 3 x render'], times['(b) render_many']
            say(f'    render_many / three renders: {sum(b) / sum(a):.3f} of the means, {min(b) / min(a):.3f} of the minima')
    if child:
        child.stdin.write('quit\n')
        child.stdin.flush()
        child.wait(timeout=60)
    # 16 views along a pan: synchronising copies
    n = args.view_size
    views = [View(view_matrix((h / 2, n / 8 + k * (w - n / 4) / 15), 4.0, 0, (n, n)), (n, n)) for k in range(16)]
    copies = [0]
    tolist = torch.Tensor.tolist

    def counting(t):
        copies[0] += int(t.is_cuda)
        return tolist(t)

    say(f'\n16 views of {n} x {n} along a pan at x4 (centre row {h / 2:g}, columns {n / 8:g} .. {w - n / 8:g}), fresh encode per round:')
    for precision in args.precisions.split(','):
        model.test_cfg = many_cfg(precision, 0)

        def singles():
            enc = model.encode(lq, max_scale=4)
            for v in views:
                model.render_view(enc, v.matrix, v.size)
            return enc.cache.builds

        def many():
            enc = model.encode(lq, max_scale=4)
            model.render_many(enc, views)
            return enc.cache.builds
        pan = (('16 x render_view', singles), ('render_many', many))
        for _, fn in pan:
            fn()
        times = {name: [] for name, _ in pan}
        seen = {}
        for _ in range(args.reps):
            for name, fn in pan:
                copies[0] = 0
                torch.Tensor.tolist = counting
                try:
                    ms, nb = timed(fn)
                finally:
                    torch.Tensor.tolist = tolist
                times[name].append(ms)
                seen[name] = (copies[0], nb)
        for name, _ in pan:
            v = times[name]
            say(f'    {precision:5s} {name:17s} wall mean {sum(v) / len(v):9.1f} ms  min {min(v):9.1f}  max {max(v):9.1f}   '
                f'synchronising copies {seen[name][0]}, scene builds {seen[name][1]}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


scales = [float(s) for s in args.scales.split(',')]
if args.legs == 'view':
    view_legs()
if args.legs == 'warp':
    warp_legs()
if args.legs == 'warp-pp':
    warp_pp_legs()
if args.legs == 'warp-area':
    warp_area_legs()
if args.legs == 'many':
    many_worker() if args.worker else many_legs()
for size in (int(v) for v in args.sizes.split(',') if args.legs == 'scene'):
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        grids = {s: (round(size * s), round(size * s)) for s in scales}
        cc = {s: tuple(t.unsqueeze(0) for t in hip_ops.make_coord_cell(*grids[s], dev)) for s in scales}
        n8 = round(size * 8)
        win = (n8 // 4, n8 // 4, min(512, n8), min(512, n8))
        enc = model.encode(lq)
        calls = {}
        for s in scales:
            calls[f'restore x{s:g}'] = lambda s=s: model.restore(lq, *cc[s])
            calls[f'render  x{s:g}'] = lambda s=s: model.render(enc, size=grids[s])
        calls[f'render  x8 window {win[2]}x{win[3]}'] = lambda: model.render(enc, size=(n8, n8), window=win)
        calls['encode'] = lambda: model.encode(lq)
        for s in scales:                                   # same image, or the comparison means nothing
            assert torch.equal(calls[f'restore x{s:g}'](), calls[f'render  x{s:g}']()), (size, precision, s)
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn)[0])
        print(f'\n{size}x{size} LR, {precision}: scene {enc.scene_bytes / 2 ** 20:.1f} MiB ({enc.scene_bytes / size / size:.0f} B per LR pixel), '
              f'planned for x{enc.max_scale:g}')
        for k, v in times.items():
            print(f'    {k:28s} mean {sum(v) / len(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}')
        for s in scales:
            a, b = times[f'render  x{s:g}'], times[f'restore x{s:g}']
            print(f'    render / restore x{s:g}: {sum(a) / sum(b):.3f} of the means, {min(a) / min(b):.3f} of the minima')
        del enc
        p_restore = peak_of(lambda: model.restore(lq, *cc[scales[0]]))
        enc = model.encode(lq)
        p_render = peak_of(lambda: model.render(enc, size=grids[scales[0]]))
        print(f'    peak allocated above the resident tensors, x{scales[0]:g}: restore loop {p_restore:.0f} MiB, render loop {p_render:.0f} MiB '
              f'(+ the scene, resident: {enc.scene_bytes / 2 ** 20:.0f} MiB)')
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
