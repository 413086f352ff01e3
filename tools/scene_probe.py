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
coordinate kernels and of the head query (every other launch of the call but denorm_clamp)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ciaosr_amd  # noqa: E402
from ciaosr_amd import _lib, hip_ops  # noqa: E402
from ciaosr_amd.config import Config  # noqa: E402
from ciaosr_amd.init_utils import seeded_init_, synthetic_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='192,48')
ap.add_argument('--precisions', default='fp32,f16')
ap.add_argument('--scales', default='4,2,3.3')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--legs', default='scene', choices=('scene', 'view'))
ap.add_argument('--view-size', type=int, default=768)
args = ap.parse_args()

dev = torch.device('cuda:0')
cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs',
                                   '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py'))
model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=dict(scale=4))
seeded_init_(model, seed=0, gain=1.0)
model = model.to(dev).eval()
print(f'library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}, reps {args.reps}')


def timed(fn):
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


def view_legs():
    from ciaosr_amd.scene import view_matrix
    size, n = int(args.sizes.split(',')[0]), args.view_size
    lq = synthetic_pair(size, size, 4)[0].to(dev)
    groups = (('view kernels', lambda k: k.startswith('view_') and k != 'view_coord_cell'),
              ('coordinates', lambda k: k in ('view_coord_cell', 'make_coord_cell_window', 'make_coord_cell')),
              ('head query', lambda k: not k.startswith(('view_', 'make_coord_cell')) and k != 'denorm_clamp'))
    for precision in args.precisions.split(','):
        model.test_cfg = dict(scale=4, precision=precision)
        enc = model.encode(lq)
        off = (size * 4 - n) // 2
        calls = {'view   0 deg': lambda: model.render_view(enc, view_matrix((size / 2, size / 2), 4.0, 0, (n, n)), (n, n)),
                 'view  30 deg': lambda: model.render_view(enc, view_matrix((size / 2, size / 2), 4.0, 30, (n, n)), (n, n)),
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
        del enc, calls
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()


scales = [float(s) for s in args.scales.split(',')]
if args.legs == 'view':
    view_legs()
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
