"""SwinIR-CiaoSR x4 at the shipped tile size (configs/001_localimplicitsr_swinir_*: tile=192, tile_overlap=32): what the opt-in
f16-linear trunk (`hip_options.swin_h16`, csrc/swinir_h16.hip) buys, and which `tile_batch` it wants (developer tool; writes
profiles/swinir_h16.txt with `--out`).

One process, seeded weights.  Inputs: one 192 x 192 tile and a 6-tile image (LR 339 x 510, the `c3s` geometry).  Three kinds of run are
ALTERNATED (one repetition of each in turn, so drift of the box hits all alike): precision='f16' with the option off, precision='f16'
with the option on at each candidate tile_batch (1, 2, 4, 7, 8), and precision='fp32'.
  trunk    per-tile kernel time of one trunk call from hip_ops.profile (B tiles per call, divided by B), by tag; the share the fp32
           3x3 convolutions and the window attention keep
  restore  wall time of the whole 6-tile restore: median of `--reps` (>= 5) after two warm-ups, encoder_ahead as shipped
`--parent-root DIR` (a built checkout of the parent commit) adds the parent library's option-off figures: the same measurements by
this script in a child process on that tree, once before and once after this tree's runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='tree whose package and library run')
ap.add_argument('--parent-root', default=None)
ap.add_argument('--batches', default='1,2,4,7,8')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--worker', action='store_true', help='print one JSON object instead of the report (the parent-tree child)')
args = ap.parse_args()
args.reps = max(args.reps, 5)

sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from ciaosr_amd import _lib, hip_ops, build_model  # noqa: E402
from ciaosr_amd.config import Config  # noqa: E402
from ciaosr_amd.init_utils import seeded_init_, synthetic_pair  # noqa: E402

TRUNK_TAGS = ('swin_', 'enc_', 'image_to_hwc4')
has_option = 'swin_h16' in hip_ops.Options._C_FIELDS
dev = torch.device('cuda:0')
cfg = Config.fromfile([os.path.join(args.root, 'configs', f) for f in sorted(os.listdir(os.path.join(args.root, 'configs')))
                       if f.startswith('001_localimplicitsr_swinir_')][0])
model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
seeded_init_(model, seed=0, gain=1.5, head_gain=6 ** 0.5)
model = model.to(dev).eval()
assert model.test_cfg['tile'] == 192 and model.test_cfg['tile_overlap'] == 32
model.test_cfg['scale'] = 4
lq = synthetic_pair(339, 510, 4)[0].to(dev)
tile8 = torch.stack([model.normalize(lq)[0, :, y:y + 192, x:x + 192] for y in (0, 147) for x in (0, 100, 200, 318)]).contiguous()
enc = model.generator._encoder_hip

runs = [('f16 off', 'f16', None, None)]
if has_option:
    runs += [(f'f16 swin_h16 tile_batch={b}', 'f16', dict(swin_h16=1), int(b)) for b in args.batches.split(',')]
runs.append(('fp32', 'fp32', None, None))


def configure(precision, hip_options, batch):
    for k in ('precision', 'hip_options', 'tile_batch'):
        model.test_cfg.pop(k, None)
    model.test_cfg['precision'] = precision
    if hip_options:
        model.test_cfg['hip_options'] = dict(hip_options)
    if batch:
        model.test_cfg['tile_batch'] = batch


def trunk_profile(precision, hip_options, batch):
    """Per-tile kernel time by tag of one trunk call on `batch` tiles (mean of 3 profiled calls after a warm-up)."""
    opt = hip_ops.Options(precision, **(hip_options or {}))
    B = batch or 1
    call = (lambda: enc.forward_hwc_batch(tile8[:B], opt)) if (hip_options and B > 1) else (lambda: [enc.forward_hwc(tile8[i], opt) for i in range(B)])
    call()
    torch.cuda.synchronize()
    with hip_ops.profile():
        for _ in range(3):
            call()
    prof = hip_ops.profile.results()
    return {k: (v['total_ms'] / 3 / B, v['launches'] / 3 / B) for k, v in prof.items() if k.startswith(TRUNK_TAGS)}


def restore_once():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.restore(lq)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure():
    res = {name: dict(wall=[]) for name, *_ in runs}
    for name, precision, hip_options, batch in runs:
        res[name]['trunk'] = trunk_profile(precision, hip_options, batch)
        configure(precision, hip_options, batch)
        for _ in range(2):
            restore_once()
    for _ in range(args.reps):                       # alternate: one repetition of every run in turn
        for name, precision, hip_options, batch in runs:
            configure(precision, hip_options, batch)
            res[name]['wall'].append(restore_once())
    return dict(version=_lib.load().ciaosr_version(), device=torch.cuda.get_device_name(0), runs=res)


def parent():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--root', args.parent_root, '--reps', str(args.reps)],
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit('parent-tree child failed:\n' + out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def trunk_ms(t):
    return sum(ms for ms, _ in t.values())


def report(title, m, lines, base=None):
    lines.append(f'\n== {title}: library version {m["version"]}, {m["device"]} ==')
    for name, r in m['runs'].items():
        t, wall = r['trunk'], sorted(r['wall'])
        tot = trunk_ms(t)
        conv = sum(ms for k, (ms, _) in t.items() if k in ('swin_group_conv', 'swin_conv_after_body'))
        att = t.get('swin_window_attention', (0.0, 0))[0]
        ratio = f', {tot / base:.3f} x the parent fp32 trunk' if base else ''
        lines.append(f'\n{name}: trunk {tot:.3f} ms per tile{ratio} (3x3 convolutions {100 * conv / tot:.1f} %, window attention {100 * att / tot:.1f} %); '
                     f'6-tile restore median {statistics.median(wall):.2f} ms of {len(wall)} (min {wall[0]:.2f}, max {wall[-1]:.2f})')
        for k, (ms, n) in sorted(t.items(), key=lambda kv: -kv[1][0]):
            lines.append(f'    {k:24s} {ms:9.4f} ms per tile {n:8.2f} launches per tile')


if args.worker:
    print(json.dumps(measure()))
    sys.exit(0)

lines = [f'tools/swinir_tile_probe.py --reps {args.reps} --batches {args.batches}: SwinIR-CiaoSR x4, tile 192 / overlap 32, LR 339 x 510 (6 tiles); '
         f'trunk = kernel time per tile of one trunk call (hip_ops.profile), restore = wall time of the whole image']
before = parent() if args.parent_root else None
mine = measure()
after = parent() if args.parent_root else None
base = None
if before:
    base = (trunk_ms(before['runs']['fp32']['trunk']) + trunk_ms(after['runs']['fp32']['trunk'])) / 2
    lines.append(f'parent fp32 trunk (the reference of the ratios): {base:.3f} ms per tile, mean of the runs before and after')
    report('parent commit, before', before, lines, base)
report('this tree', mine, lines, base)
if after:
    report('parent commit, after', after, lines, base)
if has_option:
    on = {n: statistics.median(r['wall']) for n, r in mine['runs'].items() if 'swin_h16' in n}
    best = min(on, key=on.get)
    lines.append(f'\nfastest option-on restore: {best} ({on[best]:.2f} ms); option off f16: {statistics.median(mine["runs"]["f16 off"]["wall"]):.2f} ms')
text = '\n'.join(lines) + '\n'
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text)
