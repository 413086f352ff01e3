"""EDSR-CiaoSR x4 at the shipped tile size (configs/001_localimplicitsr_edsr_*: 64 channels, 16 blocks, tile=192, tile_overlap=32): what
the opt-in trunk over tile batches (`hip_options.edsr_resident`, csrc/encoder.hip on the kernel of csrc/dense_f32.hip) buys, and which
`tile_batch` it wants (developer tool; writes profiles/edsr_resident.txt with `--out`).

Seeded weights.  Inputs: 192 x 192 tiles and a 6-tile image (LR 339 x 510).  Legs: the option off and on, on at each candidate tile_batch
(1, 4, 7, 8), each with `encoder_ahead` off and on.
  trunk    kernel time per tile of one trunk call from hip_ops.profile (B tiles per call, divided by B), by tag; mean of 3 profiled calls
           after a warm-up
  restore  wall time of the whole 6-tile restore at x4 between two device synchronisations: 2 warm-up rounds, then `--reps` (>= 5) timed
           rounds; a round runs every leg once, in turn, so drift of the box hits all legs alike.  Every round's value is written.
`--parent-root DIR` (a built checkout of the parent commit) adds the parent library's option-off legs, measured by this script in a
child process on that tree which stays up for the whole run and takes its turn in every round."""
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
ap.add_argument('--batches', default='1,4,7,8')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--worker', action='store_true', help='serve rounds on stdin / stdout instead of writing the report (the parent-tree child)')
args = ap.parse_args()
args.reps = max(args.reps, 5)
WARMUP = 2

sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from ciaosr_amd import _lib, hip_ops, build_model  # noqa: E402
from ciaosr_amd.config import Config  # noqa: E402
from ciaosr_amd.init_utils import seeded_init_, synthetic_pair  # noqa: E402

TRUNK_TAGS = ('enc_', 'image_to_hwc4')
has_option = 'edsr_resident' in hip_ops.Options._C_FIELDS
dev = torch.device('cuda:0')
cfg = Config.fromfile([os.path.join(args.root, 'configs', f) for f in sorted(os.listdir(os.path.join(args.root, 'configs')))
                       if f.startswith('001_localimplicitsr_edsr_')][0])
model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
seeded_init_(model, seed=0, gain=1.25, head_gain=6 ** 0.5)
model = model.to(dev).eval()
assert model.test_cfg['tile'] == 192 and model.test_cfg['tile_overlap'] == 32
enc = model.generator._encoder_hip
st = enc.struct(None)
assert (st.mid_channels, st.num_blocks) == (64, 16)
model.test_cfg['scale'] = 4
lq = synthetic_pair(339, 510, 4)[0].to(dev)
tile8 = torch.stack([model.normalize(lq)[0, :, y:y + 192, x:x + 192] for y in (0, 147) for x in (0, 100, 200, 318)]).contiguous()

# (name, hip_options, tile_batch, encoder_ahead)
legs = [(f'off ahead={int(a)}', None, None, a) for a in (False, True)]
if has_option and not args.worker:
    legs += [(f'edsr_resident tile_batch={b} ahead={int(a)}', dict(edsr_resident=1), int(b), a) for b in args.batches.split(',') for a in (False, True)]


def configure(hip_options, batch, ahead):
    for k in ('hip_options', 'tile_batch', 'encoder_ahead'):
        model.test_cfg.pop(k, None)
    if hip_options:
        model.test_cfg['hip_options'] = dict(hip_options)
    if batch:
        model.test_cfg['tile_batch'] = batch
    model.test_cfg['encoder_ahead'] = ahead


def trunk_profile(hip_options, batch):
    """Kernel time and launches per tile, by tag, of one trunk call on `batch` tiles."""
    opt = hip_ops.Options(**(hip_options or {}))
    B = batch or 1
    call = (lambda: enc.forward_hwc_batch(tile8[:B], opt)) if hip_options else (lambda: [enc.forward_hwc(tile8[i], opt) for i in range(B)])
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


def trunks():
    return {name: trunk_profile(ho, b) for name, ho, b, a in legs if not a}


def one_round():
    out = {}
    for name, ho, b, a in legs:
        configure(ho, b, a)
        out[name] = restore_once()
    return out


def header():
    return dict(version=_lib.load().ciaosr_version(), device=torch.cuda.get_device_name(0))


if args.worker:                                      # one JSON line per command line: 'header', 'trunks', 'round'; EOF ends it
    for line in sys.stdin:
        cmd = line.strip()
        print(json.dumps({'header': header, 'trunks': trunks, 'round': one_round}[cmd]()), flush=True)
    sys.exit(0)


class Child:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--root', root], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True)

    def ask(self, cmd):
        self.p.stdin.write(cmd + '\n')
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f'parent-tree child ended (exit status {self.p.wait()}) at {cmd!r}')
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


child = Child(args.parent_root) if args.parent_root else None
mine = dict(header(), trunk=trunks(), wall={name: [] for name, *_ in legs})
theirs = dict(child.ask('header'), trunk=child.ask('trunks'), wall={}) if child else None
for r in range(WARMUP + args.reps):
    a = one_round()
    b = child.ask('round') if child else {}
    if r >= WARMUP:
        for k, v in a.items():
            mine['wall'][k].append(v)
        for k, v in b.items():
            theirs['wall'].setdefault(k, []).append(v)
if child:
    child.close()


def trunk_ms(t):
    return sum(ms for ms, _ in t.values())


def report(title, m, lines):
    lines.append(f'\n== {title}: library version {m["version"]}, {m["device"]} ==')
    for name, t in m['trunk'].items():
        lines.append(f'\ntrunk, {name.replace(" ahead=0", "")}: {trunk_ms(t):.3f} ms per tile, {sum(n for _, n in t.values()):.2f} launches per tile')
        for k, (ms, n) in sorted(t.items(), key=lambda kv: -kv[1][0]):
            lines.append(f'    {k:24s} {ms:9.4f} ms per tile {n:8.2f} launches per tile')
    lines.append('\n6-tile restore, wall ms per round (in round order), then median and spread (max - min):')
    for name, w in m['wall'].items():
        lines.append(f'    {name:40s} ' + ' '.join(f'{v:8.2f}' for v in w) + f'   median {statistics.median(w):8.2f}  spread {max(w) - min(w):6.2f}')


lines = [f'tools/edsr_tile_probe.py --reps {args.reps} --batches {args.batches}: EDSR-CiaoSR x4 (64 channels, 16 blocks), tile 192 / overlap 32, '
         f'LR 339 x 510 (6 tiles); trunk = kernel time per tile of one trunk call (hip_ops.profile), restore = wall time of the whole image, '
         f'{WARMUP} warm-up rounds + {args.reps} timed rounds, every leg once per round in turn']
report('this tree', mine, lines)
if theirs:
    report('parent commit (child process, same rounds)', theirs, lines)
if has_option:
    med = {n: statistics.median(w) for n, w in mine['wall'].items()}
    spread = max(max(w) - min(w) for w in mine['wall'].values())
    on = {n: v for n, v in med.items() if n.startswith('edsr_resident')}
    best = min(on, key=on.get)
    lines.append(f'\nfastest option-on leg: {best} ({on[best]:.2f} ms); option off: ' + ', '.join(f'{n} {v:.2f} ms' for n, v in med.items() if n.startswith('off'))
                 + f'; largest round-to-round spread of a leg {spread:.2f} ms')
text = '\n'.join(lines) + '\n'
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text)
