#!/usr/bin/env python
"""Times the self-ensemble (CiaoSR.restore(..., self_ensemble=True)) and writes profiles/self_ensemble.txt:

    python tools/ensemble_probe.py [--size 5424x8160] [--lr 192x192] [--scale 4] [--precision fp32] [--warmup 2] [--rounds 5]
                                   [--checkpoint CKPT --lq-folder DIR --gt-folder DIR] [--out FILE]

A probe, not a gate: no threshold is set.  Legs alternating in one process, 2 warm-up + 5 timed rounds.
(1) The kernels alone on a [3, H, W] image of --size (default: the bench output): device time (an event pair around each call) of
    `hip_ops.dihedral` and of `hip_ops.dihedral_accum` for every k, every k once per round; reported per class -- the copy k = 0, the
    flips k = 1..3, the transposes k = 4..7 -- with the bytes the call must move (8 B per element for `dihedral`, 12 B for an
    accumulate that reads acc, 8 B with `first`) as a share of the HBM peak.
(2) RDN-CiaoSR of the shipped config, whole-image test_cfg, an LR image of --lr at --scale: wall time between synchronisations of
    (a) one `restore(..., self_ensemble=True)` and (b) eight plain `restore` calls of the same image.  (a) - (b) is what the eight
    transforms, the four other grids and the eight accumulates cost; an ensemble is n restores by construction.
(3) With --checkpoint, --lq-folder and --gt-folder: mean PSNR (the config's crop_border / convert_to, tools/test.py's evaluation) over
    the folder without and with the option.  Without them the quality gain is not measured: random weights have none to show.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X
CONFIG = os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
CLASSES = (('copy  k = 0   ', (0,)), ('flips k = 1..3', (1, 2, 3)), ('transp k = 4..7', (4, 5, 6, 7)))


def stats(t, unit=''):
    return f'mean {statistics.mean(t):.4f}{unit}, min {min(t):.4f}, max {max(t):.4f}'


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_legs(h, w, warmup, rounds, dev, say):
    from ciaosr_amd import hip_ops
    x = torch.rand(3, h, w, device=dev)
    acc = torch.zeros(3, h, w, device=dev)
    members = {k: hip_ops.dihedral(x, k) if k in (0, 4) else None for k in range(8)}      # one source per orientation
    legs = {}
    for k in range(8):
        src = members[4 if k & 4 else 0]
        legs[('dihedral', k)] = lambda k=k: hip_ops.dihedral(x, k)
        legs[('accum first', k)] = lambda k=k, src=src: hip_ops.dihedral_accum(acc, src, k, True)
        legs[('accum', k)] = lambda k=k, src=src: hip_ops.dihedral_accum(acc, src, k, False)
        legs[('accum / 8', k)] = lambda k=k, src=src: hip_ops.dihedral_accum(acc, src, k, False, divisor=8.0)
    times = {name: [] for name in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            t = device_ms(fn)
            if r >= warmup:
                times[name].append(t)
    n = 3 * h * w
    moved = {'dihedral': 8 * n, 'accum first': 8 * n, 'accum': 12 * n, 'accum / 8': 12 * n}
    say(f'(1) kernels on [3, {h}, {w}] fp32 ({n} elements), device ms over {rounds} rounds after {warmup} warm-up rounds:')
    for op in ('dihedral', 'accum first', 'accum', 'accum / 8'):
        for label, ks in CLASSES:
            t = [v for k in ks for v in times[(op, k)]]
            say(f'    {op:<12} {label}: {stats(t)} ms; {moved[op]} B -> {moved[op] / (statistics.mean(t) * 1e-3) / HBM_PEAK * 100:.0f} % of '
                f'the {HBM_PEAK / 1e12:.0f} TB/s HBM peak')


def build(checkpoint, scale, precision, dev, extra=None):
    import ciaosr_amd
    from ciaosr_amd.checkpoint import load_checkpoint
    from ciaosr_amd.config import Config
    from ciaosr_amd.init_utils import seeded_init_
    cfg = Config.fromfile(CONFIG)
    test_cfg = dict(scale=scale, precision=precision, **(extra or {}))
    model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=test_cfg)
    if checkpoint:
        load_checkpoint(model, checkpoint, map_location='cpu')
    else:
        seeded_init_(model, seed=0, gain=1.0)
    return cfg, model.to(dev).eval()


def restore_legs(args, dev, say):
    from ciaosr_amd import hip_ops
    from ciaosr_amd.init_utils import synthetic_pair
    h, w = (int(v) for v in args.lr.split('x'))
    _, model = build(args.checkpoint, args.scale, args.precision, dev)
    lq = synthetic_pair(h, w, int(args.scale))[0].to(dev)
    ht, wt = round(h * args.scale), round(w * args.scale)
    coord, cell = (t.unsqueeze(0) for t in hip_ops.make_coord_cell(ht, wt, dev))
    legs = {'a': lambda: model.restore(lq, coord, cell, self_ensemble=True),
            'b': lambda: [model.restore(lq, coord, cell, self_ensemble=False) for _ in range(8)]}
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    say(f'(2) RDN-CiaoSR ({"checkpoint" if args.checkpoint else "random weights"}), {args.precision}, LR {h} x {w} -> {ht} x {wt}, whole image, '
        f'wall s over {args.rounds} rounds after {args.warmup} warm-up rounds:')
    say(f'    (a) restore(self_ensemble=True)     {stats(times["a"])}  [{" ".join(f"{v:.4f}" for v in times["a"])}]')
    say(f'    (b) eight plain restore calls       {stats(times["b"])}  [{" ".join(f"{v:.4f}" for v in times["b"])}]')
    gap = statistics.mean(times['a']) - statistics.mean(times['b'])
    spread = max(max(times[k]) - min(times[k]) for k in times)
    say(f'    (a) - (b) = {gap:+.4f} s ({gap / statistics.mean(times["b"]) * 100:+.1f} % of (b)); larger round-to-round spread {spread:.4f} s: '
        f'{"separated" if abs(gap) > spread else "NOT separated"}')


def psnr_legs(args, dev, say):
    from ciaosr_amd.dataset import SRFolderDataset
    cfg, model = build(args.checkpoint, args.scale, args.precision, dev)
    metric_cfg = {k: cfg.test_cfg[k] for k in ('crop_border', 'convert_to', 'tile', 'tile_overlap') if k in cfg.test_cfg}
    data = SRFolderDataset(args.lq_folder, args.gt_folder, scale=args.scale)
    res = {False: [], True: []}
    for i in range(len(data)):
        d = data[i]
        kw = dict(lq=d['lq'].unsqueeze(0).to(dev), gt=d['gt'].unsqueeze(0).to(dev), coord=d['coord'].unsqueeze(0).to(dev),
                  cell=d['cell'].unsqueeze(0).to(dev), test_mode=True)
        for on in (False, True):
            model.test_cfg = dict(scale=args.scale, precision=args.precision, metrics=['PSNR'], self_ensemble=on, **metric_cfg)
            res[on].append(model(**kw)['eval_result']['PSNR'])
    say(f'(3) PSNR over {len(data)} images of {args.gt_folder} ({metric_cfg}): plain {statistics.mean(res[False]):.4f} dB, self-ensemble '
        f'{statistics.mean(res[True]):.4f} dB, gain {statistics.mean(res[True]) - statistics.mean(res[False]):+.4f} dB '
        f'(per image: {" ".join(f"{b - a:+.4f}" for a, b in zip(res[False], res[True]))})')


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--size', default='5424x8160', help='H x W of the image the kernels are timed on (default: the bench output)')
    p.add_argument('--lr', default='192x192', help='h x w of the LR image of the restore legs')
    p.add_argument('--scale', type=float, default=4)
    p.add_argument('--precision', default='fp32')
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--checkpoint', default=None)
    p.add_argument('--lq-folder', default=None)
    p.add_argument('--gt-folder', default=None)
    p.add_argument('--out', default=os.path.join(REPO, 'profiles', 'self_ensemble.txt'))
    args = p.parse_args(argv)
    from ciaosr_amd import _lib
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/ensemble_probe.py --size {args.size} --lr {args.lr} --scale {args.scale:g} --precision {args.precision} --warmup {args.warmup} '
        f'--rounds {args.rounds}: library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}')
    kernel_legs(*(int(v) for v in args.size.split('x')), args.warmup, args.rounds, dev, say)
    torch.cuda.empty_cache()
    restore_legs(args, dev, say)
    if args.checkpoint and args.lq_folder and args.gt_folder:
        psnr_legs(args, dev, say)
    else:
        say('(3) PSNR with and without the option: not measured (no --checkpoint / --lq-folder / --gt-folder given)')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
