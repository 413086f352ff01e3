#!/usr/bin/env python
"""Times the two PNG writers of the --save-path / --out path on uint8 device images and writes profiles/png_gpu.txt:

    python tools/png_probe.py [--sizes 5424x8160 768x768] [--contents smooth noisy] [--warmup 2] [--rounds 5] [--out FILE] [--append]

host leg:   what the default path does with a quantised device image: `imageio.imwrite(img.cpu().numpy(), path)` (PIL at its default level);
device leg: `png_hip.imwrite_gpu(img, path)` (csrc/png_u8.hip + the container on the host).
Images: `init_utils.synthetic_gt` quantised by `tensor2img_u8`, as is ('smooth') and with 2 grey levels of noise ('noisy').  The legs
alternate in one process; wall time runs from the device image (after a synchronize) to the closed file.  Device time per kernel comes
from `hip_ops.profile` in a round of its own.  The files of both writers are decoded and compared, and their sizes recorded.
"""
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


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--sizes', nargs='+', default=['5424x8160', '768x768'])
    p.add_argument('--contents', nargs='+', default=['smooth', 'noisy'], choices=['smooth', 'noisy'])
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--out', default=os.path.join(REPO, 'profiles', 'png_gpu.txt'))
    p.add_argument('--append', action='store_true', help='add to --out instead of replacing it (a run split over several calls)')
    args = p.parse_args(argv)
    from ciaosr_amd import _lib, hip_ops
    from ciaosr_amd.imageio import imread_u8, imwrite
    from ciaosr_amd.png_hip import imwrite_gpu
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/png_probe.py --sizes {" ".join(args.sizes)} --contents {" ".join(args.contents)} --warmup {args.warmup} --rounds {args.rounds}: '
        f'library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}, {os.cpu_count()} host CPUs visible')
    with tempfile.TemporaryDirectory() as tmp:
        for size in args.sizes:
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
