#!/usr/bin/env python
"""Times NIQE on the device (ciaosr_amd/niqe_hip.py) and writes profiles/niqe_gpu.txt:

    python tools/niqe_probe.py [--params tests/golden/niqe_pris_params.npz] [--sizes 5424x8160 768x768] [--host-size 768x768]
                               [--warmup 2] [--rounds 5] [--out FILE]

Images: `init_utils.synthetic_gt` quantised by `tensor2img_u8`, with 2 grey levels of noise.  Per size, legs alternating in one process,
wall time between synchronisations:
(a) `niqe_u8` -- the five launches, the copy of the block sums, the host finishing;
(b) the host finishing by itself (`features` + `finish` on block sums already on the host);
(c) at --host-size only: the float64 numpy restatement tests/niqe_ref.py on the Y plane, as the host leg (the reference itself needs
    mmcv / mmedit and is not run here; it rebuilds the gamma table five times per block on top of what the restatement does).
Kernel time per tag comes from `hip_ops.profile` in a round of its own, with each kernel's share of the HBM peak from the bytes it
must move.  The device score is compared with the restatement's at --host-size.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def make_image(h, w, dev):
    from ciaosr_amd.init_utils import synthetic_gt
    from ciaosr_amd.metrics_hip import tensor2img_u8
    img = tensor2img_u8(synthetic_gt(h, w).to(dev))
    g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
    noise = torch.randint(-2, 3, (h, w, 3), generator=g, dtype=torch.int16).to(dev)
    return (img.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8).contiguous()


def stats(t):
    return f'mean {statistics.mean(t):.5f}, min {min(t):.5f}, max {max(t):.5f}  [{" ".join(f"{v:.5f}" for v in t)}]'


def min_bytes(h, w):
    """Bytes each kernel must move for an h x w image (no crop): reads + writes of its maps, halos not counted."""
    hb, wb = h // 96 * 96, w // 96 * 96
    px, px2 = hb * wb, hb * wb // 4
    return dict(niqe_luma=h * w * (3 + 4), niqe_mscn=px * (4 + 8) + px2 * (8 + 8), niqe_half=px * 4 + px2 * 8, niqe_moments=(px + px2) * 8)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--params', default=os.path.join(REPO, 'tests', 'golden', 'niqe_pris_params.npz'))
    p.add_argument('--sizes', nargs='+', default=['5424x8160', '768x768'])
    p.add_argument('--host-size', default='768x768')
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--out', default=os.path.join(REPO, 'profiles', 'niqe_gpu.txt'))
    args = p.parse_args(argv)
    from ciaosr_amd import _lib, hip_ops, niqe_hip
    from tests import niqe_ref
    dev = torch.device('cuda', torch.cuda.current_device())
    params = niqe_hip.load_params(args.params)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/niqe_probe.py --sizes {" ".join(args.sizes)} --host-size {args.host_size} --warmup {args.warmup} --rounds {args.rounds}: '
        f'library version {_lib.load().ciaosr_version()}, {torch.cuda.get_device_name(0)}, {os.cpu_count()} host CPUs visible')
    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        img = make_image(h, w, dev)
        moments = niqe_hip.moments_u8(img, params).cpu()
        legs = {'a': lambda: niqe_hip.niqe_u8(img, params), 'b': lambda: niqe_hip.finish(niqe_hip.features(moments), params)}
        if size == args.host_size:
            y = niqe_hip.moments_u8(img, params, return_luma=True)[1].cpu().numpy()
            legs['c'] = lambda: niqe_ref.niqe(y, params)[1]
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        with hip_ops.profile():
            q = legs['a']()
        prof = hip_ops.profile.results()
        need = min_bytes(h, w)
        say(f'{h} x {w}: {moments.shape[1]} blocks, {moments.numel() * 8} bytes of block sums cross to the host; NIQE {q:.6f}; workspace '
            f'{_lib.load().ciaosr_niqe_workspace_bytes(h, w, 0)} bytes')
        say(f'  (a) niqe_u8 on the device          wall s: {stats(times["a"])}')
        say(f'  (b) host finishing by itself       wall s: {stats(times["b"])}')
        total = sum(v['total_ms'] for v in prof.values())
        say(f'  (a) kernels: {total:.3f} ms in {sum(v["launches"] for v in prof.values())} launches: '
            + ', '.join(f'{k} {v["total_ms"]:.3f} ms ({need[k] / (v["total_ms"] * 1e-3) / HBM_PEAK * 100:.0f} % of the HBM peak for {need[k]} bytes)'
                        for k, v in sorted(prof.items()) if k in need))
        if 'c' in legs:
            q_ref = legs['c']()
            say(f'  (c) float64 numpy restatement      wall s: {stats(times["c"])}')
            gap = statistics.mean(times['c']) - statistics.mean(times['a'])
            spread = max(max(times[k]) - min(times[k]) for k in ('a', 'c'))
            say(f'  (c) - (a) = {gap:.5f} s, larger round-to-round spread {spread:.5f} s: '
                f'{"device faster beyond the spread" if gap > spread else "NOT separated"}; ratio (c) / (a) '
                f'{statistics.mean(times["c"]) / statistics.mean(times["a"]):.1f}x; |device - restatement| / restatement = {abs(q - q_ref) / q_ref:.3e}')
        del img
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
