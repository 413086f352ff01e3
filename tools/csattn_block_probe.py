"""Per-tag hip_ops.profile() times of one CrossScaleAttention(64) call, whole-map against Options(csa_block_mb=...): sizes 192 x 192,
256 x 256, 226 x 340 (a DIV2K image at x6) and 512 x 512, fp32 and f16, budgets off / 512 / 1024 / 2047 MiB.  Mean of `--reps` profiled
calls after two warm-ups; one text block per case (profiles/csattn_blocks.txt).  On a tree without the option it runs the whole-map calls
only; 512 x 512 is never run whole (64 GiB of logits).  `--sizes 192x192,256x256` and `--budgets 0,1024` narrow the sweep."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciaosr_amd import _lib, hip_ops  # noqa: E402
from ciaosr_amd.nonlocal_attn import CrossScaleAttention  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='192x192,256x256,226x340,512x512')
ap.add_argument('--precisions', default='fp32,f16')
ap.add_argument('--budgets', default='0,512,1024,2047')
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()

has_option = 'csa_block_mb' in hip_ops.Options._C_FIELDS
dev = torch.device('cuda:0')
torch.manual_seed(5)
att = CrossScaleAttention(channel=64, scale=2).to(dev)
print(f'library version {_lib.load().ciaosr_version()}, csa_block_mb {"available" if has_option else "absent: whole-map calls only"}')
for size in args.sizes.split(','):
    H, W = (int(v) for v in size.split('x'))
    x = (torch.randn(1, 64, H, W, generator=torch.Generator().manual_seed(91)) * 0.5).to(dev)
    for precision in args.precisions.split(','):
        for mb in (int(v) for v in args.budgets.split(',')):
            if (mb and not has_option) or (not mb and H * W > 340 * 226):
                continue
            opt = hip_ops.Options(precision, **(dict(csa_block_mb=mb) if mb else {}))
            hip_ops.release_workspaces()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(2):
                att(x, options=opt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                att(x, options=opt)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / args.reps * 1e3
            with hip_ops.profile():
                for _ in range(args.reps):
                    att(x, options=opt)
            prof = hip_ops.profile.results()
            bands = ''
            if has_option:
                code = {'fp32': 0, 'bf16': 1, 'f16': 2}[opt.precision]
                rows = _lib.load().ciaosr_cs_attn_block_rows(H, W, 64, 2, code, opt.c_arg())
                bands = f', bands of {rows} rows x {-(-((H + 1) // 2 * 2) // rows)}'
            total = sum(v['total_ms'] for v in prof.values()) / args.reps
            print(f'\n{H}x{W} {precision} csa_block_mb={mb}{bands}: wall {wall:.3f} ms/call, kernels {total:.3f} ms/call, '
                  f'peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB')
            for k, v in sorted(prof.items(), key=lambda kv: -kv[1]['total_ms']):
                print(f'    {k:24s} {v["total_ms"] / args.reps:9.4f} ms  {v["launches"] // args.reps:4d} launches')
    del x
