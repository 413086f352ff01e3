"""Per-kernel HIP-event pass of one CrossScaleAttention(64) call at 192 x 192 LR (a C3 tile): mean ms per call of 3 after a warm-up,
   for the default route, the 96-wide items and the 16C route; one JSON line.  `--save FILE` also stores the default route's output
   (to compare two trees on the same input)."""
import json
import os
import sys
import time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciaosr_amd import hip_ops  # noqa: E402
from ciaosr_amd.nonlocal_attn import CrossScaleAttention  # noqa: E402

torch.manual_seed(5)
dev = torch.device('cuda:0')
att = CrossScaleAttention(channel=64, scale=2).to(dev)
x = (torch.randn(1, 64, 192, 192, generator=torch.Generator().manual_seed(91)) * 0.5).to(dev)
res = {}
for name, opts in (('four_block', hip_ops.Options()), ('four_block_t128', hip_ops.Options(csa_attn_tile128=1)),
                   ('16c', hip_ops.Options(csa_attn_v16=1))):
    for _ in range(2):
        y = att(x, options=opts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        att(x, options=opts)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / 3 * 1e3
    with hip_ops.profile():
        for _ in range(3):
            att(x, options=opts)
    prof = hip_ops.profile.results()
    res[name] = {'wall_ms': wall, 'kernels': {k: round(v['total_ms'] / 3, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]['total_ms'])}}
    if name == 'four_block' and '--save' in sys.argv:
        torch.save(y.cpu(), sys.argv[sys.argv.index('--save') + 1])
print(json.dumps(res))
