"""Developer probe: where a step of csa_attn_v4_kernel<192> spends its time, from cycle-counter sums of one wave of each role
   per workgroup, on one CrossScaleAttention(64) call at 192 x 192 (a C3 tile).  Needs `make -C ciaosr_amd/csrc probe`:
   CIAOSR_HIP_LIB=ciaosr_amd/csrc/libciaosr_hip_probe.so python tools/csattn_v4_probe.py [out.json]"""
import ctypes as C
import json
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciaosr_amd import _lib  # noqa: E402
from ciaosr_amd.nonlocal_attn import CrossScaleAttention  # noqa: E402

TICK_CYCLES = 1.0       # the counter advances at the shader clock here: 768 workgroups x ~245 steps x ~11k ticks = the kernel's 3 rounds
SLOTS = {'stager': ('X: exp2 + stage', 'barrier X|Y0 wait', 'Y0: logit loads issued (dy -2, -1)', 'barrier Y0|Y1 wait',
                    'Y1: logit loads issued (dy 0, 1)', 'barrier Y1|X wait'),
         'diagonal': ('X: U loads issued, then barrier X|Y0 wait', 'Y0: U tile 0 + diagonals -> A tile 0', 'barrier Y0|Y1 wait',
                      'Y1: U tile 1 + diagonals -> A tile 1', 'barrier Y1|X wait'),
         'consumer': ('Y1: first MFMAs of half 0', 'barrier Y1|X wait', 'X: rest of half 0, first of half 1', 'barrier X|Y0 wait',
                      'Y0: rest of half 1', 'barrier Y0|Y1 wait')}

torch.manual_seed(5)
dev = torch.device('cuda:0')
att = CrossScaleAttention(channel=64, scale=2).to(dev)
x = (torch.randn(1, 64, 192, 192, generator=torch.Generator().manual_seed(91)) * 0.5).to(dev)
for _ in range(2):
    att(x)
torch.cuda.synchronize()
lib = _lib.load()
buf = (C.c_ulonglong * (1024 * 48))()
lib.ciaosr_debug_probe_av4_read.restype = C.c_int
assert lib.ciaosr_debug_probe_av4_read(buf, 1024 * 48) == 0
a = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 3, 16).astype(np.int64)
a = a[a[:, 0, 15] > 0]
out = {'what': 'csa_attn_v4_kernel<192>, one 192x192 cs_attn call: cycle-counter ticks summed over the steps of a workgroup, '
               'first wave of each role (staging, diagonal, consumer), per step', 'workgroups': int(len(a))}
print(f'{len(a)} workgroups stamped; steps per workgroup {a[:, 0, 15].min()} .. {a[:, 0, 15].max()}')
for r, role in enumerate(('stager', 'diagonal', 'consumer')):
    steps = a[:, r, 15].astype(np.float64)
    life = a[:, r, 14] / steps * TICK_CYCLES
    print(f'  {role}: lifetime / steps = {life.mean():8.0f} cycles per step (min {life.min():.0f}, max {life.max():.0f})')
    out[role] = {'cycles_per_step_lifetime': round(float(life.mean()), 1)}
    for i, nm in enumerate(SLOTS[role]):
        cyc = a[:, r, i] / steps * TICK_CYCLES
        print(f'    {nm:40s} avg {cyc.mean():8.0f}  min {cyc.min():8.0f}  max {cyc.max():8.0f} cycles per step')
        out[role][nm] = round(float(cyc.mean()), 1)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1)
