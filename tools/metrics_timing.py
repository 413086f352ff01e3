#!/usr/bin/env python
"""Timing of the evaluation step on one GPU: the host path (what `evaluate` does by default) next to `test_cfg.gpu_metrics`
(numbers for the README / DESIGN; not a gate).

    python tools/metrics_timing.py [--out profiles/gpu_metrics_timing.json] [--reps 20] [--small-only]

On seeded synthetic image pairs generated on the device at 1356x2040 and 5424x8160 (crop_border 4, convert_to 'y'), in one process:
1. host path, once per size: the two device-to-host copies, `metrics.tensor2img` twice, `metrics.psnr`, `metrics.ssim`; wall clock.
2. device path, warm: HIP-event time of the quantiser (`ciaosr_tensor2img_u8`) and of the metric kernels (`ciaosr_psnr_ssim_u8`), and
   the host clock around the whole device `evaluate` (quantise both + metrics + the copy of the twelve result doubles).
3. per kernel: algorithmic bytes over its time as a share of the 8 TB/s HBM peak; fp64 FMAs over the metric kernel's time as a share
   of the 39.3 T FMA/s vector fp64 peak (256 CUs x 64 lanes x 2.4 GHz); the larger share names the bound.
4. |device - host| of PSNR and SSIM.
A run without a GPU fails.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch         # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s
FP64_FMA_PEAK = 256 * 64 * 2.4e9
FMA_PER_MAP_PIXEL = 110      # 5 quantities x 11 taps, row pass + column pass
SIZES = [(1356, 2040), (5424, 8160)]


def image_pair(h, w, dev, seed=0):
    """(output, gt) [1, 3, h, w] fp32 on the device: a smooth seeded image and the same plus noise of ~3 grey levels."""
    g = torch.Generator(device=dev).manual_seed(1234 + seed)
    y = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1)
    x = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w)
    c = torch.arange(3, device=dev, dtype=torch.float32).view(3, 1, 1)
    gt = (0.5 + 0.25 * torch.sin(x / (9.0 + 4 * c) + 0.7 * c) * torch.cos(y / (13.0 - 3 * c)) + 0.15 * torch.sin((x + 2 * y) / (31.0 + 7 * c)))
    gt = gt.clamp(0, 1).unsqueeze(0).contiguous()
    out = (gt + 0.012 * torch.randn(gt.shape, generator=g, device=dev)).clamp(0, 1)
    return out, gt


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def host_path(out, gt, crop, conv):
    from ciaosr_amd import metrics
    torch.cuda.synchronize()
    t = [time.perf_counter()]
    o, g = out.cpu(), gt.cpu()
    t.append(time.perf_counter())
    oi, gi = metrics.tensor2img(o), metrics.tensor2img(g)
    t.append(time.perf_counter())
    p = float(metrics.psnr(oi, gi, crop, conv))
    t.append(time.perf_counter())
    s = metrics.ssim(oi, gi, crop, conv)
    t.append(time.perf_counter())
    return dict(PSNR=p, SSIM=s), dict(copies_s=t[1] - t[0], tensor2img_s=t[2] - t[1], psnr_s=t[3] - t[2], ssim_s=t[4] - t[3],
                                      total_s=t[4] - t[0])


def device_path(out, gt, crop, conv, reps):
    from ciaosr_amd import metrics_hip as mh

    def evaluate():
        return mh.psnr_ssim_u8(mh.tensor2img_u8(out), mh.tensor2img_u8(gt), crop, conv)

    for _ in range(3):
        res = evaluate()
    oi, gi = mh.tensor2img_u8(out), mh.tensor2img_u8(gt)
    quant_ms = event_ms(lambda: mh.tensor2img_u8(out), reps)
    metric_ms = event_ms(lambda: mh.launch_psnr_ssim_u8(oi, gi, crop, conv), reps)
    psnr_only_ms = event_ms(lambda: mh.launch_psnr_ssim_u8(oi, gi, crop, conv, want=('PSNR',)), reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = evaluate()
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    return res, dict(quantiser_ms=quant_ms, metric_kernels_ms=metric_ms, metric_kernels_psnr_only_ms=psnr_only_ms,
                     evaluate_host_clock_ms=wall_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'gpu_metrics_timing.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--small-only', action='store_true', help='skip 5424x8160 (its host path takes about a minute)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'metrics_timing.py measures on the MI355X; there is no CPU fallback'
    assert a.reps >= 20, 'at least 20 repetitions'
    dev = torch.device('cuda:0')
    crop, conv = 4, 'y'
    res = dict(device=torch.cuda.get_device_name(0), crop_border=crop, convert_to=conv, reps=a.reps, sizes={})
    for (h, w) in SIZES[:1] if a.small_only else SIZES:
        out, gt = image_pair(h, w, dev)
        d_res, d_t = device_path(out, gt, crop, conv, a.reps)
        print(f'{h}x{w} device: {d_res}  {json.dumps({k: round(v, 4) for k, v in d_t.items()})}', flush=True)
        h_res, h_t = host_path(out, gt, crop, conv)
        print(f'{h}x{w} host:   {h_res}  {json.dumps({k: round(v, 3) for k, v in h_t.items()})}', flush=True)
        px, map_px = h * w, (h - 2 * crop - 10) * (w - 2 * crop - 10)
        q_share = 15.0 * px / (d_t['quantiser_ms'] * 1e-3) / HBM_PEAK
        m_hbm = 6.0 * px / (d_t['metric_kernels_ms'] * 1e-3) / HBM_PEAK
        m_fma = FMA_PER_MAP_PIXEL * map_px / (d_t['metric_kernels_ms'] * 1e-3) / FP64_FMA_PEAK
        entry = dict(host=dict(result=h_res, **{k: round(v, 4) for k, v in h_t.items()}),
                     device=dict(result=d_res, **{k: round(v, 4) for k, v in d_t.items()}),
                     quantiser=dict(bytes=15 * px, hbm_share=round(q_share, 4), bound='HBM'),
                     metric_kernel=dict(bytes=6 * px, hbm_share=round(m_hbm, 4), fp64_fma=FMA_PER_MAP_PIXEL * map_px,
                                        fp64_share=round(m_fma, 4), bound='fp64 VALU' if m_fma > m_hbm else 'HBM'),
                     abs_diff=dict(PSNR=abs(d_res['PSNR'] - h_res['PSNR']), SSIM=abs(d_res['SSIM'] - h_res['SSIM'])),
                     speedup=round(h_t['total_s'] * 1e3 / d_t['evaluate_host_clock_ms'], 1))
        res['sizes'][f'{h}x{w}'] = entry
        print(f'{h}x{w}: host {h_t["total_s"]:.2f} s, device evaluate {d_t["evaluate_host_clock_ms"]:.3f} ms (host clock); quantiser '
              f'{q_share:.1%} of HBM peak; metric kernels {m_hbm:.1%} of HBM peak, {m_fma:.1%} of fp64 peak; '
              f'|dPSNR| {entry["abs_diff"]["PSNR"]:.3g} dB |dSSIM| {entry["abs_diff"]["SSIM"]:.3g}', flush=True)
        del out, gt
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
