#!/usr/bin/env python
"""Timing of the GT-only test path on one GPU (numbers for the README / DESIGN; not a gate).

    python tools/degrade_timing.py [--e2e] [--out FILE.json]

1. ciaosr_resample_u8 (GT 2040x1356 -> x4, x12, x30; dst_chw written) in HIP-event milliseconds, next to Pillow's
   Image.resize(BICUBIC) of the same crop on this host.
2. --e2e: what tools/test.py does per image (SRFolderGTDataset item + CiaoSR forward_test with PSNR / SSIM on the host) for the
   RDN config (seeded weights) on a synthetic 2040x1356 GT at x12 and x30, fp32 and f16: seconds per image and the resample's share.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def gt_image(h=1356, w=2040):
    from ciaosr_amd import metrics
    from ciaosr_amd.init_utils import synthetic_gt
    return np.ascontiguousarray(metrics.tensor2img(synthetic_gt(h, w, seed=11))[:, :, ::-1])


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def resample_times(img, dev):
    from PIL import Image
    from ciaosr_amd.degrade import RandomDownSampling
    g = torch.from_numpy(img).to(dev)
    out = {}
    for scale in (4, 12, 30):
        down = RandomDownSampling(scale_min=scale, scale_max=scale)
        h_lr, w_lr, hc, wc = down.sizes(*img.shape[:2])
        for _ in range(3):
            down.apply(g, want_u8=False, want_chw=True)
        ms = event_ms(lambda: down.apply(g, want_u8=False, want_chw=True), 50)
        pim = Image.fromarray(np.ascontiguousarray(img[:hc, :wc]))
        t0 = time.perf_counter()
        for _ in range(5):
            pim.resize((w_lr, h_lr), Image.BICUBIC)
        host_ms = (time.perf_counter() - t0) / 5 * 1e3
        out[f'x{scale}'] = dict(lr=[h_lr, w_lr], gpu_ms=round(ms, 4), pillow_host_ms=round(host_ms, 2))
        print(f'resample x{scale}: {hc}x{wc} -> {h_lr}x{w_lr}: GPU {ms:.4f} ms (HIP events), Pillow on the host {host_ms:.2f} ms',
              flush=True)
    return out


def e2e_times(img, dev):
    import ciaosr_amd
    from PIL import Image
    from ciaosr_amd.config import Config
    from ciaosr_amd.dataset import build_test_dataset
    from ciaosr_amd.init_utils import seeded_init_
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, 'gt'))
    for i in range(3):
        Image.fromarray(img).save(os.path.join(tmp, 'gt', f'img{i}.png'))
    src = open(os.path.join(REPO, 'configs', '001_localimplicitsr_rdn_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')).read()
    out = {}
    for scale in (12, 30):
        path = os.path.join(tmp, f'cfg{scale}.py')
        with open(path, 'w') as f:
            f.write(src.replace('\nval_scale = 4\n', f'\nval_scale = {scale}\n'))
        cfg = Config.fromfile(path)
        cfg.data.test['gt_folder'] = os.path.join(tmp, 'gt')
        ds = build_test_dataset(cfg.data.test, dev)
        for prec in ('fp32', 'f16'):
            tcfg = dict(cfg.test_cfg, precision=prec)
            model = ciaosr_amd.build_model(cfg.model, train_cfg=None, test_cfg=tcfg)
            seeded_init_(model, seed=3)
            model = model.to(dev).eval()
            per = []
            for i in range(len(ds)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = ds[i]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                res = model(lq=d['lq'].unsqueeze(0), gt=d['gt'].unsqueeze(0), test_mode=True, coord=d['coord'].unsqueeze(0),
                            cell=d['cell'].unsqueeze(0), meta=[d['meta']])
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                per.append((t1 - t0, t2 - t1))
            load, fwd = np.mean([p[0] for p in per[1:]]), np.mean([p[1] for p in per[1:]])
            out[f'x{scale}_{prec}'] = dict(s_per_image=round(float(load + fwd), 4), item_s=round(float(load), 4),
                                           forward_eval_s=round(float(fwd), 4), psnr=round(float(res['eval_result']['PSNR']), 3))
            print(f'e2e x{scale} {prec}: {load + fwd:.3f} s/image (dataset item {load * 1e3:.1f} ms incl. PNG decode, '
                  f'forward + PSNR/SSIM {fwd:.3f} s)', flush=True)
            del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--e2e', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'degrade_timing.py measures on the MI355X'
    dev = torch.device('cuda:0')
    img = gt_image()
    res = dict(resample=resample_times(img, dev))
    if a.e2e:
        res['e2e'] = e2e_times(img, dev)
        for k, v in res['e2e'].items():
            v['resample_share'] = round(res['resample'][k.split('_')[0]]['gpu_ms'] * 1e-3 / v['s_per_image'], 6)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
