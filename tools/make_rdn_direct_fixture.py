"""Writes tests/golden/rdn_direct_29x40.npz: the RDN trunk (2 blocks, 3 layers, 64 channels) at 29 x 40 on the direct halo-resident fp32
kernel (csrc/dense_f32.hip, Options(dense_direct=1, dense_min_tiles=1)) for three seeded inputs -- the features of image 0 and the SHA-256
of the features of images 1 and 2, each from a batch-of-one call.  tests/test_edsr_resident_gpu.py holds later libraries to these bits.

The committed file was written by the library of the commit BEFORE dense_f32_kernel gained its source / destination / epilogue
arguments: check that commit out into a directory of its own, build it there, and run this script with that directory as the working
directory (it imports `ciaosr_amd` from the working directory and nothing from tests/):

    python /path/to/this/make_rdn_direct_fixture.py --out rdn_direct_29x40.npz

Developer tool; needs the MI355X."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())

WEIGHT_SEED, GAIN, INPUT_SEED, SHAPE, BLOCKS, LAYERS = 31, 1.6, 81, (29, 40), 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    from ciaosr_amd import CiaoSR, LocalImplicitSRRDN, _lib, hip_ops
    from ciaosr_amd.init_utils import seeded_init_
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[64, 64])
    gen = dict(type=LocalImplicitSRRDN,
               encoder=dict(type='RDN', in_channels=3, out_channels=3, mid_channels=64, num_blocks=BLOCKS, upscale_factor=4, num_layers=LAYERS,
                            channel_growth=64),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    model = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss', loss_weight=1.0, reduction='mean'), rgb_mean=(0.4488, 0.4371, 0.4040),
                   rgb_std=(1., 1., 1.), test_cfg=dict(scale=4)).eval()
    sha = seeded_init_(model, seed=WEIGHT_SEED, gain=GAIN)
    dev = torch.device('cuda:0')
    x = (torch.randn((3, 3) + SHAPE, generator=torch.Generator().manual_seed(INPUT_SEED)) * 0.3).to(dev)
    enc = model.to(dev).generator._encoder_hip
    opt = hip_ops.Options(dense_direct=1, dense_min_tiles=1)
    with hip_ops.profile():
        feats = [enc.forward_hwc(x[i], opt).cpu().contiguous() for i in range(3)]
    tags = {k: v['launches'] for k, v in hip_ops.profile.results().items()}
    assert tags.get('enc_dense_gather') == 3 * BLOCKS * LAYERS, tags
    digest = lambda t: hashlib.sha256(t.numpy().tobytes()).hexdigest()
    np.savez(args.out, feat0=feats[0].numpy(), sha_feat1=digest(feats[1]), sha_feat2=digest(feats[2]), weight_seed=WEIGHT_SEED, gain=GAIN,
             input_seed=INPUT_SEED, shape=np.array(SHAPE), blocks=BLOCKS, layers=LAYERS, sha=sha, library_version=_lib.load().ciaosr_version())
    print(f'{args.out}: library version {_lib.load().ciaosr_version()}, feature scale {feats[0].abs().max().item():.3f}, tags {tags}')


if __name__ == '__main__':
    main()
