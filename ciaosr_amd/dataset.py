"""SRFolderDataset + the test pipeline of the reference configs (configs/001_*_rdn_*.py:100-120,143-149):
paired LQ/GT folders -> dict(lq, gt, coord, cell, meta).  The mmedit dataset classes are external; this is
the minimum tools/test.py needs.  GenerateCoordinateAndCell follows generate_assistant.py:56-96: the target
size is the GT size, gt is reshaped to [H*W, 3], coord = make_coord(target), cell = (2/H, 2/W).

SRFolderGTDataset is the GT-only form the reference's configs switch to for val_scale > 4 (configs/001_*.py:83-98, :143-153):
the LR input is down-sampled from the GT as it is loaded (RandomDownSampling), on the GPU (degrade.py)."""
import os

import numpy as np
import torch

from .coords import make_coord, make_cell
from .imageio import imread_rgb01, imread_u8

IMG_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')


class SRFolderDataset(torch.utils.data.Dataset):
    def __init__(self, lq_folder, gt_folder, pipeline=None, scale=4, test_mode=True, filename_tmpl='{}'):
        self.lq_folder, self.gt_folder, self.scale, self.filename_tmpl = str(lq_folder), str(gt_folder), scale, filename_tmpl
        names = sorted(f for f in os.listdir(self.gt_folder) if f.lower().endswith(IMG_EXT))
        self.pairs = []
        for n in names:
            stem, ext = os.path.splitext(n)
            lq = os.path.join(self.lq_folder, self.filename_tmpl.format(stem) + ext)
            if not os.path.exists(lq):
                raise FileNotFoundError(f'{lq} is not in lq_paths.')
            self.pairs.append((lq, os.path.join(self.gt_folder, n)))

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        lq_path, gt_path = self.pairs[i]
        lq, gt = imread_rgb01(lq_path), imread_rgb01(gt_path)
        ht, wt = gt.shape[-2:]
        return dict(lq=lq, gt=gt.contiguous().view(3, -1).permute(1, 0).contiguous(), coord=make_coord((ht, wt)),
                    cell=make_cell((ht, wt)), meta=dict(gt_path=gt_path, lq_path=lq_path))

    @staticmethod
    def evaluate(results):
        """Mean of every metric over the per-image eval_result dicts (mmedit BaseSRDataset.evaluate)."""
        keys = results[0]['eval_result'].keys()
        return {k: sum(r['eval_result'][k] for r in results) / len(results) for k in keys}


# The reference's valid_pipeline (configs/001_*.py:83-98), transform by transform: (type, required arguments, optional arguments), each
# argument with the only value supported (ANY: every value).  SRFolderGTDataset runs exactly this pipeline, fused on the GPU.
ANY = object()
_GT_PIPELINE = (
    ('LoadImageFromFile', {'key': 'gt'}, {'io_backend': 'disk', 'flag': 'color', 'channel_order': 'rgb'}),
    ('RandomDownSampling', {'scale_min': ANY, 'scale_max': ANY}, {'patch_size': ANY, 'interpolation': ANY, 'backend': ANY}),
    ('RescaleToZeroOne', {'keys': ['lq', 'gt']}, {}),
    ('ImageToTensor', {'keys': ['lq', 'gt']}, {}),
    # the target size is the cropped GT's (generate_assistant.py:56-96), so `scale` only documents the config
    ('GenerateCoordinateAndCell', {}, {'scale': ANY, 'target_size': None, 'sample_quantity': None, 'reshape_gt': True}),
    ('Collect', {'keys': ['lq', 'gt', 'coord', 'cell']}, {'meta_keys': ['gt_path']}),
)


def check_gt_pipeline(pipeline):
    """Validate a GT-only test pipeline against the reference's valid_pipeline; returns the RandomDownSampling it holds (which
    refuses patch_size, a scale range and other resize modes).  Any other transform, order or argument raises ValueError naming it."""
    from .degrade import RandomDownSampling
    expected = [p[0] for p in _GT_PIPELINE]
    names = [t.get('type') for t in (pipeline or [])]
    for n in names:
        if n not in expected:
            raise ValueError(f'SRFolderGTDataset: unsupported transform {n!r} in the test pipeline; supported: the reference\'s '
                             f'valid_pipeline, {expected}')
    if names != expected:
        raise ValueError(f'SRFolderGTDataset: the test pipeline must be {expected} in this order, got {names}')
    down = None
    for t, (name, required, optional) in zip(pipeline, _GT_PIPELINE):
        args = {k: v for k, v in t.items() if k != 'type'}
        missing = [k for k in required if k not in args]
        unknown = [k for k in args if k not in required and k not in optional]
        if missing or unknown:
            raise ValueError(f'SRFolderGTDataset: {name}: missing arguments {missing}, unsupported arguments {unknown}')
        for k, v in args.items():
            want = required[k] if k in required else optional[k]
            got = list(v) if isinstance(v, (list, tuple)) else v
            if want is not ANY and got != want:
                raise ValueError(f'SRFolderGTDataset: {name}({k}={v!r}) is not supported; only {want!r}')
        if name == 'RandomDownSampling':
            down = RandomDownSampling(**args)
    return down


_U8_TO_01 = {}


def _u8_to_01(device):
    """v -> float32(v) / 255 for every byte, numpy's division (RescaleToZeroOne), as a lookup table on `device`."""
    key = (device.type, device.index)
    if key not in _U8_TO_01:
        _U8_TO_01[key] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(device)
    return _U8_TO_01[key]


class SRFolderGTDataset(torch.utils.data.Dataset):
    """GT folder only: lq = RandomDownSampling of the GT (Pillow-exact bicubic, on the GPU), as the reference's SRFolderGTDataset +
    valid_pipeline.  Items are dicts like SRFolderDataset's -- lq [3,h,w], gt [Hc*Wc,3] (the GT cropped to round(h*scale) x
    round(w*scale)), coord, cell, meta.gt_path -- built on `device`.  coord / cell are shared per target size: read them, do not
    write them."""

    def __init__(self, gt_folder, pipeline, scale, test_mode=True, filename_tmpl='{}', device=None):
        self.gt_folder, self.scale, self.filename_tmpl = str(gt_folder), scale, filename_tmpl
        self.down = check_gt_pipeline(pipeline)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.paths = [os.path.join(self.gt_folder, n) for n in sorted(os.listdir(self.gt_folder)) if n.lower().endswith(IMG_EXT)]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from . import hip_ops
        gt_path = self.paths[i]
        gt_u8 = torch.from_numpy(imread_u8(gt_path)).to(self.device)
        crop, _, lq = self.down.apply(gt_u8, want_u8=False, want_chw=True)
        ht, wt = crop.shape[0], crop.shape[1]
        gt = _u8_to_01(self.device)[crop.long()].view(ht * wt, 3)
        coord, cell = hip_ops.make_coord_cell(ht, wt, self.device)
        return dict(lq=lq, gt=gt, coord=coord, cell=cell, meta=dict(gt_path=gt_path))

    evaluate = staticmethod(SRFolderDataset.evaluate)


def build_test_dataset(cfg, device=None, lq_folder=None, gt_folder=None):
    """cfg.data.test -> the dataset its `type` names (mmedit build_dataset, test datasets only).  lq_folder / gt_folder override the
    config's folders; an LQ folder on a GT-only dataset is an error."""
    kind = cfg.get('type', 'SRFolderDataset')
    gt_folder = gt_folder or cfg['gt_folder']
    if kind == 'SRFolderDataset':
        return SRFolderDataset(lq_folder or cfg['lq_folder'], gt_folder, scale=cfg.get('scale', 4),
                               filename_tmpl=cfg.get('filename_tmpl', '{}'))
    if kind == 'SRFolderGTDataset':
        if lq_folder is not None:
            raise ValueError('an LQ folder was given, but data.test is SRFolderGTDataset: it down-samples the GT itself')
        return SRFolderGTDataset(gt_folder, cfg.get('pipeline'), cfg.get('scale', 4), filename_tmpl=cfg.get('filename_tmpl', '{}'),
                                 device=device)
    raise ValueError(f'unsupported test dataset type {kind!r}; supported: SRFolderDataset, SRFolderGTDataset')
