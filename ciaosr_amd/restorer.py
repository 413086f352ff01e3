"""Restorers: BasicRestorer / CiaoSR with the reference's call surface.

Mirrors mmedited/models/restorers/basic_restorer.py:35-124 (`__init__`, `forward`, `evaluate`) and
mmedited/models/restorers/ciaosr.py:36-58 (`__init__`), :111-203 (`forward_test`), :218-258
(`clip_test`).  Normalisation, tile blending and de-normalisation run as HIP kernels; tiles are
the unit sharded across GPUs (ciaosr_amd/tile_shard.py).  Training entry points are out of scope.
"""
import contextlib
import math
import numbers
import os.path as osp

import torch
import torch.nn as nn

from . import hip_ops, metrics, scene, scene_render
from .registry import build_backbone, build_loss


class _Cfg(dict):
    """dict with attribute access (stands in for mmcv.ConfigDict)."""
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


def _as_cfg(cfg):
    if cfg is None or isinstance(cfg, _Cfg):
        return cfg
    return _Cfg(cfg)


class BasicRestorer(nn.Module):
    allowed_metrics = {'PSNR': metrics.psnr, 'SSIM': metrics.ssim}

    def __init__(self, generator, pixel_loss, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.train_cfg = _as_cfg(train_cfg)
        self.test_cfg = _as_cfg(test_cfg)
        self.fp16_enabled = False
        self.generator = build_backbone(generator)
        # the generator sees the restorer's test_cfg (looked up per call): `allow_f16_substitute` is read from it
        self._bind_generator_cfg()
        self.init_weights(pretrained)
        self.pixel_loss = build_loss(pixel_loss)

    # `test_cfg` is a property so that REASSIGNING it (`restorer.test_cfg = {...}`, what mmedit's apis do) re-binds the generator's view
    # as well; mutating the dict in place is seen without that.
    @property
    def test_cfg(self):
        return self.__dict__.get('_test_cfg')

    @test_cfg.setter
    def test_cfg(self, cfg):
        self.__dict__['_test_cfg'] = _as_cfg(cfg)
        self._bind_generator_cfg()

    def _bind_generator_cfg(self):
        gen = self.__dict__.get('_modules', {}).get('generator', None)
        if gen is not None and hasattr(gen, 'bind_test_cfg'):
            gen.bind_test_cfg(self.__dict__.get('_test_cfg'))

    def init_weights(self, pretrained=None):
        self.generator.init_weights(pretrained)

    def forward(self, lq, gt=None, test_mode=False, **kwargs):
        if test_mode:
            return self.forward_test(lq, gt, **kwargs)
        raise NotImplementedError('forward_train / train_step are out of scope of the MI355X inference path')

    def gpu_metrics(self):
        """`test_cfg.gpu_metrics` (an extension; default off): quantise and evaluate on the device (ciaosr_amd/metrics_hip.py)."""
        return bool(self.test_cfg is not None and self.test_cfg.get('gpu_metrics', False))

    def gpu_png(self):
        """`test_cfg.gpu_png` (an extension; default off): saved images are quantised and PNG-encoded on the device
        (ciaosr_amd/png_hip.py) instead of `imageio.imwrite`; the files decode to the same pixels."""
        return bool(self.test_cfg is not None and self.test_cfg.get('gpu_png', False))

    def gpu_png_matches(self):
        """`test_cfg.gpu_png_matches` (an extension; default off, read only with `gpu_png`): the device PNG coder may use LZ77 matches
        (`png_hip.encode_png(..., matches=True)`): smaller files for flat regions, the same pixels."""
        return bool(self.gpu_png() and self.test_cfg.get('gpu_png_matches', False))

    def niqe_params(self):
        """`test_cfg.niqe_params` (an extension; default absent): the pristine NIQE model, an .npz path or a mapping
        (ciaosr_amd/niqe_hip.py), loaded once.  With it 'NIQE' may stand in `test_cfg.metrics`; without it that name is the KeyError
        of any unknown metric."""
        src = self.test_cfg.get('niqe_params', None) if self.test_cfg is not None else None
        if src is None:
            return None
        cached = self.__dict__.get('_niqe_loaded')
        if cached is None or cached[0] is not src:
            from . import niqe_hip
            cached = self.__dict__['_niqe_loaded'] = (src, niqe_hip.load_params(src))
        return cached[1]

    def needs_gt(self):
        """Whether `test_cfg.metrics` holds a metric that compares with a ground truth (every one but NIQE under `niqe_params`)."""
        names = list(self.test_cfg.get('metrics', None) or []) if self.test_cfg is not None else []
        return any(not (m == 'NIQE' and self.niqe_params() is not None) for m in names)

    def evaluate(self, output, gt, out_img=None):
        """PSNR/SSIM on uint8 BGR images as basic_restorer.py:101-124.  With `test_cfg.gpu_metrics` both tensors are quantised
        and compared on the device (`out_img`: the already quantised output, if the caller has it); the output must be there
        -- no fallback -- and a GT on the host is moved.  With `test_cfg.niqe_params`, 'NIQE' in `test_cfg.metrics` is the blind score
        of the quantised output (Y channel, `test_cfg.crop_border`), always computed on the device; `gt` may then be None if no other
        metric is asked for.  The result keeps the order of `test_cfg.metrics`."""
        names = list(self.test_cfg.metrics)
        params = self.niqe_params() if 'NIQE' in names else None
        if params is None:
            return self._evaluate_reference(names, output, gt, out_img)
        from . import metrics_hip, niqe_hip
        if out_img is None:
            out_img = metrics_hip.tensor2img_u8(output)        # a host tensor raises CiaoSRHipError: NIQE has no host path
        rest = [m for m in names if m != 'NIQE']
        res = self._evaluate_reference(rest, output, gt, out_img) if rest else {}
        res['NIQE'] = niqe_hip.niqe_u8(out_img, params, self.test_cfg.crop_border, 'y')
        return {metric: res[metric] for metric in names}

    def _evaluate_reference(self, names, output, gt, out_img=None):
        if self.gpu_metrics():
            return self._evaluate_gpu(names, output, gt, out_img)
        crop_border = self.test_cfg.crop_border
        out_img, gt_img = metrics.tensor2img(output), metrics.tensor2img(gt)
        res = {}
        for metric in names:
            fn = self.allowed_metrics[metric]
            if 'convert_to' in self.test_cfg:
                res[metric] = fn(out_img, gt_img, crop_border=crop_border, convert_to=self.test_cfg.convert_to)
            else:
                res[metric] = fn(out_img, gt_img, crop_border)
        return res

    def _evaluate_gpu(self, names, output, gt, out_img=None):
        from . import metrics_hip
        for metric in names:
            self.allowed_metrics[metric]                       # an unknown name fails as on the host path
        if not output.is_cuda:
            hip_ops.require_gpu(output)                        # raises CiaoSRHipError
        if not gt.is_cuda:
            gt = gt.to(output.device)
        if out_img is None:
            out_img = metrics_hip.tensor2img_u8(output)
        gt_img = metrics_hip.tensor2img_u8(gt)
        convert_to = self.test_cfg.convert_to if 'convert_to' in self.test_cfg else None
        res = metrics_hip.psnr_ssim_u8(out_img, gt_img, self.test_cfg.crop_border, convert_to, want=names)
        return {metric: res[metric] for metric in names}


def tile_starts(n, tile, overlap):
    """ciaosr.py:227-229."""
    stride = tile - overlap
    return list(range(0, n - tile, stride)) + [n - tile]


def tile_grid(h, w, tile, overlap):
    """Row-major (h outer, w inner) list of tile origins, the reference's blend order (ciaosr.py:233-234)."""
    tile = min(tile, h, w)
    return tile, [(hi, wi) for hi in tile_starts(h, tile, overlap) for wi in tile_starts(w, tile, overlap)]


# Tiles per call of the f16-linear SwinIR trunk (`hip_options.swin_h16`) when `test_cfg.tile_batch` is not given.
# UNMEASURED: tools/swinir_tile_probe.py times the candidates 1, 2, 4, 7, 8 at tile = 192 (profiles/swinir_h16.txt records the run
# that chose a value); until such a run exists this is 4 -- 1.23 GiB of trunk workspace at that tile size.
SWIN_TILE_BATCH = 4

# Tiles per call of the EDSR trunk over tile batches (`hip_options.edsr_resident`) when `test_cfg.tile_batch` is not given: 8, the rule
# of CiaoSR.tile_batch for a kernel whose workgroup covers 12 x 12 pixels (7 is for the 16 x 32-pixel kernels).
# Was an unmeasured placeholder until tools/edsr_tile_probe.py timed the candidates 1, 4, 7, 8 at tile = 192 (profiles/edsr_resident.txt):
# the fastest 6-tile restore (4, 168.79 ms) is 0.14 ms under 8 (168.93 ms) with a round-to-round spread of up to 0.84 ms, so it stays 8;
# it changes only if a candidate beats 8 by more than the spread of such a run.
EDSR_TILE_BATCH = 8


def effective_options(generator, options):
    """The options this generator really runs with: what `generator.forward` would turn `options` into, so that a tile loop that calls
    the trunk and the head itself shows both the same options."""
    return generator.effective_options(options) if hasattr(generator, 'effective_options') else options


def trunk_batches(generator, options):
    """Whether the tile loops feed this generator's trunk batches of tiles: it has a `forward_hwc_batch`, and -- where the trunk says
    so itself (PackedSwinIR.batches: only the opt-in f16-linear trunk shares launches) -- the options make it batch.  The options are
    the ones the generator really runs with (`effective_options`)."""
    enc = getattr(generator, '_encoder_hip', None)
    if not hasattr(enc, 'forward_hwc_batch'):
        return False
    if not hasattr(enc, 'batches'):
        return True
    return enc.batches(effective_options(generator, options))


class CiaoSR(BasicRestorer):
    def __init__(self, generator, pixel_loss, rgb_mean=(0.5, 0.5, 0.5), rgb_std=(0.5, 0.5, 0.5), train_cfg=None,
                 test_cfg=None, pretrained=None):
        super().__init__(generator, pixel_loss, train_cfg=train_cfg, test_cfg=test_cfg, pretrained=pretrained)
        self.rgb_mean = tuple(float(v) for v in rgb_mean)
        self.rgb_std = tuple(float(v) for v in rgb_std)
        # host-side float32 copies (the reference keeps them as plain tensors, ciaosr.py:52-58)
        self.lq_mean = torch.FloatTensor(rgb_mean).view(1, -1, 1, 1)
        self.lq_std = torch.FloatTensor(rgb_std).view(1, -1, 1, 1)
        self.gt_mean = torch.FloatTensor(rgb_mean).view(1, 1, -1)
        self.gt_std = torch.FloatTensor(rgb_std).view(1, 1, -1)

    def train_step(self, data_batch, optimizer):
        raise NotImplementedError('training is out of scope of the MI355X inference path')

    # -- pieces of forward_test, separately callable (bench / tile sharding) ---------------------
    @torch.no_grad()
    def normalize(self, lq):
        """(lq - mean) / std  (ciaosr.py:142-144) on the GPU."""
        lq = lq.contiguous().float()
        hip_ops.require_gpu(lq)
        return torch.stack([hip_ops.normalize(lq[b], self.rgb_mean, self.rgb_std) for b in range(lq.shape[0])])

    @torch.no_grad()
    def run_tile(self, x_norm, hi, wi, tile, sf, options=None):
        """One tile of clip_test (ciaosr.py:235-245): [B, th*tw, 3] prediction of the LR crop."""
        patch = x_norm[..., hi:hi + tile, wi:wi + tile].contiguous()
        b = patch.shape[0]
        th, tw = round(patch.shape[-2] * sf), round(patch.shape[-1] * sf)
        coord, cell = hip_ops.make_coord_cell(th, tw, patch.device)       # generated on the GPU, cached per shape
        coord = coord.unsqueeze(0).expand(b, -1, 2)
        cell = cell.unsqueeze(0).expand(b, -1, 2)
        return self.generator(patch, coord, cell, test_mode=True, options=self.options(options)), (th, tw)

    def run_tiles(self, x_norm, origins, tile, sf, options=None):
        """Several equally sized tiles of ONE image (batch 1) through one generator call: the crops are stacked into a batch, so
        the encoder's dense-layer launches are shared (encoder_hip.forward_hwc_batch); the head then runs per tile.  Returns
        ([n, th*tw, 3], (th, tw)); row i is bitwise the run_tile result of origins[i]."""
        patch = torch.cat([x_norm[..., hi:hi + tile, wi:wi + tile] for (hi, wi) in origins], 0).contiguous()
        n = patch.shape[0]
        th, tw = round(patch.shape[-2] * sf), round(patch.shape[-1] * sf)
        coord, cell = hip_ops.make_coord_cell(th, tw, patch.device)
        coord = coord.unsqueeze(0).expand(n, -1, 2)
        cell = cell.unsqueeze(0).expand(n, -1, 2)
        return self.generator(patch, coord, cell, test_mode=True, options=self.options(options)), (th, tw)

    def trunk_tiles(self, x_norm, origins, tile, options):
        """The trunk half of `run_tiles`, for a tile loop that runs the heads itself (`head_tile`): the stacked crops through one trunk
        call under the generator's `effective_options` -> (patches [n, 3, tile, tile], channels-last feature maps [n, tile, tile, C])."""
        patches = torch.cat([x_norm[..., hi:hi + tile, wi:wi + tile] for (hi, wi) in origins], 0).contiguous().float()
        return patches, self.generator._encoder_hip.forward_hwc_batch(patches, options)

    def head_tile(self, patch, feat, sf, options):
        """The head of one tile from its crop [3, th, tw] and feature map: -> ([th*sf * tw*sf, 3], (th*sf, tw*sf)), bitwise run_tile's."""
        gen = self.generator
        th, tw = round(patch.shape[-2] * sf), round(patch.shape[-1] * sf)
        coord, cell = hip_ops.make_coord_cell(th, tw, patch.device)
        return gen._head.forward(None, patch, coord, cell, gen.eval_bsize, feature_hwc=feat, options=options), (th, tw)

    def prepare(self, options=None):
        """Pack every weight the call's precision reads NOW, on the current stream (idempotent; re-packs only what changed) --
        including the 16-bit fragment copies of a 'bf16' / 'f16' call, which are otherwise packed lazily on first use.
        The tile loop runs tiles on several streams: nothing a tile reads may be first built on another tile's stream."""
        gen = self.generator
        opt = effective_options(gen, self.options(options))
        head = getattr(gen, '_head', None)
        enc = getattr(gen, '_encoder_hip', None)
        if enc is not None and enc.supported():
            # (the SwinIR trunk reads 16-bit weights only under hip_options.swin_h16: it names its own `half`)
            enc.struct(enc.trunk_half(opt) if hasattr(enc, 'trunk_half') else opt.mode.trunk)
        if getattr(gen, 'non_local_attn', False):
            gen.cs_attn.packed()
        if head is not None:      # last: the 'bf16-single' form runs a pack-time calibration through the (packed) fp32 trunk and cs_attn
            head.struct(opt.mode.head)

    @torch.no_grad()
    def clip_test(self, img_lq, model=None, tile_fn=None, options=None):
        """Tiled inference of one large image (ciaosr.py:218-258).  Returns [B, h*sf*w*sf, 3].

        Tiles are independent, so with `test_cfg.tile_streams = 2` (an extension; default 1) consecutive tiles run on two
        HIP streams: the ramp, first-load and drain phases of one tile's ~450 launches (8.5 us per dense layer, GEMM
        tails, the HBM-bound softmax / patch kernels) fill with the other tile's workgroups instead of idling the chip
        (-2 % fp32, -3.5 % bf16 on a 6-tile image).  Every tile is computed exactly as on one stream (own scratch per
        stream) and the blend stays on the caller's stream in the reference order (h outer, w inner), so the result is
        bitwise the single-stream result.  `tile_streams` is off by default because per-kernel event timings (bench.py's
        roofline leg, rocprof) are meaningless while two streams share the chip.

        `test_cfg.encoder_ahead` (default TRUE since round 5, see `trunk_ahead`) DOES put a second stream under an
        image of more than `tile_batch` tiles: the next batch's trunk runs on a cached side stream (fork / join by events,
        `record_stream` on the hand-over buffers, two batches of feature maps live).  Bitwise the one-stream image; set
        `test_cfg.encoder_ahead = False` for per-kernel timing, rocprof attribution of a multi-batch image, or when calling under
        your own stream capture ("test_cfg extensions")."""
        sf = self.test_cfg.get('scale', None)
        b, c, h, w = img_lq.shape
        tile, origins = tile_grid(h, w, self.test_cfg.get('tile', None), self.test_cfg.get('tile_overlap', None))
        E = torch.zeros(b, c, h * sf, w * sf, dtype=torch.float32, device=img_lq.device)
        Wt = torch.zeros_like(E)
        n_streams = int(self.test_cfg.get('tile_streams', 1) or 1)
        n_batch = self.tile_batch(options)
        if (tile_fn is None and n_streams <= 1 and n_batch > 1 and b == 1 and len(origins) > 1 and img_lq.is_cuda and
                trunk_batches(self.generator, self.options(options))):
            # `test_cfg.tile_batch` (an extension; default 7 or 8, see tile_batch()) consecutive tiles share the encoder's dense-layer launches; every tile
            # is bitwise the one-at-a-time result and the blend order is the reference's
            gen = self.generator
            opt = effective_options(gen, self.options(options))      # the trunk and the head see the same options
            gen._require_hip_trunk(img_lq)                           # an uncovered trunk raises CiaoSRHipError here, not a C-level argument error
            groups = [origins[i0:i0 + n_batch] for i0 in range(0, len(origins), n_batch)]
            ahead = bool(self.test_cfg.get('encoder_ahead', True)) and len(groups) > 1
            with contextlib.closing(self.trunk_ahead(groups, lambda group: self.trunk_tiles(img_lq, group, tile, opt), ahead, opt,
                                                     img_lq.device)) as trunks:
                for group in groups:
                    patches, feats = next(trunks)
                    for j, (hi, wi) in enumerate(group):
                        out, (th, tw) = self.head_tile(patches[j], feats[j], sf, opt)
                        hip_ops.tile_blend(E[0], Wt[0], out.contiguous(), hi * sf, wi * sf, th, tw)
                    del patches, feats                               # before the next trunk is launched: two groups' feature maps live, not three
            return torch.stack([hip_ops.tile_finalize(E[0], Wt[0])])
        if tile_fn is not None or n_streams <= 1 or len(origins) < 2 or not img_lq.is_cuda:
            for (hi, wi) in origins:
                out, (th, tw) = self.run_tile(img_lq, hi, wi, tile, sf, options) if tile_fn is None else tile_fn(hi, wi)
                for bi in range(b):
                    hip_ops.tile_blend(E[bi], Wt[bi], out[bi].contiguous(), hi * sf, wi * sf, th, tw)
            return torch.stack([hip_ops.tile_finalize(E[bi], Wt[bi]) for bi in range(b)])
        cur = torch.cuda.current_stream(img_lq.device)
        self.prepare(options)
        th = tw = round(tile * sf)
        hip_ops.make_coord_cell(th, tw, img_lq.device)              # cached coordinates exist before any side stream reads them
        streams = self._tile_streams(n_streams, img_lq.device)
        for st in streams:
            st.wait_stream(cur)                                      # the normalised image, E / Wt and the packed weights are ready
        pending = []                                                 # (origin, out, event) in tile order

        def blend_one():
            (hi, wi), out, ev = pending.pop(0)
            cur.wait_event(ev)
            for bi in range(b):
                hip_ops.tile_blend(E[bi], Wt[bi], out[bi], hi * sf, wi * sf, th, tw)

        for i, (hi, wi) in enumerate(origins):
            st = streams[i % n_streams]
            with torch.cuda.stream(st):
                out, _ = self.run_tile(img_lq, hi, wi, tile, sf, options)
                out = out.contiguous()
                ev = torch.cuda.Event()
                ev.record(st)
            out.record_stream(cur)                                   # consumed by the blend on the caller's stream
            pending.append(((hi, wi), out, ev))
            if len(pending) > n_streams:                             # keep at most one finished tile per stream waiting
                blend_one()
        while pending:
            blend_one()
        for st in streams:
            cur.wait_stream(st)
        return torch.stack([hip_ops.tile_finalize(E[bi], Wt[bi]) for bi in range(b)])

    def trunk_ahead(self, groups, trunk, ahead, options, device):
        """The one trunk-ahead pipeline of the tile loops: yield `trunk(group)` -- a tuple of the tensors (or lists of tensors) a group's trunk hands over to its heads --
        for every group of `groups`, in order; a group's trunk is first launched when the group is first asked for.  Without `ahead`
        that is all, on the caller's stream.  With `ahead` (`test_cfg.encoder_ahead`, an extension; ON by default since round 5 for more
        than one group) the trunk of group g + 1 is queued on the cached side stream right behind group g's, so it runs UNDER the heads
        of group g (cs_attn + fused head kernels, or a scene's prepares and queries) on the caller's stream: the trunk's 130 strictly
        dependent launches per group and the heads' long MFMA kernels fill each other's ramp / drain / memory phases.  `prepare(options)`
        runs first, so that nothing the side stream reads is first packed there; the side stream forks from the caller's, which waits
        on each group's event, every handed-over tensor gets `record_stream`, and the caller's stream joins the side stream when the
        generator ends or is closed.  Same kernels on the same data in the same per-tile order: bitwise the one-stream result."""
        if not ahead:
            for group in groups:
                yield trunk(group)
            return
        cur = torch.cuda.current_stream(device)
        self.prepare(options)
        side = self._tile_streams(1, device)[0]
        side.wait_stream(cur)

        def launch(group):
            with torch.cuda.stream(side):
                out = trunk(group)
                ev = torch.cuda.Event()
                ev.record(side)
            return out, ev

        def take(out, ev):              # a function of its own: no local of the generator keeps a tensor of a finished group alive
            cur.wait_event(ev)
            for t in out:               # tensors, or lists of them: consumed on the caller's stream
                for u in ([t] if torch.is_tensor(t) else t):
                    u.record_stream(cur)
            return out

        try:
            nxt = None
            for g, group in enumerate(groups):
                out, ev = nxt or launch(group)
                nxt = launch(groups[g + 1]) if g + 1 < len(groups) else None      # queued behind group g's trunk, runs under group g's heads
                yield take(out, ev)
        finally:
            cur.wait_stream(side)

    def _tile_streams(self, n, device):
        key = (n, device.index)
        cache = self.__dict__.setdefault('_tile_stream_cache', {})
        if key not in cache:
            cache[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
        return cache[key]

    def tile_batch(self, options=None):
        """Tiles per encoder call (`test_cfg.tile_batch`, an extension; at most 16: 32-bit buffer offsets into the batched block buffer).
        Default 7 where the trunk's dense layers run a kernel whose workgroup covers 16 x 32 pixels -- the F(4x4, 3x3) Winograd kernel
        of the fp32 trunk (dense_direct = 0) and, since round 6, the 16-bit dense kernel (dense_direct != 1): a 192 x 192 tile is 72
        workgroups / items, 8 tiles are 576 = 2.25 rounds of the 256 CUs (a third round at a quarter of the chip), 7 tiles are 504 =
        1.97 -- else 8.  The SwinIR trunk (batched only under `hip_options.swin_h16`): SWIN_TILE_BATCH.  The EDSR trunk under
        `hip_options.edsr_resident` (fp32 on the 12 x 12-pixel kernel in every precision mode): EDSR_TILE_BATCH."""
        v = self.test_cfg.get('tile_batch', None)
        if v is None:
            opt = self.options(options)
            enc = getattr(self.generator, '_encoder_hip', None)
            if hasattr(enc, 'uses_h16'):
                return SWIN_TILE_BATCH
            if getattr(enc, 'kind', None) == 'edsr' and opt.edsr_resident:
                return EDSR_TILE_BATCH
            v = 7 if (opt.dense_direct == 0 if opt.mode.trunk is None else opt.dense_direct != 1) else 8
        return min(int(v or 1), 16)

    def options(self, options=None):
        """The hip_ops.Options a call runs with: the explicit argument if given, else `test_cfg.precision`
        ('fp32' default | 'bf16'; an extension absent from the reference) + `test_cfg.hip_options` (dict of
        ciaosr_options_t fields).  Nothing process-global: two restorers in one process can differ."""
        if options is not None:
            return hip_ops.as_options(options)
        cfg = self.test_cfg or {}
        extra = dict(cfg.get('hip_options', None) or {})
        prec = cfg.get('precision', None)
        if prec is None and not extra:
            return hip_ops.DEFAULT_OPTIONS
        return hip_ops.Options(prec or 'fp32', **extra)          # 'fp32' | 'bf16' | 'f16' | 'f16-pairs'

    def ensemble_ids(self, self_ensemble=None):
        """The member ids a call runs with: `scene.dihedral_ids` of the explicit argument, or of `test_cfg.self_ensemble` (an extension;
        default off) when the argument is None; None = off (pass False to turn a configured ensemble off for one call).  ValueError
        for anything that is neither True nor a sequence of distinct ids in 0..7."""
        if self_ensemble is None and self.test_cfg is not None:
            self_ensemble = self.test_cfg.get('self_ensemble', None)
        return scene.dihedral_ids(self_ensemble)

    @torch.no_grad()
    def restore(self, lq, coord=None, cell=None, options=None, self_ensemble=None):
        """forward_test body from normalised LR on device to de-normalised, clamped output
        [B,3,round(h*s),round(w*s)] on device (ciaosr.py:142-169) -- the timed region of bench.py.
        `options` / `test_cfg.precision = 'bf16'` (an extension, absent from the reference) runs the dense layers
        with bf16 MFMA inputs; the default is the exact-fp32 path.
        `self_ensemble` (default `test_cfg.self_ensemble`; an extension, default off): True, or a sequence of distinct ids in 0..7 --
        the geometric self-ensemble, `restore_ensemble`."""
        ids = self.ensemble_ids(self_ensemble)
        if ids is not None:
            return self.restore_ensemble(lq, coord, cell, ids, self.options(options))
        return self._restore(lq, coord, cell, self.options(options))

    def restore_ensemble(self, lq, coord, cell, ids, options):
        """The mean over the members `ids` (scene.py, "self-ensemble"): member k is `_restore(T_k(lq), coord_k, cell_k)` -- the plain
        restore of the flipped / transposed image under the same test_cfg and options, de-normalised and clamped; coord_k, cell_k are
        the caller's tensors for k < 4 (the grid is the same) and `hip_ops.make_coord_cell(Wt, Ht)` for k & 4, (Ht, Wt) the target
        size `_restore` derives.  The members are mapped back and summed in fp32 in the order given, one rounded add each, and the
        sum is divided by their number, once (`hip_ops.dihedral_accum`).  One accumulator the size of the output; a member's output
        is consumed before the next member runs."""
        lq = lq.contiguous().float()
        hip_ops.require_gpu(lq)
        ih, iw = lq.shape[-2:]
        if coord is not None:
            s = math.sqrt(coord.shape[1] / (ih * iw))                 # `_restore`'s own size rule
            ht, wt = round(ih * s), round(iw * s)
        acc = None
        for i, k in enumerate(ids):
            ck, cl = coord, cell
            if (k & 4) and coord is not None:
                ck, cl = (t.unsqueeze(0).expand(lq.shape[0], -1, 2) for t in hip_ops.make_coord_cell(wt, ht, lq.device))
            out = self._restore(hip_ops.dihedral(lq, k), ck, cl, options)
            if acc is None:
                oh, ow = out.shape[-2:]
                acc = torch.empty(*out.shape[:2], *((ow, oh) if k & 4 else (oh, ow)), dtype=torch.float32, device=out.device)
            hip_ops.dihedral_accum(acc, out, k, first=(i == 0), divisor=float(len(ids)) if i == len(ids) - 1 else 0.0)
            del out
        return acc

    @torch.no_grad()
    def clip_test_any_scale(self, img_lq, ht, wt, options=None):
        """Opt-in tiled inference for non-integer / > 4 scales (tile_plan.py): the reference's LR tiling and
        uniform blending, HR rectangles by pixel-centre membership, tile-local coordinates and cells.
        Returns [B, ht*wt, 3]."""
        from . import tile_plan
        b, c, h, w = img_lq.shape
        tiles = tile_plan.plan(h, w, ht, wt, self.test_cfg.get('tile'), self.test_cfg.get('tile_overlap', 0) or 0)
        E = torch.zeros(b, c, ht, wt, dtype=torch.float32, device=img_lq.device)
        Wt = torch.zeros_like(E)
        for t in tiles:
            patch = img_lq[..., t['y0']:t['y0'] + t['th'], t['x0']:t['x0'] + t['tw']].contiguous()
            coord = t['coord'].to(img_lq.device).unsqueeze(0).expand(b, -1, 2)
            cell = t['cell'].to(img_lq.device).unsqueeze(0).expand(b, -1, 2)
            out = self.generator(patch, coord, cell, test_mode=True, options=self.options(options))
            for bi in range(b):
                hip_ops.tile_blend(E[bi], Wt[bi], out[bi].contiguous(), t['i0'], t['j0'], t['i1'] - t['i0'], t['j1'] - t['j0'])
        return torch.stack([hip_ops.tile_finalize(E[bi], Wt[bi]) for bi in range(b)])

    # -- encode once, render any scale, window or view (an extension, absent from the reference): scene_render.py ----------------------
    @torch.no_grad()
    def encode(self, lq, options=None, max_scale=None, self_ensemble=None):
        """Everything `restore` computes from the LR image alone, kept: -> scene.EncodedImage for `render`.  Without `test_cfg.tile` the
        whole image's trunk and head scene, built here when `max_scale` is known (the argument, else `test_cfg.scale`; else at the first
        render, from its scale).  With `test_cfg.tile` one scene per LR tile, each built when a render first touches the tile and held
        under `test_cfg.scene_cache_mb` (default 4096) MiB, least recently used first out.  `max_scale` sizes the plan of every scene:
        the full (tile) grid at that scale is the largest render whose route is `restore`'s own (include/ciaosr_hip.h, q_plan).
        `self_ensemble` (default `test_cfg.self_ensemble`, as `restore`): -> scene.EnsembleEncoded, one plain encode per member T_k(lq),
        `scene_cache_mb` split evenly over them; `render` / `render_many` of it give the windows of `restore(..., self_ensemble=ids)`,
        bitwise.  `render_view`, `View` targets, `render_pyramid` and `prefetch` refuse such a record (ValueError)."""
        return scene_render.encode(self, lq, options, max_scale, self_ensemble)

    @torch.no_grad()
    def encode_rgba(self, lq4, options=None, max_scale=None, self_ensemble=None):
        """`encode` of an RGBA image [1, 4, h, w] (float, R G B A in [0, 1]) as a batch of two: item 0 the colour as stored (not
        premultiplied, whatever lies under transparent pixels), item 1 the alpha plane in all three channels; both go through the same
        model, options, tiling and scenes, and `enc.alpha` is set.  Every render of such an encode returns with `as_u8` ONE uint8
        [H, W, 4] device image, bytes B G R A (`metrics_hip.tensor2img_bgra_u8`: the colour bytes are `tensor2img_u8`'s of item 0,
        bitwise the render of the colour image alone; A = (4899 R + 9617 G + 1868 B + 8192) >> 14 of item 1's bytes), and without it
        the fp32 batch of two (colour, alpha as grey).  Outside a view the alpha item is 0 and the colour item the caller's `fill`.
        `render_pyramid` resizes colour and alpha separately below the LR size (not Pillow's premultiplied RGBA resize).  A tensor
        that is not [1, 4, h, w] is a ValueError, and so is `self_ensemble` (the argument or `test_cfg.self_ensemble`): RGBA encodes have
        no ensemble."""
        return scene_render.encode_rgba(self, lq4, options, max_scale, self_ensemble)

    @torch.no_grad()
    def encode_grey(self, lq1, options=None, max_scale=None, self_ensemble=None):
        """`encode` of grey images [B, 1, h, w] (float in [0, 1]) as the colour images (v, v, v): the same model, options, tiling,
        scenes and (with `self_ensemble`) ensemble record, marked `enc.grey`.  Every render of such a record returns with `as_u8` a
        uint8 [H, W] device image (`metrics_hip.tensor2img_grey_u8`): with (B, G, R) = `tensor2img_u8`'s bytes of the render,
        L = (19595 R + 38470 G + 7471 B + 32768) >> 16 -- `Image.convert('L')` of the colour render, so the answer is grey whatever
        the model's three output rows do; quantised once, after the tile blend, the view fill and the ensemble mean (outside a view:
        the byte of (fill, fill, fill)).  Without `as_u8` the fp32 [B, 3, H, W] of the plain encode, bit for bit.  `render_pyramid`
        resizes the grey smallest model level below the LR size (Pillow's BICUBIC of the L image).  A tensor that is not
        [B, 1, h, w] is a ValueError."""
        return scene_render.encode_grey(self, lq1, options, max_scale, self_ensemble)

    @torch.no_grad()
    def render(self, enc, size=None, scale=None, window=None, as_u8=False, as_u16=False):
        """The window (i0, j0, h, w) (HR pixels; default: the whole grid) of the image `restore` gives for the Ht x Wt target -- `size`, or
        round(h * scale), round(w * scale) -- under the same test_cfg, from an `encode` result: [B, 3, h, w], de-normalised and clamped,
        or with `as_u8` the metrics_hip.tensor2img_u8 image of it.  Only the LR tiles whose HR rectangle meets the window are touched.
        `as_u16`: the same render as torch.uint16 samples, q16(v) = rint(fp32(clamp(v, 0, 1) * 65535)) -- [H, W, 3] B G R
        (`metrics_hip.tensor2img_u16`), or [H, W] on an `encode_grey` record (`tensor2img_grey_u16`: L16 of the three samples) --
        quantised once, after the tile blend, the view fill and the ensemble mean.  It is NOT the `as_u8` image shifted left, and its
        high byte is NOT the `as_u8` byte.  With `as_u8` as well, or on an `encode_rgba` record, a ValueError before any device work
        (`render_view` and `render_many` likewise)."""
        scene_render.check_quant(enc, as_u8, as_u16)
        if scene_render.is_ensemble(enc):
            return scene_render.render_ensemble(self, enc, [scene.Grid(size, scale, window)], as_u8, as_u16=as_u16)[0]
        return scene_render.render_one(self, enc, scene_render.resolve(self, enc, [scene.Grid(size, scale, window)])[0], as_u8, as_u16)

    @torch.no_grad()
    def render_view(self, enc, matrix, size, fill=0.0, as_u8=False, as_u16=False):
        """The Hv x Wv (`size`) affine view `matrix` = (m_yy, m_yx, t_y, m_xy, m_xx, t_x) of an `encode` result (scene.py: the definition,
        `view_matrix`, `view_of_window`): [B, 3, Hv, Wv], de-normalised and clamped, or with `as_u8` the metrics_hip.tensor2img_u8 image
        of it.  A pixel whose centre falls outside the image holds `fill` (one number or three, in the output's [0, 1]).  The queries are
        made, sorted into the LR tiles (the whole image without `test_cfg.tile`) and blended back on the device, in the reference's
        row-major tile order; a tile without a member is neither built nor queried.  With `test_cfg.tile` this needs
        `test_cfg.tile_any_scale`.  Per batch item ONE device-to-host copy -- the tiles' member counts, which size the per-tile query
        lists -- is the only synchronisation of a view render.  An axis-aligned view is not bitwise the window `render` shows (its
        coordinates differ by up to 2^-22, see `scene.view_of_window`).  `as_u16`: see `render`; outside the view a grey record holds
        L16 of (q16(fill), q16(fill), q16(fill))."""
        scene_render.check_quant(enc, as_u8, as_u16)
        scene_render.refuse_ensemble(enc, 'render_view')
        return scene_render.render_one(self, enc, scene_render.resolve(self, enc, [scene.View(matrix, size, fill)])[0], as_u8, as_u16)

    @torch.no_grad()
    def render_warp(self, enc, homography=None, map=None, size=None, footprint=None, fill=0.0, as_u8=False, as_u16=False,
                    footprint_range=None, minify='clamp', max_samples=4):
        """The Hv x Wv (`size`) warp of an `encode` result (scene.py: the definition): every output pixel is answered by the model at its
        own LR position, which comes from ONE of two point sources.  `homography` = (h00, h01, h02, h10, h11, h12, h20, h21, h22), y
        first: y_lr = Y / D, x_lr = X / D of Y = (h00 v + h01 u) + h02, X = (h10 v + h11 u) + h12, D = (h20 v + h21 u) + h22 at the pixel
        centre (v, u) = (i + 0.5, j + 0.5), fp64 (`scene.homography_from_points`, `scene.homography_of_view`); D must be positive on the
        whole output.  `map`: a device tensor [Hv, Wv, 2] of (y_lr, x_lr), float64 (float32 is widened exactly; `size` defaults to its
        shape; NaN or infinite: the pixel holds `fill`).  `footprint` = (f_y, f_x), the LR extent of an output pixel along each LR axis, is
        what the model sees as the cell -- ONE per warp: default for a homography its Jacobian at the output centre
        (`scene.warp_footprint`), required for a map (`scene.map_footprint` offers one, at the cost of a copy).  Under strong perspective
        the local scale varies over the output: `footprint='per-pixel'` gives every output pixel its own footprint -- the norms of the
        rows of the homography's Jacobian at the pixel, or central differences of the map -- and a device tensor [Hv, Wv, 2] of
        (g_y, g_x) gives the caller's own; both are clamped to `footprint_range` = (lo, hi), default (1 / max_scale, 1.0) with the
        encode's max_scale (else `test_cfg.scale`), the warp plans for max_scale = 1 / lo, a pixel whose footprint is NaN or undefined
        holds `fill`, and the head is asked with chunk = 1 so that the shift radius of a query comes from its own cell (scene.py,
        "per-pixel warps": the definition).  A per-pixel warp whose footprints are constant is bitwise the single-footprint warp of
        that constant.  A footprint above hi is clamped, so where the warp minifies a pixel is one point query and aliases:
        `minify='area'` (a homography with a per-pixel footprint; `max_samples` = N in 1, 2, 4, 8) gives such a pixel n_y x n_x samples,
        n = the smallest power of two <= N with g <= hi n per axis, each with the footprint g / n, and the pixel holds the mean of
        their finished values -- the caller's `fill` for a sample outside the image, so RGBA alpha is the covered fraction (scene.py,
        "area-sampled warps": the definition).  The head answers exactly the samples that lie inside; where nothing minifies the
        render is bitwise `minify='clamp'`, the default.  Everything else is `render_view`'s: tiles (with
        `test_cfg.tile`: `tile_any_scale`), row-major blend, `fill`, `as_u8` / `as_u16`, grey and RGBA records, one device-to-host copy per
        batch item.  A warp that is affine -- last row (0, 0, 1), or a map of a view's points with its footprint -- is bitwise
        `render_view` of that matrix.  `test_cfg.view_blocks` is ignored.  ValueError before any device work for what
        `scene.check_warp` lists, and for a self-ensemble encode."""
        scene_render.check_quant(enc, as_u8, as_u16)
        scene_render.refuse_ensemble(enc, 'render_warp')
        target = scene.Warp(homography, map, size, footprint, fill, footprint_range, minify, max_samples)
        return scene_render.render_one(self, enc, scene_render.resolve(self, enc, [target])[0], as_u8, as_u16)

    @torch.no_grad()
    def render_many(self, enc, targets, as_u8=False, as_u16=False):
        """Every target of the list -- scene.Grid(size, scale, window): `render`'s arguments, scene.View(matrix, size, fill):
        `render_view`'s, scene.Warp(homography, map, size, footprint, fill, footprint_range, minify, max_samples): `render_warp`'s (each warp is counted by its own launch
        pair; its counts ride in the views' one copy) -- from ONE walk over the tile scenes: -> list of [B, 3, h, w], outs[k] bitwise what the single call returns on an
        encode with the same max_scale under the same test_cfg (with `as_u8` the same uint8 image).  Per batch item the union of the
        tiles the targets touch is walked in row-major order; each tile's scene is taken from the cache once and every target that
        touches it is queried from it, in list order, into the target's own accumulators -- so each target sees its tiles in the
        reference's blend order.  Coordinates are made right before the query that reads them, as `render` makes them (the 16-bit
        head's grid-width hint is kept for the last 64 coordinate tensors only).  A call builds exactly the scenes of the union that the
        cache lacks, under any budget that holds one scene (cached scenes the walk still needs are evicted last), from trunk features
        made `tile_batch()` tiles per trunk call where the trunk batches tiles, with `test_cfg.encoder_ahead` (default on) the next
        group's trunk on the cached side stream under the current group's heads.  All views are counted in one `view_count_many` and
        one device-to-host copy per call (none for grids alone).  An image that is one frame (no `test_cfg.tile`, or an image no larger
        than the tile) has no schedule to make: its targets are the single calls, in list order.  `as_u16`: see `render`."""
        return scene_render.render_many(self, enc, targets, as_u8, as_u16)

    @torch.no_grad()
    def prefetch(self, enc, targets):
        """Build the scenes `render_many(enc, targets)` would touch and the cache lacks, rendering nothing: the same plan and the same
        batched builder, row-major per batch item, stopping before a build would exceed `scene_cache_mb` -- nothing is evicted.
        -> the number of scenes built."""
        return scene_render.prefetch(self, enc, targets)

    @torch.no_grad()
    def render_pyramid(self, enc, size=None, scale=None, as_u16=False):
        """The levels of the Deep Zoom pyramid (pyramid.py) whose top is the `size` / `scale` render of `enc`: list of uint8 [H_l, W_l, 3]
        device images (`render(..., as_u8=True)`'s), level 0 (1 x 1) first.  A level at least as large as the LR image on both sides is a
        model level: all of them are Grid(size=(H_l, W_l)) targets of ONE `render_many`, hence one walk over the tile scenes, and each is
        bitwise `render(enc, size=(H_l, W_l), as_u8=True)`.  Every smaller level is `degrade.resize_bicubic_u8` -- Pillow's BICUBIC
        resize, exactly -- of the smallest model level, each taken from it directly.  ValueError before any device work: a batch, a top
        level below the LR size, `test_cfg.tile` without `tile_any_scale`, and whatever `scene.Grid` raises.
        `as_u16`: torch.uint16 levels ([H_l, W_l, 3] B G R, or [H_l, W_l] on an `encode_grey` record).  The model levels are the
        `as_u16` targets of the one `render_many`, each bitwise `render(enc, size=(H_l, W_l), as_u16=True)`; below the LR size every
        level is the integer box halving of the level ABOVE it (`tiff_hip.halve_box_u16`: the rounded mean of 2 x 2 samples, the last
        row / column repeated on odd sizes), a chain from the smallest model level -- not a bicubic resize: Pillow has no exact 16-bit
        one to be held to.  On an `encode_rgba` record a ValueError (no 16-bit alpha).  Without the keyword nothing changes."""
        if as_u16:
            return scene_render.render_pyramid(self, enc, size, scale, as_u16=True)
        return scene_render.render_pyramid(self, enc, size, scale)

    def _plan_pyramid(self, enc, size=None, scale=None):
        return scene_render.plan_pyramid(self, enc, size, scale)

    def _restore(self, lq, coord=None, cell=None, options=None):
        x = self.normalize(lq)
        if self.test_cfg.get('tile', None) and self.test_cfg.get('tile_any_scale', False) and coord is not None:
            ih, iw = lq.shape[-2:]
            s = math.sqrt(coord.shape[1] / (ih * iw))                 # the reference's own size rule (ciaosr.py:166-169)
            pred = self.clip_test_any_scale(x, round(ih * s), round(iw * s), options)
            n_q = pred.shape[1]
        elif self.test_cfg.get('tile', None):
            pred = self.clip_test(x, self.generator, options=options)
            n_q = pred.shape[1]
        else:
            pred = self.generator(x, coord, cell, test_mode=True, options=options)
            n_q = coord.shape[1]
        ih, iw = lq.shape[-2:]
        s = math.sqrt(n_q / (ih * iw))
        H, W = round(ih * s), round(iw * s)
        return torch.stack([hip_ops.denorm_clamp(pred[b].contiguous(), H, W, self.rgb_mean, self.rgb_std)
                            for b in range(lq.shape[0])])

    def graphed_restore(self, lq, coord=None, cell=None, warmup=2, options=None):
        """Capture `restore(lq)` (a few hundred short launches for a 48x48 tile) into one hipGraph and return a
        callable `run(new_lq=None) -> output` that replays it; input and output live in static buffers.  All
        kernels are launched on torch's current stream, workspaces are allocated during the warm-up calls, and
        nothing in the path synchronises, so the whole step is capturable.  Not with `test_cfg.self_ensemble` (ValueError): the ensemble
        is not captured."""
        if self.ensemble_ids() is not None:
            raise ValueError('graphed_restore does not capture a self-ensemble: turn test_cfg.self_ensemble off, or call restore')
        static_lq = lq.clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self.prepare(options)
            for _ in range(max(warmup, 1)):
                self.restore(static_lq, coord, cell, options)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # capture on the SAME stream the warm-up ran on: hip_ops' scratch is per stream, so every workspace the captured launches
        # point into already exists (nothing is allocated under capture) ...
        with torch.cuda.graph(graph, stream=side):
            static_out = self.restore(static_lq, coord, cell, options)

        # ... and is handed over to this closure: the graph holds raw pointers into the scratch buffers, the coordinate tensors
        # and the packed weights that were live during capture, so exactly those objects live as long as the graph does and no
        # longer (take_workspaces removes them from hip_ops' cache: a later eager call on a stream that re-uses the handle gets
        # fresh scratch, and dropping `run` frees the memory).  Weights must not change after capture (a repack would be
        # invisible to the captured launches).
        # With test_cfg.tile_streams > 1 or test_cfg.encoder_ahead the captured launches also point into the scratch of the restorer's
        # cached side streams: those buffers are taken too (a later, larger eager call on such a stream would otherwise re-grow -- i.e.
        # free -- a buffer the graph still reads and writes).
        scratch = hip_ops.take_workspaces(side)
        for streams in self.__dict__.get('_tile_stream_cache', {}).values():
            for st in streams:
                scratch.update(hip_ops.take_workspaces(st))
        keep = (scratch, dict(hip_ops._coord_cache),
                [getattr(m, '_packed', None) for m in self.modules()],
                [(getattr(o, '_st', None), getattr(o, '_keep', None), getattr(o, '_mask_keep', None),
                  dict(getattr(o, '_st_half', None) or {}))
                 for m in self.modules() for o in (getattr(m, '_head', None), getattr(m, '_encoder_hip', None)) if o is not None])

        def run(new_lq=None):
            if new_lq is not None:
                static_lq.copy_(new_lq)
            graph.replay()
            return static_out
        run.graph = graph
        run.keep = keep
        return run

    def forward_test(self, lq, gt, coord=None, cell=None, meta=None, save_image=False, save_path=None,
                     iteration=None):
        """Same contract as ciaosr.py:111-203."""
        pred = self.restore(lq, coord, cell)
        if gt is not None:
            shape = [lq.shape[0], pred.shape[2], pred.shape[3], 3]
            gt = gt.view(*shape).permute(0, 3, 1, 2).contiguous()
        out_img = None
        if (self.gpu_metrics() or self.gpu_png()) and save_image:
            from . import metrics_hip
            out_img = metrics_hip.tensor2img_u8(pred)              # quantised once, for the metrics and for the file
        if self.test_cfg is not None and self.test_cfg.get('metrics', None):
            assert gt is not None or not self.needs_gt(), 'evaluation with metrics must have gt images.'
            results = dict(eval_result=self.evaluate(pred, gt, out_img))
        else:
            results = dict(lq=lq.cpu(), output=pred.cpu())
            if gt is not None:
                results['gt'] = gt.cpu()
        if save_image:
            if 'gt_path' in meta[0]:
                folder_name = osp.splitext(osp.basename(meta[0]['gt_path']))[0]
            else:
                folder_name = osp.splitext(osp.basename(meta[0]['lq_path']))[0]
            if isinstance(iteration, numbers.Number):
                save_path = osp.join(save_path, folder_name, f'{folder_name}-{iteration + 1:06d}.png')
            elif iteration is None:
                save_path = osp.join(save_path, f'{folder_name}.png')
            else:
                raise ValueError(f'iteration should be number or None, but got {type(iteration)}')
            if self.gpu_png():
                from .png_hip import imwrite_gpu
                imwrite_gpu(out_img, save_path, matches=self.gpu_png_matches())
            else:
                from .imageio import imwrite
                imwrite(out_img.cpu().numpy() if out_img is not None else metrics.tensor2img(pred), save_path)
        return results

    def init_weights(self, pretrained=None, strict=True):
        self.generator.init_weights(pretrained, strict)
