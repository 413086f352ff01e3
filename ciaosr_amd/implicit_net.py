"""LocalImplicitSR generators: the reference's plugin surface over the HIP head.

Mirrors mmedited/models/backbones/sr_backbones/ciaosr_net.py:
  LocalImplicitSRNet   (:17-264)   ctor kwargs, dims wiring (:56-85), forward (:88-110),
                                   query_rgb (:113-224), batched_predict (:226-248), init_weights (:250)
  LocalImplicitSRRDN   (:267-342)  re-parents sfe1/sfe2/rdbs/gff, deletes `encoder`
  LocalImplicitSREDSR  (:345-408)  re-parents conv_first/body/conv_after_body
Same constructor arguments, attribute and state_dict names, argument meaning and error behaviour.
The arithmetic of query_rgb / batched_predict AND of the encoder trunks (gen_feature) runs in libciaosr_hip.so
(hand-written gfx950 kernels).  There is no PyTorch trunk in the product: a trunk configuration the HIP library
does not cover raises CiaoSRHipError (the PyTorch restatements live in tests/torch_trunks.py as checkers).
Inference only.
"""
import copy

import torch
import torch.nn as nn

from . import hip_ops
from ._lib import CiaoSRHipError
from .head_hip import PackedHead
from .encoder_hip import PackedEncoder
from .nonlocal_attn import CrossScaleAttention
from .registry import build_backbone, build_component


class EncodedFeatures:
    """What `LocalImplicitSRNet.encode` keeps of a batch: one head Scene per item, the normalised LR batch (for the bilinear residual)
    and the Options the scenes were built with."""
    __slots__ = ('scenes', 'x', 'options')

    def __init__(self, scenes, x, options):
        self.scenes, self.x, self.options = scenes, x, options

    @property
    def nbytes(self):
        return sum(s.nbytes for s in self.scenes)


class LocalImplicitSRNet(nn.Module):
    def __init__(self, encoder, imnet_q, imnet_k, imnet_v, query_mlp=None, key_mlp=None, value_mlp=None,
                 local_size=2, feat_unfold=True, eval_bsize=None, non_local_attn=True, multi_scale=[2],
                 softmax_scale=1):
        super().__init__()
        self.feat_unfold = feat_unfold
        self.eval_bsize = eval_bsize
        self.local_size = local_size
        self.non_local_attn = non_local_attn
        self.multi_scale = list(multi_scale)
        self.softmax_scale = softmax_scale
        imnet_q, imnet_k, imnet_v = copy.deepcopy(imnet_q), copy.deepcopy(imnet_k), copy.deepcopy(imnet_v)
        self.encoder = build_backbone(encoder)
        dim = self.encoder.mid_channels if hasattr(self.encoder, 'mid_channels') else self.encoder.embed_dim
        self.imnet_dim = dim
        # dims wiring, ciaosr_net.py:61-76
        if not feat_unfold and non_local_attn:
            # the reference builds imnet_v with the non-local channels (ciaosr_net.py:73-76) but only concatenates the
            # non-local map inside `if self.feat_unfold:` (:129-141): its own forward fails on the shape mismatch
            raise ValueError('feat_unfold=False needs non_local_attn=False (the reference concatenates the non-local map '
                             'only on the unfold branch, ciaosr_net.py:129-141)')
        mult = 9 if feat_unfold else 1                      # ciaosr_net.py:61-68
        imnet_q['in_dim'] = dim * mult
        imnet_k['in_dim'] = imnet_k['out_dim'] = dim * mult
        imnet_v['in_dim'] = imnet_v['out_dim'] = dim * mult
        imnet_k['in_dim'] += 4
        imnet_v['in_dim'] += 4
        if non_local_attn:
            imnet_q['in_dim'] += dim * len(multi_scale)
            imnet_v['in_dim'] += dim * len(multi_scale)
            imnet_v['out_dim'] += dim * len(multi_scale)
        self.imnet_q = build_component(imnet_q)
        self.imnet_k = build_component(imnet_k)
        self.imnet_v = build_component(imnet_v)
        if non_local_attn:
            self.cs_attn = CrossScaleAttention(channel=dim, scale=multi_scale)
        self._head = PackedHead(self)

    # -- the reference interface ---------------------------------------------------------------
    def gen_feature(self, x, options=None):
        raise NotImplementedError('subclasses define gen_feature')

    def forward(self, x, coord, cell, test_mode=False, options=None):
        """x [B,3,H,W] normalised LR, coord/cell [B,Q,2] (y,x) -> [B,Q,3]   (ciaosr_net.py:88-110).
        `options` (extension, absent from the reference): hip_ops.Options / 'bf16' / None = exact-fp32 defaults."""
        chunk = None if (self.eval_bsize is None or not test_mode) else self.eval_bsize
        options = self.effective_options(options)
        enc = getattr(self, '_encoder_hip', None)
        if enc is not None:
            # HIP trunk: channels-last feature map goes straight into the head (no NCHW round trip)
            self._require_hip_trunk(x)
            x = x.contiguous().float()
            if hasattr(enc, 'forward_hwc_batch'):            # RDN: the batch shares the trunk's dense-layer launches
                feats = enc.forward_hwc_batch(x, options)
            else:
                feats = [enc.forward_hwc(x[b], options) for b in range(x.shape[0])]
            outs = [self._head.forward(None, x[b], coord[b], cell[b], chunk, feature_hwc=feats[b], options=options)
                    for b in range(x.shape[0])]
            return torch.stack(outs, 0)
        features = self.gen_feature(x, options)
        return self._predict(features, coord, cell, chunk, x, options)

    @torch.no_grad()
    def encode(self, x, options=None, q_plan=None):
        """The part of `forward` that depends on the LR batch only, once: trunk, then per item the head's per-image stages into a Scene
        (head_hip.PackedHead.prepare).  `q_plan`: the query count of the largest full render intended (default: the x4 grid).  An
        extension, absent from the reference.  The two halves are callable on their own: `encode_trunk`, `encode_scenes`."""
        x, feats, options = self.encode_trunk(x, options)
        return self.encode_scenes(x, feats, options, q_plan)

    @torch.no_grad()
    def encode_trunk(self, x, options=None):
        """The trunk half of `encode`: -> (x as the trunk read it, channels-last feature maps feats[b], the effective Options).  The
        items of a batch share the trunk's launches where the trunk has a `forward_hwc_batch`; item b is bitwise the batch-1 call."""
        options = self.effective_options(options)
        enc = getattr(self, '_encoder_hip', None)
        if enc is None:
            raise CiaoSRHipError('encode needs a generator with a HIP trunk')
        self._require_hip_trunk(x)
        x = x.contiguous().float()
        if hasattr(enc, 'forward_hwc_batch'):
            feats = enc.forward_hwc_batch(x, options)
        else:
            feats = [enc.forward_hwc(x[b], options) for b in range(x.shape[0])]
        return x, feats, options

    @torch.no_grad()
    def encode_scenes(self, x, feats, options, q_plan=None):
        """The prepare half of `encode`: one Scene per item of `x` from its feature map (`encode_trunk`'s results, or slices of them)."""
        if q_plan is None:
            q_plan = 16 * x.shape[-2] * x.shape[-1]
        return EncodedFeatures([self._head.prepare(None, options, q_plan, feature_hwc=feats[b]) for b in range(x.shape[0])], x, options)

    @torch.no_grad()
    def render(self, enc, coord, cell, return_flags=False, chunk=None):
        """`forward(x, coord, cell, test_mode=True)` from an `encode` result: coord/cell [B,Q,2] (or [Q,2], shared by the batch) -> [B,Q,3],
        for any Q, any number of times.  `chunk`: the number of consecutive queries that share the shift radius of their first one,
        None: `eval_bsize` (1: every query has the radius of its own cell -- per-pixel warps).  `return_flags`: -> ([B,Q,3], [B] int32 on the device), per item the flag of
        `PackedHead.query(..., return_flag=True)` (scenes on the chained 16-bit kv kernel only)."""
        outs, flags = [], []
        for b, scene in enumerate(enc.scenes):
            cq, cl = (coord, cell) if coord.dim() == 2 else (coord[b], cell[b])
            out = self._head.query(scene, enc.x[b], cq, cl, self.eval_bsize if chunk is None else chunk, return_flag=return_flags)
            if return_flags:
                out, flag = out
                flags.append(flag)
            outs.append(out)
        if return_flags:
            return torch.stack(outs, 0), torch.cat(flags)
        return torch.stack(outs, 0)

    def scene_chained(self, h, w, q_plan, options=None):
        """Whether a scene of an h x w LR map planned for `q_plan` queries under `options` would answer queries with the chained 16-bit
        kv kernel (ciaosr_head_route_code, bit 8; `Scene.chained` of the scene once built).  Launches nothing."""
        from .head_hip import route_chained
        try:
            return route_chained(self._head.route_code(h, w, q_plan, self.effective_options(options)))
        except CiaoSRHipError:
            return False

    def effective_options(self, options=None):
        """The hip_ops.Options a call on THIS generator really runs with (subclasses may narrow what they accept)."""
        return hip_ops.as_options(options)

    def bind_test_cfg(self, test_cfg):
        """The restorer's test_cfg dict (kept by reference: later edits are seen), for the extensions a generator reads from it."""
        object.__setattr__(self, '_test_cfg', test_cfg)

    def _require_hip_trunk(self, x):
        """No silent PyTorch trunk: CPU input or a trunk shape outside the HIP library's coverage is an error."""
        hip_ops.require_gpu(x.contiguous() if x.dtype == torch.float32 else x.float().contiguous())
        enc = self._encoder_hip
        if not enc.supported():
            raise CiaoSRHipError('no HIP trunk for this encoder configuration (and no PyTorch fallback): ' + enc.why_unsupported())

    def _gen_feature_hip(self, x, options=None):
        """gen_feature of the three adapters: [B,3,H,W] -> [[B,C,H,W]] through the HIP trunk."""
        self._require_hip_trunk(x)
        x = x.contiguous().float()
        enc = self._encoder_hip
        return [torch.stack([hip_ops.hwc_to_nchw(enc.forward_hwc(x[b], options)) for b in range(x.shape[0])])]

    def query_rgb(self, features, coord, scale=None, options=None):
        """ciaosr_net.py:113-224 (no bilinear residual); `scale` is the cell tensor."""
        return self._predict(features, coord, scale, None, None, options)

    def batched_predict(self, x, coord, cell, options=None):
        """ciaosr_net.py:226-248: `x` is the feature list; eval_bsize chunking only matters through
        which query's cell defines the shift radius -- the kernels take it as `chunk`."""
        return self._predict(x, coord, cell, self.eval_bsize, None, options)

    def init_weights(self, pretrained=None, strict=True):
        if isinstance(pretrained, str):
            from .checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=strict)
        elif pretrained is not None:
            raise TypeError(f'"pretrained" must be a str or None. But received {type(pretrained)}.')

    # -- HIP path ------------------------------------------------------------------------------
    @torch.no_grad()
    def _predict(self, features, coord, cell, chunk, x_lr, options=None):
        options = self.effective_options(options)
        if isinstance(features, torch.Tensor):
            features = [features]
        if len(features) != 1:
            raise NotImplementedError('one feature map per image (every encoder adapter returns [feat])')
        feature = features[0]
        hip_ops.require_gpu(feature.contiguous(), coord.contiguous(), cell.contiguous())
        outs = []
        for b in range(feature.shape[0]):
            outs.append(self._head.forward(feature[b], None if x_lr is None else x_lr[b], coord[b], cell[b], chunk,
                                           options=options))
        return torch.stack(outs, 0)


class LocalImplicitSRRDN(LocalImplicitSRNet):
    def __init__(self, encoder, imnet_q, imnet_k, imnet_v, query_mlp=None, key_mlp=None, value_mlp=None,
                 local_size=2, feat_unfold=True, eval_bsize=None, non_local_attn=True, multi_scale=[2],
                 softmax_scale=1):
        super().__init__(encoder=encoder, imnet_q=imnet_q, imnet_k=imnet_k, imnet_v=imnet_v, query_mlp=query_mlp,
                         key_mlp=key_mlp, value_mlp=value_mlp, local_size=local_size, feat_unfold=feat_unfold,
                         eval_bsize=eval_bsize, non_local_attn=non_local_attn, multi_scale=multi_scale,
                         softmax_scale=softmax_scale)
        self.sfe1 = self.encoder.sfe1
        self.sfe2 = self.encoder.sfe2
        self.rdbs = self.encoder.rdbs
        self.gff = self.encoder.gff
        self.num_blocks = self.encoder.num_blocks
        del self.encoder
        self._encoder_hip = PackedEncoder(self, 'rdn')

    def gen_feature(self, x, options=None):
        """ciaosr_net.py:321-342 on the HIP trunk (csrc/encoder.hip)."""
        return self._gen_feature_hip(x, options)


class LocalImplicitSREDSR(LocalImplicitSRNet):
    def __init__(self, encoder, imnet_q, imnet_k, imnet_v, query_mlp=None, key_mlp=None, value_mlp=None,
                 local_size=2, feat_unfold=True, eval_bsize=None, non_local_attn=True, multi_scale=[2],
                 softmax_scale=1):
        super().__init__(encoder=encoder, imnet_q=imnet_q, imnet_k=imnet_k, imnet_v=imnet_v, query_mlp=query_mlp,
                         key_mlp=key_mlp, value_mlp=value_mlp, local_size=local_size, feat_unfold=feat_unfold,
                         eval_bsize=eval_bsize, non_local_attn=non_local_attn, multi_scale=multi_scale,
                         softmax_scale=softmax_scale)
        self.conv_first = self.encoder.conv_first
        self.body = self.encoder.body
        self.conv_after_body = self.encoder.conv_after_body
        del self.encoder
        self._encoder_hip = PackedEncoder(self, 'edsr')

    def gen_feature(self, x, options=None):
        """ciaosr_net.py:393-408 on the HIP trunk (csrc/encoder.hip)."""
        return self._gen_feature_hip(x, options)


class LocalImplicitSRSWINIR(LocalImplicitSRNet):
    """ciaosr_net.py:411-525: SwinIR trunk (HIP: csrc/swinir.hip) + the HIP head.  Leading `window_size` argument."""

    def __init__(self, window_size, encoder, imnet_q, imnet_k, imnet_v, query_mlp=None, key_mlp=None, value_mlp=None,
                 local_size=2, feat_unfold=True, eval_bsize=None, non_local_attn=True, multi_scale=[2],
                 softmax_scale=1):
        super().__init__(encoder=encoder, imnet_q=imnet_q, imnet_k=imnet_k, imnet_v=imnet_v, query_mlp=query_mlp,
                         key_mlp=key_mlp, value_mlp=value_mlp, local_size=local_size, feat_unfold=feat_unfold,
                         eval_bsize=eval_bsize, non_local_attn=non_local_attn, multi_scale=multi_scale,
                         softmax_scale=softmax_scale)
        self.window_size = window_size
        self.conv_first = self.encoder.conv_first
        self.patch_embed = self.encoder.patch_embed
        self.pos_drop = self.encoder.pos_drop
        self.layers = self.encoder.layers
        self.norm = self.encoder.norm
        self.patch_unembed = self.encoder.patch_unembed
        self.conv_after_body = self.encoder.conv_after_body
        del self.encoder
        from .swinir_hip import PackedSwinIR
        self._encoder_hip = PackedSwinIR(self)

    def gen_feature(self, img, options=None):
        """ciaosr_net.py:475-525 (reflect-pad to a window multiple, trunk, crop) on the HIP trunk (csrc/swinir.hip)."""
        return self._gen_feature_hip(img, options)

    _warned_bf16 = False
    allow_f16_substitute = False

    def effective_options(self, options=None):
        """`precision='bf16'` on the SwinIR-CiaoSR head (C = 180: 1620-wide logit dot products in front of the 4-way softmax) runs as
        **'bf16x3'**: bf16 hi + lo pairs for the head's weights AND activations (three MFMAs per product, fp32 Z, fp32 tables).  The
        plain bf16 forms -- 8-bit ACTIVATIONS, whatever the weights -- leave rms 3.6e-3 = 0.060 dB at a 30-dB quality level against the
        reference at BASELINE config 5's own size, six times the 0.01 dB gate, and are therefore not offered here; the pair form measures
        max |delta| 9.3e-6, 0.00005 dB (inside the fp32 tolerance) at 3.83 ms per image (f16: 3.71, fp32: 4.97).  `effective_options(opt)`
        returns what actually runs (labels and ratios are taken from it: bench.py does).  Rounds 4-5 refused the name or, on
        `test_cfg.allow_f16_substitute = True` (or the generator attribute), ran the IEEE-half kernels with a warning: that opt-in is
        still honoured.

        The SwinIR trunk is fp32 in every mode unless the options carry `swin_h16=1` (`test_cfg.hip_options`): then the modes whose trunk
        element type is f16 -- `opt.mode.trunk == 'f16'`: 'f16', 'f16-pairs', 'f16x3-fast' -- run qkv / proj / fc1 / fc2 of every Swin block on
        the f16 MFMA (csrc/swinir_h16.hip, PSNR-gated) and batches of tiles share those launches.  In 'fp32', 'f16x3' and every bf16 mode
        the option is ignored: 'f16x3' and 'bf16x3' promise the fp32 tolerance with an fp32 trunk, and 'bf16' here runs as 'bf16x3'.  The
        rule is applied to what this function RETURNS (PackedSwinIR.uses_h16)."""
        opt = hip_ops.as_options(options)
        if opt.mode.name not in ('bf16', 'bf16-single'):      # 'bf16x3' asked for by name, or not a bf16 mode
            return opt
        cfg = getattr(self, '_test_cfg', None)
        if not (self.allow_f16_substitute or (cfg is not None and cfg.get('allow_f16_substitute', False))):
            return opt.replace(precision='bf16x3')             # bf16 as named: the pair form that meets the gate
        if not LocalImplicitSRSWINIR._warned_bf16:
            import warnings
            warnings.warn("precision='bf16' on the SwinIR-CiaoSR head does not meet the 0.01 dB PSNR gate (8-bit activations in front of "
                          "the local attention: 0.060 dB at 30 dB on BASELINE config 5); running the IEEE-half ('f16') kernels instead "
                          "(allow_f16_substitute)", RuntimeWarning, stacklevel=3)
            LocalImplicitSRSWINIR._warned_bf16 = True
        return opt.replace(precision='f16')
