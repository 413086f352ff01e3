"""Weight packing + launch of the HIP SwinIR trunk (ciaosr_swinir_forward_f32, csrc/swinir.hip; with `Options(swin_h16=1)` in the
modes whose trunk element type is f16: ciaosr_swinir_forward_batch_f16, csrc/swinir_h16.hip): LocalImplicitSRSWINIR.gen_feature
(ciaosr_net.py:475-525) without PyTorch kernels."""
import ctypes as C

import torch

from . import _lib, hip_ops
from .encoder_hip import _pack_conv


def _ld(c):
    return (c + 63) // 64 * 64


def _pad_cols(w, ld):
    w = w.detach().float()
    if w.shape[1] < ld:
        w = torch.nn.functional.pad(w, (0, ld - w.shape[1]))
    return w.contiguous()


class PackedSwinIR:
    """Packed weights of the re-parented SwinIR trunk of a LocalImplicitSRSWINIR generator."""

    def __init__(self, net):
        self.net = net
        self._key = None
        self._st = None
        self._keep = None
        self._masks = {}
        self._lin32 = None       # per block: the padded fp32 (qkv, proj, fc1, fc2) weights the f16 copies are cast from
        self._has16 = False

    @staticmethod
    def uses_h16(options=None):
        """Whether a call with these options takes the f16-linear trunk: `swin_h16=1` AND a mode whose trunk element type is f16
        ('f16', 'f16-pairs', 'f16x3-fast').  fp32, 'f16x3' and every bf16 mode keep the fp32 trunk whatever the option says."""
        opt = hip_ops.as_options(options)
        return bool(opt.swin_h16) and opt.mode.trunk == 'f16'

    def trunk_half(self, options=None):
        """The `half` argument of struct() for a call with these options."""
        return 'f16' if self.uses_h16(options) else None

    def _params(self):
        n = self.net
        return [p for m in (n.conv_first, n.patch_embed, n.layers, n.norm, n.conv_after_body) for p in m.parameters()]

    def supported(self):
        n = self.net
        try:
            blk = n.layers[0].residual_group.blocks[0]
            c = n.conv_first.out_channels
            ws = n.window_size
            ok = isinstance(n.layers[0].conv, torch.nn.Conv2d) and isinstance(n.conv_after_body, torch.nn.Conv2d)
            ok = ok and n.conv_first.in_channels == 3 and c % 4 == 0 and c <= 512 and blk.mlp.fc1.out_features % 4 == 0
            ok = ok and ws * ws <= 64 and c % blk.num_heads == 0 and c // blk.num_heads <= 32 and (c // blk.num_heads) % 2 == 0
            ok = ok and n.patch_embed.norm is not None
            depths = {len(l.residual_group.blocks) for l in n.layers}
            return ok and len(depths) == 1 and all(b.window_size == ws for l in n.layers for b in l.residual_group.blocks)
        except (AttributeError, IndexError):
            return False

    def why_unsupported(self):
        n = self.net
        return (f'SwinIR trunk (embed_dim={n.conv_first.out_channels}, window_size={n.window_size}): the HIP trunk needs 3 input '
                f'channels, resi_connection="1conv", patch_norm=True, window_size <= 8, head_dim even and <= 32, embed_dim <= 512 '
                f'(a token in one wavefront\'s registers in the LayerNorms), embed_dim and the MLP width multiples of 4, and the same depth '
                f'in every group')

    def struct(self, half=None):
        """The packed fp32 struct; `half == 'f16'` adds (on first use, keyed like the fp32 struct) the IEEE-half copies of the four
        Linear weights of every block, cast on the device from the padded fp32 tensors."""
        key = tuple((p.data_ptr(), p._version) for p in self._params())
        if self._st is None or key != self._key:
            self._build(key)
        if half == 'f16' and not self._has16:
            for sb, ws32 in zip(self._st.blocks[:self._st.num_groups * self._st.depth], self._lin32):
                w16 = [w.to(torch.float16) for w in ws32]
                self._keep += w16
                sb.qkv_w16, sb.proj_w16, sb.fc1_w16, sb.fc2_w16 = (w.data_ptr() for w in w16)
            self._has16 = True
        return self._st

    def _build(self, key):
        n, keep = self.net, []
        lin32 = []
        dev = n.conv_first.weight.device
        Cc = n.conv_first.out_channels
        blk0 = n.layers[0].residual_group.blocks[0]
        heads, ws, hid = blk0.num_heads, n.window_size, blk0.mlp.fc1.out_features
        ld, ldh, d = _ld(Cc), _ld(hid), Cc // heads
        st = _lib.SwinirWeightsT()
        st.embed_dim, st.num_heads, st.window_size, st.hidden = Cc, heads, ws, hid
        st.num_groups, st.depth = len(n.layers), len(n.layers[0].residual_group.blocks)
        st.conv_first = _pack_conv(n.conv_first, keep, pad_cin_to=4)
        st.conv_after_body = _pack_conv(n.conv_after_body, keep, pad_cin_to=ld, frag=True)
        st.conv_after_body.cin = ld

        def dptr(t):
            t = t.detach().float().contiguous().to(dev)
            keep.append(t)
            return t.data_ptr()

        st.pe_norm_w, st.pe_norm_b = dptr(n.patch_embed.norm.weight), dptr(n.patch_embed.norm.bias)
        st.norm_w, st.norm_b = dptr(n.norm.weight), dptr(n.norm.bias)
        blocks = (_lib.SwinBlockT * (st.num_groups * st.depth))()
        gconv = (_lib.ConvT * st.num_groups)()
        for g, layer in enumerate(n.layers):
            for l, b in enumerate(layer.residual_group.blocks):
                sb = blocks[g * st.depth + l]
                a = b.attn
                scale = torch.ones(3 * Cc, device=dev)
                scale[:Cc] = a.scale                                    # q = (x W_q^T + b_q) * scale  (swinir_net.py:125)
                sb.ln1_w, sb.ln1_b = dptr(b.norm1.weight), dptr(b.norm1.bias)
                sb.qkv_w = dptr(_pad_cols(a.qkv.weight.detach().float() * scale[:, None], ld))
                i_qkv = len(keep) - 1
                sb.qkv_b = dptr(a.qkv.bias.detach().float() * scale)
                nn_ = ws * ws
                bias = a.relative_position_bias_table[a.relative_position_index.view(-1)].view(nn_, nn_, heads)
                sb.bias = dptr(bias.permute(2, 0, 1))
                sb.proj_w = dptr(_pad_cols(a.proj.weight, ld))
                i_proj = len(keep) - 1
                sb.proj_b = dptr(a.proj.bias)
                sb.ln2_w, sb.ln2_b = dptr(b.norm2.weight), dptr(b.norm2.bias)
                sb.fc1_w = dptr(_pad_cols(b.mlp.fc1.weight, ld))
                i_fc1 = len(keep) - 1
                sb.fc1_b = dptr(b.mlp.fc1.bias)
                sb.fc2_w = dptr(_pad_cols(b.mlp.fc2.weight, ldh))
                i_fc2 = len(keep) - 1
                sb.fc2_b = dptr(b.mlp.fc2.bias)
                lin32.append(tuple(keep[i] for i in (i_qkv, i_proj, i_fc1, i_fc2)))
                sb.shift = int(b.shift_size)
                sb.mask = None
            gconv[g] = _pack_conv(layer.conv, keep, pad_cin_to=ld, frag=True)
            gconv[g].cin = ld
        st.blocks, st.group_conv = blocks, gconv
        keep += [blocks, gconv]
        self._st, self._keep, self._key = st, keep, key
        self._lin32, self._has16 = lin32, False

    def _mask(self, hp, wp, dev):
        """calculate_mask (swinir_net.py:192-213) for the padded map size, shift = window_size // 2."""
        k = (hp, wp, str(dev))
        if k not in self._masks:
            from .encoders.swinir import shift_mask
            ws = self.net.window_size
            self._masks[k] = shift_mask(hp, wp, ws, ws // 2).contiguous().to(dev)
        return self._masks[k]

    def _set_masks(self, st, hp, wp, dev):
        # shifted blocks: the block's own attn_mask buffer when the map has its input_resolution, else calculate_mask(x_size)
        # -- exactly the reference's choice (swinir_net.py:233-236)
        self._mask_keep = []
        for g, layer in enumerate(self.net.layers):
            for l, b in enumerate(layer.residual_group.blocks):
                sb = st.blocks[g * st.depth + l]
                if b.shift_size > 0:
                    if tuple(b.input_resolution) == (hp, wp) and b.attn_mask is not None:
                        m = b.attn_mask.detach().float().contiguous()
                    else:
                        m = self._mask(hp, wp, dev)
                    hip_ops.require_gpu(m)
                    self._mask_keep.append(m)
                    sb.mask = m.data_ptr()
                else:
                    sb.mask = None

    @torch.no_grad()
    def forward_hwc(self, x_chw, options=None):
        """x [3,H,W] normalised LR (GPU) -> feature [H,W,C] channels-last.  The fp32 trunk unless `uses_h16(options)`: then the
        f16-linear entry with B = 1."""
        if self.uses_h16(options):
            return self._forward_h16(x_chw.unsqueeze(0), options)[0]
        x, st, wsb, out = self._prelude(x_chw)
        _lib.call('ciaosr_swinir_forward_f32', hip_ops.ptr(x), x.shape[1], x.shape[2], C.byref(st), hip_ops.ptr(out),
                  hip_ops.ptr(wsb), wsb.numel(), hip_ops.stream_ptr())
        return out

    def batches(self, options=None):
        """Whether forward_hwc_batch shares launches between the images of a batch with these options (the tile loops ask)."""
        return self.uses_h16(options)

    @torch.no_grad()
    def forward_hwc_batch(self, x_bchw, options=None):
        """x [B,3,H,W] normalised LR crops of one size (GPU) -> features [B,H,W,C] channels-last.  With `uses_h16(options)` the B images
        share every Swin-block launch (ciaosr_swinir_forward_batch_f16; image b bitwise the forward_hwc result).  Otherwise there is no
        batched fp32 entry: a LIST of the B forward_hwc results, launch for launch what a loop over the images runs."""
        if not self.uses_h16(options):
            return [self.forward_hwc(x_bchw[i], options) for i in range(x_bchw.shape[0])]
        return self._forward_h16(x_bchw, options)

    def _forward_h16(self, x_bchw, options):
        x, st, wsb, out = self._prelude(x_bchw, 'f16')
        B, _, H, W = x.shape
        _lib.call('ciaosr_swinir_forward_batch_f16', hip_ops.ptr(x), B, H, W, C.byref(st), hip_ops.ptr(out), hip_ops.as_options(options).c_arg(),
                  hip_ops.ptr(wsb), wsb.numel(), hip_ops.stream_ptr())
        return out

    def _prelude(self, x, half=None):
        """What both entries need for x [3,H,W] (fp32 entry) or [B,3,H,W] (`half`): x as contiguous fp32 on the GPU, the struct with
        this map size's masks set, the entry's workspace and the empty output [H,W,C] / [B,H,W,C]."""
        x = x.contiguous().float()
        hip_ops.require_gpu(x)
        *lead, _, H, W = x.shape
        st = self.struct(half)
        ws = st.window_size
        self._set_masks(st, (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws, x.device)
        lib = _lib.load()
        nbytes = lib.ciaosr_swinir_workspace_bytes_batch_f16(*lead, H, W, C.byref(st)) if half else lib.ciaosr_swinir_workspace_bytes(H, W, C.byref(st))
        wsb = hip_ops.workspace(nbytes, x.device, slot='encoder')
        return x, st, wsb, torch.empty(*lead, H, W, st.embed_dim, dtype=torch.float32, device=x.device)
