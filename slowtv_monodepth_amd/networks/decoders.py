"""Monodepth(2) decoder — registry key `monodepth` (reference: `src/networks/decoders/monodepth.py:14-89`) — and the CADepth decoder built on it —
registry key `cadepth` (reference: `src/networks/decoders/cadepth.py`) — and the DDVNet decoder — registry key `ddvnet` (reference:
`src/networks/decoders/ddvnet.py`) — and the DiffNet decoder — registry key `diffnet` (reference: `src/networks/decoders/diffnet.py`) — and the SuperDepth
decoder — registry key `superdepth` (reference: `src/networks/decoders/superdepth.py`)."""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..registry import register

__all__ = ['MonodepthDecoder', 'CaDepthDecoder', 'DetailEmphasis', 'DDVNetDecoder', 'SelfAttentionBlock', 'DiffNetDecoder', 'AttentionBlock', 'ChannelAttention', 'SuperdepthDecoder',
           'SubPixelConv', 'ACT']

ACT = {'sigmoid': nn.Sigmoid(), 'relu': nn.ReLU(inplace=True), 'none': nn.Identity(), None: nn.Identity()}


def conv3x3(cin: int, cout: int) -> nn.Conv2d:
    """3x3 conv with reflection padding (src/networks/decoders/utils.py:44-46)."""
    return nn.Conv2d(cin, cout, 3, padding=1, padding_mode='reflect')


class ConvELU(nn.Sequential):
    def __init__(self, cin, cout): super().__init__(conv3x3(cin, cout), nn.ELU(inplace=True))


@register('monodepth')
class MonodepthDecoder(nn.Module):
    """Five up-convolution stages (256..16 channels) with encoder skips where a matching stride exists, and a
    3x3 output head per requested scale.

    :param num_ch_enc / enc_sc: channels and strides of the encoder features.
    :param out_sc: scales (as log2 stride) at which to emit a prediction; out_ch / out_act: its channels / activation.
    """
    def __init__(self, num_ch_enc, enc_sc, upsample_mode: str = 'nearest', use_skip: bool = True,
                 out_sc=(0, 1, 2, 3), out_ch: int = 1, out_act: str = 'sigmoid'):
        super().__init__()
        if out_act not in ACT: raise KeyError(f'Invalid activation key. ({out_act} vs. {tuple(ACT.keys())}')
        self.num_ch_enc, self.enc_sc = list(num_ch_enc), list(enc_sc)
        self.upsample_mode, self.use_skip, self.out_sc, self.out_ch = upsample_mode, use_skip, list(out_sc), out_ch
        self.act = ACT[out_act]
        self.num_ch_dec = [16, 32, 64, 128, 256]
        self.up0, self.up1, self.out = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        for i in range(4, -1, -1):
            cin = self.num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]
            self.up0[str(i)] = ConvELU(cin, self.num_ch_dec[i])
            cin = self.num_ch_dec[i]
            if use_skip and 2**i in self.enc_sc: cin += self.num_ch_enc[self.enc_sc.index(2**i)]
            self.up1[str(i)] = ConvELU(cin, self.num_ch_dec[i])
        for i in self.out_sc: self.out[str(i)] = conv3x3(self.num_ch_dec[i], out_ch)

    def forward(self, feat):
        x = feat[-1]
        amp_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and (amp_bf16 or not torch.is_autocast_enabled()) and self.upsample_mode == 'nearest':
            return self._forward_glued(feat, torch.bfloat16 if amp_bf16 else None)
        out = {}
        for i in range(4, -1, -1):
            x = F.interpolate(self.up0[str(i)](x), scale_factor=2, mode=self.upsample_mode)
            if self.use_skip and 2**i in self.enc_sc: x = torch.cat((x, feat[self.enc_sc.index(2**i)]), 1)
            x = self.up1[str(i)](x)
            if i in self.out_sc: out[i] = self.act(self.out[str(i)](x))
        return out

    def _forward_glued(self, feat, out_dtype=None):
        """Same network, same parameters; the ops BETWEEN the convolutions (ELU, nearest x2, cat, reflection pad) run as
        the two gather kernels of `csrc/smd_decoder.hip`, each writing the next convolution's padded input, and the
        padded ELU output of a stage is shared by its output head and the next stage (the reference pads it twice)."""
        from .. import functional as HF
        conv = self._conv_glued
        out = {}
        xp = HF.elu_pad(feat[-1], apply_elu=False, out_dtype=out_dtype)   # under bf16 autocast the glue writes bf16 for the bf16 convolutions
        for i in range(4, -1, -1):
            m0, m1 = self.up0[str(i)][0], self.up1[str(i)][0]
            skip = feat[self.enc_sc.index(2**i)] if (self.use_skip and 2**i in self.enc_sc) else None
            c = conv(m1, HF.elu_up_cat_pad(conv(m0, xp), skip, bias=m0.bias.float(), out_dtype=out_dtype))
            if i in self.out_sc or i > 0: xp = HF.elu_pad(c, bias=m1.bias.float(), apply_elu=True, out_dtype=out_dtype)
            if i in self.out_sc: out[i] = self._head_glued(i, xp)
        return out

    @staticmethod
    def _conv_glued(m, xp):
        """The bias-free 3x3 convolution of an already reflection-padded input; the bias is added by whoever consumes the result."""
        from .. import functional as HF
        co, ci = m.weight.shape[:2]
        if (co % 32 == 0 and ci % 16 == 0) or (co == 16 and ci in (16, 32)):
            # smd_conv3x3_mfma_* (bf16 matrix cores; fp32 tensors: three-way split operands, fp32-class results; bf16 tensors under autocast: one piece) or, per
            # operator and shape by this box's A/B, MIOpen (the wide stages) / the f32-MFMA kernels smd_conv3x3_thin_* (the 16-channel last stage in fp32)
            return HF.conv3x3_wide(xp, m.weight.float())
        return F.conv2d(xp, m.weight)

    def _head_glued(self, i, xp):
        """The output head of scale i on the padded activation `xp`."""
        return self._head_stencil(self.out[str(i)], xp)

    def _head_stencil(self, m, xp):
        """The head convolution `m` with this decoder's activation on the padded activation `xp`."""
        from .. import functional as HF
        if self.out_ch == 1 and isinstance(self.act, (nn.Sigmoid, nn.Identity)):   # a one-channel head is a stencil: smd_conv3x3_head_* (fp32 or bf16 activation in, fp32 out)
            return HF.conv3x3_head(xp, m.weight.float(), m.bias.float() if m.bias is not None else None, 'sigmoid' if isinstance(self.act, nn.Sigmoid) else None)
        if 1 <= self.out_ch <= 4 and isinstance(self.act, (nn.Sigmoid, nn.ReLU, nn.Identity)):   # a few channels (or one with relu) are still a stencil: smd_conv3x3_headn_* (the mask decoder)
            act = 'sigmoid' if isinstance(self.act, nn.Sigmoid) else ('relu' if isinstance(self.act, nn.ReLU) else None)
            return HF.conv3x3_headn(xp, m.weight.float(), m.bias.float() if m.bias is not None else None, act)
        return self.act(F.conv2d(xp, m.weight, m.bias))


class DetailEmphasis(nn.Module):
    """Detail emphasis of CADepth (src/networks/decoders/cadepth.py:30-46): conv3x3 + BatchNorm + ReLU, then the squeeze-excite gate `x + x*att(x)`.
    Same sub-module names as the reference's, so its state-dict entries load as they are."""
    def __init__(self, ch: int):
        super().__init__()
        self.conv = nn.Sequential(conv3x3(ch, ch), nn.BatchNorm2d(ch), nn.ReLU(inplace=True))
        self.att = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(ch, ch, 1), nn.ReLU(inplace=True), nn.Conv2d(ch, ch, 1), nn.Sigmoid())

    def forward(self, x):
        x = self.conv(x)
        return x + x*self.att(x)


@register('cadepth')
class CaDepthDecoder(MonodepthDecoder):
    """CADepth (https://arxiv.org/abs/2112.13047; reference: src/networks/decoders/cadepth.py:49-126): the Monodepth decoder with structure perception
    (channel self-attention) on the deepest encoder feature and detail emphasis (conv + BN + ReLU + squeeze-excite gate) on every stage's concatenation.
    Same constructor arguments as `MonodepthDecoder`; `de[str(i)]` is the reference's `detail_emphasis_{i}` (`networks/checkpoint.py` translates the names).

    Precision: on CUDA the glued path computes in fp32, also under bf16 autocast.  It then takes fp32 time and returns fp32 disparities while the encoder
    around it runs in bf16; a bf16 form of this decoder does not exist (`forward` says what was measured).  Autocast to fp16 takes the plain ATen path."""

    def __init__(self, num_ch_enc, enc_sc, upsample_mode: str = 'nearest', use_skip: bool = True,
                 out_sc=(0, 1, 2, 3), out_ch: int = 1, out_act: str = 'sigmoid'):
        super().__init__(num_ch_enc, enc_sc, upsample_mode, use_skip, out_sc, out_ch, out_act)
        self.de = nn.ModuleDict({str(i): DetailEmphasis(self.up1[str(i)][0].in_channels) for i in range(4, -1, -1)})
        self._glued = True

    @contextlib.contextmanager
    def plain_path(self):
        """Within the block THIS decoder evaluates its plain ATen path wherever its tensors live (the yardstick the glued path is compared and timed against)."""
        prev, self._glued = self._glued, False
        try: yield self
        finally: self._glued = prev

    @staticmethod
    def structure_perception(x):
        b, c, h, w = x.shape
        v = x.view(b, c, -1)
        att = v @ v.permute(0, 2, 1)
        att = att.max(dim=-1, keepdim=True)[0] - att
        return x + (att.softmax(dim=-1) @ v).view(b, c, h, w)

    def forward(self, feat):
        x = feat[-1]
        amp_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if self._glued and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and (amp_bf16 or not torch.is_autocast_enabled()) and self.upsample_mode == 'nearest':
            # Under bf16 autocast this decoder stays in fp32: with its convolutions in bf16 the feature gradients are 6e-2 ... 9e-2 of their sum of magnitudes off
            # the fp32 run (ATen's own autocast of the plain path: 9e-2 ... 15e-2), outside the 5e-2 the Monodepth decoder's bf16 path holds
            with torch.autocast('cuda', enabled=False): return self._forward_glued([f.float() for f in feat])
        out = {}
        x = self.structure_perception(x)
        for i in range(4, -1, -1):
            x = F.interpolate(self.up0[str(i)](x), scale_factor=2, mode=self.upsample_mode)
            if self.use_skip and 2**i in self.enc_sc: x = torch.cat((x, feat[self.enc_sc.index(2**i)]), 1)
            x = self.up1[str(i)](self.de[str(i)](x))
            if i in self.out_sc: out[i] = self.act(self.out[str(i)](x))
        return out

    # Static routing of the two attention operators by channel count, from profiles/cadepth_times.txt (b = 12 at 192 x 640, forward + backward, kernel vs ATen):
    #   channel_attention (12,128,6,20) 0.08 vs 0.28 ms, (12,256,6,20) 0.16 vs 0.32 ms: the kernel pair wins; (12,512,6,20) 0.49 vs 0.30 ms, (12,1024,6,20) 1.43 vs
    #     0.51 ms: rocBLAS's batched GEMMs win, and at any batch (the grid scales with B: (4,512,6,20) 0.29 vs 0.28 ms, forward alone 0.086 vs 0.062).  C >= 512 goes to ATen.
    #   se_gate (12,512,12,40) 0.38 vs 0.28 ms, but (12,256,24,80) 0.14 vs 0.28 and 2.6-3.3x from there down: the per-sample block that does the two
    #     C x C matrix-vector products is the cost at C = 512.  C >= 512 goes to ATen.
    @staticmethod
    def _attention_plain(x): return x.shape[1] >= 512

    @staticmethod
    def _gate_plain(x): return x.shape[1] >= 512

    def _forward_glued(self, feat):
        """Same network, same parameters, fp32.  `smd_channel_attention_*` on the deepest feature; per stage the Monodepth glue (`elu_up_cat_pad` writes the
        padded concatenation the detail-emphasis convolution reads), `batch_norm_act` for BN + ReLU (eval mode: the ATen affine form on the running statistics),
        `smd_se_gate_*` for the gate, `elu_pad` for the paddings, the stencil heads."""
        from .. import functional as HF
        conv = self._conv_glued
        out = {}
        x = feat[-1]
        xp = HF.elu_pad(self.structure_perception(x) if self._attention_plain(x) else HF.channel_attention(x), apply_elu=False)
        for i in range(4, -1, -1):
            m0, m1, de = self.up0[str(i)][0], self.up1[str(i)][0], self.de[str(i)]
            dc, bn = de.conv[0], de.conv[1]
            skip = feat[self.enc_sc.index(2**i)] if (self.use_skip and 2**i in self.enc_sc) else None
            d = conv(dc, HF.elu_up_cat_pad(conv(m0, xp), skip, bias=m0.bias)) + dc.bias.view(1, -1, 1, 1)
            if bn.training and bn.track_running_stats and bn.momentum is not None and bn.affine:
                d = HF.batch_norm_act(d, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=bn.momentum, eps=bn.eps, relu=True)
                with torch.no_grad(): bn.num_batches_tracked += 1
            else:
                d = F.relu(bn(d), inplace=True)
            g = d + d*de.att(d) if self._gate_plain(d) else HF.se_gate(d, de.att[1].weight, de.att[1].bias, de.att[3].weight, de.att[3].bias)
            c = conv(m1, HF.elu_pad(g, apply_elu=False))
            if i in self.out_sc or i > 0: xp = HF.elu_pad(c, bias=m1.bias, apply_elu=True)
            if i in self.out_sc: out[i] = self._head_glued(i, xp)
        return out


class SelfAttentionBlock(nn.Module):
    """The self-attention block of DDVNet (src/networks/decoders/ddvnet.py:37-54): three 1x1 convolutions + ReLU, then `softmax(q k^T) v` over CHANNELS
    (the C x C matrix), no residual.  Same sub-module names as the reference's."""
    def __init__(self, ch: int):
        super().__init__()
        self.query_conv = nn.Sequential(nn.Conv2d(ch, ch, 1), nn.ReLU(inplace=True))
        self.key_conv = nn.Sequential(nn.Conv2d(ch, ch, 1), nn.ReLU(inplace=True))
        self.value_conv = nn.Sequential(nn.Conv2d(ch, ch, 1), nn.ReLU(inplace=True))

    def forward(self, x):
        b, c, h, w = x.shape
        q, k, v = self.query_conv(x).flatten(-2, -1), self.key_conv(x).flatten(-2, -1).permute(0, 2, 1), self.value_conv(x).flatten(-2, -1)
        return ((q @ k).softmax(dim=-1) @ v).view(b, c, h, w)


@register('ddvnet')
class DDVNetDecoder(MonodepthDecoder):
    """DDVNet (https://arxiv.org/abs/2003.13951; reference: src/networks/decoders/ddvnet.py:57-152): the Monodepth decoder behind a self-attention block on the
    deepest encoder feature, with heads that emit 128 logits per output channel — a discrete disparity volume — and return its expectation over the bin
    values `bins[k] = k/128`.  Same constructor arguments as `MonodepthDecoder`; `out_act` is validated but, as in the reference, not applied.  `att` is the
    reference's `convs['att']` (`networks/checkpoint.py` translates the names).

    On CUDA (fp32, nearest up-sampling) the stages run on the Monodepth glue and every head is `functional.ddv_head`: convolution, softmax and expectation
    in one kernel that never writes the logit volume.  That path leaves `self.logits` EMPTY (nothing in the reference reads it); the plain ATen path (CPU,
    other up-sampling modes, `plain_path()`) fills `self.logits[i]` as the reference does.  The attention block stays on ATen: every supported encoder
    gives it 512 channels or more, where rocBLAS's batched GEMMs win (profiles/cadepth_times.txt).

    Precision: on CUDA the glued path computes in fp32, also under bf16 autocast (the rule `CaDepthDecoder` follows): it then takes fp32 time and returns
    fp32 disparities while the encoder around it runs in bf16.  Autocast to fp16 takes the plain ATen path."""
    num_bins = 128

    def __init__(self, num_ch_enc, enc_sc, upsample_mode: str = 'nearest', use_skip: bool = True,
                 out_sc=(0, 1, 2, 3), out_ch: int = 1, out_act: str = 'sigmoid'):
        super().__init__(num_ch_enc, enc_sc, upsample_mode, use_skip, out_sc, out_ch, out_act)
        self.bins = nn.Parameter((torch.arange(self.num_bins)/self.num_bins).view(1, self.num_bins, 1, 1), requires_grad=False)
        self.att = SelfAttentionBlock(self.num_ch_enc[-1])
        for i in self.out_sc: self.out[str(i)] = conv3x3(self.num_ch_dec[i], self.num_bins*out_ch)
        self.logits = {}
        self._glued = True

    @contextlib.contextmanager
    def plain_path(self):
        """Within the block THIS decoder evaluates its plain ATen path wherever its tensors live (the yardstick the glued path is compared and timed against)."""
        prev, self._glued = self._glued, False
        try: yield self
        finally: self._glued = prev

    def expected_disparity(self, logits):
        """(b, 128, h, w) logits -> (b, 1, h, w): the expectation of the bin values under softmax(logits) (ddvnet.py:116-124)."""
        return (logits.softmax(dim=1)*self.bins).sum(dim=1, keepdim=True)

    def forward(self, feat):
        x = feat[-1]
        amp_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if self._glued and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and (amp_bf16 or not torch.is_autocast_enabled()) and self.upsample_mode == 'nearest' \
                and 1 <= self.out_ch <= 4:
            with torch.autocast('cuda', enabled=False): return self._forward_glued([f.float() for f in feat])
        out = {}
        x = self.att(x)
        for i in range(4, -1, -1):
            x = F.interpolate(self.up0[str(i)](x), scale_factor=2, mode=self.upsample_mode)
            if self.use_skip and 2**i in self.enc_sc: x = torch.cat((x, feat[self.enc_sc.index(2**i)]), 1)
            x = self.up1[str(i)](x)
            if i in self.out_sc: out[i] = self._head_plain(i, x)
        return out

    def _head_plain(self, i, x):
        """The head of scale i on the (unpadded) stage output, the reference's sequence; fills `self.logits[i]`."""
        logits = self.out[str(i)](x)
        self.logits[i] = logits
        return torch.cat([self.expected_disparity(l) for l in logits.chunk(self.out_ch, dim=1)], dim=1)

    def _forward_glued(self, feat):
        """Same network, same parameters, fp32: the attention block on ATen, the Monodepth stage glue (`elu_pad`, `elu_up_cat_pad`, the routed convolutions),
        `ddv_head` on the padded stage output it shares with the next stage."""
        from .. import functional as HF
        conv = self._conv_glued
        out = {}
        self.logits = {}
        xp = HF.elu_pad(self.att(feat[-1]), apply_elu=False)
        for i in range(4, -1, -1):
            m0, m1 = self.up0[str(i)][0], self.up1[str(i)][0]
            skip = feat[self.enc_sc.index(2**i)] if (self.use_skip and 2**i in self.enc_sc) else None
            c = conv(m1, HF.elu_up_cat_pad(conv(m0, xp), skip, bias=m0.bias))
            if i in self.out_sc or i > 0: xp = HF.elu_pad(c, bias=m1.bias, apply_elu=True)
            if i in self.out_sc: out[i] = self._head_glued(i, xp)
        return out

    def _head_glued(self, i, xp):
        from .. import functional as HF
        m = self.out[str(i)]
        return HF.ddv_head(xp, m.weight, m.bias, self.out_ch)


def conv_block(cin: int, cout: int) -> nn.Sequential:
    """conv3x3 + ELU under the reference's sub-module names (src/networks/decoders/utils.py:49-54)."""
    return nn.Sequential(OrderedDict(conv=conv3x3(cin, cout), act=nn.ELU(inplace=True)))


def upsample_block(cin: int, cout: int, upsample_mode: str = 'nearest') -> nn.Sequential:
    """A stage without a skip connection (diffnet.py:12-18): conv + ELU, x2, conv + ELU."""
    return nn.Sequential(conv_block(cin, cout), nn.Upsample(scale_factor=2, mode=upsample_mode), conv_block(cout, cout))


class ChannelAttention(nn.Module):
    """The squeeze-excite gate of DiffNet (diffnet.py:21-47): `x * sigmoid(fc(mean_hw(x)))` with two bias-free Linear layers around a `ch // ratio`
    bottleneck.  `flatten(1)` where the reference squeezes: the same for every batch size, 1 included."""
    def __init__(self, ch: int, ratio: int = 16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(ch, ch//ratio, bias=False), nn.ReLU(inplace=True), nn.Linear(ch//ratio, ch, bias=False))

    def forward(self, x):
        return x*self.fc(self.avg_pool(x).flatten(1)).sigmoid()[..., None, None]


class AttentionBlock(nn.Module):
    """A stage with a skip connection (diffnet.py:50-74): `cat(x2(x), skip)` -> channel attention -> conv3x3 -> ReLU.  Same sub-module names as the reference's."""
    def __init__(self, in_ch: int, skip_ch: int, out_ch: int | None = None, upsample_mode: str = 'nearest'):
        super().__init__()
        self.in_ch, self.out_ch, self.upsample_mode = in_ch + skip_ch, out_ch or in_ch, upsample_mode
        self.layers = nn.Sequential(ChannelAttention(self.in_ch), conv3x3(self.in_ch, self.out_ch), nn.ReLU(inplace=True))

    def forward(self, x, x_skip):
        return self.layers(torch.cat((F.interpolate(x, scale_factor=2, mode=self.upsample_mode), x_skip), dim=1))


@register('diffnet')
class DiffNetDecoder(nn.Module):
    """DiffNet (https://arxiv.org/abs/2110.09482; reference: src/networks/decoders/diffnet.py:77-146): five stages (256..16 channels); a stage whose
    stride is among `enc_sc` is an `AttentionBlock` on the concatenation with that encoder feature, the others are `upsample_block`s.  Same constructor
    arguments, sub-module names and double registration (`convs`, a ModuleDict, and `decoder`, a ModuleList of the same modules) as the reference, so its
    state dict IS the reference's: `networks/checkpoint.py` passes the names through.  `outconv_0..3` always exist; they are applied for the scales in `out_sc`.

    On CUDA (fp32, nearest up-sampling) everything in front of an attention stage's convolution — up-sampling, concatenation, pooling, gate, multiply,
    reflection padding — is `functional.up_cat_gate_pad`, one pass that writes the convolution's padded input; the stage's ReLU and bias are folded into the
    next stage's call and into `functional.relu_pad`, whose output the head reads.  The plain ATen path (CPU, other up-sampling modes, `plain_path()`) is the
    reference's sequence.

    Precision: on CUDA the glued path computes in fp32, also under bf16 autocast (the rule `CaDepthDecoder` follows): it then takes fp32 time and returns
    fp32 disparities while the encoder around it runs in bf16.  Autocast to fp16 takes the plain ATen path."""

    def __init__(self, num_ch_enc, enc_sc, upsample_mode: str = 'nearest', use_skip: bool = True,
                 out_sc=(0, 1, 2, 3), out_ch: int = 1, out_act: str = 'sigmoid'):
        super().__init__()
        if out_act not in ACT: raise KeyError(f'Invalid activation key. ({out_act} vs. {tuple(ACT.keys())}')
        self.num_ch_enc, self.enc_sc = list(num_ch_enc), list(enc_sc)
        self.upsample_mode, self.use_skip, self.out_sc, self.out_ch, self.out_act = upsample_mode, use_skip, list(out_sc), out_ch, out_act
        self.act = ACT[out_act]
        self.num_ch_dec = [16, 32, 64, 128, 256]
        self.convs = nn.ModuleDict()
        for i in range(4, -1, -1):
            cin, cout = (self.num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]), self.num_ch_dec[i]
            if self._has_skip(i): self.convs[f'upconv_{i}'] = AttentionBlock(cin, self.num_ch_enc[self.enc_sc.index(2**i)], cout, upsample_mode)
            else: self.convs[f'upconv_{i}'] = upsample_block(cin, cout, upsample_mode)
        for i in range(4): self.convs[f'outconv_{i}'] = conv3x3(self.num_ch_dec[i], out_ch)
        self.decoder = nn.ModuleList(list(self.convs.values()))
        self._glued = True

    def _has_skip(self, i: int) -> bool: return self.use_skip and 2**i in self.enc_sc

    @contextlib.contextmanager
    def plain_path(self):
        """Within the block THIS decoder evaluates its plain ATen path wherever its tensors live (the yardstick the glued path is compared and timed against)."""
        prev, self._glued = self._glued, False
        try: yield self
        finally: self._glued = prev

    def forward(self, feat):
        x = feat[-1]
        amp_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if self._glued and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and (amp_bf16 or not torch.is_autocast_enabled()) and self.upsample_mode == 'nearest' \
                and self._stages_glue():
            with torch.autocast('cuda', enabled=False): return self._forward_glued([f.float() for f in feat])
        out = {}
        for i in range(4, -1, -1):
            m = self.convs[f'upconv_{i}']
            x = m(x, feat[self.enc_sc.index(2**i)]) if self._has_skip(i) else m(x)
            if i in self.out_sc: out[i] = self.act(self.convs[f'outconv_{i}'](x))
        return out

    def _stages_glue(self) -> bool:
        """The glue hands an attention stage a raw tensor with the ReLU code or none: no attention stage may follow an `upsample_block` (whose activation is
        ELU) and the gate needs a bottleneck of at least one channel.  Every ResNet and ConvNeXt trunk qualifies."""
        skips = [self._has_skip(i) for i in range(4, -1, -1)]
        return all(a or not b for a, b in zip(skips, skips[1:])) and all(m.layers[0].fc[0].out_features >= 1 for m in self.convs.values() if isinstance(m, AttentionBlock))

    def _forward_glued(self, feat):
        """Same network, same parameters, fp32.  Per attention stage `up_cat_gate_pad` writes the padded, gated concatenation and the routed bias-free
        convolution reads it; the raw result goes, with its bias and the ReLU code, into the next stage's `up_cat_gate_pad`, and through `relu_pad` to the
        stage's head and to a following `upsample_block`.  Those run on the Monodepth glue (`elu_up_cat_pad` without a skip, `elu_pad`)."""
        from .. import functional as HF
        conv = MonodepthDecoder._conv_glued
        out = {}
        raw, bias, act, xp = feat[-1], None, None, None          # (raw, bias, act): what the next attention stage takes as `a`
        for i in range(4, -1, -1):
            m = self.convs[f'upconv_{i}']
            if self._has_skip(i):
                gate, cv = m.layers[0], m.layers[1]
                xin = HF.up_cat_gate_pad(raw, feat[self.enc_sc.index(2**i)], gate.fc[0].weight, gate.fc[2].weight, bias=bias, act=act)
                raw, bias, act = conv(cv, xin), cv.bias, 'relu'
                if i in self.out_sc or (i > 0 and not self._has_skip(i - 1)): xp = HF.relu_pad(raw, bias)
            else:
                m0, m1 = m[0].conv, m[2].conv
                if xp is None: xp = HF.elu_pad(feat[-1], apply_elu=False)
                c = conv(m1, HF.elu_up_cat_pad(conv(m0, xp), None, bias=m0.bias))
                if i in self.out_sc or i > 0: xp = HF.elu_pad(c, bias=m1.bias, apply_elu=True)
            if i in self.out_sc: out[i] = MonodepthDecoder._head_stencil(self, self.convs[f'outconv_{i}'], xp)
        return out


class SubPixelConv(nn.Module):
    """Sub-pixel convolution (src/networks/decoders/superdepth.py:13-26): a depth-wise 3x3 convolution that makes `up_factor**2` channels of every input
    channel, then `PixelShuffle(up_factor)`.  The reference's initialisation: zero bias, and the rows of the weight equal in groups of FOUR (its literal 4,
    whatever `up_factor` is).  Same sub-module names as the reference's."""
    def __init__(self, ch_in: int, up_factor: int):
        super().__init__()
        self.up_factor = up_factor
        self.conv = nn.Conv2d(ch_in, ch_in*up_factor**2, kernel_size=(3, 3), groups=ch_in, padding=1)
        self.shuffle = nn.PixelShuffle(up_factor)
        self.init_weights()

    def init_weights(self):
        nn.init.zeros_(self.conv.bias)
        self.conv.weight = nn.Parameter(self.conv.weight[::4].repeat_interleave(4, 0))

    def forward(self, x):
        return self.shuffle(self.conv(x))


@register('superdepth')
class SuperdepthDecoder(nn.Module):
    """SuperDepth (https://arxiv.org/abs/1806.01260; reference: src/networks/decoders/superdepth.py:29-118): the Monodepth stages (256..16 channels) with a
    `SubPixelConv(2)` + ReLU where Monodepth up-samples, and heads that shuffle scale i up by `2**i`: EVERY head returns a full-resolution map (the
    reference's behaviour).  Same constructor arguments, sub-module names and registration as the reference — `convs` is a plain `OrderedDict`, only
    `decoder`, a ModuleList of its values, is registered — so its state dict IS the reference's (`decoder.N.*` alone): `networks/checkpoint.py` passes the
    names through.  `upsample_mode` is accepted and, as in the reference, unused.

    On CUDA (fp32) everything between a stage's two convolutions — ELU, the depth-wise convolution, the shuffle, ReLU, the concatenation with the encoder
    feature, the reflection padding — is `functional.subpixel_conv`, one pass from the raw convolution output to the next convolution's padded input; the
    heads of scales 1..3 are `conv3x3_headn` and `subpixel_conv` with the output activation, the head of scale 0 is the Monodepth stencil.  The plain ATen path
    (the reference's sequence) serves the CPU, fp16 autocast, `upsample_mode != 'nearest'`, `plain_path()`, and the heads with more than four channels.

    Precision: on CUDA the glued path computes in fp32, also under bf16 autocast (the rule `CaDepthDecoder` and `DiffNetDecoder` follow): it then takes fp32
    time and returns fp32 disparities while the encoder around it runs in bf16.  Autocast to fp16 takes the plain ATen path."""

    def __init__(self, num_ch_enc, enc_sc, upsample_mode: str = 'nearest', use_skip: bool = True,
                 out_sc=(0, 1, 2, 3), out_ch: int = 1, out_act: str = 'sigmoid'):
        super().__init__()
        if out_act not in ACT: raise KeyError(f'Invalid activation key. ({out_act} vs. {tuple(ACT.keys())}')
        self.num_ch_enc, self.enc_sc = list(num_ch_enc), list(enc_sc)
        self.upsample_mode, self.use_skip, self.out_sc, self.out_ch, self.out_act = upsample_mode, use_skip, list(out_sc), out_ch, out_act
        self.activation = ACT[out_act]
        self.num_ch_dec = [16, 32, 64, 128, 256]
        self.convs = OrderedDict()
        for i in range(4, -1, -1):
            cin, cout = (self.num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]), self.num_ch_dec[i]
            self.convs[f'upconv_{i}_0'] = nn.Sequential(conv_block(cin, cout), SubPixelConv(cout, up_factor=2), nn.ReLU(inplace=True))
            cin = cout + (self.num_ch_enc[self.enc_sc.index(2**i)] if self._has_skip(i) else 0)
            self.convs[f'upconv_{i}_1'] = conv_block(cin, cout)
        for i in self.out_sc:
            if i == 0: self.convs[f'outconv_{i}'] = nn.Sequential(conv3x3(self.num_ch_dec[i], out_ch), self.activation)
            else: self.convs[f'outconv_{i}'] = nn.Sequential(conv_block(self.num_ch_dec[i], out_ch), SubPixelConv(out_ch, up_factor=2**i), self.activation)
        self.decoder = nn.ModuleList(list(self.convs.values()))
        self._glued = True

    def _has_skip(self, i: int) -> bool: return self.use_skip and 2**i in self.enc_sc

    @property
    def act(self): return self.activation      # (the name `MonodepthDecoder._head_stencil` reads)

    @contextlib.contextmanager
    def plain_path(self):
        """Within the block THIS decoder evaluates its plain ATen path wherever its tensors live (the yardstick the glued path is compared and timed against)."""
        prev, self._glued = self._glued, False
        try: yield self
        finally: self._glued = prev

    def forward(self, feat):
        x = feat[-1]
        amp_bf16 = torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
        if self._glued and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and (amp_bf16 or not torch.is_autocast_enabled()) and self.upsample_mode == 'nearest':
            with torch.autocast('cuda', enabled=False): return self._forward_glued([f.float() for f in feat])
        out = {}
        for i in range(4, -1, -1):
            x = [self.convs[f'upconv_{i}_0'](x)]
            if self._has_skip(i): x += [feat[self.enc_sc.index(2**i)]]
            x = self.convs[f'upconv_{i}_1'](torch.cat(x, 1))
            if i in self.out_sc: out[i] = self.convs[f'outconv_{i}'](x)
        return out

    def _act_name(self):
        return 'sigmoid' if isinstance(self.activation, nn.Sigmoid) else ('relu' if isinstance(self.activation, nn.ReLU) else None)

    def _forward_glued(self, feat):
        """Same network, same parameters, fp32.  Per stage: the routed bias-free convolution on the padded input, `subpixel_conv` (its bias and ELU, the
        sub-pixel convolution, ReLU, the skip, the padding), the second routed convolution, `elu_pad`, whose output the head and the next stage share."""
        from .. import functional as HF
        conv = MonodepthDecoder._conv_glued
        out = {}
        xp = HF.elu_pad(feat[-1], apply_elu=False)
        for i in range(4, -1, -1):
            m0, sp, m1 = self.convs[f'upconv_{i}_0'][0].conv, self.convs[f'upconv_{i}_0'][1].conv, self.convs[f'upconv_{i}_1'].conv
            skip = feat[self.enc_sc.index(2**i)] if self._has_skip(i) else None
            xin = HF.subpixel_conv(conv(m0, xp), sp.weight, sp.bias, 2, pre_bias=m0.bias, pre_act='elu', act='relu', skip=skip, pad=True)
            c = conv(m1, xin)
            if i in self.out_sc or i > 0: xp = HF.elu_pad(c, bias=m1.bias, apply_elu=True)
            if i in self.out_sc: out[i] = self._head_glued(i, xp)
        return out

    # Static routing of the heads' sub-pixel convolution by up-sampling factor, from profiles/superdepth_times.txt (b = 12 at 192 x 640, one channel, kernel vs
    # ATen): forward alone the kernel wins at every factor (r = 2: 0.017 vs 0.048 ms, r = 4: 0.018 vs 0.047, r = 8: 0.017 vs 0.046); forward + backward r = 2 wins
    # (0.097 vs 0.170), r = 4 ties (0.181 vs 0.179, at a third of the peak memory) and r = 8 loses (0.575 vs 0.150: the input-gradient gather sums 9 r^2 = 576
    # terms a pixel on a one-channel tensor too small to fill the device).  r >= 8 goes to ATen whenever a gradient may be asked for.
    @staticmethod
    def _head_plain(r): return r >= 8 and torch.is_grad_enabled()

    def _head_glued(self, i, xp):
        """The head of scale i on the padded stage output: scale 0 is the Monodepth stencil; scale i > 0 with at most four channels is the n-channel stencil
        (bias included, no activation) and `subpixel_conv` with the ELU in front and the output activation behind; wider heads, and the r = 8 head while gradients are recorded (`_head_plain`), run on ATen."""
        from .. import functional as HF
        m = self.convs[f'outconv_{i}']
        if i == 0: return MonodepthDecoder._head_stencil(self, m[0], xp)
        if 1 <= self.out_ch <= 4 and isinstance(self.activation, (nn.Sigmoid, nn.ReLU, nn.Identity)) and not self._head_plain(2**i):
            raw = HF.conv3x3_headn(xp, m[0].conv.weight, m[0].conv.bias, None)
            return HF.subpixel_conv(raw, m[1].conv.weight, m[1].conv.bias, 2**i, pre_act='elu', act=self._act_name())
        return self.activation(m[1](F.elu(F.conv2d(xp, m[0].conv.weight, m[0].conv.bias))))
