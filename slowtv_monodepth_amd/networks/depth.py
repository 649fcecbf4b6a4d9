"""`DepthNet` — registry key `depth` (reference: `src/networks/depth.py:16-156`)."""
from __future__ import annotations

import torch.nn as nn

from ..registry import DEC_REG, register
from .encoders import create_encoder

__all__ = ['DepthNet', 'MASKS']

MASKS = {'explainability': 'sigmoid', 'uncertainty': 'relu'}   # mask kind -> activation of the mask decoder's heads (src/networks/depth.py:12)


@register('depth')
class DepthNet(nn.Module):
    """Image -> multi-scale sigmoid disparity {s: (b,1,h/2^s,w/2^s)} + encoder features, and with `mask_name` the predictive
    masks {s: (b,num_ch_mask,h/2^s,w/2^s)} of a second decoder on the same features (src/networks/depth.py:108-114).

    Same constructor kwargs as the reference.  `mask_name`: 'explainability' (sigmoid heads) or 'uncertainty' (relu heads), one
    channel per support frame.  Virtual stereo and stereo blending are not served by the constructor and raise `NotImplementedError`;
    `forward_blended` is the blended forward as a method of its own.
    """
    def __init__(self, enc_name: str = 'resnet18', pretrained: bool = True, dec_name: str = 'monodepth', out_scales=(0, 1, 2, 3),
                 mask_name=None, num_ch_mask=None, use_virtual_stereo: bool = False, use_stereo_blend: bool = False):
        super().__init__()
        if dec_name not in DEC_REG: raise KeyError(f'Invalid decoder. ({dec_name} vs. {list(DEC_REG)}')
        if mask_name not in {None, 'explainability', 'uncertainty'}: raise KeyError(f'Invalid mask. ({mask_name})')
        if dec_name == 'ddvnet' and mask_name: raise KeyError('DDVNet is not compatible with mask prediction.')   # (src/networks/depth.py:81-82)
        if use_virtual_stereo: raise NotImplementedError('use_virtual_stereo (a three-channel disparity head and `disp_stereo`) is not served by this package')
        if use_stereo_blend: raise NotImplementedError('use_stereo_blend (a second, flipped forward pass blended into the first) is not served by this package')
        if mask_name and (num_ch_mask is None or int(num_ch_mask) <= 0):
            raise ValueError(f'Invalid number of mask channels. ({num_ch_mask} vs. >=1)')
        self.enc_name, self.pretrained, self.dec_name = enc_name, pretrained, dec_name
        self.out_scales = [out_scales] if isinstance(out_scales, int) else list(out_scales)
        self.mask_name, self.num_ch_mask = mask_name, num_ch_mask
        self.use_virtual_stereo, self.use_stereo_blend = use_virtual_stereo, use_stereo_blend
        self.encoder = create_encoder(enc_name, in_chans=3, pretrained=pretrained)
        self.num_ch_enc, self.enc_sc = self.encoder.feature_info.channels(), self.encoder.feature_info.reduction()
        self.decoders = nn.ModuleDict({'disp': DEC_REG[dec_name](
            num_ch_enc=self.num_ch_enc, enc_sc=self.enc_sc, upsample_mode='nearest', use_skip=True,
            out_sc=self.out_scales, out_ch=1, out_act='sigmoid')})
        if mask_name:   # same ModuleDict key as the reference: a reference checkpoint's `decoders.mask.*` entries load as they are
            self.decoders['mask'] = DEC_REG[dec_name](
                num_ch_enc=self.num_ch_enc, enc_sc=self.enc_sc, upsample_mode='nearest', use_skip=True,
                out_sc=self.out_scales, out_ch=int(num_ch_mask), out_act=MASKS[mask_name])

    def forward(self, x):
        feat = self.encoder(x)
        out = {'depth_feats': feat}
        for k, dec in self.decoders.items(): out[k] = dict(sorted(dec(feat).items()))
        return out

    def forward_blended(self, x):
        """`forward(x)` with every `disp*` pyramid blended with the prediction for the mirrored image: two passes, as the reference's `use_stereo_blend`
        network runs them (src/networks/depth.py:148-156), and ONE `flip_blend_pyramid` call per pyramid, which reads the second pass's disparities
        mirrored instead of flipping them back.  Differentiable; every other key is the first pass's."""
        from ..blend import flip_blend_pyramid
        out, mirrored = self.forward(x), self.forward(x.flip(dims=[-1]))
        for k in [k for k in out if k.startswith('disp')]: out[k] = flip_blend_pyramid(out[k], mirrored[k])
        return out
