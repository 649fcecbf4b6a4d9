"""`AutoencoderNet` — registry key `autoencoder` (reference: `src/networks/autoencoder.py:12-65`): FeatDepth's image autoencoder, whose encoder features
the feature-metric losses (`feat_recon`, `feat_peaky`, `feat_smooth`) read and whose reconstructions `autoenc_recon` trains."""
from __future__ import annotations

import torch.nn as nn

from ..registry import DEC_REG, register
from .encoders import create_encoder

__all__ = ['AutoencoderNet']


@register('autoencoder')
class AutoencoderNet(nn.Module):
    """Image -> encoder features + multi-scale sigmoid RGB reconstructions {s: (b,3,h/2^s,w/2^s)}.  The depth network's layout with one decoder, three
    output channels and NO skip connections (it is an autoencoder).  Same constructor kwargs and sub-module names (`encoder`, `decoder`) as the reference, so
    its `encoder.*` / `decoder.*` state-dict entries load and are emitted as they are (`networks/checkpoint.py` translates the names).

    The decoder is the registered one: its glued GPU path takes `use_skip=False` (the stage glue without a skip operand) and its three-channel heads run
    on `smd_conv3x3_headn_*`."""
    def __init__(self, enc_name: str = 'resnet18', pretrained: bool = True, dec_name: str = 'monodepth', out_scales=(0, 1, 2, 3)):
        super().__init__()
        if dec_name not in DEC_REG: raise KeyError(f'Invalid decoder key. ({dec_name} vs. {list(DEC_REG)}')
        self.enc_name, self.pretrained, self.dec_name = enc_name, pretrained, dec_name
        self.out_scales = [out_scales] if isinstance(out_scales, int) else list(out_scales)
        self.encoder = create_encoder(enc_name, in_chans=3, pretrained=pretrained)
        self.num_ch_enc, self.enc_sc = self.encoder.feature_info.channels(), self.encoder.feature_info.reduction()
        self.decoder = DEC_REG[dec_name](num_ch_enc=self.num_ch_enc, enc_sc=self.enc_sc, upsample_mode='nearest', use_skip=False,
                                         out_sc=self.out_scales, out_ch=3, out_act='sigmoid')

    def forward(self, x):
        feat = self.encoder(x)
        return {'autoenc_feats': feat, 'autoenc_imgs': dict(sorted(self.decoder(feat).items()))}
