"""Seeded inputs of the SuperDepth fixtures (`op_subpixel.npz`, `net_decoder_superdepth_64x96.npz`), shared by tests/golden/make_golden_superdepth.py and the tests."""
from __future__ import annotations

import torch

from exact_inputs import DECODER_KW, decoder_state

__all__ = ['SUBPIXEL_CASES', 'SUBPIXEL_SATURATED', 'SUBPIXEL_NAMES', 'SUPERDEPTH_KW', 'SUPERDEPTH_BATCH', 'subpixel_case', 'subpixel_aten', 'superdepth_out_grads',
           'superdepth_state']

# (B, C, Cs, h, w, r, pre_act, act, pad): odd sizes with a skip and the pad corners; a single pixel (every tap but the centre is zero padding, the reflection is
# of a 2 x 2 plane); r = 4; r = 8 (the scale-3 head); no pre-bias, no activations; an output row of 134 columns (crosses a wave); more than one block per reduced
# sum; and the first shape saturated: x + pre_bias down to -50, v spanning +-40 under the sigmoid
SUBPIXEL_CASES = [(2, 3, 2, 3, 5, 2, 'elu', 'relu', True), (1, 1, 0, 1, 1, 2, 'elu', 'relu', True), (1, 2, 0, 2, 3, 4, 'elu', 'sigmoid', False),
                  (2, 1, 0, 3, 2, 8, 'elu', 'sigmoid', False), (1, 2, 0, 2, 3, 4, 'none', 'none', False), (1, 16, 8, 4, 67, 2, 'elu', 'relu', True),
                  (2, 16, 0, 24, 40, 2, 'elu', 'relu', True), (2, 3, 2, 3, 5, 2, 'elu', 'sigmoid', True)]
SUBPIXEL_SATURATED = 7
SUBPIXEL_NAMES = ('out', 'grad_x', 'grad_pre_bias', 'grad_weight', 'grad_bias', 'grad_skip')
SUPERDEPTH_KW = dict(DECODER_KW)
SUPERDEPTH_BATCH = 1


def subpixel_case(k: int):
    """-> dict(x (B,C,h,w), pre_bias (C) | None, weight (C r^2,1,3,3), bias (C r^2), skip (B,Cs,rh,rw) | None, gout (the output's shape)).  Case 4 ('none' in
    front) has no pre-bias.  Every row of the weight is drawn by itself, so a wrong shuffle order shows."""
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]
    g = torch.Generator().manual_seed(900 + k)
    sat = k == SUBPIXEL_SATURATED
    x = torch.randn(B, C, h, w, generator=g)
    pre_bias = 0.5*torch.randn(C, generator=g) if pre == 'elu' else None
    weight = torch.randn(C*r*r, 1, 3, 3, generator=g)/3.0
    bias = 0.5*torch.randn(C*r*r, generator=g)
    if sat:      # x + pre_bias from about -50 to +13; v = bias + sum w u spans more than +-40
        x = 16.0*x - 18.0
        weight, bias = 4.0*weight, 8.0*bias
    skip = torch.randn(B, Cs, r*h, r*w, generator=g) if Cs else None
    gout = torch.randn(B, C + Cs, r*h + 2*pad, r*w + 2*pad, generator=g)
    return dict(x=x, pre_bias=pre_bias, weight=weight, bias=bias, skip=skip, gout=gout)


def subpixel_aten(x, pre_bias, weight, bias, skip, r, pre_act, act, pad):
    """The ATen sequence `subpixel_conv` replaces, operator by operator (the tests run it in fp64 as the truth and in fp32 as the yardstick)."""
    import torch.nn.functional as TF
    u = x if pre_bias is None else x + pre_bias.view(1, -1, 1, 1)
    if pre_act == 'elu': u = TF.elu(u)
    z = TF.pixel_shuffle(TF.conv2d(u, weight, bias, padding=1, groups=x.shape[1]), r)
    if act == 'relu': z = TF.relu(z)
    elif act == 'sigmoid': z = z.sigmoid()
    if skip is not None: z = torch.cat((z, skip), 1)
    return TF.pad(z, (1, 1, 1, 1), mode='reflect') if pad else z


def superdepth_out_grads(seed: int = 109, b: int = 1, h: int = 64, w: int = 96) -> dict:
    """Every head of this decoder is full-resolution: one (b,1,h,w) gradient per scale."""
    g = torch.Generator().manual_seed(seed)
    return {i: torch.randn(b, 1, h, w, generator=g) for i in SUPERDEPTH_KW['out_sc']}


def superdepth_state(shapes: dict, seed: int = 77) -> dict:
    """`exact_inputs.decoder_state`, then every sub-pixel weight and bias (the depth-wise `(C r^2, 1, 3, 3)` convolutions and their `(C r^2)` biases — the
    entries `decoder.N.1.conv.*`) drawn again at unit-order scale: the four rows of a group differ and the biases are not zero."""
    state = decoder_state(shapes, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    for k in sorted(shapes):
        if '.1.conv.' not in k: continue
        state[k] = torch.randn(tuple(shapes[k]), generator=g)/3.0 if k.endswith('weight') else 0.2*torch.randn(tuple(shapes[k]), generator=g)
    return state
