"""Seeded inputs of the DDVNet fixtures (`op_ddv_head.npz`, `net_decoder_ddvnet_64x96.npz`), shared by tests/golden/make_golden_ddvnet.py and the tests."""
from __future__ import annotations

import torch

from exact_inputs import DECODER_KW, decoder_state

__all__ = ['DDV_CASES', 'DDV_OVERFLOW', 'DDVNET_KW', 'DDVNET_BATCH', 'NUM_BINS', 'ddv_case', 'ddvnet_state', 'bins']

NUM_BINS = 128
# (B, C, h, w, out_ch, weight scale): C = 16 and 32, out_ch = 1 and 2; the last case's logits span more than 88, where an unshifted exp overflows fp32
DDV_CASES = [(2, 16, 5, 7, 1, 1.0), (1, 32, 4, 6, 1, 1.0), (1, 16, 6, 5, 2, 4.0), (2, 32, 3, 4, 2, 60.0)]
DDV_OVERFLOW = 3
DDVNET_KW = dict(DECODER_KW)
DDVNET_BATCH = 1


def bins(dtype=torch.float32):
    return (torch.arange(NUM_BINS)/NUM_BINS).view(1, NUM_BINS, 1, 1).to(dtype)


def ddv_case(k: int):
    """-> x (B,C,h,w) (unpadded: the reference's conv3x3 pads it), weight (128 out_ch,C,3,3), bias (128 out_ch), gout (B,out_ch,h,w)."""
    B, C, h, w, G, scale = DDV_CASES[k]
    g = torch.Generator().manual_seed(300 + k)
    x = torch.randn(B, C, h, w, generator=g)
    weight = torch.randn(NUM_BINS*G, C, 3, 3, generator=g)*(scale/float(9*C)**0.5)
    bias = 0.1*scale*torch.randn(NUM_BINS*G, generator=g)
    return x, weight, bias, torch.randn(B, G, h, w, generator=g)


def ddvnet_state(shapes: dict, seed: int = 77) -> dict:
    """`exact_inputs.decoder_state` for every entry but `bins`, which keeps the reference's values."""
    state = decoder_state({k: s for k, s in shapes.items() if not k.endswith('bins')}, seed)
    for k in shapes:
        if k.endswith('bins'): state[k] = bins()
    return state
