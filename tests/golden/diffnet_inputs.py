"""Seeded inputs of the DiffNet fixtures (`op_diffnet_fuse.npz`, `net_decoder_diffnet_64x96.npz`), shared by tests/golden/make_golden_diffnet.py and the tests."""
from __future__ import annotations

import re

import torch

from exact_inputs import DECODER_KW, decoder_state

__all__ = ['FUSE_CASES', 'FUSE_SATURATED', 'DIFFNET_KW', 'DIFFNET_BATCH', 'DIFFNET_ORDER', 'fuse_case', 'diffnet_state']

# (B, Ca, Cs, h, w, weight scale): the bottleneck is the reference's (Ca + Cs) // 16; the last case's Linear weights are x 40, which drives gates to 0 and 1
FUSE_CASES = [(2, 16, 16, 3, 5, 1.0), (1, 40, 24, 4, 6, 1.0), (2, 32, 64, 2, 3, 1.0), (1, 24, 8, 5, 4, 40.0)]
FUSE_SATURATED = 3
DIFFNET_KW = dict(DECODER_KW)
DIFFNET_BATCH = 1
DIFFNET_ORDER = [f'upconv_{i}' for i in range(4, -1, -1)] + [f'outconv_{k}' for k in range(4)]    # the reference's `decoder` ModuleList (diffnet.py:128)


def fuse_case(k: int):
    """-> a (B,Ca,h,w), bias (Ca), skip (B,Cs,2h,2w), w1 (R,C), w2 (C,R), gout (B,C,2h+2,2w+2).  Every channel has a mean of its own, so the gates differ."""
    B, Ca, Cs, h, w, scale = FUSE_CASES[k]
    C = Ca + Cs
    R = C//16
    g = torch.Generator().manual_seed(500 + k)
    a = torch.randn(B, Ca, h, w, generator=g) + torch.randn(1, Ca, 1, 1, generator=g)
    bias = 0.5*torch.randn(Ca, generator=g)
    skip = torch.randn(B, Cs, 2*h, 2*w, generator=g) + torch.randn(1, Cs, 1, 1, generator=g)
    w1 = torch.randn(R, C, generator=g)*(scale/float(C)**0.5)
    w2 = torch.randn(C, R, generator=g)*(scale/float(R)**0.5)
    return a, bias, skip, w1, w2, torch.randn(B, C, 2*h + 2, 2*w + 2, generator=g)


def diffnet_state(shapes: dict, seed: int = 77) -> dict:
    """`exact_inputs.decoder_state` for the `convs.*` entries; every `decoder.{n}.*` entry is the tensor of the module it shares with `convs`."""
    state = decoder_state({k: s for k, s in shapes.items() if '.convs.' in k or k.startswith('convs.')}, seed)
    for k in shapes:
        m = re.fullmatch(r'(.*?)decoder\.(\d+)\.(.*)', k)
        if m and k not in state: state[k] = state[f'{m.group(1)}convs.{DIFFNET_ORDER[int(m.group(2))]}.{m.group(3)}']
    return state
