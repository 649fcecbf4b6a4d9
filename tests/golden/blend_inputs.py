"""Seeded inputs of the flip-and-blend fixture (`blend_stereo.npz`), shared by tests/golden/make_golden_blend.py and the tests."""
from __future__ import annotations

import torch

__all__ = ['BLEND_CASES', 'BLEND_PYRAMID', 'BLEND_SCALED', 'BLEND_RANGE', 'blend_case', 'blend_expected']

WIDTHS, HEIGHTS, CHANNELS, BATCH = (1, 2, 3, 20, 21, 41, 67), (1, 3), (1, 2), 2
PYRAMID = ((8, 24), (4, 12), (2, 6), (1, 3))
# (b, c, h, w).  w = 1: the blend is the mean; 2, 3: the ramp is all zero / has one interior column and the middle column mirrors onto itself; 21: x_1 = 0.05
# exactly, the clamp's edge; 20, 41: the 5 % edge falls between columns; 67: sixteen whole four-column groups and a tail of 3; then the four levels of a pyramid
BLEND_CASES = [(BATCH, c, h, w) for w in WIDTHS for h in HEIGHTS for c in CHANNELS] + [(BATCH, 1, h, w) for h, w in PYRAMID]
BLEND_PYRAMID = list(range(len(BLEND_CASES) - len(PYRAMID), len(BLEND_CASES)))
# the cases also recorded behind to_scaled(min, max): h = 3 and c = 2 at w = 2, 21 and 67, and the pyramid
BLEND_SCALED = [k for k, (b, c, h, w) in enumerate(BLEND_CASES[:-len(PYRAMID)]) if (c == 2 and h == 3 and w in (2, 21, 67))] + BLEND_PYRAMID
BLEND_RANGE = (0.1, 100)


def blend_case(k: int):
    """-> dict(l, r (the right disparity, ALREADY flipped back), g (the incoming gradient)), each (b,c,h,w): sigmoid disparities in (0.01, 0.99), a normal gradient."""
    gen = torch.Generator().manual_seed(20260 + k)
    shape = BLEND_CASES[k]
    return dict(l=0.01 + 0.98*torch.rand(*shape, generator=gen), r=0.01 + 0.98*torch.rand(*shape, generator=gen), g=torch.randn(*shape, generator=gen))


def blend_expected(g: dict, k: int, scaled: bool = False):
    """-> (out, grad_l, grad_r) of case k from the loaded fixture, which stores each quantity as ONE flat array over the cases in order (`out`, `grad_l`, `grad_r`
    over BLEND_CASES; `outs`, `grads_l`, `grads_r` over BLEND_SCALED)."""
    cases = BLEND_SCALED if scaled else list(range(len(BLEND_CASES)))
    numel = lambda j: BLEND_CASES[j][0]*BLEND_CASES[j][1]*BLEND_CASES[j][2]*BLEND_CASES[j][3]
    first = sum(numel(j) for j in cases[:cases.index(k)])
    tag = 's' if scaled else ''
    return tuple(g[f'{n}{tag}' if n == 'out' else n.replace('grad', f'grad{tag}')][first:first + numel(k)].reshape(BLEND_CASES[k]) for n in ('out', 'grad_l', 'grad_r'))
