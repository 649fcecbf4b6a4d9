"""Seeded inputs of the validation-metric tests (host and GPU files share them; each file restates the metrics itself)."""
import math

import torch


def _field(gen, b, h, w, lo=2.0, hi=60.0):
    """Smooth positive depth-like field in [lo, hi]."""
    ys, xs = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing='ij')
    ph = torch.rand(b, 4, 1, 1, generator=gen)*2*math.pi
    u = 0.5 + 0.25*torch.sin(5*xs + ph[:, 0])*torch.cos(3*ys + ph[:, 1]) + 0.25*torch.sin(7*ys + 2*xs + ph[:, 2])*torch.cos(ph[:, 3])
    return (lo*(hi/lo)**u.clamp(0, 1))[:, None]


def _pair(seed, b, hw, HW, density=0.5, scale=0.37, spread=0.25):
    """pred (b,1,h,w), target (b,1,H,W): the target is the field at the target's size times log-normal noise (so that the spread of
    log p - log t is `spread` >= 0.1: the subtraction under LogSI's root is nowhere near cancelling), kept at `density` of the pixels;
    the prediction is the field at its own size times `scale` (what the median alignment has to undo)."""
    gen = torch.Generator().manual_seed(seed)
    (h, w), (H, W) = hw, HW
    big = _field(gen, b, 4*max(h, H), 4*max(w, W))
    pred = torch.nn.functional.interpolate(big, size=(h, w), mode='area')*scale
    target = torch.nn.functional.interpolate(big, size=(H, W), mode='area')*torch.exp(spread*torch.randn(b, 1, H, W, generator=gen))
    keep = torch.rand(b, 1, H, W, generator=gen) < density
    return pred.contiguous(), torch.where(keep, target, torch.zeros_like(target)).contiguous()


def make_case(name):
    """-> (pred, target, min_depth, max_depth)."""
    if name == 'equal':          # b = 3, 16x24: sample 0 odd n, sample 1 even n, sample 2 no valid pixel
        pred, target = _pair(1, 3, (16, 24), (16, 24))
        for i, parity in ((0, 1), (1, 0)):
            if int((target[i] > 0).sum()) % 2 != parity:
                idx = torch.nonzero(target[i].flatten() > 0)[0]
                target[i].view(-1)[idx] = 0.
        target[2] = 0.
        return pred, target, None, None
    if name == 'tiny':           # n = 1 and n = 2 in a 5x7 map
        pred, t = _pair(2, 2, (5, 7), (5, 7), density=1.0)
        target = torch.zeros_like(t)
        target[0, 0, 2, 3] = t[0, 0, 2, 3]
        target[1, 0, 1, 1], target[1, 0, 4, 5] = t[1, 0, 1, 1], t[1, 0, 4, 5]
        return pred, target, None, None
    if name == 'ties':           # target quantised to 4 values; more than half of the prediction clamps at hi
        pred, target = _pair(3, 2, (12, 20), (12, 20))
        levels = torch.tensor([3., 7., 19., 42.])
        q = levels[torch.bucketize(target, torch.tensor([5., 12., 30.]))]
        target = torch.where(target > 0, q, torch.zeros_like(target))
        pred = pred*(2.2*100/pred.flatten(1).median(dim=1).values)[:, None, None, None]
        return pred.contiguous(), target.contiguous(), None, None
    if name == 'up': return (*_pair(4, 2, (6, 10), (13, 37)), None, None)             # 481 pixels: not a multiple of 64
    if name == 'down': return (*_pair(5, 2, (24, 40), (9, 15)), None, None)
    if name == 'multi': return (*_pair(26, 2, (48, 160), (96, 320)), None, None)       # 30720 pixels: more than one block per sample
    if name == 'range': return (*_pair(7, 2, (10, 18), (21, 33)), 1e-3, 80)           # other range arguments (more of the far field falls outside)
    if name == 'nan_neg':        # NaN and negative entries in the target are invalid
        pred, target = _pair(8, 2, (9, 14), (18, 28))
        target[0, 0, 3, ::3] = float('nan')
        target[1, 0, ::4, 5] = -target[1, 0, ::4, 5].abs() - 1.
        target[1, 0, 7, 7] = float('nan')
        return pred, target, None, None
    raise KeyError(name)


CASES = ['equal', 'tiny', 'ties', 'up', 'down', 'multi', 'range', 'nan_neg']
