"""Monodepth's flip-and-blend post-process as a `torch.autograd.Function` over `smd_flip_blend_*` (csrc/smd_blend.hip): the prediction for an image blended
with the prediction for its mirror image, for one tensor or a whole pyramid in one launch, optionally with `to_scaled`'s disparity scaling folded in.
`functional` re-exports `flip_blend` and `flip_blend_pyramid`; `plain_flip_blend` is the same computation as the reference's ATen sequence
(`flip` + `blend_stereo`, src/tools/geometry.py:94-129, + `to_scaled`, :63-76) and is what CPU tensors, other dtypes than float32 and one-column maps run."""
from __future__ import annotations

import torch

from ._device import _check, _on, _ptrs, _stream, call
from ._lib import int_array, ptr_array
from .recon_ops import _depth_range

__all__ = ['flip_blend', 'flip_blend_pyramid', 'plain_flip_blend', 'blend_ramp']

MIRROR, SCALE = 0x1, 0x2      # SMD_BLEND_MIRROR / SMD_BLEND_SCALE
_ramps: dict = {}


def blend_ramp(device, w: int) -> torch.Tensor:
    """m_l (w,) float32 on `device`: `(20*(linspace(0, 1, w) - 0.05)).clamp(0, 1)` (src/tools/geometry.py:115-121), cached per (device, w).  torch's own
    `linspace` on the host, copied once: the kernel never re-derives it, and a GPU sees the bits the CPU path blends with."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None or device.type != 'cuda' else torch.cuda.current_device(), int(w))
    ramp = _ramps.get(key)
    if ramp is None:
        ramp = _ramps[key] = (20*(torch.linspace(0, 1, int(w)) - 0.05)).clamp(min=0, max=1).to(device)
    return ramp


def _scaling(min_depth, max_depth):
    """-> None, or (scale, offset) = (1/min - 1/max, 1/max) as `to_scaled` forms them, in Python floats; the range is validated by `_depth_range`."""
    mn, mx = _depth_range(min_depth, max_depth)
    if not mn:
        if mx: raise ValueError(f'max_depth ({max_depth}) needs a min_depth: the scaling is (1/min - 1/max)*disp + 1/max')
        return None
    i_max, i_min = 1/mn, (1/mx) if mx else 0
    return i_max - i_min, i_min


def plain_flip_blend(l: torch.Tensor, r_raw: torch.Tensor, *, min_depth=None, max_depth=None, mirror: bool = True) -> torch.Tensor:
    """The ATen sequence.  l, r_raw (..., h, w) of one shape; `mirror`: r_raw is the prediction for the mirrored image and is flipped back first."""
    if l.shape != r_raw.shape: raise ValueError(f'Non-matching shapes. ({l.shape} vs. {r_raw.shape})')
    k = _scaling(min_depth, max_depth)
    r = r_raw.flip(dims=[-1]) if mirror else r_raw
    mask_l = blend_ramp(l.device, l.shape[-1])
    mask_r = mask_l.flip(dims=[-1])
    mask_mu = 1.0 - mask_l - mask_r
    mu = (l + r)/2
    out = mask_r*l + mask_l*r + mask_mu*mu
    if k is not None: out = k[0]*out + k[1]
    return out


class _FlipBlend(torch.autograd.Function):
    """(flags, scale, offset, S, l_0 .. l_{S-1}, r_0 .. r_{S-1}) -> (out_0 .. out_{S-1}); level s is (planes, h_s, w_s) in any leading shape."""
    @staticmethod
    def forward(ctx, flags, scale, offset, S, *ts):
        ls = [_check(f'l[{s}]', t, align=False) for s, t in enumerate(ts[:S])]
        rs = [_check(f'r[{s}]', t, tuple(ls[s].shape), align=False) for s, t in enumerate(ts[S:])]
        hs, ws = [t.shape[-2] for t in ls], [t.shape[-1] for t in ls]
        planes = ls[0].numel()//(hs[0]*ws[0])
        ramps = [blend_ramp(ls[0].device, w) for w in ws]
        outs = [torch.empty(tuple(t.shape), device=t.device, dtype=torch.float32) for t in ls]
        call('smd_flip_blend_fwd', _ptrs(ls), _ptrs(rs), _ptrs(ramps), _ptrs(outs), int_array(hs), int_array(ws), S, planes, flags, scale, offset, _stream())
        ctx.cfg = (flags, scale, S, hs, ws, planes, ramps, [tuple(t.shape) for t in ls])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        flags, scale, S, hs, ws, planes, ramps, shapes = ctx.cfg
        need = ctx.needs_input_grad[4:]
        if not any(need): return (None,)*(4 + 2*S)
        dev = _on(ramps[0])
        gs = [_check(f'grad(out[{s}])', g, shapes[s], align=False) for s, g in enumerate(gs)]
        g_l = [torch.empty(shapes[s], device=dev, dtype=torch.float32) if need[s] else None for s in range(S)]
        g_r = [torch.empty(shapes[s], device=dev, dtype=torch.float32) if need[S + s] else None for s in range(S)]
        opt = lambda ts: _ptrs_opt(ts) if any(t is not None for t in ts) else None
        call('smd_flip_blend_bwd', _ptrs(gs), _ptrs(ramps), opt(g_l), opt(g_r), int_array(hs), int_array(ws), S, planes, flags, scale, _stream())
        return (None, None, None, None, *g_l, *g_r)


def _ptrs_opt(ts):
    """The pointer array of per-level outputs of which some are not asked for (NULL entries)."""
    return ptr_array([t.data_ptr() if t is not None else None for t in ts])


def _served(l, r) -> bool:
    """The kernel's operands: float32 on one GPU, more than one column."""
    return l.is_cuda and r.is_cuda and l.device == r.device and l.dtype == torch.float32 and r.dtype == torch.float32 and l.shape[-1] > 1 and l.numel() > 0


def _operands(name, l, r):
    for n, t in ((name[0], l), (name[1], r)):
        if not isinstance(t, torch.Tensor): raise TypeError(f'{n} must be a Tensor, got {type(t)}')
    if l.ndim != 4: raise ValueError(f'{name[0]}: expected (b,c,h,w), got {tuple(l.shape)}')
    if l.shape != r.shape: raise ValueError(f'Non-matching shapes. ({l.shape} vs. {r.shape})')


def flip_blend(l: torch.Tensor, r_raw: torch.Tensor, *, min_depth=None, max_depth=None, mirror: bool = True) -> torch.Tensor:
    """Blend the prediction `l` (b,c,h,w) for an image with `r_raw`, the prediction for the mirrored image as the network returned it: `blend_stereo(l,
    r_raw.flip(-1))` (src/tools/geometry.py:94-129) without the flipped copy, per plane, and with a depth range `to_scaled(.., min_depth, max_depth)[0]`
    (:63-76) of it in the same pass.  `mirror=False`: `r_raw` is already flipped back.  Differentiable in both operands.  float32 on the GPU runs
    `smd_flip_blend_*`; CPU tensors, other dtypes and w == 1 run `plain_flip_blend`."""
    k = _scaling(min_depth, max_depth)
    _operands(('l', 'r_raw'), l, r_raw)
    if not _served(l, r_raw): return plain_flip_blend(l, r_raw, min_depth=min_depth, max_depth=max_depth, mirror=mirror)
    flags = (MIRROR if mirror else 0) | (SCALE if k is not None else 0)
    return _FlipBlend.apply(flags, *(k or (1.0, 0.0)), 1, l, r_raw)[0]


def flip_blend_pyramid(ls: dict, rs_raw: dict, *, min_depth=None, max_depth=None, mirror: bool = True) -> dict:
    """`flip_blend` of every level of a pyramid {key: (b,c,h_s,w_s)} in ONE launch (at most 8 levels per launch) -> {key: blended}, in `ls`'s order."""
    k = _scaling(min_depth, max_depth)
    if list(ls) != list(rs_raw): raise ValueError(f'Non-matching pyramid keys. ({list(ls)} vs. {list(rs_raw)})')
    for key in ls: _operands((f'ls[{key!r}]', f'rs_raw[{key!r}]'), ls[key], rs_raw[key])
    out = {key: None for key in ls}
    lead = {(tuple(ls[key].shape[:2]), ls[key].device) for key in ls}
    if len(lead) > 1: raise ValueError(f'the levels of a pyramid share (b,c) and the device, got {sorted(map(str, lead))}')
    fused = [key for key in ls if _served(ls[key], rs_raw[key])]
    flags = (MIRROR if mirror else 0) | (SCALE if k is not None else 0)
    for i in range(0, len(fused), 8):
        keys = fused[i:i + 8]
        res = _FlipBlend.apply(flags, *(k or (1.0, 0.0)), len(keys), *[ls[key] for key in keys], *[rs_raw[key] for key in keys])
        out.update(zip(keys, res))
    for key in ls:
        if out[key] is None: out[key] = plain_flip_blend(ls[key], rs_raw[key], min_depth=min_depth, max_depth=max_depth, mirror=mirror)
    return out
