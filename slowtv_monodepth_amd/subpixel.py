"""The SuperDepth decoder's sub-pixel convolution as a `torch.autograd.Function` (`smd_subpixel_*`: csrc/smd_subpixel.hip).
`functional` re-exports `subpixel_conv`."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, _workspace, call

__all__ = ['subpixel_conv']

_PRE = {None: 0, 'none': 0, 'elu': 1}                       # SMD_SP_PRE_NONE / SMD_SP_PRE_ELU
_ACT = {None: 0, 'none': 0, 'relu': 1, 'sigmoid': 2}        # SMD_SP_NONE / SMD_SP_RELU / SMD_SP_SIGMOID


def _shapes(x, weight, bias, r, pre_bias, skip, pad):
    """Shape refusals that need no device: x a non-empty (B,C,h,w), weight (C r^2,1,3,3), bias (C r^2), pre_bias (C), skip (B,Cs >= 1,r h,r w) and only with pad."""
    if x.ndim != 4 or x.numel() == 0: raise ValueError(f'x: expected a non-empty (B,C,h,w), got {tuple(x.shape)}')
    B, C, h, w = x.shape
    if tuple(weight.shape) != (C*r*r, 1, 3, 3): raise ValueError(f'weight: expected shape {(C*r*r, 1, 3, 3)}, got {tuple(weight.shape)}')
    if tuple(bias.shape) != (C*r*r,): raise ValueError(f'bias: expected shape {(C*r*r,)}, got {tuple(bias.shape)}')
    if isinstance(pre_bias, torch.Tensor) and tuple(pre_bias.shape) != (C,): raise ValueError(f'pre_bias: expected shape {(C,)}, got {tuple(pre_bias.shape)}')
    if skip is not None:
        if not pad: raise ValueError('skip is concatenated in front of the padding: it needs pad=True')
        if not isinstance(skip, torch.Tensor): raise TypeError(f'skip must be a Tensor or None, got {type(skip)}')
        if skip.ndim != 4 or skip.shape[1] < 1 or tuple(skip.shape) != (B, skip.shape[1], r*h, r*w):
            raise ValueError(f'skip: expected shape ({B}, Cs >= 1, {r*h}, {r*w}), got {tuple(skip.shape)}')


class _SubPixelConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pre_bias, weight, bias, skip, r, pre_act, act, pad):
        x = _check('x', x)
        B, C, h, w = x.shape
        Cs = skip.shape[1] if skip is not None else 0
        weight = _check('weight', weight, (C*r*r, 1, 3, 3)); bias = _check('bias', bias, (C*r*r,))
        if pre_bias is not None: pre_bias = _check('pre_bias', pre_bias, (C,))
        if skip is not None: skip = _check('skip', skip, (B, Cs, r*h, r*w))
        if _lib.lib.smd_subpixel_workspace_bytes(B, C, Cs, h, w, r, pad) == 0:
            raise ValueError(f'subpixel_conv does not serve the sizes B={B} C={C} Cs={Cs} h={h} w={w} r={r} pad={pad}')
        out = torch.empty((B, C + Cs, r*h + 2*pad, r*w + 2*pad), device=x.device, dtype=torch.float32)
        call('smd_subpixel_fwd', x.data_ptr(), _ptr(pre_bias), weight.data_ptr(), bias.data_ptr(), _ptr(skip), out.data_ptr(), B, C, Cs, h, w, r, pre_act, act, pad,
             _stream())
        ctx.save_for_backward(x, pre_bias, weight, out if act else None)      # (`out` carries the derivative of `act`; the next convolution holds it alive anyway)
        ctx.cfg = (Cs, r, pre_act, act, pad)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, pre_bias, weight, out = ctx.saved_tensors
        dev = _on(x)
        B, C, h, w = x.shape
        Cs, r, pre_act, act, pad = ctx.cfg
        need = ctx.needs_input_grad
        g_x = torch.empty_like(x) if need[0] else None
        g_pb = torch.empty_like(pre_bias) if (pre_bias is not None and need[1]) else None
        g_w = torch.empty_like(weight) if need[2] else None
        g_b = torch.empty((C*r*r,), device=dev, dtype=torch.float32) if need[3] else None
        g_skip = torch.empty((B, Cs, r*h, r*w), device=dev, dtype=torch.float32) if (Cs and need[4]) else None
        if g_x is None and g_pb is None and g_w is None and g_b is None and g_skip is None: return (None,)*9
        g_out = _check('grad(out)', g_out, (B, C + Cs, r*h + 2*pad, r*w + 2*pad))
        ws, nbytes = _workspace(dev, _lib.lib.smd_subpixel_workspace_bytes, B, C, Cs, h, w, r, pad)
        call('smd_subpixel_bwd', x.data_ptr(), _ptr(pre_bias), weight.data_ptr(), _ptr(out), g_out.data_ptr(), _ptr(g_x), _ptr(g_pb), _ptr(g_w), _ptr(g_b),
             _ptr(g_skip), ws.data_ptr(), nbytes, B, C, Cs, h, w, r, pre_act, act, pad, _stream())
        return g_x, g_pb, g_w, g_b, g_skip, None, None, None, None


def subpixel_conv(x, weight, bias, up_factor: int, *, pre_bias=None, pre_act: str | None = None, act: str | None = None, skip=None, pad: bool = False):
    """SuperDepth's `SubPixelConv` (src/networks/decoders/superdepth.py:13-26: a depth-wise 3x3 convolution to `up_factor**2` channels per input channel,
    then `PixelShuffle(up_factor)`) with the operators around it in one pass: `z = act(shuffle(conv(pre_act(x + pre_bias))))`, returned as it is or, with
    `pad`, as `reflect_pad1(cat(z, skip))` — the next 3x3 convolution's padded input.  x (B,C,h,w) a raw (bias-free) convolution output, weight
    (C r^2,1,3,3) and bias (C r^2) the reference Conv2d's, pre_bias (C) or None, skip (B,Cs,r h,r w) or None (only with `pad`), all fp32 on the GPU;
    up_factor 2 | 4 | 8, pre_act 'elu' | None, act 'relu' | 'sigmoid' | None -> (B,C,r h,r w) or (B,C+Cs,r h+2,r w+2)."""
    if up_factor not in (2, 4, 8) or isinstance(up_factor, bool): raise ValueError(f'up_factor must be 2, 4 or 8, got {up_factor!r}')
    if pre_act not in _PRE: raise ValueError(f"pre_act must be 'elu' or None, got {pre_act!r}")
    if act not in _ACT: raise ValueError(f"act must be 'relu', 'sigmoid' or None, got {act!r}")
    for name, t in (('x', x), ('weight', weight), ('bias', bias)):
        if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    if pre_bias is not None and not isinstance(pre_bias, torch.Tensor): raise TypeError(f'pre_bias must be a Tensor or None, got {type(pre_bias)}')
    _shapes(x, weight, bias, up_factor, pre_bias, skip, pad)
    return _SubPixelConv.apply(x, pre_bias, weight, bias, skip, int(up_factor), _PRE[pre_act], _ACT[act], 1 if pad else 0)
