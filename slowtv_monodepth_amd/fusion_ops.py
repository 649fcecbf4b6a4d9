"""The DiffNet decoder's glue as `torch.autograd.Function`s (`smd_up_cat_gate_pad_*`, `smd_relu_pad_*`: csrc/smd_decoder.hip).
`functional` re-exports `up_cat_gate_pad` and `relu_pad`."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, _workspace, call

__all__ = ['up_cat_gate_pad', 'relu_pad']

_ACT = {None: 0, 'none': 0, 'relu': 1}       # SMD_UCG_NONE / SMD_UCG_RELU


def _shapes(a, skip, w1, w2, bias):
    """Shape refusals that need no device: a a non-empty (B,Ca,h,w), skip (B,Cs,2h,2w) with Cs >= 1, w1 (R,Ca+Cs) and w2 (Ca+Cs,R) with R >= 1, bias (Ca)."""
    if not all(isinstance(t, torch.Tensor) for t in (a, skip, w1, w2)): return
    if a.ndim != 4 or a.numel() == 0: raise ValueError(f'a: expected a non-empty (B,Ca,h,w), got {tuple(a.shape)}')
    B, Ca, h, w = a.shape
    if skip.ndim != 4 or skip.shape[1] < 1 or tuple(skip.shape) != (B, skip.shape[1], 2*h, 2*w):
        raise ValueError(f'skip: expected shape ({B}, Cs >= 1, {2*h}, {2*w}), got {tuple(skip.shape)}')
    C = Ca + skip.shape[1]
    if w1.ndim != 2 or w1.shape[0] < 1 or w1.shape[1] != C: raise ValueError(f'w1: expected shape (R >= 1, {C}), got {tuple(w1.shape)}')
    if tuple(w2.shape) != (C, w1.shape[0]): raise ValueError(f'w2: expected shape {(C, w1.shape[0])}, got {tuple(w2.shape)}')
    if isinstance(bias, torch.Tensor) and tuple(bias.shape) != (Ca,): raise ValueError(f'bias: expected shape {(Ca,)}, got {tuple(bias.shape)}')


class _UpCatGatePad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bias, skip, w1, w2, act):
        a = _check('a', a)
        B, Ca, h, w = a.shape
        Cs, R = skip.shape[1], w1.shape[0]
        C = Ca + Cs
        skip = _check('skip', skip, (B, Cs, 2*h, 2*w))
        w1 = _check('w1', w1, (R, C)); w2 = _check('w2', w2, (C, R))
        if bias is not None: bias = _check('bias', bias, (Ca,))
        nbytes = _lib.lib.smd_up_cat_gate_pad_workspace_bytes(B, Ca, Cs, h, w, R)
        if nbytes == 0: raise ValueError(f'up_cat_gate_pad does not serve the sizes B={B} Ca={Ca} Cs={Cs} h={h} w={w} R={R}')
        dev = a.device
        out = torch.empty((B, C, 2*h + 2, 2*w + 2), device=dev, dtype=torch.float32)
        gate, mean, hid = (torch.empty((B, n), device=dev, dtype=torch.float32) for n in (C, C, R))
        ws, nbytes = _workspace(dev, nbytes)
        call('smd_up_cat_gate_pad_fwd', a.data_ptr(), _ptr(bias), skip.data_ptr(), w1.data_ptr(), w2.data_ptr(), out.data_ptr(), gate.data_ptr(), mean.data_ptr(),
             hid.data_ptr(), ws.data_ptr(), nbytes, B, Ca, Cs, h, w, R, act, _stream())
        ctx.save_for_backward(a, bias, skip, w1, w2, gate, mean, hid); ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g_out):
        a, bias, skip, w1, w2, gate, mean, hid = ctx.saved_tensors
        dev = _on(a)
        B, Ca, h, w = a.shape
        Cs, R = skip.shape[1], w1.shape[0]
        need = ctx.needs_input_grad
        g_a = torch.empty_like(a) if need[0] else None
        g_b = torch.empty_like(bias) if (bias is not None and need[1]) else None
        g_skip = torch.empty_like(skip) if need[2] else None
        g_w1, g_w2 = (torch.empty_like(w1), torch.empty_like(w2)) if (need[3] or need[4]) else (None, None)
        if g_a is None and g_b is None and g_skip is None and g_w1 is None: return None, None, None, None, None, None
        g_out = _check('grad(out)', g_out, (B, Ca + Cs, 2*h + 2, 2*w + 2))
        ws, nbytes = _workspace(dev, _lib.lib.smd_up_cat_gate_pad_workspace_bytes, B, Ca, Cs, h, w, R)
        call('smd_up_cat_gate_pad_bwd', a.data_ptr(), _ptr(bias), skip.data_ptr(), w1.data_ptr(), w2.data_ptr(), gate.data_ptr(), mean.data_ptr(), hid.data_ptr(),
             g_out.data_ptr(), _ptr(g_a), _ptr(g_skip), _ptr(g_b), _ptr(g_w1), _ptr(g_w2), ws.data_ptr(), nbytes, B, Ca, Cs, h, w, R, ctx.act, _stream())
        return g_a, g_b, g_skip, (g_w1 if need[3] else None), (g_w2 if need[4] else None), None


def up_cat_gate_pad(a, skip, w1, w2, bias=None, act: str | None = None):
    """The attention stage of the DiffNet decoder in front of its convolution (src/networks/decoders/diffnet.py:44-47, 70-74), written as that
    convolution's reflection-padded input: with `src = cat(nearest_x2(act(a + bias)), skip)` and `gate = sigmoid(relu(mean_hw(src) @ w1.T) @ w2.T)`,
    `reflect_pad1(src * gate[..., None, None])`.  a (B,Ca,h,w), skip (B,Cs,2h,2w), w1 (R,Ca+Cs), w2 (Ca+Cs,R) — the two bias-free Linear layers' weights
    — bias (Ca) or None, all fp32; act 'relu' | None -> (B,Ca+Cs,2h+2,2w+2).  `src` is never written."""
    if act not in _ACT: raise ValueError(f"act must be 'relu' or None, got {act!r}")
    for name, t in (('a', a), ('skip', skip), ('w1', w1), ('w2', w2)):
        if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    _shapes(a, skip, w1, w2, bias)
    return _UpCatGatePad.apply(a, bias, skip, w1, w2, _ACT[act])


class _ReluPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        x = _check('x', x)
        B, C, h, w = x.shape
        if bias is not None: bias = _check('bias', bias, (C,))
        out = torch.empty((B, C, h + 2, w + 2), device=x.device, dtype=torch.float32)
        call('smd_relu_pad_fwd', x.data_ptr(), _ptr(bias), out.data_ptr(), B, C, h, w, _stream())
        ctx.save_for_backward(x, bias)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, bias = ctx.saved_tensors
        _on(x)
        B, C, h, w = x.shape
        g_out = _check('grad(out)', g_out, (B, C, h + 2, w + 2))
        g_x = torch.empty_like(x)
        g_b = torch.empty_like(bias) if (bias is not None and ctx.needs_input_grad[1]) else None
        ws, nbytes = _workspace(x.device, _lib.lib.smd_decoder_glue_workspace_bytes, B, C, h, w) if g_b is not None else (None, 0)
        call('smd_relu_pad_bwd', x.data_ptr(), _ptr(bias), g_out.data_ptr(), g_x.data_ptr(), _ptr(g_b), _ptr(ws), nbytes, B, C, h, w, _stream())
        return g_x, g_b


def relu_pad(x, bias=None):
    """reflect_pad1(relu(x + bias)): the padded activation of a DiffNet attention stage (diffnet.py:64-68), read by its output head and by a following
    up-sample block.  x (B,C,h,w) the raw (bias-free) convolution output, bias (C) or None, fp32 -> (B,C,h+2,w+2)."""
    if isinstance(x, torch.Tensor) and (x.ndim != 4 or x.numel() == 0): raise ValueError(f'expected a non-empty (B,C,h,w), got {tuple(x.shape)}')
    return _ReluPad.apply(x, bias)
