"""The attention blocks of the CADepth decoder as `torch.autograd.Function`s (`smd_channel_attention_*`, `smd_se_gate_*`: csrc/smd_attention.hip).
`functional` re-exports `channel_attention` and `se_gate`."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, _workspace, call

__all__ = ['channel_attention', 'se_gate']


def _shapes(x, **operands):
    """Shape refusals that need no device: x a non-empty (B,C,h,w), every other tensor operand of the shape given for it (a function of C)."""
    if not isinstance(x, torch.Tensor): return
    if x.ndim != 4 or x.numel() == 0: raise ValueError(f'expected a non-empty (B,C,h,w), got {tuple(x.shape)}')
    for name, (t, shape) in operands.items():
        if isinstance(t, torch.Tensor) and tuple(t.shape) != shape: raise ValueError(f'{name}: expected shape {shape}, got {tuple(t.shape)}')


class _ChannelAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _check('x', x)
        B, C, h, w = x.shape
        nbytes = _lib.lib.smd_channel_attention_workspace_bytes(B, C, h*w, 0)
        if nbytes == 0: raise ValueError(f'channel_attention does not serve the sizes B={B} C={C} n={h*w}')
        out = torch.empty_like(x)
        stats = torch.empty((2, B, C), device=x.device, dtype=torch.float32)
        ws, nbytes = _workspace(x.device, nbytes)
        call('smd_channel_attention_fwd', x.data_ptr(), out.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, B, C, h*w, _stream())
        ctx.save_for_backward(x, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        _on(x)
        B, C, h, w = x.shape
        g = _check('grad(out)', g, x.shape)
        g_x = torch.empty_like(x)
        ws, nbytes = _workspace(x.device, _lib.lib.smd_channel_attention_workspace_bytes, B, C, h*w, 1)
        call('smd_channel_attention_bwd', x.data_ptr(), stats.data_ptr(), g.data_ptr(), g_x.data_ptr(), ws.data_ptr(), nbytes, B, C, h*w, _stream())
        return g_x


def channel_attention(x):
    """Structure perception of CADepth (src/networks/decoders/cadepth.py:14-27): with V = x.view(B,C,h*w) and A = V V^T,
    `x + (softmax(A.max(-1, keepdim=True)[0] - A, -1) @ V).view_as(x)`.  x (B,C,h,w) fp32, any C and h*w -> (B,C,h,w) fp32."""
    _shapes(x)
    return _ChannelAttention.apply(x)


class _SeGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = _check('x', x)
        B, C, h, w = x.shape
        w1 = _check('w1', w1, (C, C)); w2 = _check('w2', w2, (C, C))
        b1 = _check('b1', b1, (C,)); b2 = _check('b2', b2, (C,))
        nbytes = _lib.lib.smd_se_gate_workspace_bytes(B, C, h*w)
        if nbytes == 0: raise ValueError(f'se_gate does not serve the sizes B={B} C={C} hw={h*w}')
        y = torch.empty_like(x)
        save = torch.empty((3, B, C), device=x.device, dtype=torch.float32)
        ws, nbytes = _workspace(x.device, nbytes)
        call('smd_se_gate_fwd', x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), save.data_ptr(), ws.data_ptr(), nbytes,
             B, C, h*w, _stream())
        ctx.save_for_backward(x, w1, w2, save)
        gate = save[0]
        ctx.mark_non_differentiable(gate)
        return y, gate

    @staticmethod
    def backward(ctx, g_y, _g_gate):
        x, w1, w2, save = ctx.saved_tensors
        dev = _on(x)
        B, C, h, w = x.shape
        need_x, need_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:])
        if not (need_x or need_p): return None, None, None, None, None
        g_y = _check('grad(y)', g_y, x.shape)
        g_x = torch.empty_like(x) if need_x else None
        g_w1 = g_b1 = g_w2 = g_b2 = None
        if need_p:
            g_w1 = torch.empty((C, C), device=dev, dtype=torch.float32); g_w2 = torch.empty((C, C), device=dev, dtype=torch.float32)
            g_b1 = torch.empty((C,), device=dev, dtype=torch.float32); g_b2 = torch.empty((C,), device=dev, dtype=torch.float32)
        ws, nbytes = _workspace(dev, _lib.lib.smd_se_gate_workspace_bytes, B, C, h*w)
        call('smd_se_gate_bwd', x.data_ptr(), g_y.data_ptr(), w1.data_ptr(), w2.data_ptr(), save.data_ptr(), _ptr(g_x), _ptr(g_w1), _ptr(g_b1), _ptr(g_w2), _ptr(g_b2),
             ws.data_ptr(), nbytes, B, C, h*w, _stream())
        return g_x, g_w1, g_b1, g_w2, g_b2


def se_gate(x, w1, b1, w2, b2, return_gate: bool = False):
    """The squeeze-excite gate of CADepth's detail emphasis (src/networks/decoders/cadepth.py:35-41, 45): `x + x*a` with
    `a = sigmoid(conv1x1(relu(conv1x1(mean_hw(x), w1, b1)), w2, b2))`.  x (B,C,h,w) fp32; w1, w2 (C,C) or the 1x1 convolutions' (C,C,1,1); b1, b2 (C)
    -> y (B,C,h,w), and with `return_gate` the gate a (B,C) (detached: the gradient flows through y)."""
    w1 = w1.reshape(w1.shape[:2]) if isinstance(w1, torch.Tensor) and w1.ndim == 4 and tuple(w1.shape[2:]) == (1, 1) else w1
    w2 = w2.reshape(w2.shape[:2]) if isinstance(w2, torch.Tensor) and w2.ndim == 4 and tuple(w2.shape[2:]) == (1, 1) else w2
    if isinstance(x, torch.Tensor) and x.ndim == 4: _shapes(x, w1=(w1, (x.shape[1],)*2), b1=(b1, x.shape[1:2]), w2=(w2, (x.shape[1],)*2), b2=(b2, x.shape[1:2]))
    else: _shapes(x)
    y, gate = _SeGate.apply(x, w1, b1, w2, b2)
    return (y, gate.detach()) if return_gate else y
