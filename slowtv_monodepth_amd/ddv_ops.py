"""The output head of the DDVNet decoder as a `torch.autograd.Function` (`smd_ddv_head_*`: csrc/smd_ddv.hip).  `functional` re-exports `ddv_head`."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, _workspace, call
from .conv_ops import conv3x3_wide_backward, pack_weights

__all__ = ['ddv_head', 'NUM_BINS']

NUM_BINS = 128     # bins per output channel (src/networks/decoders/ddvnet.py:90); the kernels are built for this count


class _DdvHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, weight, bias, G):
        xp = _check('xp', xp)
        B, C, H, W = xp.shape
        h, w = H - 2, W - 2
        M = NUM_BINS*G
        weight = _check('weight', weight, (M, C, 3, 3))
        bias = _check('bias', bias, (M,))
        if _lib.lib.smd_ddv_head_workspace_bytes(B, C, G, h, w) == 0: raise ValueError(f'ddv_head does not serve the sizes B={B} C={C} out_ch={G} h={h} w={w}')
        wf, _ = pack_weights(weight, C, M, 3, True, False)
        disp = torch.empty((B, G, h, w), device=xp.device, dtype=torch.float32)
        stats = torch.empty((B, G, 2, h, w), device=xp.device, dtype=torch.float32)
        call('smd_ddv_head_fwd', xp.data_ptr(), wf.data_ptr(), bias.data_ptr(), disp.data_ptr(), stats.data_ptr(), B, C, G, h, w, _stream())
        ctx.save_for_backward(xp, weight, bias, wf, disp, stats)
        ctx.G = G
        return disp

    @staticmethod
    def backward(ctx, g_disp):
        xp, weight, bias, wf, disp, stats = ctx.saved_tensors
        dev = _on(xp)
        B, C, H, W = xp.shape
        h, w, G = H - 2, W - 2, ctx.G
        M = NUM_BINS*G
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b): return None, None, None, None
        g_disp = _check('grad(disp)', g_disp, disp.shape)
        g_logits = torch.empty((B, M, h, w), device=dev, dtype=torch.float32)     # the one volume the backward writes: dL/dy of the convolution
        g_bias = torch.empty((M,), device=dev, dtype=torch.float32) if need_b else None
        ws, nbytes = _workspace(dev, _lib.lib.smd_ddv_head_workspace_bytes, B, C, G, h, w)
        call('smd_ddv_head_bwd_logits', xp.data_ptr(), wf.data_ptr(), bias.data_ptr(), disp.data_ptr(), stats.data_ptr(), g_disp.data_ptr(), g_logits.data_ptr(),
             _ptr(g_bias), ws.data_ptr(), nbytes, B, C, G, h, w, _stream())
        g_xp, g_w = conv3x3_wide_backward(xp, weight, g_logits, need_x=need_x, need_w=need_w, deterministic_ref=True)
        return g_xp, g_w, g_bias, None


def ddv_head(xp, weight, bias, out_ch: int = 1):
    """The DDVNet output head (src/networks/decoders/ddvnet.py:110, 116-124, 147-150) on an already reflection-padded input: with
    `logits = F.conv2d(xp, weight, bias)` of 128 bins per output channel, `cat([(l.softmax(1) * bins).sum(1, keepdim=True) for l in logits.chunk(out_ch, 1)], 1)`,
    `bins[k] = k/128`.  xp (B,C,h+2,w+2) fp32 with C a multiple of 16, weight (128*out_ch,C,3,3), bias (128*out_ch), out_ch in 1..4 -> disp (B,out_ch,h,w) fp32.
    The forward keeps neither the logits nor the probabilities (per pixel: the row maximum and the reciprocal exponential sum); the backward recomputes the
    logits, writes their gradient once and hands it to the routed data / weight gradients of `conv3x3_wide`."""
    if not isinstance(out_ch, int) or isinstance(out_ch, bool) or not 1 <= out_ch <= 4: raise ValueError(f'out_ch must be an int in 1..4, got {out_ch!r}')
    if isinstance(xp, torch.Tensor):
        if xp.ndim != 4 or xp.numel() == 0 or xp.shape[2] < 3 or xp.shape[3] < 3: raise ValueError(f'expected a non-empty padded (B,C,h+2,w+2), got {tuple(xp.shape)}')
        C, M = xp.shape[1], NUM_BINS*out_ch
        if C % 16: raise ValueError(f'ddv_head takes C a multiple of 16, got C={C}')
        if isinstance(weight, torch.Tensor) and tuple(weight.shape) != (M, C, 3, 3): raise ValueError(f'weight: expected shape {(M, C, 3, 3)}, got {tuple(weight.shape)}')
        if isinstance(bias, torch.Tensor) and tuple(bias.shape) != (M,): raise ValueError(f'bias: expected shape {(M,)}, got {tuple(bias.shape)}')
    return _DdvHead.apply(xp, weight, bias, out_ch)
