"""The ResNet encoders' 3x3 stride-2 convolutions as a `torch.autograd.Function`: forward, data gradient and weight gradient on the split-bf16 MFMA kernels
(`smd_conv3x3s2_mfma_*`, `smd_conv3x3s2d_mfma_*`) or on MIOpen, each as `conv_routing.serve` decides.  `functional` re-exports the wrapper."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _stream, _workspace, call
from .conv_ops import _mfma_pack
from .conv_routing import may_serve, serve


class _Conv3x3s2(torch.autograd.Function):
    """`conv3x3_s2`.  Each of the three operators on the kernels or MIOpen as `serve` says (ops `fwd_s2`, `data_t2`, `wgt_s2`)."""
    @staticmethod
    def forward(ctx, x, weight):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (B,C,H,W), got {tuple(x.shape)}')
        B, C, H, W = x.shape
        if weight.ndim != 4 or tuple(weight.shape[1:]) != (C, 3, 3): raise ValueError(f'weight: expected (CO,{C},3,3), got {tuple(weight.shape)}')
        CO = weight.shape[0]
        weight = _check('weight', weight, (CO, C, 3, 3))
        ho, wo = (H - 1)//2 + 1, (W - 1)//2 + 1
        nws = _lib.lib.smd_conv3x3s2_mfma_workspace_bytes(B, C, CO, H, W)   # (0: a shape the kernels do not serve — the reference serves every operator)
        nwd = _lib.lib.smd_conv3x3s2d_mfma_workspace_bytes(B, C, CO, H, W) if ctx.needs_input_grad[0] else 0
        # The data gradient's operand image rides in the forward's pack launch (`conv_ops._Conv3x3Wide` does the same) where the backward may read it and the
        # kernels are known to serve this forward: the forward's own A/B times the forward's pack alone (the second image costs 2 - 12 us, profiles/s2_data_convs.txt)
        want_bwd = nwd > 0 and may_serve(('data_t2', B, C, CO, H, W)) and may_serve(('fwd_s2', B, C, CO, H, W), unknown=False)
        y = torch.empty((B, CO, ho, wo), device=x.device, dtype=torch.float32)
        packed = {}

        def run_mfma():                                     # the pack included: every call pays it
            wf, packed['wb'] = _mfma_pack(weight, C, CO, 3, True, want_bwd)
            ws, n = _workspace(x.device, nws, floor=256)
            call('smd_conv3x3s2_mfma_fwd', x.data_ptr(), wf.data_ptr(), y.data_ptr(), ws.data_ptr(), n, B, C, CO, H, W, _stream())
            return y
        y = serve(('fwd_s2', B, C, CO, H, W), run_mfma, lambda: torch.conv2d(x, weight, None, 2, 1), eligible=nws > 0)
        ctx.save_for_backward(x, weight, packed.get('wb'))
        ctx.nws, ctx.nwd = nws, nwd
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, wp_bwd = ctx.saved_tensors
        dev = _on(x)
        B, C, H, W = x.shape
        CO = weight.shape[0]
        need_x, need_w = ctx.needs_input_grad
        g_y = _check('grad(y)', g_y, (B, CO, (H - 1)//2 + 1, (W - 1)//2 + 1))
        cb = lambda mask: torch.ops.aten.convolution_backward(g_y, x, weight, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, mask)
        g_x = g_w = None
        if need_x:
            g_x = torch.empty_like(x)
            packed = {'wb': wp_bwd}

            def run_data():                                 # (MIOpen served the forward, or the route was not known then: the pack is paid here)
                if packed['wb'] is None: packed['wb'] = _mfma_pack(weight, C, CO, 3, False, True)[1]
                ws, n = _workspace(dev, ctx.nwd, floor=256)
                call('smd_conv3x3s2d_mfma_bwd_data', g_y.data_ptr(), packed['wb'].data_ptr(), g_x.data_ptr(), ws.data_ptr(), n, B, C, CO, H, W, _stream())
                return g_x
            g_x = serve(('data_t2', B, C, CO, H, W), run_data, lambda: cb([True, False, False])[0], eligible=ctx.nwd > 0)
        if need_w:
            g_w = torch.empty_like(weight)

            def run_wgt():
                ws, n = _workspace(dev, ctx.nws, floor=256)
                call('smd_conv3x3s2_mfma_bwd_weight', x.data_ptr(), g_y.data_ptr(), g_w.data_ptr(), ws.data_ptr(), n, B, C, CO, H, W, _stream())
                return g_w
            g_w = serve(('wgt_s2', B, C, CO, H, W), run_wgt, lambda: cb([False, True, False])[1], eligible=ctx.nws > 0)
        return g_x, g_w


def conv3x3_s2(x, weight):
    """`F.conv2d(x, weight (CO,C,3,3), stride=2, padding=1)`, bias-free: `conv1` of the first BasicBlock of layer2 / layer3 / layer4 of the ResNet encoders
    (the timm blocks built at src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,H,W) fp32 -> (B,CO,(H-1)//2+1,(W-1)//2+1) fp32.  C % 16 == 0
    with CO % 32 == 0: forward, data gradient and weight gradient on the split-bf16 MFMA kernels (`smd_conv3x3s2_mfma_*`, `smd_conv3x3s2d_mfma_bwd_data`, the
    zero padding done inside them) or MIOpen, per operator and shape (`conv_routing._conv_route`, ops `fwd_s2` / `data_t2` / `wgt_s2`; `set_conv_route('mfma')`
    pins the kernels); any other channel count goes to MIOpen."""
    return _Conv3x3s2.apply(x, weight)
