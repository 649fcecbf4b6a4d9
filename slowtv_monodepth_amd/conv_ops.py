"""The routed convolutions as `torch.autograd.Function`s: every operator (forward, data gradient, weight gradient) runs on the split-bf16 MFMA kernels
(`smd_conv3x3_mfma_*`, `smd_conv3x3z_mfma_*`, `smd_conv7x7s2_*`; the stride-2 3x3 layers: `conv_s2`) or on its reference, as `conv_routing.serve` decides.  `functional` re-exports the wrappers."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._device import _check, _check_fb, _on, _ptr, _stream, _workspace, call
from .conv_routing import serve

_BF = torch.bfloat16


def _thin_bwd(xp, weight, g_y, want_x, want_w):
    """The f32-MFMA kernels of the last stage (`smd_conv3x3_thin_bwd`; fp32 tensors only): (g_xp, g_w), None where not wanted."""
    if not (want_x or want_w): return None, None
    B, C, H, W = xp.shape
    g_xp = torch.empty_like(xp) if want_x else None
    g_w = torch.empty_like(weight) if want_w else None
    ws, nbytes = _workspace(xp.device, _lib.lib.smd_conv3x3_thin_workspace_bytes, B, C, H - 2, W - 2, floor=256) if want_w else (None, 0)
    call('smd_conv3x3_thin_bwd', xp.data_ptr(), weight.data_ptr(), g_y.data_ptr(), _ptr(g_xp), _ptr(g_w), _ptr(ws), nbytes, B, C, H - 2, W - 2, _stream())
    return g_xp, g_w


class _Conv3x3Thin(torch.autograd.Function):
    """`conv3x3_thin`: the f32 MFMA (`smd_conv3x3_thin_*`: `v_mfma_f32_16x16x4_f32`, operands staged through LDS); `conv3x3_wide` routes to it per operator."""
    @staticmethod
    def forward(ctx, xp, weight):
        xp = _check('xp', xp)
        if xp.ndim != 4 or xp.shape[2] < 4 or xp.shape[3] < 4: raise ValueError(f'expected a padded (B,C,h+2,w+2) with h, w >= 2, got {tuple(xp.shape)}')
        B, C, H, W = xp.shape
        weight = _check('weight', weight, (16, C, 3, 3))
        y = torch.empty((B, 16, H - 2, W - 2), device=xp.device, dtype=torch.float32)
        call('smd_conv3x3_thin_fwd', xp.data_ptr(), weight.data_ptr(), y.data_ptr(), B, C, H - 2, W - 2, _stream())
        ctx.save_for_backward(xp, weight)
        return y

    @staticmethod
    def backward(ctx, g_y):
        xp, weight = ctx.saved_tensors
        _on(xp)
        B, C, H, W = xp.shape
        g_y = _check('grad(y)', g_y, (B, 16, H - 2, W - 2))
        return _thin_bwd(xp, weight, g_y, *ctx.needs_input_grad)


def conv3x3_thin(xp, weight):
    """`F.conv2d(xp, weight)` for sixteen output channels and an input that is already reflection-padded: the thin up-convolution of the decoder's last
    stage (src/networks/decoders/monodepth.py:45-50, 80-84), bias-free (the next glue kernel adds it).  xp (B,C,h+2,w+2), weight (16,C,3,3) -> (B,16,h,w);
    C = 16 or 32 (`_lib.Unsupported` otherwise)."""
    return _Conv3x3Thin.apply(xp, weight)


_Served = namedtuple('_Served', 'fwd data wgt thin sized')


def _served(C, CO, zpad, sized) -> _Served:
    """What the 3x3 MFMA kernels serve for one layer — the Python statement of `smd::conv_mfma_served` (csrc/smd_kernels.h), made once per forward and read
    from `ctx` by the backward; thin: the last stage (its reference is the f32-MFMA kernel); sized: the workspace query took the sizes (or `force`)."""
    thin = CO == 16 and C in (16, 32) and not zpad
    return _Served(fwd=(C % 16 == 0 and CO % 32 == 0) or thin,
                   data=(CO % 16 == 0 and C % 32 == 0) or (C == 16 and CO == 16 and not zpad),   # the data gradient's own operand order
                   wgt=CO % 32 == 0 or thin, thin=thin, sized=sized)


def _mfma_pack(weight, C, CO, pieces, want_fwd, want_bwd):
    nbytes = _lib.lib.smd_conv3x3_mfma_packed_bytes(C, CO, pieces)
    wf = _workspace(weight.device, nbytes, floor=256)[0] if want_fwd else None
    wb = _workspace(weight.device, nbytes, floor=256)[0] if want_bwd else None
    call('smd_conv3x3_mfma_pack', weight.data_ptr(), _ptr(wf), _ptr(wb), C, CO, pieces, _stream())
    return wf, wb


def _mfma_ws_bytes(B, C, CO, h, w, zpad):
    return (_lib.lib.smd_conv3x3z_mfma_workspace_bytes if zpad else _lib.lib.smd_conv3x3_mfma_workspace_bytes)(B, C, CO, h, w)


def _mfma_launch(entry, zpad, a, b, out, nws, dims, pieces):
    """`smd_conv3x3[z]_mfma_<entry>` into `out` (returned) on a workspace of its own; `dims` = (B, C, CO, h, w)."""
    ws, nws = _workspace(out.device, nws, floor=256)
    call(('smd_conv3x3z_mfma_' if zpad else 'smd_conv3x3_mfma_') + entry, a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), nws, *dims, pieces, _stream())
    return out


class _Conv3x3Wide(torch.autograd.Function):
    """`F.conv2d(xp, weight (CO,C,3,3))` on an already reflection-padded input; each of the three operators (forward, data gradient, weight gradient) runs
    on the bf16 matrix cores (`smd_conv3x3_mfma_*`) or through the alternative — MIOpen, or for the 16-channel last stage in fp32 the f32-MFMA kernels
    `smd_conv3x3_thin_*` — as `conv_routing.serve` says (`force`: always the MFMA kernels).  fp32 tensors: every operand split into three bf16 pieces, fp32-class
    results.  bfloat16 tensors (bf16 autocast): one piece, bf16 in and out, the weights as their bf16 rounding, fp32 accumulation and an fp32 weight gradient.
    `zpad`: the zero-padded "same" layer on the UNPADDED x instead (`conv3x3_same`; fp32 only), routed under `fwd_z` / `data_z` / `wgt_z`."""
    @staticmethod
    def forward(ctx, xp, weight, pieces, force, zpad=False):
        xp = _check_fb('xp', xp)
        if zpad and xp.dtype != torch.float32: raise TypeError(f'the zero-padded convolution takes float32 tensors, got {xp.dtype}')
        if xp.ndim != 4 or (not zpad and (xp.shape[2] < 3 or xp.shape[3] < 3)):
            raise ValueError(f'expected {"(B,C,h,w)" if zpad else "a padded (B,C,h+2,w+2)"}, got {tuple(xp.shape)}')
        B, C, H, W = xp.shape
        if weight.ndim != 4 or tuple(weight.shape[1:]) != (C, 3, 3): raise ValueError(f'weight: expected (CO,{C},3,3), got {tuple(weight.shape)}')
        CO = weight.shape[0]
        weight = _check('weight', weight, (CO, C, 3, 3))
        h, w = (H, W) if zpad else (H - 2, W - 2)
        dims = (B, C, CO, h, w)
        bf = xp.dtype == _BF
        if bf: pieces = 1
        nws = _mfma_ws_bytes(*dims, zpad)                   # (0: sizes the kernels do not take — the reference serves every operator)
        sv = _served(C, CO, zpad, force or nws > 0)
        if force and not sv.fwd:
            raise _lib.Unsupported(f'the MFMA forward serves C % 16 == 0 with CO % 32 == 0{"" if zpad else ", or CO = 16 with C = 16 | 32"}, not C={C} CO={CO}')
        y = torch.empty((B, CO, h, w), device=xp.device, dtype=xp.dtype)
        packed = {}

        def run_mfma():                                     # the pack included: production pays it on every call, so the A/B times it too
            packed['wf'], packed['wb'] = _mfma_pack(weight, C, CO, pieces, True, sv.data)
            return _mfma_launch('fwd', zpad, xp, packed['wf'], y, nws, dims, pieces)

        def run_ref():
            if zpad: return torch.conv2d(xp, weight, None, 1, 1)
            if bf: return torch.conv2d(xp, weight.to(_BF))
            if sv.thin: call('smd_conv3x3_thin_fwd', xp.data_ptr(), weight.data_ptr(), y.data_ptr(), B, C, h, w, _stream()); return y
            return torch.conv2d(xp, weight)
        op = 'fwd_z' if zpad else 'fwd_bf16' if bf else 'fwd'
        out = serve((op, *dims), run_mfma, run_ref, eligible=sv.fwd and sv.sized, force=force)
        ctx.save_for_backward(xp, weight, packed.get('wb'))
        ctx.pieces, ctx.force, ctx.zpad, ctx.served = pieces, force, zpad, sv
        return out

    @staticmethod
    def backward(ctx, g_y):
        xp, weight, wp_bwd = ctx.saved_tensors
        return (*_wide_backward(xp, weight, wp_bwd, g_y, ctx.pieces, ctx.force, ctx.zpad, ctx.served, *ctx.needs_input_grad[:2]), None, None, None)


def _wide_backward(xp, weight, wp_bwd, g_y, pieces, force, zpad, sv, need_x, need_w, deterministic_ref=False):
    """(g_xp, g_w) of `_Conv3x3Wide` for dL/dy = g_y, None where not needed: each operator on the MFMA kernels or its reference, as `serve` says.  Also the
    tail of `ddv_ops.ddv_head`'s backward, whose dL/dy is the recomputed logit gradient.  `deterministic_ref`: where MIOpen serves an operator it is asked for
    its deterministic solvers (left to itself it may pick one that accumulates with atomics: other bits on every run)."""
    _on(xp)
    B, C, H, W = xp.shape
    CO = weight.shape[0]
    h, w = (H, W) if zpad else (H - 2, W - 2)
    dims = (B, C, CO, h, w)
    bf = xp.dtype == _BF
    g_y = _check_fb('grad(y)', g_y.to(xp.dtype), (B, CO, h, w))
    g_xp = g_w = None
    w_ref = weight.to(_BF) if bf else weight
    pad = [1, 1] if zpad else [0, 0]
    def cb(mask):
        # deterministic_ref: ONLY `torch.backends.cudnn.deterministic` is set, and restored (`torch.backends.cudnn.flags(...)` would also switch `enabled` off
        # and with it MIOpen itself: ATen's im2col fallback would serve the call)
        det = torch.backends.cudnn.deterministic
        if deterministic_ref: torch.backends.cudnn.deterministic = True
        try: return torch.ops.aten.convolution_backward(g_y, xp, w_ref, None, [1, 1], pad, [1, 1], False, [0, 0], 1, mask)
        finally: torch.backends.cudnn.deterministic = det
    thin_ref = sv.thin and not bf                       # (the last stage in fp32: the reference is the f32-MFMA kernel)
    sfx = '_z' if zpad else '_bf16' if bf else ''
    nws = _mfma_ws_bytes(*dims, zpad) if sv.sized and ((need_x and sv.data) or (need_w and sv.wgt)) else 0
    if need_x:
        g_xp = torch.empty_like(xp)
        packed = {'wb': wp_bwd}

        def run_data():
            if packed['wb'] is None: packed['wb'] = _mfma_pack(weight, C, CO, pieces, False, True)[1]
            return _mfma_launch('bwd_data', zpad, g_y, packed['wb'], g_xp, nws, dims, pieces)
        ref_data = (lambda: _thin_bwd(xp, weight, g_y, True, False)[0]) if thin_ref else (lambda: cb([True, False, False])[0])
        g_xp = serve(('data' + sfx, *dims), run_data, ref_data, eligible=sv.data and sv.sized, force=force)
    if need_w:
        g_w = torch.empty_like(weight)
        run_wgt = lambda: _mfma_launch('bwd_weight', zpad, xp, g_y, g_w, nws, dims, pieces)
        ref_wgt = (lambda: _thin_bwd(xp, weight, g_y, False, True)[1]) if thin_ref else (lambda: cb([False, True, False])[1].float())
        g_w = serve(('wgt' + sfx, *dims), run_wgt, ref_wgt, eligible=sv.wgt and sv.sized, force=force)
    return g_xp, g_w


def conv3x3_mfma(xp, weight, pieces: int = 3):
    """`F.conv2d(xp, weight)` for an input that is already reflection-padded, ALWAYS through the split-bf16 MFMA kernels (`smd_conv3x3_mfma_*`): the wide
    up-convolutions of the decoder (src/networks/decoders/monodepth.py:40-50, 71-84), bias-free (the next glue kernel adds it).  xp (B,C,h+2,w+2) fp32,
    weight (CO,C,3,3) fp32 -> (B,CO,h,w) fp32; C % 16 == 0 and CO % 32 == 0, or the thin stage CO = 16 with C = 16 | 32 (`_lib.Unsupported` otherwise).  Every fp32 operand is split exactly into three
    bf16 pieces and six products are kept per fp32 product (`pieces=3`: fp32-class error, see csrc/smd_conv_mfma.hip; `pieces=2` is an experiment setting)."""
    return _Conv3x3Wide.apply(xp, weight, int(pieces), True)


def conv3x3_wide(xp, weight):
    """The same convolution, each operator through whichever of the MFMA kernels and MIOpen won this box's A/B for its shape (`conv_routing._conv_route`)."""
    return _Conv3x3Wide.apply(xp, weight, 3, False)


def conv3x3_same(x, weight):
    """`F.conv2d(x, weight (CO,C,3,3), padding=1)`, bias-free, zero padding: the ResNet encoders' 3x3 stride-1 convolutions (the timm blocks built at
    src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,h,w) fp32 -> (B,CO,h,w) fp32.  Each operator runs on the split-bf16 MFMA kernels
    (`smd_conv3x3z_mfma_*`, the padding done inside them) or MIOpen, as `conv_routing._conv_route` says under `fwd_z` / `data_z` / `wgt_z`
    (`set_conv_route('mfma')` pins the kernels); channel counts or sizes the kernels do not take go to MIOpen."""
    return _Conv3x3Wide.apply(x, weight, 3, False, True)


class _Conv7x7s2Stem(torch.autograd.Function):
    """`conv7x7s2_stem`.  The input is normally the image; a data gradient, where asked for, is ATen's."""
    @staticmethod
    def forward(ctx, x, weight):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (B,C,H,W), got {tuple(x.shape)}')
        B, C, H, W = x.shape
        if weight.ndim != 4 or tuple(weight.shape[1:]) != (C, 7, 7): raise ValueError(f'weight: expected (CO,{C},7,7), got {tuple(weight.shape)}')
        CO = weight.shape[0]
        weight = _check('weight', weight, (CO, C, 7, 7))
        ho, wo = (H - 1)//2 + 1, (W - 1)//2 + 1
        served = _lib.lib.smd_conv7x7s2_workspace_bytes(B, C, CO, H, W) > 0
        y = torch.empty((B, CO, ho, wo), device=x.device, dtype=torch.float32)

        def run_mfma():                                     # the pack included: every call pays it
            wp, _ = _workspace(x.device, _lib.lib.smd_conv7x7s2_packed_bytes, C, CO)
            call('smd_conv7x7s2_pack', weight.data_ptr(), wp.data_ptr(), C, CO, _stream())
            call('smd_conv7x7s2_fwd', x.data_ptr(), wp.data_ptr(), y.data_ptr(), B, C, CO, H, W, _stream())
            return y
        y = serve(('fwd_s', B, C, CO, H, W), run_mfma, lambda: torch.conv2d(x, weight, None, 2, 3), eligible=served)
        ctx.save_for_backward(x, weight)
        ctx.served = served
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight = ctx.saved_tensors
        dev = _on(x)
        B, C, H, W = x.shape
        CO = weight.shape[0]
        need_x, need_w = ctx.needs_input_grad
        g_y = _check('grad(y)', g_y, (B, CO, (H - 1)//2 + 1, (W - 1)//2 + 1))
        cb = lambda mask: torch.ops.aten.convolution_backward(g_y, x, weight, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1, mask)
        g_x = cb([True, False, False])[0] if need_x else None
        g_w = None
        if need_w:
            g_w = torch.empty_like(weight)

            def run_wgt():
                ws, nws = _workspace(dev, _lib.lib.smd_conv7x7s2_workspace_bytes, B, C, CO, H, W, floor=256)
                call('smd_conv7x7s2_bwd_weight', x.data_ptr(), g_y.data_ptr(), g_w.data_ptr(), ws.data_ptr(), nws, B, C, CO, H, W, _stream())
                return g_w
            g_w = serve(('wgt_s', B, C, CO, H, W), run_wgt, lambda: cb([False, True, False])[1], eligible=ctx.served)
        return g_x, g_w


def conv7x7s2_stem(x, weight):
    """`F.conv2d(x, weight (CO,C,7,7), stride=2, padding=3)`, bias-free: the ResNet encoders' stem (`conv1` of the timm ResNets built at
    src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,H,W) fp32 -> (B,CO,(H-1)//2+1,(W-1)//2+1) fp32.  CO = 64 with C = 3 or 6: forward and
    weight gradient on the split-bf16 MFMA kernels (`smd_conv7x7s2_*`) or MIOpen, per operator and shape (`conv_routing._conv_route`, ops `fwd_s` / `wgt_s`;
    `set_conv_route('mfma')` pins the kernels); any other channel count goes to MIOpen."""
    return _Conv7x7s2Stem.apply(x, weight)
