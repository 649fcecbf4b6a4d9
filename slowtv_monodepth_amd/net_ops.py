"""The network glue as `torch.autograd.Function`s: the decoder's activation / padding / head kernels and the encoders' normalisation, pooling and depthwise
layers (`smd_elu_*`, `smd_conv3x3_head*`, `smd_bn_*`, `smd_maxpool3x3s2_*`, `smd_dwconv7x7_*`, `smd_layernorm_cf_*`).  `functional` re-exports the wrappers."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _aligned, _check, _check_fb, _on, _ptr, _stream, _workspace, call

_BF = torch.bfloat16


class _EluPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, apply_elu, out_dtype):
        x = _check_fb('x', x)
        if x.ndim != 4: raise ValueError(f'expected (B,C,h,w), got {tuple(x.shape)}')
        B, C, h, w = x.shape
        if bias is not None: bias = _check('bias', bias, (C,))
        out = torch.empty((B, C, h + 2, w + 2), device=x.device, dtype=out_dtype)
        dt = (1 if x.dtype == _BF else 0) | (4 if out_dtype == _BF else 0)
        call('smd_elu_pad_fwd', x.data_ptr(), _ptr(bias), out.data_ptr(), B, C, h, w, int(apply_elu), dt, _stream())
        ctx.save_for_backward(x, bias); ctx.apply_elu, ctx.dt, ctx.out_dtype = int(apply_elu), dt, out_dtype
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, bias = ctx.saved_tensors
        _on(x)
        B, C, h, w = x.shape
        g_x = torch.empty_like(x)
        g_b = torch.empty_like(bias) if (bias is not None and ctx.needs_input_grad[1]) else None
        ws, nbytes = _workspace(x.device, _lib.lib.smd_decoder_glue_workspace_bytes, B, C, h, w) if g_b is not None else (None, 0)
        call('smd_elu_pad_bwd', x.data_ptr(), _ptr(bias), _aligned(g_out.to(ctx.out_dtype)).data_ptr(), g_x.data_ptr(), _ptr(g_b), _ptr(ws), nbytes, B, C, h, w,
             ctx.apply_elu, ctx.dt, _stream())
        return g_x, g_b, None, None


def elu_pad(x, bias=None, apply_elu: bool = True, out_dtype=None):
    """reflect_pad1(elu(x + bias)) (or just bias + padding): the input of the next 3x3 convolution of the decoder.
    x float32 or bfloat16; `out_dtype` (default: x's) may be bfloat16 for a bf16 consumer; bias and arithmetic are fp32."""
    return _EluPad.apply(x, bias, apply_elu, out_dtype or x.dtype)


class _Conv3x3Head(torch.autograd.Function):
    """`act(conv3x3(xp, weight (1,C,3,3)) + bias)` on an already reflection-padded input (`smd_conv3x3_head_*`): the decoder's output heads.  xp may be bfloat16
    (the decoder under bf16 autocast): the output, the weights' gradient and every sum stay fp32, `g_xp` comes back in xp's type."""
    @staticmethod
    def forward(ctx, xp, weight, bias, act):
        xp = _check_fb('xp', xp)
        if xp.ndim != 4 or xp.shape[2] < 4 or xp.shape[3] < 4: raise ValueError(f'expected a padded (B,C,h+2,w+2) with h, w >= 2, got {tuple(xp.shape)}')
        B, C, H, W = xp.shape
        weight = _check('weight', weight, (1, C, 3, 3))
        if bias is not None: bias = _check('bias', bias, (1,))
        y = torch.empty((B, 1, H - 2, W - 2), device=xp.device, dtype=torch.float32)
        act = int(act) | (2 if xp.dtype == _BF else 0)            # SMD_HEAD_X_BF16
        call('smd_conv3x3_head_fwd', xp.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), B, C, H - 2, W - 2, act, _stream())
        ctx.save_for_backward(xp, weight, y); ctx.act, ctx.has_bias = act, bias is not None
        return y

    @staticmethod
    def backward(ctx, g_y):
        xp, weight, y = ctx.saved_tensors
        dev = _on(xp)
        B, C, H, W = xp.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g_y = _check('grad(y)', g_y.float(), (B, 1, H - 2, W - 2))
        g_xp = torch.empty_like(xp) if need_x else None
        g_w = torch.empty_like(weight) if (need_w or need_b) else None
        g_b = torch.empty(1, device=dev, dtype=torch.float32) if need_b else None
        ws, nbytes = _workspace(dev, _lib.lib.smd_conv3x3_head_workspace_bytes, B, C, H - 2, W - 2, floor=256) if g_w is not None else (None, 0)
        if g_xp is not None or g_w is not None:
            call('smd_conv3x3_head_bwd', xp.data_ptr(), weight.data_ptr(), y.data_ptr(), g_y.data_ptr(), _ptr(g_xp), _ptr(g_w), _ptr(g_b), _ptr(ws), nbytes, B, C, H - 2,
                 W - 2, ctx.act, _stream())
        return g_xp, (g_w if need_w else None), g_b, None


def conv3x3_head(xp, weight, bias=None, act: str | None = 'sigmoid'):
    """`act(F.conv2d(xp, weight, bias))` for ONE output channel and an input that is already reflection-padded (`elu_pad`'s output): the decoder's
    output heads (src/networks/decoders/monodepth.py:52, 86-87).  xp (B,C,h+2,w+2) fp32 or bf16, weight (1,C,3,3), bias (1) or None -> (B,1,h,w) fp32; act 'sigmoid' | None."""
    if act not in ('sigmoid', 'none', None): raise ValueError(f"act must be 'sigmoid' or None, got {act!r}")
    return _Conv3x3Head.apply(xp, weight, bias, 1 if act == 'sigmoid' else 0)


_HEADN_ACT = {None: 0, 'none': 0, 'sigmoid': 1, 'relu': 2}


class _Conv3x3HeadN(torch.autograd.Function):
    """`act(conv3x3(xp, weight (n,C,3,3)) + bias)`, 1 <= n <= 4, on an already reflection-padded input (`smd_conv3x3_headn_*`): the mask decoder's output heads.
    The padded activation is read once for all n channels.  xp may be bfloat16; the output, the weights' gradient and every sum stay fp32."""
    @staticmethod
    def forward(ctx, xp, weight, bias, act):
        xp = _check_fb('xp', xp)
        if xp.ndim != 4 or xp.shape[2] < 4 or xp.shape[3] < 4: raise ValueError(f'expected a padded (B,C,h+2,w+2) with h, w >= 2, got {tuple(xp.shape)}')
        B, C, H, W = xp.shape
        if not isinstance(weight, torch.Tensor) or weight.ndim != 4 or not 1 <= weight.shape[0] <= 4:
            raise ValueError(f'conv3x3_headn serves 1 to 4 output channels, got a weight of shape {tuple(getattr(weight, "shape", ()))}')
        n = weight.shape[0]
        weight = _check('weight', weight, (n, C, 3, 3))
        if bias is not None: bias = _check('bias', bias, (n,))
        y = torch.empty((B, n, H - 2, W - 2), device=xp.device, dtype=torch.float32)
        act = int(act) | (4 if xp.dtype == _BF else 0)            # SMD_HEADN_X_BF16
        call('smd_conv3x3_headn_fwd', xp.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), B, C, n, H - 2, W - 2, act, _stream())
        ctx.save_for_backward(xp, weight, y); ctx.act, ctx.has_bias = act, bias is not None
        return y

    @staticmethod
    def backward(ctx, g_y):
        xp, weight, y = ctx.saved_tensors
        dev = _on(xp)
        B, C, H, W = xp.shape
        n = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g_y = _check('grad(y)', g_y.float(), (B, n, H - 2, W - 2))
        g_xp = g_w = g_b = None
        if need_x:
            g_xp = torch.empty_like(xp)
            call('smd_conv3x3_headn_bwd_data', weight.data_ptr(), y.data_ptr(), g_y.data_ptr(), g_xp.data_ptr(), B, C, n, H - 2, W - 2, ctx.act, _stream())
        if need_w or need_b:
            g_w = torch.empty_like(weight)
            g_b = torch.empty(n, device=dev, dtype=torch.float32) if need_b else None
            ws, nbytes = _workspace(dev, _lib.lib.smd_conv3x3_headn_workspace_bytes, B, C, n, H - 2, W - 2, floor=256)
            call('smd_conv3x3_headn_bwd_wgt', xp.data_ptr(), y.data_ptr(), g_y.data_ptr(), g_w.data_ptr(), _ptr(g_b), ws.data_ptr(), nbytes, B, C, n, H - 2, W - 2, ctx.act,
                 _stream())
        return g_xp, (g_w if need_w else None), g_b, None


def conv3x3_headn(xp, weight, bias=None, act: str | None = 'sigmoid'):
    """`act(F.conv2d(xp, weight, bias))` for 1 to 4 output channels and an input that is already reflection-padded (`elu_pad`'s output): the output heads of
    the predictive-mask decoder (src/networks/depth.py:108-114, src/networks/decoders/monodepth.py:52, 86-87).
    xp (B,C,h+2,w+2) fp32 or bf16, weight (n,C,3,3), bias (n) or None -> (B,n,h,w) fp32; act 'sigmoid' | 'relu' | None."""
    if act not in _HEADN_ACT: raise ValueError(f"act must be 'sigmoid', 'relu' or None, got {act!r}")
    return _Conv3x3HeadN.apply(xp, weight, bias, _HEADN_ACT[act])


class _EluUpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bias, skip, out_dtype):
        a = _check_fb('a', a)
        if a.ndim != 4: raise ValueError(f'expected (B,C,h,w), got {tuple(a.shape)}')
        B, Ca, h, w = a.shape
        if bias is not None: bias = _check('bias', bias, (Ca,))
        Cs = 0
        if skip is not None:
            Cs = skip.shape[1]
            skip = _check_fb('skip', skip, (B, Cs, 2*h, 2*w))
        out = torch.empty((B, Ca + Cs, 2*h + 2, 2*w + 2), device=a.device, dtype=out_dtype)
        dt = (1 if a.dtype == _BF else 0) | (2 if (skip is not None and skip.dtype == _BF) else 0) | (4 if out_dtype == _BF else 0)
        call('smd_elu_up_cat_pad_fwd', a.data_ptr(), _ptr(bias), _ptr(skip), out.data_ptr(), B, Ca, Cs, h, w, dt, _stream())
        ctx.save_for_backward(a, bias)
        ctx.Cs, ctx.dt, ctx.out_dtype, ctx.skip_dtype = Cs, dt, out_dtype, (skip.dtype if skip is not None else None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        a, bias = ctx.saved_tensors
        _on(a)
        B, Ca, h, w = a.shape
        Cs = ctx.Cs
        g_b = torch.empty_like(bias) if (bias is not None and ctx.needs_input_grad[1]) else None
        g_a = torch.empty_like(a) if (ctx.needs_input_grad[0] or g_b is not None) else None
        g_skip = torch.empty((B, Cs, 2*h, 2*w), device=a.device, dtype=ctx.skip_dtype) if (Cs and ctx.needs_input_grad[2]) else None
        if g_a is None and g_skip is None: return None, None, None, None
        ws, nbytes = _workspace(a.device, _lib.lib.smd_decoder_glue_workspace_bytes, B, Ca, h, w) if g_b is not None else (None, 0)
        call('smd_elu_up_cat_pad_bwd', a.data_ptr(), _ptr(bias), _aligned(g_out.to(ctx.out_dtype)).data_ptr(), _ptr(g_a), _ptr(g_skip), _ptr(g_b), _ptr(ws), nbytes, B,
             Ca, Cs, h, w, ctx.dt, _stream())
        return g_a, g_b, g_skip, None


def elu_up_cat_pad(a, skip=None, bias=None, out_dtype=None):
    """reflect_pad1(cat(nearest_x2(elu(a + bias)), skip)): (B,Ca,h,w) [+ (B,Cs,2h,2w)] -> (B,Ca+Cs,2h+2,2w+2).
    a / skip float32 or bfloat16 (independently); `out_dtype` defaults to a's."""
    return _EluUpCatPad.apply(a, bias, skip, out_dtype or a.dtype)


class _BatchNormAct(torch.autograd.Function):
    """Training-mode BatchNorm2d + optional residual add + optional ReLU (`smd_bn_*`)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, momentum, eps, relu):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (N,C,H,W), got {tuple(x.shape)}')
        N, C, H, W = x.shape
        if N*H*W < 2: raise ValueError('Expected more than 1 value per channel when training')   # F.batch_norm's own check
        if residual is not None: residual = _check('residual', residual, x.shape)
        weight = _check('weight', weight, (C,)); bias = _check('bias', bias, (C,))
        for nm, r in (('running_mean', running_mean), ('running_var', running_var)):     # updated IN PLACE, one element at a time: never copied, so they must be usable as they are
            if r is not None and not (isinstance(r, torch.Tensor) and r.dtype == torch.float32 and r.device == x.device and tuple(r.shape) == (C,) and r.is_contiguous()):
                raise ValueError(f'{nm} must be a contiguous float32 ({C},) tensor on {x.device} (it is updated in place)')
        y = torch.empty_like(x)
        save = torch.empty((2, C), device=x.device, dtype=torch.float32)
        ws, nbytes = _workspace(x.device, _lib.lib.smd_bn_workspace_bytes, N, C, H*W)
        call('smd_bn_fwd', x.data_ptr(), _ptr(residual), weight.data_ptr(), bias.data_ptr(), _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), int(relu),
             y.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), ws.data_ptr(), nbytes, N, C, H*W, _stream())
        ctx.save_for_backward(x, y if relu else None, weight, save)
        ctx.relu, ctx.has_res = bool(relu), residual is not None
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, y, weight, save = ctx.saved_tensors
        _on(x)
        N, C, H, W = x.shape
        g_y = _aligned(g_y)
        g_x = torch.empty_like(x)
        g_res = None
        if ctx.has_res and ctx.needs_input_grad[1]: g_res = torch.empty_like(x) if ctx.relu else g_y   # without ReLU the branch gradient IS g_y
        g_w = torch.empty_like(weight); g_b = torch.empty_like(weight)
        ws, nbytes = _workspace(x.device, _lib.lib.smd_bn_workspace_bytes, N, C, H*W)
        call('smd_bn_bwd', x.data_ptr(), _ptr(y), g_y.data_ptr(), weight.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), int(ctx.relu), g_x.data_ptr(),
             g_res.data_ptr() if (g_res is not None and ctx.relu) else None, g_w.data_ptr(), g_b.data_ptr(), ws.data_ptr(), nbytes, N, C, H*W, _stream())
        return g_x, g_res, g_w, g_b, None, None, None, None, None


def batch_norm_act(x, weight, bias, running_mean=None, running_var=None, *, residual=None, momentum: float = 0.1, eps: float = 1e-5, relu: bool = False):
    """relu?(batch_norm_train(x) [+ residual]); running statistics are updated in place like `F.batch_norm(training=True)`."""
    return _BatchNormAct.apply(x, residual, weight, bias, running_mean, running_var, momentum, eps, relu)


class _MaxPool3x3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (N,C,H,W), got {tuple(x.shape)}')
        N, C, H, W = x.shape
        Ho, Wo = (H - 1)//2 + 1, (W - 1)//2 + 1
        y = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
        idx = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.uint8)
        call('smd_maxpool3x3s2_fwd', x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, C, H, W, _stream())
        ctx.save_for_backward(idx); ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, g_y):
        (idx,) = ctx.saved_tensors
        _on(idx)
        N, C, H, W = ctx.shape
        g_x = torch.empty((N, C, H, W), device=idx.device, dtype=torch.float32)
        call('smd_maxpool3x3s2_bwd', _aligned(g_y).data_ptr(), idx.data_ptr(), g_x.data_ptr(), N, C, H, W, _stream())
        return g_x


def max_pool3x3s2(x):
    """`F.max_pool2d(x, 3, 2, 1)` with a one-byte argmax and a gather backward."""
    return _MaxPool3x3s2.apply(x)


class _DwConv7x7(torch.autograd.Function):
    """Depthwise 7x7 convolution, stride 1, padding 3 (`smd_dwconv7x7_*`)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (N,C,H,W), got {tuple(x.shape)}')
        N, C, H, W = x.shape
        weight = _check('weight', weight, (C, 1, 7, 7))
        if bias is not None: bias = _check('bias', bias, (C,))
        y = torch.empty_like(x)
        call('smd_dwconv7x7_fwd', x.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), N, C, H, W, 0, _stream())
        ctx.save_for_backward(x, weight); ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight = ctx.saved_tensors
        _on(x)
        N, C, H, W = x.shape
        g_y = _aligned(g_y)
        g_x = g_w = g_b = None
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(x)
            call('smd_dwconv7x7_fwd', g_y.data_ptr(), weight.data_ptr(), None, g_x.data_ptr(), N, C, H, W, 1, _stream())
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            g_w = torch.empty_like(weight)
            g_b = torch.empty((C,), device=x.device, dtype=torch.float32) if ctx.has_bias else None
            ws, nbytes = _workspace(x.device, _lib.lib.smd_dwconv7x7_workspace_bytes, C, H, W)
            call('smd_dwconv7x7_wrw', x.data_ptr(), g_y.data_ptr(), g_w.data_ptr(), _ptr(g_b), ws.data_ptr(), nbytes, N, C, H, W, _stream())
        return g_x, g_w, g_b


def dwconv7x7(x, weight, bias=None):
    """`F.conv2d(x, weight (C,1,7,7), bias, padding=3, groups=C)`."""
    return _DwConv7x7.apply(x, weight, bias)


class _LayerNormCF(torch.autograd.Function):
    """LayerNorm over the channel dimension of an NCHW tensor (`smd_layernorm_cf_*`)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_bf16):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (N,C,H,W), got {tuple(x.shape)}')
        N, C, H, W = x.shape
        weight = _check('weight', weight, (C,)); bias = _check('bias', bias, (C,))
        y = torch.empty_like(x, dtype=torch.bfloat16 if out_bf16 else torch.float32)
        stats = torch.empty((2, N*H*W), device=x.device, dtype=torch.float32)
        call('smd_layernorm_cf_fwd', x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), int(out_bf16), stats[0].data_ptr(), stats[1].data_ptr(), N, C, H*W,
             float(eps), _stream())
        ctx.save_for_backward(x, weight, stats)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, stats = ctx.saved_tensors
        _on(x)
        N, C, H, W = x.shape
        if g_y.dtype not in (torch.float32, torch.bfloat16): g_y = g_y.float()
        g_y = _aligned(g_y)
        g_x = torch.empty_like(x); g_w = torch.empty_like(weight); g_b = torch.empty_like(weight)
        ws, nbytes = _workspace(x.device, _lib.lib.smd_layernorm_cf_workspace_bytes, N, C, H*W)
        call('smd_layernorm_cf_bwd', x.data_ptr(), g_y.data_ptr(), int(g_y.dtype == torch.bfloat16), weight.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
             g_x.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), ws.data_ptr(), nbytes, N, C, H*W, _stream())
        return g_x, g_w, g_b, None, None


def layer_norm_cf(x, weight, bias, eps: float = 1e-6, out_dtype=torch.float32):
    """`F.layer_norm(x.permute(0,2,3,1), (C,), weight, bias, eps).permute(0,3,1,2)` without the permutes.  `out_dtype=bfloat16`
    writes the result (and reads its gradient) in bf16 for a bf16 consumer; the arithmetic is fp32."""
    if out_dtype not in (torch.float32, torch.bfloat16): raise TypeError(f'out_dtype must be float32 or bfloat16, got {out_dtype}')
    return _LayerNormCF.apply(x, weight, bias, eps, out_dtype == torch.bfloat16)
