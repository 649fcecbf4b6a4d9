"""The un-fused, class-level operators as `torch.autograd.Function`s: what `ViewSynth`, `PhotoError`, `RegressionLoss`, `ReconstructionLoss` and the
mask / occlusion regularisers call one at a time, the augmentation's crop + resize, and the DPP self-test.  `functional` re-exports the wrappers."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _aligned, _check, _on, _ptr, _ptrs, _stream, _workspace, call
from ._lib import FLAGS, REGR_FLAGS, int_array


class _ViewSynth(torch.autograd.Function):
    """`ViewSynth.forward` (src/tools/geometry.py:366-391) for any channel count."""

    @staticmethod
    def forward(ctx, inp, depth, T, K, K_inv):
        B, Cc, h, w = inp.shape
        inp = _check('input', inp, (B, Cc, h, w)); depth = _check('depth', depth, (B, 1, h, w))
        T = _check('T', T, (B, 4, 4)); K = _check('K', K, (B, 4, 4)); K_inv = _check('K_inv', K_inv, (B, 4, 4))
        warp = torch.empty_like(inp)
        dwarp = torch.empty((B, 1, h, w), device=inp.device, dtype=torch.float32)
        valid = torch.empty((B, 1, h, w), device=inp.device, dtype=torch.uint8)
        call('smd_view_synth_fwd', inp.data_ptr(), depth.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(), warp.data_ptr(), dwarp.data_ptr(), valid.data_ptr(), B,
             Cc, h, w, _stream())
        ctx.save_for_backward(inp, depth, T, K, K_inv)
        ctx.mark_non_differentiable(valid)
        return warp, dwarp, valid

    @staticmethod
    def backward(ctx, g_warp, g_dwarp, _g_valid):
        inp, depth, T, K, K_inv = ctx.saved_tensors
        B, Cc, h, w = inp.shape
        dev = _on(inp)
        g_warp = _check('grad(warp)', g_warp if g_warp is not None else torch.zeros_like(inp))
        g_dwarp = _check('grad(depth_warp)', g_dwarp) if g_dwarp is not None else None
        need_in, need_k = ctx.needs_input_grad[0], (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        g_in = torch.empty_like(inp) if need_in else None
        g_depth = torch.empty_like(depth)
        g_T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
        g_K, g_Ki = (torch.empty((B, 4, 4), device=dev, dtype=torch.float32), torch.empty((B, 4, 4), device=dev, dtype=torch.float32)) if need_k else (None, None)
        ws, nbytes = _workspace(dev, _lib.lib.smd_view_synth_workspace_bytes, B, h, w)
        call('smd_view_synth_bwd', inp.data_ptr(), depth.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(), g_warp.data_ptr(), _ptr(g_dwarp), _ptr(g_in),
             g_depth.data_ptr(), g_T.data_ptr(), _ptr(g_K), _ptr(g_Ki), ws.data_ptr(), nbytes, B, Cc, h, w, _stream())
        return g_in, g_depth, g_T, (g_K if ctx.needs_input_grad[3] else None), (g_Ki if ctx.needs_input_grad[4] else None)


def view_synth(inp, depth, T, K, K_inv=None):
    """-> (input_warp (B,C,h,w), depth_warp (B,1,h,w), mask_valid (B,1,h,w) bool)."""
    if K_inv is None: K_inv = torch.linalg.inv(K)
    warp, dwarp, valid = _ViewSynth.apply(inp, depth, T, K, K_inv)
    return warp, dwarp, valid.bool()


class _PhotoError(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, flags, weight_ssim):
        if pred.ndim != 4: raise ValueError(f'photometric error expects (N,C,h,w) tensors, got {tuple(pred.shape)}')
        N, c, h, w = pred.shape
        pred = _check('pred', pred, (N, c, h, w)); target = _check('target', target, (N, c, h, w))
        err = torch.empty((N, 1, h, w), device=pred.device, dtype=torch.float32)
        call('smd_photo_error_fwd', pred.data_ptr(), target.data_ptr(), err.data_ptr(), N, c, h, w, int(flags), float(weight_ssim), _stream())
        ctx.save_for_backward(pred, target); ctx.flags, ctx.weight_ssim = int(flags), float(weight_ssim)
        return err

    @staticmethod
    def backward(ctx, g_err):
        pred, target = ctx.saved_tensors
        _on(pred)
        N, c, h, w = pred.shape
        g_err = _check('grad(err)', g_err)
        g_pred = torch.empty_like(pred)
        ws, nbytes = _workspace(pred.device, _lib.lib.smd_photo_error_workspace_bytes, N, c, h, w)
        call('smd_photo_error_bwd', pred.data_ptr(), target.data_ptr(), g_err.data_ptr(), g_pred.data_ptr(), ws.data_ptr(), nbytes, N, c, h, w, ctx.flags, ctx.weight_ssim,
             _stream())
        return g_pred, None, None, None


def photo_error(pred, target, loss_name: str = 'ssim', weight_ssim: float = 0.85):
    """(N,C,h,w) x2 -> (N,1,h,w): weight_ssim * SSIM + (1 - weight_ssim) * L1 ('ssim'; `PhotoError(weight_ssim)`,
    src/losses/photometric.py:65-88), channel-mean |.| ('l1') or Euclidean distance ('l2')."""
    if loss_name not in ('ssim', 'l1', 'l2'): raise KeyError(loss_name)
    if not (0 <= weight_ssim <= 1): raise ValueError(f'Invalid SSIM weight. ({weight_ssim} vs. [0, 1])')
    return _PhotoError.apply(pred, target, {'ssim': 0, 'l1': FLAGS['loss_l1'], 'l2': FLAGS['loss_l2']}[loss_name], weight_ssim)


class _Regression(torch.autograd.Function):
    """`RegressionLoss.forward` (src/losses/regression.py:69-75); gradients to both `pred` and `target`."""

    @staticmethod
    def forward(ctx, pred, target, mask, flags):
        pred = _check('pred', pred); target = _check('target', target, pred.shape)
        if mask is not None:
            if tuple(mask.shape) != tuple(pred.shape): raise ValueError(f'mask: expected shape {tuple(pred.shape)}, got {tuple(mask.shape)}')
            # The reference multiplies by the mask (`mask*err`, `err.sum()/mask.sum()`, src/losses/regression.py:72-74), so a float mask
            # there is a per-pixel WEIGHT; the kernel implements the 0/1 case every caller on this path uses (automask, validity).
            if mask.dtype.is_floating_point: raise TypeError('RegressionLoss: pass a bool (or uint8 0/1) mask; weighting masks are not part of the accelerated path')
            mask = _aligned(mask if mask.dtype == torch.bool else mask != 0).view(torch.uint8)
        N, dev = pred.numel(), pred.device
        loss = torch.empty((), device=dev, dtype=torch.float32); err = torch.empty_like(pred)
        stats = torch.zeros(8, device=dev, dtype=torch.float32)
        ws, nbytes = _workspace(dev, _lib.lib.smd_regression_workspace_bytes, N)
        call('smd_regression_fwd', pred.data_ptr(), target.data_ptr(), _ptr(mask), N, int(flags), loss.data_ptr(), err.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes,
             _stream())
        ctx.save_for_backward(pred, target, mask, stats); ctx.flags = int(flags)
        ctx.mark_non_differentiable(err)
        return loss, err

    @staticmethod
    def backward(ctx, g_loss, _g_err):
        pred, target, mask, stats = ctx.saved_tensors
        _on(pred)
        N = pred.numel()
        g_pred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        g_target = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        if g_pred is None and g_target is None: return None, None, None, None
        ws, nbytes = _workspace(pred.device, _lib.lib.smd_regression_workspace_bytes, N)
        call('smd_regression_bwd', pred.data_ptr(), target.data_ptr(), _ptr(mask), N, ctx.flags, stats.data_ptr(), _aligned(g_loss.to(torch.float32)).data_ptr(),
             _ptr(g_pred), _ptr(g_target), ws.data_ptr(), nbytes, _stream())
        return g_pred, g_target, None, None


def regression_loss(pred, target, mask=None, *, loss_name: str = 'berhu', invert: bool = False):
    """Masked mean of a dense regression error -> (loss, err).  loss_name in {'l1', 'log_l1', 'berhu'}."""
    if loss_name not in ('l1', 'log_l1', 'berhu'): raise KeyError(loss_name)
    return _Regression.apply(pred, target, mask, REGR_FLAGS[loss_name] | (REGR_FLAGS['invert'] if invert else 0))


class _ReconReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, err_warp, err_static, mask, noise, seed, flags):
        n, B, h, w = err_warp.shape
        err_warp = _check('err_warp', err_warp, (n, B, h, w))
        if err_static is not None: err_static = _check('err_static', err_static, (n, B, h, w))
        if mask is not None: mask = _check('mask', mask, (B, n, h, w))
        if noise is not None: noise = _check('noise', noise.reshape(B, h, w), (B, h, w))
        dev = err_warp.device
        err = torch.empty((B, h, w), device=dev, dtype=torch.float32)
        sel = torch.empty((B, h, w), device=dev, dtype=torch.uint8)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        ws, nbytes = _workspace(dev, _lib.lib.smd_recon_reduce_workspace_bytes, B, h, w)
        call('smd_recon_reduce_fwd', err_warp.data_ptr(), _ptr(err_static), _ptr(mask), _ptr(noise), int(seed) & (2**64 - 1), err.data_ptr(), sel.data_ptr(),
             loss.data_ptr(), ws.data_ptr(), nbytes, n, B, h, w, int(flags), _stream())
        if mask is not None: ctx.save_for_backward(sel, err_warp, err_static, mask)   # the masked forms' derivatives need the errors and the mask
        else: ctx.save_for_backward(sel, None, None, None)
        ctx.meta = (n, B, h, w, int(flags))
        ctx.mark_non_differentiable(err, sel)
        return loss, err, sel

    @staticmethod
    def backward(ctx, g_loss, *_):
        sel, err_warp, err_static, mask = ctx.saved_tensors
        _on(sel)
        n, B, h, w, flags = ctx.meta
        g = torch.empty((n, B, h, w), device=sel.device, dtype=torch.float32)
        g_mask = torch.empty_like(mask) if mask is not None else None
        call('smd_recon_reduce_bwd', sel.data_ptr(), _aligned(g_loss.to(torch.float32)).data_ptr(), g.data_ptr(), _ptr(err_warp), _ptr(err_static), _ptr(mask),
             _ptr(g_mask), n, B, h, w, flags, _stream())
        return g, None, g_mask, None, None, None


def recon_reduce(err_warp, err_static=None, *, use_min: bool = False, noise=None, seed: int = 0, mask=None, mask_name: str | None = None):
    """Per-support error maps (n,B,h,w) [+ static ones] -> (loss, err (B,h,w), sel uint8 (B,h,w); 255 = auto-masked).

    `mask` (B,n,h,w) with `mask_name` 'explainability' | 'uncertainty': the predictive weighting of `ReconstructionLoss.apply_mask`
    (src/losses/reconstruction.py:46-57), applied to the warped and the static errors before the reductions; differentiable."""
    if mask_name not in {'explainability', 'uncertainty', None}: raise ValueError(f'Invalid mask type: {mask_name}')
    if mask_name and mask is None: raise ValueError("Must provide a 'mask' when masking...")
    flags = (FLAGS['use_min'] if use_min else 0) | (FLAGS['use_automask'] if err_static is not None else 0)
    if mask_name:
        flags |= FLAGS['mask_' + mask_name]
        if mask.shape[1] == 1 and err_warp.shape[0] > 1: mask = mask.expand(-1, err_warp.shape[0], -1, -1)   # one mask for every support (broadcast in the reference)
    return _ReconReduce.apply(err_warp, err_static, mask if mask_name else None, noise, seed, flags)


class _UpsampleStack(torch.autograd.Function):
    """`smd_upsample_stack_*`: S tensors (b,n,hs,ws) -> the scale-major stack (S,b,n,h,w), bilinear, align_corners=False; one launch each way."""
    @staticmethod
    def forward(ctx, size, *xs):
        h, w = size
        xs = [_check(f'x[{i}]', x) for i, x in enumerate(xs)]
        b, n = xs[0].shape[:2]
        for x in xs:
            if x.ndim != 4 or tuple(x.shape[:2]) != (b, n): raise ValueError(f'every scale must be (b,n,hs,ws) with b={b}, n={n}, got {tuple(x.shape)}')
        S, hs, ws = len(xs), [x.shape[2] for x in xs], [x.shape[3] for x in xs]
        out = torch.empty((S, b, n, h, w), device=xs[0].device, dtype=torch.float32)
        call('smd_upsample_stack_fwd', _ptrs(xs), int_array(hs), int_array(ws), S, b, n, h, w, out.data_ptr(), _stream())
        ctx.meta, ctx.dev = (hs, ws, S, b, n, h, w), xs[0].device
        return out

    @staticmethod
    def backward(ctx, g_out):
        hs, ws, S, b, n, h, w = ctx.meta
        g_out = _check('grad(out)', g_out, (S, b, n, h, w))
        _on(g_out)
        gs = [torch.empty((b, n, hs[s], ws[s]), device=g_out.device, dtype=torch.float32) for s in range(S)]
        call('smd_upsample_stack_bwd', int_array(hs), int_array(ws), S, b, n, h, w, g_out.data_ptr(), _ptrs(gs), _stream())
        return (None, *gs)


def upsample_stack(xs, size):
    """xs: sequence of (b,n,hs,ws) -> (S,b,n,h,w): `F.interpolate(x, size, mode='bilinear', align_corners=False)` of every scale, stacked scale-major, in one launch
    (`ops.interpolate_like` per scale, src/core/trainer.py:323-324).  CPU tensors take the torch expression (host-logic tests; the training path is on the GPU)."""
    xs, size = list(xs), tuple(int(v) for v in size)
    if not xs: raise ValueError('no scales given')
    if not xs[0].is_cuda: return torch.stack([torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=False) for x in xs])
    return _UpsampleStack.apply(size, *xs)


_MEAN_MODES = {'bce_ones': 0, 'identity': 1, 'negate': 2}
_mean_ws = {}    # (device, stream) -> workspace whose arrival counter is zero between calls (the kernel leaves it so)


def _scale_mean_ws(dev, nbytes):
    key = (dev, _stream())
    ws = _mean_ws.get(key)
    if ws is None or ws.numel() < nbytes: ws = _mean_ws[key] = torch.zeros(max(nbytes, 4096), device=dev, dtype=torch.uint8)
    return ws


class _ScaleMean(torch.autograd.Function):
    """`smd_scale_mean_*`: mean over the tensors of the mean of f(x) over each tensor's elements."""
    @staticmethod
    def forward(ctx, mode, *xs):
        xs = [_check(f'x[{i}]', x) for i, x in enumerate(xs)]
        numel = _lib.i64_array([x.numel() for x in xs])
        nbytes = _lib.lib.smd_scale_mean_workspace_bytes(numel, len(xs))
        if nbytes == 0: raise ValueError(f'scale_mean serves 1 to {_lib.MAX_SCALES} non-empty tensors')
        ws = _scale_mean_ws(xs[0].device, nbytes)
        loss = torch.empty((), device=xs[0].device, dtype=torch.float32)
        call('smd_scale_mean_fwd', _ptrs(xs), numel, len(xs), mode, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        ctx.save_for_backward(*xs); ctx.mode = mode
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        xs = ctx.saved_tensors
        _on(xs[0])
        g_loss = _aligned(g_loss.float())
        gs = [torch.empty_like(x) for x in xs]
        call('smd_scale_mean_bwd', _ptrs(xs), _lib.i64_array([x.numel() for x in xs]), len(xs), ctx.mode, g_loss.data_ptr(), _ptrs(gs), _stream())
        return (None, *gs)


def scale_mean(xs, mode: str):
    """mean_s(mean(f(x_s))) over a sequence of tensors of any sizes, in one launch (`handlers.disp_mask` / `disp_occ`, src/core/handlers.py:314-347).
    mode 'bce_ones': f = binary cross-entropy against ones (`MaskReg`, src/regularizers/mask.py:29); 'identity' / 'negate': f(x) = x / -x (`OccReg`,
    src/regularizers/occlusion.py:39).  CPU tensors take the torch expression."""
    if mode not in _MEAN_MODES: raise ValueError(f'mode must be one of {tuple(_MEAN_MODES)}, got {mode!r}')
    xs = list(xs)
    if not xs: raise ValueError('no tensors given')
    if not xs[0].is_cuda:
        if mode == 'bce_ones': return torch.stack([torch.nn.functional.binary_cross_entropy(x, torch.ones_like(x)) for x in xs]).mean()
        return torch.stack([(x.mean() if mode == 'identity' else -x.mean()) for x in xs]).mean()
    return _ScaleMean.apply(_MEAN_MODES[mode], *xs)

def crop_resize(tensors, crop_shape, out_shape, K=None):
    """Centre crop + bilinear resize of every tensor in `tensors` ((..., H, W) float32, same H, W) and of the intrinsics `K`
    (..., 4, 4), in one launch: `crop_aug` + `resize_aug` of src/core/aspect_ratio.py:67-151 without materialising the crop.
    -> ([(..., oh, ow) ...], K' or None).  Not differentiable (the reference runs it under `no_grad`, on the data)."""
    if not 1 <= len(tensors) <= 8: raise ValueError('1 to 8 tensors per call')
    H, W = tensors[0].shape[-2:]
    ch, cw = (int(v) for v in crop_shape); oh, ow = (int(v) for v in out_shape)
    ts = []
    for i, t in enumerate(tensors):
        t = _check(f'tensors[{i}]', t.detach())
        if tuple(t.shape[-2:]) != (H, W): raise ValueError(f'tensors[{i}]: expected (..., {H}, {W}), got {tuple(t.shape)}')
        ts.append(t)
    outs = [torch.empty((*t.shape[:-2], oh, ow), device=t.device, dtype=torch.float32) for t in ts]
    Kc = Ko = None
    if K is not None:
        Kc = _check('K', K.detach())
        if tuple(Kc.shape[-2:]) != (4, 4): raise ValueError(f'K must be (..., 4, 4), got {tuple(K.shape)}')
        Ko = torch.empty_like(Kc)
    call('smd_crop_resize', _ptrs(ts), _ptrs(outs), int_array([t.numel()//(H*W) for t in ts]), len(ts), H, W, ch, cw, oh, ow, _ptr(Kc), _ptr(Ko),
         Kc.numel()//16 if Kc is not None else 0, _stream())
    return outs, Ko


def lane_shift_selftest(device='cuda'):
    """Returns (left, right): left[l] = l-1 (0 at lane 0), right[l] = l+1 (0 at lane 63) if the DPP wave shifts that the
    stencil kernels rely on behave as documented."""
    left = torch.empty(64, device=device, dtype=torch.float32); right = torch.empty_like(left)
    call('smd_debug_lane_shift', left.data_ptr(), right.data_ptr(), _stream())
    return left, right
