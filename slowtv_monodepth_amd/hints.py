"""The Depth-Hints proxy-depth regression as ONE `torch.autograd.Function` over `smd_hints_regr_*` (csrc/smd_hints.hip): the loss of `handlers.depth_regr`
(src/core/handlers.py:201-259) over every scale without expanding the depths, the hints or the mask to (S*b, ...), the mask built in the same sweep from the
hints and, for `RegressionLoss(use_automask=True)`, from the photometric errors of the supports warped by the prediction and by the hints.  Those errors come
from one call of the fused reconstruction forward on the stack [hints, depth_0 .. depth_{S-1}] (`depth_regr_fused`): no warp is written, and the hints' error
is computed once, not once per scale.  `handlers.depth_regr_fused` is the caller; `handlers.depth_regr` (the reference's structure on the un-fused operators)
is what CPU tensors, other dtypes and criteria the fused forward does not serve run.  The names stay out of `functional.__all__` (this operator's
gradient-subset, hostile-memory and value-edge cases live in its own test file)."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _stream, call
from ._lib import MAX_SCALES, REGR_FLAGS

__all__ = ['hints_regr', 'hints_photo_errors', 'depth_regr_fused', 'served']


class _HintsRegr(torch.autograd.Function):
    """(depth (S,b,h,w), hints (b,h,w), err (S+1,b,h,w) | None, flags) -> (loss (), mask0 (b,1,h,w) bool); differentiable in `depth` only."""
    @staticmethod
    def forward(ctx, depth, hints, err, flags):
        if depth.ndim != 4: raise ValueError(f'depth: expected (S,b,h,w), got {tuple(depth.shape)}')
        S, b, h, w = depth.shape
        if not 1 <= S <= MAX_SCALES: raise ValueError(f'depth: {S} scales, the operator takes 1..{MAX_SCALES}')
        depth = _check('depth', depth, align=False); hints = _check('hints', hints, (b, h, w), align=False)
        if bool(flags & REGR_FLAGS['automask']) != (err is not None): raise ValueError('err goes with the automask flag')
        if err is not None: err = _check('err', err, (S + 1, b, h, w), align=False)
        dev = depth.device
        nbytes = _lib.lib.smd_hints_regr_workspace_bytes(S, b, h, w)
        if nbytes == 0: raise ValueError(f'hints_regr: sizes that are not served {(S, b, h, w)} (every size >= 1, b*h*w < 2^31)')
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)      # the blocks' fp64 sums
        loss = torch.empty((), device=dev, dtype=torch.float32)
        mask0 = torch.empty((b, 1, h, w), device=dev, dtype=torch.uint8)
        bits = torch.empty((b*h*w + 3)//4, device=dev, dtype=torch.int32)
        stats = torch.zeros(8, device=dev, dtype=torch.float32)
        call('smd_hints_regr_fwd', depth.data_ptr(), hints.data_ptr(), err.data_ptr() if err is not None else None, S, b, h, w, int(flags), loss.data_ptr(),
             mask0.data_ptr(), bits.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, _stream())
        ctx.save_for_backward(depth, hints, bits, stats); ctx.flags = int(flags)
        mask0 = mask0.view(torch.bool)
        ctx.mark_non_differentiable(mask0)
        return loss, mask0

    @staticmethod
    def backward(ctx, g_loss, _g_mask):
        if not ctx.needs_input_grad[0]: return None, None, None, None
        depth, hints, bits, stats = ctx.saved_tensors
        _on(depth)
        S, b, h, w = depth.shape
        g_loss = _check('grad(loss)', g_loss, (), align=False)
        g_depth = torch.empty_like(depth)
        call('smd_hints_regr_bwd', depth.data_ptr(), hints.data_ptr(), bits.data_ptr(), stats.data_ptr(), g_loss.data_ptr(), g_depth.data_ptr(), S, b, h, w, ctx.flags,
             _stream())
        return g_depth, None, None, None


def hints_regr(depth: torch.Tensor, hints: torch.Tensor, err: torch.Tensor | None = None, *, loss_name: str = 'log_l1', invert: bool = False):
    """depth (S,b,h,w) | (S,b,1,h,w), hints (b,h,w) | (b,1,h,w) (0 = no hint), err None or (S+1,b,h,w) | (S+1,b,1,h,w) photometric errors ([0]: under the
    hints, [1+s]: under depth[s]) -> (loss, mask0 (b,1,h,w) bool): the masked mean of `loss_name`'s error over m = hints > 0 [& err[1+s] > err[0]], and the
    mask of scale 0.  float32 GPU tensors only (`_check` refuses anything else); neither `hints` nor `err` may require a gradient."""
    if loss_name not in ('l1', 'log_l1', 'berhu'): raise KeyError(loss_name)
    for n, t in (('hints', hints), ('err', err)):
        if t is not None and t.requires_grad: raise ValueError(f'{n} must not require a gradient: the mask is a comparison and the hints are a target')
    if depth.ndim == 5: depth = depth.squeeze(2)
    if hints.ndim == 4: hints = hints.squeeze(1)
    if err is not None and err.ndim == 5: err = err.squeeze(2)
    flags = REGR_FLAGS[loss_name] | (REGR_FLAGS['invert'] if invert else 0) | (REGR_FLAGS['automask'] if err is not None else 0)
    return _HintsRegr.apply(depth, hints, err, flags)


def hints_photo_errors(photo_crit, depth: torch.Tensor, hints: torch.Tensor, imgs, supp_imgs, Ts, Ks) -> torch.Tensor:
    """-> (S+1,b,1,h,w): `photo_crit.compute_photo(warp, imgs)` of the supports warped by the hints ([0]) and by every scale of `depth` (S,b,h,w) ([1+s]), from
    the fused reconstruction forward on the stack [hints, depth_0 ..] (no warp written, no automask, nothing differentiable).  More slices than one call
    takes: two calls."""
    from . import functional as F
    flags = F.recon_flags(photo_crit.loss_name, photo_crit.use_min, False)
    with torch.no_grad():
        stack = torch.cat((hints.reshape(1, *depth.shape[1:]), depth.detach()))
        K_inv = F.inv_intrinsics(Ks)
        errs = [F.image_recon_fused(part, imgs, supp_imgs, Ts, Ks, K_inv, flags=flags, want_err=True, want_warp=False)[1]
                for part in (stack.split(MAX_SCALES) if stack.shape[0] > MAX_SCALES else (stack,))]
        return errs[0] if len(errs) == 1 else torch.cat(errs)


def served(crit, photo, depths, targets, imgs, supp_imgs, Ts, Ks) -> bool:
    """What `depth_regr_fused` runs on the kernel: float32 tensors on one GPU, at most MAX_SCALES scales, nothing empty; and with the automask a `photo` that is
    the bound `compute_photo` of a plain `ReconstructionLoss` ('ssim' | 'l1', no predictive mask) on 3-channel images, with poses and intrinsics that take
    no gradient (the mask is a comparison either way)."""
    from .losses import ReconstructionLoss, RegressionLoss
    if type(crit) is not RegressionLoss: return False
    ds = list(depths.values())
    ts = [*ds, targets] + ([imgs, supp_imgs, Ts, Ks] if crit.use_automask else [])
    dev = targets.device
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.numel() > 0 for t in ts): return False
    if not 1 <= len(ds) <= MAX_SCALES or targets.ndim != 4 or targets.shape[1] != 1 or any(tuple(d.shape) != tuple(targets.shape) for d in ds): return False
    if targets.requires_grad: return False
    if crit.use_automask:
        owner = getattr(photo, '__self__', None)
        if type(owner) is not ReconstructionLoss or getattr(photo, '__func__', None) is not ReconstructionLoss.compute_photo: return False
        if owner.loss_name not in ('ssim', 'l1') or owner.mask_name: return False
        if imgs.ndim != 4 or imgs.shape[1] != 3 or supp_imgs.ndim != 5 or supp_imgs.shape[2] != 3 or supp_imgs.shape[0] < 1: return False
        if Ts.requires_grad or Ks.requires_grad: return False
    return True


def depth_regr_fused(crit, synth, photo, depths: dict, targets, imgs, supp_imgs, Ts, Ks):
    """`handlers.depth_regr` with the same signature and return value, on `smd_hints_regr_*`: (loss, {'mask_regr': (b,1,h,w) bool of scale 0}).  What `served`
    declines runs `handlers.depth_regr`.  No shape is routed to the plain handler by a timing rule: none lost to it (profiles/hints_times.txt)."""
    from . import handlers
    if not served(crit, photo, depths, targets, imgs, supp_imgs, Ts, Ks): return handlers.depth_regr(crit, synth, photo, depths, targets, imgs, supp_imgs, Ts, Ks)
    stacked = getattr(depths, 'stacked', None)
    if stacked is None: stacked = torch.stack(list(depths.values()))
    depth = stacked.squeeze(2)
    hints = targets.detach().squeeze(1)
    err = hints_photo_errors(photo.__self__, depth, hints, imgs, supp_imgs, Ts.detach(), Ks.detach()) if crit.use_automask else None
    loss, mask0 = hints_regr(depth, hints, err, loss_name=crit.loss_name, invert=crit.invert)
    return loss, {'mask_regr': mask0}
