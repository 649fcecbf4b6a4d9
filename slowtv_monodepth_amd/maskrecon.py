"""The image reconstruction loss with a predictive weighting mask (SfM-Learner's explainability mask, Klodt's uncertainty) as ONE `torch.autograd.Function` over
`smd_mask_recon_*` (csrc/smd_maskrecon.hip): what `handlers.image_recon` (src/core/handlers.py:14-67) computes for a criterion built with `mask_name` — every
support warped at every scale, the photometric error of the warps and of the un-warped supports, the mask on the per-support errors, the reduction over the
supports, the automask and the mean — without the (n, S*b, 3, h, w) warps, the two (n, S*b, h, w) error stacks and what autograd keeps for their backward.
The gradient goes to the depth, the mask and the poses.  `handlers.image_recon_masked_fused` is the caller (`HipLossBackend.image_recon` reaches it when masks are
given); `handlers.image_recon` (the reference's structure on the un-fused operators) is what everything `served` declines runs.
The names stay out of `functional.__all__` (this operator's gradient-subset, hostile-memory and value-edge cases live in its own test file)."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, call
from ._lib import FLAGS, MAX_SCALES, MAX_SUPPORTS

__all__ = ['mask_recon_loss', 'image_recon_masked_fused', 'served']

MAX_SIDE = 2048      # frames up to this many pixels a side (smd_maskrecon.hip: mask_recon_sizes_ok)


class _MaskRecon(torch.autograd.Function):
    """(depth (S,b,h,w), mask (S,b,n,h,w), tgt (b,3,h,w), supp (n,b,3,h,w), Ts (n,b,4,4), K, K_inv (b,4,4), noise (S,b,h,w) | None, seed, flags, want_warp)
    -> (loss (), sel (S,b,h,w) uint8, stat (S,b,h,w) uint8 | None, warp0 (n,b,3,h,w) | None); differentiable in `depth`, `mask` and `Ts`."""
    @staticmethod
    def forward(ctx, depth, mask, tgt, supp, Ts, K, K_inv, noise, seed, flags, want_warp):
        S, b, h, w = depth.shape
        n = supp.shape[0]
        depth = _check('depth', depth, (S, b, h, w), align=False); mask = _check('mask', mask, (S, b, n, h, w), align=False)
        tgt = _check('imgs', tgt, (b, 3, h, w), align=False); supp = _check('supp_imgs', supp, (n, b, 3, h, w), align=False)
        Ts = _check('Ts', Ts, (n, b, 4, 4), align=False); K = _check('K', K, (b, 4, 4), align=False); K_inv = _check('K_inv', K_inv, (b, 4, 4), align=False)
        if noise is not None: noise = _check('noise', noise, (S, b, h, w), align=False)
        dev = depth.device
        dims = (S, b, n, h, w)
        nbytes = _lib.lib.smd_mask_recon_workspace_bytes(*dims)
        if nbytes == 0: raise ValueError(f'mask_recon_loss: sizes that are not served (S, b, n, h, w) = {dims}')
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)      # the blocks' fp64 sums (the backward allocates its own, with the pose sums behind them)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        sel = torch.empty((S, b, h, w), device=dev, dtype=torch.uint8)
        both = (flags & FLAGS['use_min']) and (flags & FLAGS['use_automask'])
        stat = torch.empty((S, b, h, w), device=dev, dtype=torch.uint8) if both else None      # the static winner: the backward reads decisions, it never re-decides
        warp = torch.empty((n, b, 3, h, w), device=dev, dtype=torch.float32) if want_warp else None
        call('smd_mask_recon_fwd', depth.data_ptr(), mask.data_ptr(), tgt.data_ptr(), supp.data_ptr(), Ts.data_ptr(), K.data_ptr(), K_inv.data_ptr(), _ptr(noise),
             int(seed) & (2**64 - 1), loss.data_ptr(), sel.data_ptr(), _ptr(stat), _ptr(warp), ws.data_ptr(), nbytes, *dims, int(flags), _stream())
        ctx.save_for_backward(depth, mask, tgt, supp, Ts, K, K_inv, sel, stat)
        ctx.cfg = (dims, int(flags), nbytes)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (sel, stat, warp) if t is not None))
        return loss, sel, stat, warp

    @staticmethod
    def backward(ctx, g_loss, _g_sel, _g_stat, _g_warp):
        need_d, need_m, need_T = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]
        if g_loss is None or not (need_d or need_m or need_T): return (None,)*11
        depth, mask, tgt, supp, Ts, K, K_inv, sel, stat = ctx.saved_tensors
        dev = _on(depth)
        dims, flags, nbytes = ctx.cfg
        S, b, n = dims[:3]
        g_loss = _check('grad(loss)', g_loss, (), align=False)
        g_depth = torch.empty_like(depth) if need_d else None
        g_mask = torch.empty_like(mask) if need_m else None
        g_T = torch.empty((n, b, 4, 4), device=dev, dtype=torch.float32) if need_T else None
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)
        call('smd_mask_recon_bwd', depth.data_ptr(), mask.data_ptr(), tgt.data_ptr(), supp.data_ptr(), Ts.data_ptr(), K.data_ptr(), K_inv.data_ptr(), sel.data_ptr(),
             _ptr(stat), g_loss.data_ptr(), _ptr(g_depth), _ptr(g_mask), _ptr(g_T), ws.data_ptr(), nbytes, *dims, flags, _stream())
        return g_depth, g_mask, None, None, g_T, None, None, None, None, None, None


def _operands(depth, mask, imgs, supp_imgs, Ts, K, K_inv, noise):
    """The refusals that need no device: types, ranks, matching sizes, dtypes, who may require a gradient."""
    named = (('depth', depth), ('mask', mask), ('imgs', imgs), ('supp_imgs', supp_imgs), ('Ts', Ts), ('K', K)) + ((('K_inv', K_inv),) if K_inv is not None else ()) + \
        ((('noise', noise),) if noise is not None else ())
    for name, t in named:
        if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    if depth.ndim != 4: raise ValueError(f'depth: expected (S,b,h,w) or (S,b,1,h,w), got {tuple(depth.shape)}')
    S, b, h, w = depth.shape
    if not 1 <= S <= MAX_SCALES: raise ValueError(f'depth: {S} scales, the operator takes 1..{MAX_SCALES}')
    if tuple(imgs.shape) != (b, 3, h, w): raise ValueError(f'imgs: expected shape {(b, 3, h, w)}, got {tuple(imgs.shape)}')
    if supp_imgs.ndim != 5 or tuple(supp_imgs.shape[1:]) != (b, 3, h, w): raise ValueError(f'supp_imgs: expected (n,{b},3,{h},{w}), got {tuple(supp_imgs.shape)}')
    n = supp_imgs.shape[0]
    if not 1 <= n <= MAX_SUPPORTS: raise ValueError(f'supp_imgs: {n} supports, the operator takes 1..{MAX_SUPPORTS}')
    if tuple(mask.shape) != (S, b, n, h, w): raise ValueError(f'mask: expected shape {(S, b, n, h, w)} (one channel per support), got {tuple(mask.shape)}')
    if tuple(Ts.shape) != (n, b, 4, 4): raise ValueError(f'Ts: expected shape {(n, b, 4, 4)}, got {tuple(Ts.shape)}')
    for name, t in (('K', K), ('K_inv', K_inv)):
        if t is not None and tuple(t.shape) != (b, 4, 4): raise ValueError(f'{name}: expected shape {(b, 4, 4)}, got {tuple(t.shape)}')
    if noise is not None and tuple(noise.shape) != (S, b, h, w): raise ValueError(f'noise: expected shape {(S, b, h, w)}, got {tuple(noise.shape)}')
    for name, t in named:
        if t.dtype != torch.float32: raise TypeError(f'{name} must be float32 (the loss path is fp32 only), got {t.dtype}')
    for name, t in (('imgs', imgs), ('supp_imgs', supp_imgs), ('K', K), ('K_inv', K_inv), ('noise', noise)):
        if t is not None and t.requires_grad:
            raise ValueError(f'{name} must not require a gradient: the operator differentiates the depth, the mask and the poses (learned intrinsics run `handlers.image_recon`)')


def mask_recon_loss(depth, mask, imgs, supp_imgs, Ts, K, K_inv=None, *, loss_name: str, use_min: bool, use_automask: bool, mask_name: str, noise=None, seed: int = 0,
                    want_warp: bool = False):
    """depth (S,b,h,w) | (S,b,1,h,w), mask (S,b,n,h,w), imgs (b,3,h,w), supp_imgs (n,b,3,h,w), Ts (n,b,4,4), K [, K_inv] (b,4,4)
    -> (loss, sel (S,b,h,w) uint8: the winning support, 255 where the automask removed the pixel, stat (S,b,h,w) uint8 | None: the support whose masked static
    error is the smallest (with `use_min` and `use_automask` together), warp0 (n,b,3,h,w) | None: the warps of scale 0).

    `ReconstructionLoss(loss_name, use_min, use_automask, mask_name)` of the supports warped into the target view at every scale; `loss_name` 'ssim' | 'l1',
    `mask_name` 'explainability' | 'uncertainty'.  `noise` (S,b,h,w) replaces the automask's tie-break draw, else `seed` selects it (equal seeds:
    `functional.recon_reduce`'s noise).  Differentiable in `depth`, `mask` and `Ts`; float32 GPU tensors only."""
    if loss_name not in ('ssim', 'l1'): raise KeyError(loss_name)
    if mask_name not in ('explainability', 'uncertainty'): raise ValueError(f'Invalid mask type: {mask_name}')
    if isinstance(depth, torch.Tensor) and depth.ndim == 5 and depth.shape[2] == 1: depth = depth.squeeze(2)
    if isinstance(noise, torch.Tensor) and isinstance(depth, torch.Tensor) and noise.numel() == depth.numel(): noise = noise.reshape(depth.shape)
    _operands(depth, mask, imgs, supp_imgs, Ts, K, K_inv, noise)
    if K_inv is None:
        from . import functional as F
        K_inv = F.inv_intrinsics(K)
    flags = (FLAGS['loss_l1'] if loss_name == 'l1' else 0) | (FLAGS['use_min'] if use_min else 0) | (FLAGS['use_automask'] if use_automask else 0) | \
        FLAGS['mask_explainability' if mask_name == 'explainability' else 'mask_uncertainty']
    return _MaskRecon.apply(depth, mask, imgs, supp_imgs, Ts, K, K_inv, noise, seed, flags, bool(want_warp))


def served(crit, depths, masks, imgs, supp_imgs, Ts, Ks, K_inv=None) -> bool:
    """What `image_recon_masked_fused` runs on the kernel: a plain `ReconstructionLoss` ('ssim' | 'l1') built with `mask_name`, masks given, float32 tensors of one
    GPU, 3-channel images, fixed intrinsics, 1..8 supports and scales, frames up to 2048 a side, masks of the image's size at every scale.  Nothing is launched
    or materialised here: a `LazyDepths` that is still pending is asked for its size only.  No shape is routed to the plain handler by a timing rule (README)."""
    from .losses import ReconstructionLoss
    if type(crit) is not ReconstructionLoss or crit.loss_name not in ('ssim', 'l1') or crit.mask_name not in ('explainability', 'uncertainty') or masks is None: return False
    ts = (imgs, supp_imgs, Ts, Ks) + ((K_inv,) if K_inv is not None else ())
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == imgs.device and t.dtype == torch.float32 and t.numel() > 0 for t in ts): return False
    if Ks.requires_grad or (K_inv is not None and K_inv.requires_grad): return False
    if imgs.ndim != 4 or imgs.shape[1] != 3 or supp_imgs.ndim != 5: return False
    b, _, h, w = imgs.shape
    n = supp_imgs.shape[0]
    if tuple(supp_imgs.shape[1:]) != (b, 3, h, w) or tuple(Ts.shape) != (n, b, 4, 4) or tuple(Ks.shape) != (b, 4, 4): return False
    if K_inv is not None and tuple(K_inv.shape) != (b, 4, 4): return False
    S = len(depths)
    if not (1 <= n <= MAX_SUPPORTS and 1 <= S <= MAX_SCALES and 2 <= h <= MAX_SIDE and 2 <= w <= MAX_SIDE) or len(masks) != S: return False
    if getattr(depths, 'pending', False):      # handlers.LazyDepths before its K0 launch: (b,1,h,w) float32 per scale, on the disparities' device
        d0 = depths.disps[0]
        if tuple(depths.size) != (h, w) or not d0.is_cuda or d0.device != imgs.device or d0.shape[0] != b: return False
    else:
        for d in depths.values():
            if not (isinstance(d, torch.Tensor) and d.is_cuda and d.device == imgs.device and d.dtype == torch.float32 and tuple(d.shape) == (b, 1, h, w)): return False
    for m in masks.values():
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == imgs.device and m.dtype == torch.float32 and tuple(m.shape) == (b, n, h, w)): return False
    return _lib.lib.smd_mask_recon_workspace_bytes(S, b, n, h, w) > 0


def _stacked(d):
    s = getattr(d, 'stacked', None)      # a `ScaleDict` (no copy); a pending `LazyDepths` runs its K0 launch here, as `torch.stack(list(depths.values()))` would
    return s if s is not None else torch.stack(list(d.values()))


def image_recon_masked_fused(crit, synth, depths: dict, masks, imgs, supp_imgs, Ts, Ks, *, K_inv=None, noise=None, want_warp: bool = True, prepared=None):
    """`handlers.image_recon` with the same signature and return value, for a criterion with a predictive mask, on `smd_mask_recon_*`:
    (loss, {'supp_imgs_warp': (n,b,3,h,w) of scale 0 if `want_warp`, 'automask': (b,1,h,w) bool of scale 0 with the automask}).  What `served` declines runs
    `handlers.image_recon`.  `prepared` (the un-masked fused kernels' frame buffer) is accepted and ignored: nothing here reads it."""
    from . import handlers
    if (synth is not None and tuple(synth.shape) != tuple(imgs.shape[-2:])) or not served(crit, depths, masks, imgs, supp_imgs, Ts, Ks, K_inv):
        return handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks, K_inv=K_inv, noise=noise, want_warp=want_warp, prepared=prepared)
    loss, sel, _, warp0 = mask_recon_loss(_stacked(depths), _stacked(masks), imgs, supp_imgs, Ts, Ks, K_inv, loss_name=crit.loss_name,
                                          use_min=crit.use_min, use_automask=crit.use_automask, mask_name=crit.mask_name, noise=noise, seed=crit.next_seed(),
                                          want_warp=want_warp)
    ld = {}
    if crit.use_automask: ld['automask'] = (sel[0] != 255).unsqueeze(1)
    if want_warp: ld['supp_imgs_warp'] = warp0
    return loss, ld
