"""FeatDepth's feature-metric reconstruction loss as ONE `torch.autograd.Function` over `smd_feat_recon_*` (csrc/smd_featrecon.hip): what `handlers.feat_recon`
(src/core/handlers.py:70-119) computes — the features up-sampled to the depth map, the supports warped, the dense l1 / l2 error, the automask and the reduction
over the supports — from the LOW-resolution features, without the up-sampled (1 + n, b, C, H, W) tensors, the (n, b, C, H, W) warp (unless the image logger asks
for it) and what autograd keeps for their backward.  The features are detached in the reference, so the gradient goes to the depth and the poses only.
`handlers.feat_recon_fused` is the caller; `handlers.feat_recon` (the reference's structure on the un-fused operators) is what everything `served` declines runs.
The names stay out of `functional.__all__` (this operator's gradient-subset, hostile-memory and value-edge cases live in its own test file)."""
from __future__ import annotations

import torch

from . import _lib
from ._device import _check, _on, _ptr, _stream, call
from ._lib import FLAGS, MAX_SUPPORTS

__all__ = ['feat_recon_loss', 'feat_recon_fused', 'served']


class _FeatRecon(torch.autograd.Function):
    """(depth (b,1,H,W), feats (b,C,hf,wf), supp (n,b,C,hf,wf), Ts (n,b,4,4), K, K_inv (b,4,4), noise (b,1,H,W) | None, seed, flags, want_warp)
    -> (loss (), sel (b,1,H,W) uint8, warp (n,b,C,H,W) | None); differentiable in `depth` and `Ts`."""
    @staticmethod
    def forward(ctx, depth, feats, supp, Ts, K, K_inv, noise, seed, flags, want_warp):
        b, _, H, W = depth.shape
        n, _, C, hf, wf = supp.shape
        depth = _check('depth', depth, (b, 1, H, W), align=False); feats = _check('feats', feats, (b, C, hf, wf), align=False)
        supp = _check('supp_feats', supp, (n, b, C, hf, wf), align=False); Ts = _check('Ts', Ts, (n, b, 4, 4), align=False)
        K = _check('K', K, (b, 4, 4), align=False); K_inv = _check('K_inv', K_inv, (b, 4, 4), align=False)
        if noise is not None: noise = _check('noise', noise, (b, 1, H, W), align=False)
        dev = depth.device
        dims = (b, n, C, H, W, hf, wf)
        nbytes = _lib.lib.smd_feat_recon_workspace_bytes(*dims)
        if nbytes == 0: raise ValueError(f'feat_recon_loss: sizes that are not served (b, n, C, H, W, hf, wf) = {dims}')
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)      # the blocks' fp64 sums (the backward allocates its own, with the pose sums behind them)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        sel = torch.empty((b, 1, H, W), device=dev, dtype=torch.uint8)
        warp = torch.empty((n, b, C, H, W), device=dev, dtype=torch.float32) if want_warp else None
        call('smd_feat_recon_fwd', depth.data_ptr(), feats.data_ptr(), supp.data_ptr(), Ts.data_ptr(), K.data_ptr(), K_inv.data_ptr(), _ptr(noise),
             int(seed) & (2**64 - 1), loss.data_ptr(), sel.data_ptr(), _ptr(warp), ws.data_ptr(), nbytes, *dims, int(flags), _stream())
        ctx.save_for_backward(depth, feats, supp, Ts, K, K_inv, sel)
        ctx.cfg = (dims, int(flags), nbytes)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(sel)
        if warp is not None: ctx.mark_non_differentiable(warp)
        return loss, sel, warp

    @staticmethod
    def backward(ctx, g_loss, _g_sel, _g_warp):
        need_d, need_T = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        if g_loss is None or not (need_d or need_T): return (None,)*10
        depth, feats, supp, Ts, K, K_inv, sel = ctx.saved_tensors
        dev = _on(depth)
        dims, flags, nbytes = ctx.cfg
        b, n = dims[:2]
        g_loss = _check('grad(loss)', g_loss, (), align=False)
        g_depth = torch.empty_like(depth) if need_d else None
        g_T = torch.empty((n, b, 4, 4), device=dev, dtype=torch.float32) if need_T else None
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)
        call('smd_feat_recon_bwd', depth.data_ptr(), feats.data_ptr(), supp.data_ptr(), Ts.data_ptr(), K.data_ptr(), K_inv.data_ptr(), sel.data_ptr(), g_loss.data_ptr(),
             _ptr(g_depth), _ptr(g_T), ws.data_ptr(), nbytes, *dims, flags, _stream())
        return g_depth, None, None, g_T, None, None, None, None, None, None


def _operands(depth, feats, supp_feats, Ts, K, K_inv, noise):
    """The refusals that need no device: types, ranks, matching sizes, dtypes, who may require a gradient."""
    named = (('depth', depth), ('feats', feats), ('supp_feats', supp_feats), ('Ts', Ts), ('K', K)) + ((('K_inv', K_inv),) if K_inv is not None else ()) + \
        ((('noise', noise),) if noise is not None else ())
    for name, t in named:
        if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    if depth.ndim != 4 or depth.shape[1] != 1: raise ValueError(f'depth: expected (b,1,H,W), got {tuple(depth.shape)}')
    b, _, H, W = depth.shape
    if feats.ndim != 4 or feats.shape[0] != b: raise ValueError(f'feats: expected (b,C,hf,wf) with b = {b}, got {tuple(feats.shape)}')
    C, hf, wf = feats.shape[1:]
    if supp_feats.ndim != 5 or tuple(supp_feats.shape[1:]) != (b, C, hf, wf): raise ValueError(f'supp_feats: expected (n,{b},{C},{hf},{wf}), got {tuple(supp_feats.shape)}')
    n = supp_feats.shape[0]
    if not 1 <= n <= MAX_SUPPORTS: raise ValueError(f'supp_feats: {n} supports, the operator takes 1..{MAX_SUPPORTS}')
    if hf > H or wf > W: raise ValueError(f'features larger than the depth map ({hf}x{wf} vs. {H}x{W}): the operator up-samples')
    if tuple(Ts.shape) != (n, b, 4, 4): raise ValueError(f'Ts: expected shape {(n, b, 4, 4)}, got {tuple(Ts.shape)}')
    for name, t in (('K', K), ('K_inv', K_inv)):
        if t is not None and tuple(t.shape) != (b, 4, 4): raise ValueError(f'{name}: expected shape {(b, 4, 4)}, got {tuple(t.shape)}')
    if noise is not None and tuple(noise.shape) != (b, 1, H, W): raise ValueError(f'noise: expected shape {(b, 1, H, W)}, got {tuple(noise.shape)}')
    for name, t in named:
        if t.dtype != torch.float32: raise TypeError(f'{name} must be float32 (the loss path is fp32 only), got {t.dtype}')
    for name, t in (('feats', feats), ('supp_feats', supp_feats), ('K', K), ('K_inv', K_inv), ('noise', noise)):
        if t is not None and t.requires_grad:
            raise ValueError(f'{name} must not require a gradient: the features are detached (handlers.py:102-110) and learned intrinsics run `handlers.feat_recon`')


def feat_recon_loss(depth, feats, supp_feats, Ts, K, K_inv=None, *, loss_name: str, use_min: bool, use_automask: bool, noise=None, seed: int = 0, want_warp: bool = False):
    """depth (b,1,H,W), feats (b,C,hf,wf), supp_feats (n,b,C,hf,wf) at any resolution up to the depth map's, Ts (n,b,4,4), K [, K_inv] (b,4,4)
    -> (loss, sel (b,1,H,W) uint8: the winning support, 255 where the automask removed the pixel, warp (n,b,C,H,W) | None).

    `ReconstructionLoss(loss_name, use_min, use_automask)` of the supports' up-sampled features warped into the target view against the target's up-sampled
    features; `loss_name` 'l1' | 'l2'.  `noise` (b,1,H,W) replaces the automask's tie-break draw, else `seed` selects it (equal seeds: `functional.recon_reduce`'s
    noise).  Differentiable in `depth` and `Ts`; float32 GPU tensors only."""
    if loss_name not in ('l1', 'l2'): raise KeyError(loss_name)
    _operands(depth, feats, supp_feats, Ts, K, K_inv, noise)
    if K_inv is None:
        from . import functional as F
        K_inv = F.inv_intrinsics(K)
    flags = (FLAGS['loss_l1'] if loss_name == 'l1' else FLAGS['loss_l2']) | (FLAGS['use_min'] if use_min else 0) | (FLAGS['use_automask'] if use_automask else 0)
    return _FeatRecon.apply(depth, feats, supp_feats, Ts, K, K_inv, noise, seed, flags, bool(want_warp))


def served(crit, depths, masks, feats, supp_feats, Ts, Ks) -> bool:
    """What `feat_recon_fused` runs on the kernel: a plain `ReconstructionLoss` ('l1' | 'l2', no predictive mask) on float32 tensors of one GPU, fixed intrinsics,
    features no larger than the depth map, sizes `smd_feat_recon_workspace_bytes` accepts.  (`feats` / `supp_feats`: the 1/4-scale tensors, any float dtype.)"""
    from .losses import ReconstructionLoss
    if type(crit) is not ReconstructionLoss or crit.loss_name not in ('l1', 'l2') or crit.mask_name or masks is not None: return False
    depth = depths[0]
    ts = (depth, feats, supp_feats, Ts, Ks)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == depth.device and t.numel() > 0 for t in ts): return False
    if not all(t.dtype == torch.float32 for t in (depth, Ts, Ks)) or not feats.is_floating_point() or not supp_feats.is_floating_point(): return False
    if Ks.requires_grad or depth.ndim != 4 or feats.ndim != 4 or supp_feats.ndim != 5: return False
    b, n = depth.shape[0], supp_feats.shape[0]
    C, hf, wf = feats.shape[1:]
    if depth.shape[1] != 1 or feats.shape[0] != b or tuple(supp_feats.shape[1:]) != (b, C, hf, wf) or tuple(Ts.shape) != (n, b, 4, 4) or tuple(Ks.shape) != (b, 4, 4): return False
    return _lib.lib.smd_feat_recon_workspace_bytes(b, n, C, *depth.shape[-2:], hf, wf) > 0


def feat_recon_fused(crit, synth, depths: dict, masks, feats, supp_feats, Ts, Ks, *, noise=None, want_warp: bool = True):
    """`handlers.feat_recon` with the same signature and return value, on `smd_feat_recon_*`: (loss, {'supp_feats_warp': (n,b,c,h,w)} if `want_warp` else {}).
    What `served` declines runs `handlers.feat_recon`.  No shape is routed to the plain handler by a timing rule: none lost to it (profiles/featrecon_times.txt)."""
    from . import handlers
    if isinstance(feats, (list, tuple)): feats, supp_feats = feats[-4], supp_feats[-4]
    if not served(crit, depths, masks, feats, supp_feats, Ts, Ks): return handlers.feat_recon(crit, synth, depths, masks, feats, supp_feats, Ts, Ks, noise=noise)
    feats, supp_feats = feats.detach().float(), supp_feats.detach().float()      # at the low resolution: 1/16 of what the plain handler converts
    loss, _, warp = feat_recon_loss(depths[0], feats, supp_feats, Ts, Ks, loss_name=crit.loss_name, use_min=crit.use_min, use_automask=crit.use_automask, noise=noise,
                                    seed=crit.next_seed(), want_warp=want_warp)
    return loss, ({'supp_feats_warp': warp} if want_warp else {})
