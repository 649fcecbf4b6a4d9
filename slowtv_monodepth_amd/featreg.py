"""FeatDepth's two feature regularisers as ONE `torch.autograd.Function` over `smd_feat_regs_*` (csrc/smd_featreg.hip): `FeatPeakReg` and `FeatSmoothReg`
(src/regularizers/smooth.py:100-176) read the same features and the same image, so one sweep forward and one backward serve both, for one feature map or a
whole pyramid (`mean_s(loss_s / 2**s)`, src/core/handlers.py:304-305) in one launch.  `plain_feat_regs` is the same computation on the plain regularisers
(`regularizers/feature.py`) and is what CPU tensors, other dtypes than float32 and empty tensors run.  `handlers.feat_smooth` is the caller; the names stay
out of `functional.__all__` (this operator's gradient-subset and hostile-memory cases live in its own test file)."""
from __future__ import annotations

import torch

from ._device import _check, _on, _ptr, _ptrs, _stream, call
from ._lib import MAX_SCALES, int_array, lib

__all__ = ['feat_regs', 'feat_regs_pyramid', 'plain_feat_regs']

PEAKY_EDGES, SMOOTH_EDGES, PEAKY, SMOOTH = 0x1, 0x2, 0x4, 0x8      # SMD_FEATREG_*


def plain_feat_regs(feats, imgs, peaky_edges: bool, smooth_edges: bool, want_peaky: bool = True, want_smooth: bool = True):
    """The per-scale loop over the plain regularisers: -> (mean_s(peaky_s / 2**s) | None, mean_s(smooth_s / 2**s) | None)."""
    from .regularizers import FeatPeakReg, FeatSmoothReg
    out = []
    for want, crit in ((want_peaky, FeatPeakReg(peaky_edges)), (want_smooth, FeatSmoothReg(smooth_edges))):
        out.append(torch.stack([crit(f, i)[0]/2**s for s, (f, i) in enumerate(zip(feats, imgs))]).mean() if want else None)
    return tuple(out)


class _FeatRegs(torch.autograd.Function):
    """(flags, S, feat_0 .. feat_{S-1}, img_0 .. img_{S-1}) -> (l_peaky, l_smooth), 0-dim each; a loss the flags do not select is 0 and has no gradient."""
    @staticmethod
    def forward(ctx, flags, S, *ts):
        feats = [_check(f'feat[{s}]', t, align=False) for s, t in enumerate(ts[:S])]
        B = feats[0].shape[0]
        imgs = [_check(f'img[{s}]', t, (B, 3, *feats[s].shape[-2:]), align=False) for s, t in enumerate(ts[S:])]
        dev = feats[0].device
        dims = [int_array([f.shape[d] for f in feats]) for d in (1, 2, 3)]
        nbytes = lib.smd_feat_regs_workspace_bytes(*dims, S, B)
        if nbytes == 0: raise ValueError(f'feat_regs: a level of 2^31 elements or more ({[tuple(f.shape) for f in feats]})')
        ws = torch.empty(nbytes//8, device=dev, dtype=torch.float64)      # the blocks' fp64 sums (a float64 tensor: its base is 8-byte aligned wherever it comes from)
        l_p, l_s = torch.empty((), device=dev, dtype=torch.float32), torch.empty((), device=dev, dtype=torch.float32)
        call('smd_feat_regs_fwd', _ptrs(feats), _ptrs(imgs), *dims, S, B, flags, l_p.data_ptr(), l_s.data_ptr(), ws.data_ptr(), nbytes, _stream())
        ctx.cfg = (flags, S, B)
        ctx.save_for_backward(*feats, *imgs)
        ctx.set_materialize_grads(False)
        return l_p, l_s

    @staticmethod
    def backward(ctx, g_p, g_s):
        flags, S, B = ctx.cfg
        need = ctx.needs_input_grad[2:2 + S]
        if not flags & PEAKY: g_p = None
        if not flags & SMOOTH: g_s = None
        if not any(need) or (g_p is None and g_s is None): return (None,)*(2 + 2*S)
        feats, imgs = ctx.saved_tensors[:S], ctx.saved_tensors[S:]
        _on(feats[0])
        g_p, g_s = (_check(n, g, (), align=False) if g is not None else None for n, g in (('grad(l_peaky)', g_p), ('grad(l_smooth)', g_s)))
        dims = [int_array([f.shape[d] for f in feats]) for d in (1, 2, 3)]
        g_feats = [torch.empty_like(f) for f in feats]      # (a level nobody asks about is written too: the levels' coefficients depend on their position)
        call('smd_feat_regs_bwd', _ptrs(feats), _ptrs(imgs), _ptr(g_p), _ptr(g_s), _ptrs(g_feats), *dims, S, B, flags, _stream())
        return (None, None, *[g if n else None for g, n in zip(g_feats, need)], *(None,)*S)


def _operands(feats, imgs):
    for s, (f, i) in enumerate(zip(feats, imgs)):
        for n, t in ((f'feat[{s}]', f), (f'img[{s}]', i)):
            if not isinstance(t, torch.Tensor): raise TypeError(f'{n} must be a Tensor, got {type(t)}')
        if f.ndim != 4: raise ValueError(f'feat[{s}]: expected (b,c,h,w), got {tuple(f.shape)}')
        if tuple(i.shape) != (f.shape[0], 3, *f.shape[-2:]): raise ValueError(f'img[{s}]: expected shape {(f.shape[0], 3, *f.shape[-2:])} (the image resized to the features), got {tuple(i.shape)}')
        if f.shape[0] != feats[0].shape[0]: raise ValueError(f'the levels of a pyramid share the batch size, got {[t.shape[0] for t in feats]}')
        if i.requires_grad: raise ValueError(f'img[{s}] must not require a gradient: the regularisers\' image term has no adjoint here')


def _served(feats, imgs) -> bool:
    """The kernel's operands: float32 on one GPU, nothing empty, at most MAX_SCALES levels."""
    dev = feats[0].device
    return len(feats) <= MAX_SCALES and all(t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.numel() > 0 for t in (*feats, *imgs))


def feat_regs_pyramid(feats, imgs, peaky_edges: bool, smooth_edges: bool, want_peaky: bool = True, want_smooth: bool = True):
    """Both regularisers over a pyramid in ONE launch: feats [(b,c_s,h_s,w_s)], imgs [(b,3,h_s,w_s)] (the image resized to every level, no gradient)
    -> (mean_s(peaky_s / 2**s), mean_s(smooth_s / 2**s)), 0-dim float32 each; None for a loss that is not wanted.  Differentiable in the features."""
    feats, imgs = list(feats), list(imgs)
    if not feats or len(feats) != len(imgs): raise ValueError(f'Non-matching pyramids. ({len(feats)} feature levels vs. {len(imgs)} image levels)')
    if not (want_peaky or want_smooth): raise ValueError('nothing to compute: neither loss is wanted')
    _operands(feats, imgs)
    if not _served(feats, imgs): return plain_feat_regs(feats, imgs, peaky_edges, smooth_edges, want_peaky, want_smooth)
    flags = (PEAKY if want_peaky else 0) | (SMOOTH if want_smooth else 0) | (PEAKY_EDGES if peaky_edges and want_peaky else 0) | (SMOOTH_EDGES if smooth_edges and want_smooth else 0)
    l_p, l_s = _FeatRegs.apply(flags, len(feats), *feats, *imgs)
    return (l_p if want_peaky else None), (l_s if want_smooth else None)


def feat_regs(feat: torch.Tensor, img: torch.Tensor, peaky_edges: bool, smooth_edges: bool, want_peaky: bool = True, want_smooth: bool = True):
    """`FeatPeakReg(peaky_edges)(feat, img)[0]` and `FeatSmoothReg(smooth_edges)(feat, img)[0]` (src/regularizers/smooth.py:100-176) in one pass:
    feat (b,c,h,w), img (b,3,h,w) -> (l_peaky, l_smooth).  float32 on the GPU runs `smd_feat_regs_*`; CPU tensors, other dtypes and empty tensors run
    the plain regularisers."""
    return feat_regs_pyramid([feat], [img], peaky_edges, smooth_edges, want_peaky, want_smooth)
