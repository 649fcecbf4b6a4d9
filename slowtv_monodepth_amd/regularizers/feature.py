"""FeatDepth's feature regularisers (reference: `src/regularizers/smooth.py:100-176`) — registry keys `feat_peaky` and `feat_smooth`.

`forward` is the reference's arithmetic on plain ATen: the CPU path and the parity baseline of the fused operator `featreg.feat_regs`
(csrc/smd_featreg.hip), which `handlers.feat_smooth` calls for fp32 GPU tensors.  The conventions both sides keep:
`compute_grad` appends a ZERO last column / row, and the second-order differences are taken of those padded maps, so `dxx[..., w-2]` is
`|dx[w-2] - 0|` and the last column is 0; `abs` has gradient 0 at 0; the image term is the channel MEAN of the absolute differences (second-order for
`feat_smooth`); `feat_peaky` is negated."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import register

__all__ = ['FeatPeakReg', 'FeatSmoothReg', 'compute_grad', 'compute_laplacian']


def compute_grad(x: torch.Tensor, ch_mean: bool = False):
    """Absolute forward differences in x and y, each padded with a zero last column / row (smooth.py:12-30).  (b,c,h,w) -> two (b,c|1,h,w)."""
    b, c, h, w = x.shape
    dx = torch.cat(((x[..., :, :-1] - x[..., :, 1:]).abs(), x.new_zeros((b, c, h, 1))), dim=-1)
    dy = torch.cat(((x[..., :-1, :] - x[..., 1:, :]).abs(), x.new_zeros((b, c, 1, w))), dim=-2)
    if ch_mean: dx, dy = dx.mean(dim=1, keepdim=True), dy.mean(dim=1, keepdim=True)
    return dx, dy


def compute_laplacian(x: torch.Tensor, ch_mean: bool = False):
    """Absolute second-order differences (xx, yy, xy, yx): `compute_grad` of `compute_grad`'s padded maps (smooth.py:33-48)."""
    dx, dy = compute_grad(x)
    dxx, dxy = compute_grad(dx)
    dyx, dyy = compute_grad(dy)
    if ch_mean: dxx, dyy, dxy, dyx = (d.mean(dim=1, keepdim=True) for d in (dxx, dyy, dxy, dyx))
    return dxx, dyy, dxy, dyx


def _feat_grad(a, b): return (a.pow(2) + b.pow(2)).clamp(min=torch.finfo(a.dtype).eps).sqrt()


@register('feat_peaky')
class FeatPeakReg(nn.Module):
    """Feature gradient peakiness (FeatDepth, https://arxiv.org/abs/2007.10603): the NEGATED mean first-order feature gradient, so that features stay
    discriminative in smooth image regions.  `use_edges`: weighted by `exp(-|image gradient|)`."""
    def __init__(self, use_edges: bool = False):
        super().__init__()
        self.use_edges = use_edges

    def forward(self, feat, img):
        """feat (b,c,h,w), img (b,3,h,w) -> (loss, {'feat_grad': (b,c,h,w)})"""
        dx, dy = compute_grad(feat)
        feat_grad = _feat_grad(dx, dy)
        if self.use_edges:
            ix, iy = compute_grad(img, ch_mean=True)
            dx, dy = dx*(-ix).exp(), dy*(-iy).exp()
        return -(dx.mean() + dy.mean()), {'feat_grad': feat_grad}


@register('feat_smooth')
class FeatSmoothReg(nn.Module):
    """Second-order feature smoothness (FeatDepth): the mean of the four second-order feature gradients.  `use_edges`: each weighted by
    `exp(-|second-order image gradient|)`."""
    def __init__(self, use_edges: bool = False):
        super().__init__()
        self.use_edges = self.edge_aware = use_edges      # (`edge_aware` is the reference's attribute name)

    def forward(self, feat, img):
        """feat (b,c,h,w), img (b,3,h,w) -> (loss, {'feat_grad': (b,c,h,w)})"""
        dxx, dyy, dxy, dyx = compute_laplacian(feat)
        feat_grad = _feat_grad(dxx, dyy)
        if self.use_edges:
            ixx, iyy, ixy, iyx = compute_laplacian(img, ch_mean=True)
            dxx, dyy, dxy, dyx = dxx*(-ixx).exp(), dyy*(-iyy).exp(), dxy*(-ixy).exp(), dyx*(-iyx).exp()
        return dxx.mean() + dyy.mean() + dxy.mean() + dyx.mean(), {'feat_grad': feat_grad}
