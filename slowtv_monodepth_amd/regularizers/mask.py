"""`MaskReg` — registry key `disp_mask` (reference: `src/regularizers/mask.py:11-30`)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import register

__all__ = ['MaskReg']


@register('disp_mask')
class MaskReg(nn.Module):
    """Regulariser of the `explainability` mask (SfM-Learner): binary cross-entropy against ones, which keeps the per-pixel weights of the photometric
    error from collapsing to zero.  `handlers.disp_mask` evaluates every scale in one launch; called directly it serves one tensor the same way."""
    def forward(self, x: torch.Tensor):
        """x (*) sigmoid explainability mask -> (loss (), {})."""
        from .. import functional as F
        return F.scale_mean([x], 'bce_ones'), {}
