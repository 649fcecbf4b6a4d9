"""`OccReg` — registry key `disp_occ` (reference: `src/regularizers/occlusion.py:9-40`)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import register

__all__ = ['OccReg']


@register('disp_occ')
class OccReg(nn.Module):
    """Occlusion regulariser (DVSO): the mean disparity, which favours background disparities.  It is applied to the raw sigmoid disparity — mean
    normalisation would fix the mean at 1.

    :param invert: favour foreground disparities instead (the sign of the loss flips).
    """
    def __init__(self, invert: bool = False):
        super().__init__()
        self.invert = invert
        self._sign = -1 if self.invert else 1

    def forward(self, x: torch.Tensor):
        """x (*) sigmoid disparities -> (loss (), {})."""
        from .. import functional as F
        return F.scale_mean([x], 'negate' if self.invert else 'identity'), {}
