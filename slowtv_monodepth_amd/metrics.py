"""Depth metrics monitored while training (reference: `src/utils/metrics.py`), without torchmetrics: `nn.Module`s with two non-persistent
buffers (`metric`: running sum of per-sample values, `total`: samples seen) and `update` / `compute` / `reset` / `sync`."""
from __future__ import annotations

import torch
import torch.distributed as dist
from torch import nn

__all__ = ['MAE', 'RMSE', 'ScaleInvariant', 'AbsRel', 'SqRel', 'DeltaAcc', 'sync_metrics']

_MODES = {'raw', 'log', 'inv'}


def _nanmean(x, dim): return x.nanmean(dim=dim)


class BaseMetric(nn.Module):
    """Base class: `mode` maps both inputs to log-depth ('log') or disparity ('inv') first; `sf` aligns significant figures."""
    higher_is_better = False

    def __init__(self, mode: str = 'raw'):
        super().__init__()
        if mode not in _MODES: raise ValueError(f'Invalid mode! ({mode} vs. {_MODES})')
        self.mode = mode
        self.sf = {'raw': 1, 'log': 100, 'inv': 1000}[mode]
        # non-persistent: the metric state is not part of a checkpoint (the reference's torchmetrics states are not either)
        self.register_buffer('metric', torch.tensor(0.), persistent=False)
        self.register_buffer('total', torch.tensor(0), persistent=False)

    def _preprocess(self, x):
        if self.mode == 'log': return x.log()
        if self.mode == 'inv': return 1/x.clip(min=1e-3)
        return x

    def _compute(self, pred, target):
        """(b,n), (b,n) NaN-masked -> (b,) per-sample metric."""
        raise NotImplementedError

    def accumulate(self, value_sum: torch.Tensor, n: int) -> None:
        """Add the (already scaled) sum of `n` per-sample values to the state: what the fused operator's columns feed."""
        self.metric += value_sum
        self.total += n

    @torch.no_grad()
    def update(self, pred, target) -> torch.Tensor:
        """pred, target (b,n) masked with NaNs.  -> the batch's own sum (scaled)."""
        s = self.sf*self._compute(self._preprocess(pred), self._preprocess(target)).sum()
        self.accumulate(s, pred.shape[0])
        return s

    def forward(self, pred, target) -> torch.Tensor:
        """Update the state and return the value of THIS batch."""
        return self.update(pred, target)/pred.shape[0]

    def compute(self) -> torch.Tensor: return self.metric/self.total

    def reset(self) -> None:
        self.metric.zero_(); self.total.zero_()

    def sync(self) -> None:
        """Sum the state over the ranks of an initialised process group (one all-reduce).  Call once, before `compute()`, then `reset()`."""
        sync_metrics([self])


def sync_metrics(metrics) -> None:
    """ONE all-reduce of the stacked (metric, total) states of every metric in `metrics`; no-op without a process group."""
    metrics = list(metrics)
    if not metrics or not (dist.is_available() and dist.is_initialized()): return
    state = torch.stack([v.double() for m in metrics for v in (m.metric, m.total)])
    dist.all_reduce(state, op=dist.ReduceOp.SUM)
    for k, m in enumerate(metrics):
        m.metric.copy_(state[2*k]); m.total.copy_(state[2*k + 1])


class MAE(BaseMetric):
    def _compute(self, pred, target): return _nanmean((pred - target).abs(), 1)


class RMSE(BaseMetric):
    def _compute(self, pred, target): return _nanmean((pred - target).pow(2), 1).sqrt()


class ScaleInvariant(BaseMetric):
    def _compute(self, pred, target):
        err = pred - target
        return (_nanmean(err.pow(2), 1) - _nanmean(err, 1).pow(2)).sqrt()   # (not clamped under the root, as the reference)


class AbsRel(BaseMetric):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.sf = 100  # as %

    def _compute(self, pred, target): return _nanmean((pred - target).abs()/target, 1)


class SqRel(BaseMetric):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.sf = 100  # as %

    def _compute(self, pred, target): return _nanmean((pred - target).pow(2)/target.pow(2), 1)


class DeltaAcc(BaseMetric):
    higher_is_better = True

    def __init__(self, delta: float, **kw):
        super().__init__(**kw)
        if self.mode != 'raw': raise ValueError('DeltaAcc should only be computed using raw depths.')
        self.delta = delta
        self.sf = 100  # as %

    def _compute(self, pred, target):
        thresh = torch.max(target/pred, pred/target)
        # the count over the SUM of the ratios (not over the number of valid pixels): what the reference computes, kept
        return (thresh < self.delta).nansum(dim=1)/thresh.nansum(dim=1)
