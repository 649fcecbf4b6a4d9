"""The validation depth metrics as one operator (`smd_depth_metrics`): resize, clamp, range mask, per-sample median alignment and the five
per-sample metrics of the reference's `MonoDepthModule.compute_metrics` (src/core/trainer.py:531-552).  `functional` re-exports the wrapper."""
import torch

from ._device import _check, _stream, _workspace, call
from ._lib import lib

METRIC_ORDER = ('MAE', 'RMSE', 'LogSI', 'AbsRel', 'Acc')   # the columns of `values`


def _range(min_depth, max_depth):
    """`min_depth or 0.1`, `max_depth or 100` (src/core/trainer.py:540), validated as the C call validates them."""
    lo, hi = float(min_depth or 0.1), float(max_depth or 100)
    if not lo > 0: raise ValueError(f'Min depth must be greater than 0. ({lo:g})')
    if not (hi > lo and hi < float('inf')): raise ValueError(f'Max depth must be finite and greater than min. ({hi:g} vs. {lo:g})')
    return lo, hi


def _depth_metrics_torch(pred, target, lo, hi):
    """The operator restated on ATen, for tensors that are not on the GPU (host tests, the oracle backend)."""
    b = pred.shape[0]
    p0 = pred if pred.shape[-2:] == target.shape[-2:] else torch.nn.functional.interpolate(pred, size=target.shape[-2:], mode='bilinear', align_corners=False)
    p0, t = p0.clamp(lo, hi).flatten(1), target.flatten(1)
    m = (t > lo) & (t < hi)
    n = m.sum(dim=1)
    nan = torch.full_like(t, float('nan'))
    med = torch.stack([torch.where(m, p0, nan).nanmedian(dim=1).values, torch.where(m, t, nan).nanmedian(dim=1).values], dim=1)
    p = (p0*(med[:, 1]/med[:, 0])[:, None]).clamp(lo, hi)
    zero = torch.zeros_like(t)
    mean = lambda v: torch.where(m, v, zero).sum(dim=1)/n          # n = 0: 0/0 = NaN, the reference's nanmean of an all-NaN row
    d, ts, ps = p - t, torch.where(m, t, torch.ones_like(t)), torch.where(m, p, torch.ones_like(t))   # (masked-out entries made harmless before log and division)
    e = ps.log() - ts.log()
    q = torch.max(ts/ps, ps/ts)
    acc = torch.where(m, (q < 1.25).to(t.dtype), zero).sum(dim=1)/torch.where(m, q, zero).sum(dim=1)   # over the SUM of q, as the reference's DeltaAcc
    values = torch.stack([mean(d.abs()), mean(d*d).sqrt(), 100*(mean(e*e) - mean(e)**2).sqrt(), 100*mean(d.abs()/ts), 100*acc], dim=1)
    return values, med, n.to(torch.int32)


@torch.no_grad()
def depth_metrics(pred, target, min_depth=None, max_depth=None):
    """pred (b,1,h,w) depth, target (b,1,H,W) -> (values (b,5) in `METRIC_ORDER`, medians (b,2) = (med_pred, med_target), counts (b,) int32).
    Not differentiable.  One call, no synchronisation, bit-reproducible; the batch value of a metric is `values[:, k].sum()/b`."""
    lo, hi = _range(min_depth, max_depth)
    if pred.ndim != 4 or target.ndim != 4 or pred.shape[1] != 1 or target.shape[1] != 1 or pred.shape[0] != target.shape[0]:
        raise ValueError(f'pred and target must be (b,1,h,w) and (b,1,H,W), got {tuple(pred.shape)} and {tuple(target.shape)}')
    if not (pred.is_cuda and target.is_cuda):
        if pred.is_cuda != target.is_cuda: raise RuntimeError('pred and target must live on the same device')
        return _depth_metrics_torch(pred.detach().float(), target.detach().float(), lo, hi)
    pred = _check('pred', pred.detach()); target = _check('target', target.detach())
    if target.device != pred.device: raise RuntimeError('pred and target must live on the same device')
    b, _, h, w = pred.shape
    H, W = target.shape[-2:]
    values = torch.empty((b, 5), device=pred.device, dtype=torch.float32)
    medians = torch.empty((b, 2), device=pred.device, dtype=torch.float32)
    counts = torch.empty((b,), device=pred.device, dtype=torch.int32)
    ws, nbytes = _workspace(pred.device, lib.smd_depth_metrics_workspace_bytes, b, H, W, floor=256)
    call('smd_depth_metrics', pred.data_ptr(), target.data_ptr(), b, h, w, H, W, lo, hi, values.data_ptr(), medians.data_ptr(), counts.data_ptr(),
         ws.data_ptr(), nbytes, _stream())
    return values, medians, counts
