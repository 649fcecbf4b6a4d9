"""Offline evaluation's two operators over `smd_eval_metrics` / `smd_eval_pointcloud` (csrc/smd_eval.hip): `eval_metrics` resizes, inverts, masks, aligns,
scales and scores a batch of predictions (`MonoDepthEvaluator.__call__`, src/core/evaluator.py:65-94, with `metrics_eigen` / `metrics_benchmark`,
src/core/metrics.py:39-105), `eval_pointcloud` back-projects the aligned depth and the target and finds the exact nearest neighbours of both directions
(`metrics_pointcloud`, metrics.py:111-165).  GPU float32 only and not differentiable; `evaluator.MonoDepthEvaluator` is the caller and holds the plain
sequence every other operand runs.  Neither is re-exported by `functional`."""
from __future__ import annotations

import torch

from ._device import _check, _ptr, _stream, _workspace, call
from ._lib import lib

__all__ = ['eval_metrics', 'eval_pointcloud', 'pointcloud_values', 'EVAL_COLUMNS', 'EIGEN_KEYS', 'BENCHMARK_KEYS', 'POINTCLOUD_KEYS', 'STATUS']

ALIGN = {'factor': 0, 'median': 1, 'lsqr': 2}                    # SMD_EVAL_ALIGN_*
EIGEN, BENCHMARK, NEAREST = 0x1, 0x2, 0x4                        # SMD_EVAL_EIGEN / _BENCHMARK / _NEAREST
STATUS = ('scored', 'empty mask', 'zero prediction sum')         # SMD_EVAL_SCORED / _EMPTY_MASK / _ZERO_PRED
EIGEN_KEYS = ('AbsRel', 'SqRel', 'RMSE', 'LogRMSE', '$\\delta_{.05}$', '$\\delta_{.1}$', '$\\delta_{.25}$', '$\\delta_{.25^2}$', '$\\delta_{.25^3}$')
BENCHMARK_KEYS = ('MAE', 'RMSE', 'InvMAE', 'InvRMSE', 'LogMAE', 'LogRMSE', 'LogSI', 'AbsRel', 'SqRel')
POINTCLOUD_KEYS = ('Chamfer', 'F-Score (5)', 'IoU (5)', 'F-Score (10)', 'IoU (10)', 'F-Score (20)', 'IoU (20)')
EVAL_COLUMNS = ('Scale', 'Shift') + tuple(f'eigen/{k}' for k in EIGEN_KEYS) + tuple(f'benchmark/{k}' for k in BENCHMARK_KEYS)   # the columns of `values`


def _mask_u8(name, mask, shape, device):
    if mask.dtype not in (torch.uint8, torch.bool): raise TypeError(f'{name} must be bool or uint8, got {mask.dtype}')
    if tuple(mask.shape) != tuple(shape): raise ValueError(f'{name}: expected shape {tuple(shape)}, got {tuple(mask.shape)}')
    if mask.device != device: raise RuntimeError(f'{name} must live on the operands\' device')
    return mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()


@torch.no_grad()
def eval_metrics(disp, target, mask=None, *, min_depth=1e-3, max_depth=None, align='median', factor=1.0, interp='bilinear', crop=None,
                 groups=('eigen', 'benchmark'), want_depth=False, want_valid=False, want_resized=False):
    """disp (b,1,h,w) scaleless disparity, target (b,1,H,W), mask (b,1,H,W) bool / uint8 or None -> dict(values (b,20) float64 in `EVAL_COLUMNS`,
    counts (b,) int32, status (b,) int32 indexing `STATUS`, medians (b,2), and on request depth (b,1,H,W) the aligned prediction at the valid pixels (0
    elsewhere), valid (b,1,H,W) uint8, resized (b,1,H,W) the resized disparity).  `align`: 'factor' (with `factor`), 'median', 'lsqr'; `interp`: 'bilinear'
    (ATen's align_corners=False taps) or 'nearest' (floor(dst*in/out)); `crop` = (y0, y1, x0, x1) or None; `max_depth` None: no upper bound.  One launch
    sequence, no synchronisation; two calls give the same bits."""
    if align not in ALIGN: raise ValueError(f'align must be one of {sorted(ALIGN)}, got {align!r}')
    if interp not in ('bilinear', 'nearest'): raise ValueError(f'interp must be bilinear or nearest here, got {interp!r}')
    flags = (EIGEN if 'eigen' in groups else 0) | (BENCHMARK if 'benchmark' in groups else 0) | (NEAREST if interp == 'nearest' else 0)
    if disp.ndim != 4 or target.ndim != 4 or disp.shape[1] != 1 or target.shape[1] != 1 or disp.shape[0] != target.shape[0]:
        raise ValueError(f'disp and target must be (b,1,h,w) and (b,1,H,W), got {tuple(disp.shape)} and {tuple(target.shape)}')
    disp = _check('disp', disp.detach(), align=False); target = _check('target', target.detach(), align=False)
    if target.device != disp.device: raise RuntimeError('disp and target must live on the same device')
    dev = disp.device
    b, _, h, w = disp.shape
    H, W = target.shape[-2:]
    if mask is not None: mask = _mask_u8('mask', mask, target.shape, dev)
    y0, y1, x0, x1 = (0, H, 0, W) if crop is None else (int(v) for v in crop)
    out = dict(values=torch.empty((b, 20), device=dev, dtype=torch.float64), counts=torch.empty((b,), device=dev, dtype=torch.int32),
               status=torch.empty((b,), device=dev, dtype=torch.int32), medians=torch.empty((b, 2), device=dev, dtype=torch.float32))
    out['depth'] = torch.empty((b, 1, H, W), device=dev, dtype=torch.float32) if want_depth else None
    out['valid'] = torch.empty((b, 1, H, W), device=dev, dtype=torch.uint8) if want_valid else None
    out['resized'] = torch.empty((b, 1, H, W), device=dev, dtype=torch.float32) if want_resized else None
    ws, nbytes = _workspace(dev, lib.smd_eval_metrics_workspace_bytes, b, H, W, floor=256)
    call('smd_eval_metrics', disp.data_ptr(), target.data_ptr(), _ptr(mask), b, h, w, H, W, y0, y1, x0, x1, float(min_depth), float(max_depth or 0.0),
         ALIGN[align], float(factor), flags, out['values'].data_ptr(), out['counts'].data_ptr(), out['status'].data_ptr(), out['medians'].data_ptr(),
         _ptr(out['depth']), _ptr(out['valid']), _ptr(out['resized']), ws.data_ptr(), nbytes, _stream())
    return out


@torch.no_grad()
def eval_pointcloud(depth, target, mask, K_inv):
    """depth, target (b,1,H,W) float32, mask (b,1,H,W) bool / uint8, K_inv (b,4,4) -> (nn (b,2,ceil(H*W/2)) the nearest-neighbour distances of every second
    masked point of the prediction's cloud in the target's and the other way round (0 past an item's ceil(n/2) queries), stats (b,2,4) float64 = per direction
    the sum of the distances and the counts below 0.05 / 0.1 / 0.2, counts (b,) int32 = n).  The prefix sum of the mask is a `torch.cumsum` (no
    synchronisation: `nonzero` would need one); `pointcloud_values` turns a row of `stats` into the seven reported values on the host."""
    depth = _check('depth', depth.detach(), align=False); target = _check('target', target.detach(), tuple(depth.shape), align=False)
    if depth.ndim != 4 or depth.shape[1] != 1: raise ValueError(f'depth must be (b,1,H,W), got {tuple(depth.shape)}')
    dev = depth.device
    b, _, H, W = depth.shape
    mask = _mask_u8('mask', mask, depth.shape, dev)
    K_inv = _check('K_inv', K_inv.detach(), (b, 4, 4), align=False)
    if target.device != dev or K_inv.device != dev: raise RuntimeError('the operands must live on one device')
    prefix = torch.cumsum((mask != 0).view(b, H*W), dim=1, dtype=torch.int32)
    nq = (H*W + 1)//2
    nn = torch.empty((b, 2, nq), device=dev, dtype=torch.float32)
    stats = torch.empty((b, 2, 4), device=dev, dtype=torch.float64)
    counts = torch.empty((b,), device=dev, dtype=torch.int32)
    ws, nbytes = _workspace(dev, lib.smd_eval_pointcloud_workspace_bytes, b, H, W, floor=256)
    call('smd_eval_pointcloud', depth.data_ptr(), target.data_ptr(), mask.data_ptr(), prefix.data_ptr(), K_inv.data_ptr(), b, H, W, nn.data_ptr(),
         stats.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return nn, stats, counts


def _metrics_pts(P: float, R: float):
    """`_metrics_pts` (metrics.py:111-119) from the two fractions, including its `(0, 0)` early return."""
    if (P < 1e-3) and (R < 1e-3): return 0.0, 0.0
    return 100*(2*P*R/(P + R + 1e-5)), 100*(P*R/(P + R - (P*R) + 1e-5))


def pointcloud_values(stats, n: int) -> dict:
    """One item's (2,4) `stats` (host numbers) and its point count n -> {'Chamfer', 'F-Score (5)', 'IoU (5)', ...} as `metrics_pointcloud` reports them."""
    nq = (int(n) + 1)//2
    s = [[float(v) for v in row] for row in stats]
    out = {'Chamfer': s[0][0]/nq + s[1][0]/nq}
    for k, th in enumerate((5, 10, 20)):
        out[f'F-Score ({th})'], out[f'IoU ({th})'] = _metrics_pts(s[0][1 + k]/nq, s[1][1 + k]/nq)
    return out
