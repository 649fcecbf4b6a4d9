"""Offline evaluation of depth predictions: `MonoDepthEvaluator` (src/core/evaluator.py:30-256) with the reference's constructor, methods and results.

float32 tensors on the GPU are scored by the fused operators of `eval_metrics` (one launch sequence per batch of equally shaped items and ONE copy of
the result table to the host); everything else runs `plain_evaluate`, the reference's sequence restated on torch: CPU tensors and numpy arrays, other
dtypes, `interp_mode='bicubic'`, a `max` of 0, a negative `min`, and subclasses that override `upsample`, `align`, `scale` or `get_mask`."""
from __future__ import annotations

import numpy as np
import torch

from . import eval_metrics as E
from .geometry import to_inv

__all__ = ['MonoDepthEvaluator', 'plain_evaluate', 'plain_eigen', 'plain_benchmark', 'plain_pointcloud', 'plain_chamfer', 'median']

GROUPS = ('eigen', 'benchmark', 'pointcloud', 'ibims')
IBIMS = ("the 'ibims' edge metrics are not implemented: they need a Canny edge detector and a Euclidean distance transform whose parity with "
         "skimage / scipy could not be pinned")
_INTERP = {'nearest': 'nearest', 'bilinear': 'bilinear', 'bicubic': 'bicubic'}


def _to_host(table: torch.Tensor) -> torch.Tensor:
    """THE device-to-host copy of the fused path: one call per batch of equally shaped items (the tests count the calls)."""
    return table.cpu()


def _tensor(x, dtype=None, device=None) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype) if (dtype is not None or device is not None) else t


def median(x: torch.Tensor) -> torch.Tensor:
    """`np.median` of a 1-d tensor: the middle value, or for an even count the mean of the two middle values in the tensor's dtype (one rounded sum,
    then an exact halving).  `torch.median` returns the lower of the two."""
    s = x.sort().values
    n = s.numel()
    return (s[(n - 1)//2] + s[n//2])*0.5


def _mean(x: torch.Tensor) -> float:
    return x.double().mean().item()


def plain_eigen(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """`metrics_eigen` (src/core/metrics.py:39-59) on the masked float32 values.  The terms are formed and averaged in float64, as the fused kernel forms them
    (numpy's float32 terms and pairwise sums carry their own rounding; LogSI, a root of a small difference, shows it); the threshold ratio stays float32
    against float32 constants, which is what decides the counts.  `SqRel` is err^2/target here."""
    thresh = torch.maximum(target/pred, pred/target)
    p, t = pred.double(), target.double()
    err = (p - t).abs()
    return {'AbsRel': _mean(err/t), 'SqRel': _mean(err**2/t), 'RMSE': _mean(err**2)**0.5, 'LogRMSE': _mean((p.log() - t.log())**2)**0.5,
            '$\\delta_{.05}$': 100*_mean(thresh < 1.05), '$\\delta_{.1}$': 100*_mean(thresh < 1.1), '$\\delta_{.25}$': 100*_mean(thresh < 1.25),
            '$\\delta_{.25^2}$': 100*_mean(thresh < 1.25**2), '$\\delta_{.25^3}$': 100*_mean(thresh < 1.25**3)}


def plain_benchmark(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """`metrics_benchmark` (src/core/metrics.py:80-105), terms in float64 as in `plain_eigen`; `SqRel` is 100*err^2/target^2 here."""
    p, t = pred.double(), target.double()
    err = (p - t).abs()
    err_inv = 1000*(1/p - 1/t).abs()
    err_log = 100*(p.log() - t.log())
    ml, ml2 = _mean(err_log), _mean(err_log**2)
    return {'MAE': _mean(err), 'RMSE': _mean(err**2)**0.5, 'InvMAE': _mean(err_inv), 'InvRMSE': _mean(err_inv**2)**0.5, 'LogMAE': _mean(err_log.abs()),
            'LogRMSE': ml2**0.5, 'LogSI': float(np.sqrt(np.float64(ml2 - ml**2))), 'AbsRel': _mean(100*(err/t)), 'SqRel': _mean(100*(err**2/t**2))}


def backproject(depth: torch.Tensor, K_inv: torch.Tensor) -> torch.Tensor:
    """`BackprojectDepth.forward` (src/tools/geometry.py:297-316) for one (h,w) map -> (h*w, 3): K_inv[:3,:3] @ (x, y, 1), times the depth."""
    h, w = depth.shape
    xs, ys = torch.meshgrid(torch.arange(w, device=depth.device), torch.arange(h, device=depth.device), indexing='xy')
    pix = torch.stack((xs, ys, torch.ones_like(xs))).view(3, -1).to(depth.dtype)
    return ((K_inv[:3, :3] @ pix)*depth.flatten()).T


def plain_chamfer(pred_pts: torch.Tensor, target_pts: torch.Tensor, budget: int = 1 << 24):
    """`_chamfer_dist` (metrics.py:122-132) without the kd-tree: for every second point of each (n,3) cloud the distance to its nearest neighbour in the other,
    by chunked `torch.cdist(...).min` on the float64 differences (never the |a|^2 + |b|^2 - 2ab expansion, which cancels), rounded to float32 at the end as
    the reference rounds the kd-tree's float64 distances."""
    def nn(q, d):
        q, d = q.double(), d.double()
        step = max(1, budget//max(1, d.shape[0]))
        out = [torch.cdist(q[i:i + step], d, compute_mode='donot_use_mm_for_euclid_dist').min(dim=1).values for i in range(0, q.shape[0], step)]
        return torch.cat(out).float()
    return nn(pred_pts[::2], target_pts), nn(target_pts[::2], pred_pts)


def plain_pointcloud(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, K) -> dict:
    """`metrics_pointcloud` (metrics.py:136-165): K's inverse is torch's, in float32 on the host."""
    K_inv = torch.linalg.inv(_tensor(K, torch.float32).cpu()).to(pred.device)
    m = mask.flatten()
    pred_nn, target_nn = plain_chamfer(backproject(pred, K_inv)[m], backproject(target, K_inv)[m])
    out = {'Chamfer': _mean(pred_nn) + _mean(target_nn)}
    for th in (0.05, 0.1, 0.2):
        out[f'F-Score ({th*100:.0f})'], out[f'IoU ({th*100:.0f})'] = E._metrics_pts(_mean(pred_nn < th), _mean(target_nn < th))
    return out


def plain_evaluate(ev: 'MonoDepthEvaluator', pred, target, metrics, K=None, mask=None) -> dict:
    """The reference's `__call__` (evaluator.py:65-94) step by step on torch tensors of any device: resize -> `to_inv` -> mask -> align on the masked values ->
    scale and clip -> metric groups merged in the caller's order.  Goes through `ev`'s own `upsample`, `get_mask`, `align` and `scale`."""
    if 'ibims' in metrics: raise NotImplementedError(IBIMS)
    target = _tensor(target).to(torch.float32)
    pred = _tensor(pred).to(target.device)
    pred = to_inv(ev.upsample(pred, target))
    mask = torch.ones_like(target, dtype=torch.bool) if mask is None else _tensor(mask).to(target.device, torch.bool).clone()   # the caller's array stays as it is
    mask &= ev.get_mask(target) & (pred > 0)
    if mask.sum() == 0: return {}
    pred_mask, target_mask = pred[mask], target[mask]
    if pred_mask.sum() == 0: return {}
    inv = ev.align_mode == 'lsqr'
    a, b = ev.align(pred_mask, target_mask, inv=inv)
    pred, pred_mask = ev.scale(pred, a, b, inv=inv), ev.scale(pred_mask, a, b, inv=inv)
    ms = {'Scale': a, 'Shift': b}
    for m in metrics:
        if m == 'eigen': ms |= plain_eigen(pred_mask, target_mask)
        elif m == 'benchmark': ms |= plain_benchmark(pred_mask, target_mask)
        elif m == 'pointcloud': ms |= plain_pointcloud(pred, target, mask, K)
    return ms


class MonoDepthEvaluator:
    """Evaluate scaleless disparity predictions against ground-truth depth, as the reference's class does (src/core/evaluator.py:30-256).

    :param metrics: metric groups {benchmark, eigen, pointcloud, ibims}.
    :param align_mode: 'median', 'lsqr', or a float: the prediction is metric up to this factor.
    :param interp_mode: {nearest, bilinear, bicubic}: how a smaller prediction is resized to the target.
    :param min, max: ground-truth range; `max=None` disables the upper bound.
    :param use_eigen_crop, use_nyud_crop: border crops (see below).
    :param device: where `run` evaluates numpy inputs: default the GPU when there is one.

    What the reference computes is reproduced, including what looks odd:
      * order: resize -> `to_inv` -> mask -> align on the MASKED values -> scale and clip -> metrics;
      * the mask is `target > min`, with `max` also `target < max`; the crop, the caller's mask and `pred > 0` are ANDed in;
      * an empty mask returns `{}`; so does a masked prediction that sums to 0 (with `pred > 0` in the mask no finite input reaches that second return);
      * `get_mask` applies the NYU-D rectangle under `use_eigen_crop` and the Eigen rectangle under `use_nyud_crop` (evaluator.py:179-180): swapped, and kept;
      * the groups are merged with `|=` in the caller's order, so `eigen` and `benchmark` overwrite each other's AbsRel, SqRel, RMSE and LogRMSE, and the two
        SqRel differ (err^2/target against 100*err^2/target^2);
      * 'Scale' and 'Shift' are reported; least squares is solved, and applied, in disparity space;
      * `np.median` of an even count is the float32 mean of the two middle values;
      * `run` drops empty items before averaging, raises on a length mismatch and when `pointcloud` is asked for without `K`, and appends `Cat` / `SubCat`
        when the data carries them.
    Two things differ on purpose: the caller's `mask` is not modified in place, and `ibims` raises NotImplementedError (it needs Canny edges and a Euclidean
    distance transform).  Resizing follows ATen's `interpolate` (align_corners=False), not `cv2.resize`: equality with cv2 is not claimed.  `run` keeps `nproc`
    and `chunks` in its signature and ignores them: no process pool is started."""

    def __init__(self, metrics=('benchmark', 'pointcloud'), align_mode=1, interp_mode: str = 'bilinear', min: float = 1e-3, max=None,
                 use_eigen_crop: bool = False, use_nyud_crop: bool = False, *, device=None):
        self.align_mode = align_mode
        self.metrics = metrics
        self.min = min
        self.max = max
        self.use_eigen_crop = use_eigen_crop
        self.use_nyud_crop = use_nyud_crop
        self.interp_mode = _INTERP[interp_mode]
        self.device = torch.device(device) if device is not None else torch.device('cuda' if torch.cuda.is_available() else 'cpu')

    # ---- one item -------------------------------------------------------------------------------------------------------------------------------
    def __call__(self, pred, target, metrics, K=None, mask=None) -> dict:
        """pred (h', w') disparity, target (h, w) depth, K (4,4) or None, mask (h, w) or None -> {name: float}; `{}` for an item without valid pixels."""
        if 'ibims' in metrics: raise NotImplementedError(IBIMS)
        if self._fused(pred, target):
            return self._fused_group(pred[None], target[None], None if K is None else [K], None if mask is None else _tensor(mask)[None], metrics)[0]
        return plain_evaluate(self, pred, target, metrics, K, mask)

    def _fused(self, pred, target) -> bool:
        """The static rule: float32 tensors on one GPU, a mode the kernel resizes in, a range whose values order like their bit patterns, no overridden step."""
        cls = type(self)
        if any(getattr(cls, n) is not getattr(MonoDepthEvaluator, n) for n in ('upsample', 'align', 'scale', 'get_mask')): return False
        if not (isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor) and pred.is_cuda and target.is_cuda and pred.device == target.device): return False
        if pred.dtype != torch.float32 or target.dtype != torch.float32 or self.interp_mode == 'bicubic': return False
        if not (self.min >= 0) or (self.max is not None and not self.max > self.min): return False
        return isinstance(self.align_mode, (int, float)) or self.align_mode in ('median', 'lsqr')

    def _crop(self, shape):
        """The rectangle `get_mask` crops to, as (y0, y1, x0, x1)."""
        h, w = shape
        y0, y1, x0, x1 = 0, h, 0, w
        if self.use_eigen_crop:
            assert tuple(shape) == (480, 640)
            y0, y1, x0, x1 = 45, 471, 41, 601
        if self.use_nyud_crop:
            c = np.array([0.40810811*h, 0.99189189*h, 0.03594771*w, 0.96405229*w], dtype=int)
            y0, y1, x0, x1 = max(y0, c[0]), min(y1, c[1]), max(x0, c[2]), min(x1, c[3])
        return int(y0), int(y1), int(x0), int(x1)

    def _fused_group(self, preds, targets, Ks, masks, metrics) -> list:
        """preds (b,h',w'), targets (b,h,w) float32 on the GPU, Ks a list of (4,4) or None, masks (b,h,w) or None -> the b metric dicts.  Two operator calls
        and one copy to the host."""
        b = preds.shape[0]
        mode = self.align_mode if self.align_mode in ('median', 'lsqr') else 'factor'
        pc = 'pointcloud' in metrics
        if pc and Ks is None: raise ValueError('Missing intrinsics when computing pointcloud metrics!')
        if masks is not None: masks = masks.to(targets.device, torch.bool)[:, None]
        r = E.eval_metrics(preds[:, None], targets[:, None], masks, min_depth=self.min, max_depth=self.max, align=mode,
                           factor=(self.align_mode or 1) if mode == 'factor' else 1.0, interp=self.interp_mode, crop=self._crop(targets.shape[-2:]),
                           want_depth=pc, want_valid=pc)
        cols = [r['values'], r['counts'].double()[:, None], r['status'].double()[:, None]]
        if pc:
            K_inv = torch.linalg.inv(torch.stack([_tensor(K, torch.float32).cpu() for K in Ks])).to(targets.device)
            _, stats, n = E.eval_pointcloud(r['depth'], targets[:, None], r['valid'], K_inv)
            cols += [stats.view(b, 8), n.double()[:, None]]
        table = _to_host(torch.cat(cols, dim=1)).numpy()
        out = []
        for row in table:
            if int(row[21]) != 0: out.append({}); continue
            ms = {'Scale': float(row[0]), 'Shift': float(row[1])}
            for m in metrics:
                if m == 'eigen': ms |= dict(zip(E.EIGEN_KEYS, (float(v) for v in row[2:11])))
                elif m == 'benchmark': ms |= dict(zip(E.BENCHMARK_KEYS, (float(v) for v in row[11:20])))
                elif m == 'pointcloud': ms |= E.pointcloud_values(row[22:30].reshape(2, 4), int(row[30]))
            out.append(ms)
        return out

    # ---- a dataset ------------------------------------------------------------------------------------------------------------------------------
    def run(self, preds, data, nproc=None, chunks: int = 1, max_items=None):
        """preds: (n,h',w') disparities (or a list of maps of different shapes); data: dict with `depth` and optionally `K`, `edge`, `cat`, `subcat`
        -> (mean metrics, the per-item metrics without the empty items).  `nproc` and `chunks` are ignored."""
        targets, Ks, edges = data['depth'], data.get('K'), data.get('edge')
        cats, subcats = data.get('cat'), data.get('subcat')
        if Ks is None and 'pointcloud' in self.metrics: raise ValueError('Missing intrinsics when computing pointcloud metrics!')
        if edges is None and 'ibims' in self.metrics: raise ValueError('Missing edge masks when computing IBIMS metrics!')
        if (a := len(preds)) != (b := len(targets)): raise ValueError(f'Non-matching preds and targets! ({a} vs. {b})')
        n = min(len(targets), max_items) if max_items else len(targets)
        preds, targets = preds[:n], targets[:n]

        metrics = self._run(preds, targets, [m for m in self.metrics if m != 'ibims'], Ks)
        if edges is not None:
            edge_metrics = self._run(preds, targets, self.metrics, Ks, edges)
            for m1, m2 in zip(metrics, edge_metrics): m1.update({f'{k}-Edges': v for k, v in m2.items()})
        if cats is not None: self.add_cats(metrics, cats, subcats)
        if len(metrics) != n: raise ValueError(f'Non-matching metrics and targets! ({len(metrics)} vs. {n})')
        metrics = [m for m in metrics if m]
        mean_metrics = self.average(metrics)
        self.summarize(mean_metrics)
        return mean_metrics, metrics

    def _run(self, preds, targets, metrics, Ks=None, masks=None) -> list:
        """The items grouped by (prediction shape, target shape), each group as one batch; results in the items' order."""
        if 'ibims' in metrics: raise NotImplementedError(IBIMS)
        n = len(preds)
        groups: dict = {}
        for i in range(n): groups.setdefault((tuple(preds[i].shape), tuple(targets[i].shape)), []).append(i)
        out = [None]*n
        for idxs in groups.values():
            stack = lambda xs, dt: torch.stack([_tensor(xs[i]).to(dt) for i in idxs]).to(self.device)
            p, t = stack(preds, torch.float32), stack(targets, torch.float32)
            if self._fused(p, t):
                res = self._fused_group(p, t, None if Ks is None else [Ks[i] for i in idxs], None if masks is None else stack(masks, torch.bool), metrics)
            else:
                res = [plain_evaluate(self, p[k], t[k], metrics, None if Ks is None else Ks[i], None if masks is None else masks[i]) for k, i in enumerate(idxs)]
            for i, ms in zip(idxs, res): out[i] = ms
        return out

    def summarize(self, mean_metrics: dict) -> None:
        """Print the mean metrics as a plain two-column table."""
        width = max([len(k) for k in mean_metrics] + [6])
        print('\n'.join([f'{"Metric":<{width}}  Value'] + [f'{k:<{width}}  {v:.4f}' for k, v in mean_metrics.items()]))

    # ---- the steps (tensors in, tensors out; a subclass that overrides one is evaluated by `plain_evaluate`) -----------------------------------------
    def upsample(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """Resize the prediction to the target's (h, w) with `interpolate(mode=interp_mode, align_corners=False)`; equal shapes pass through."""
        if pred.shape == target.shape: return pred
        kw = {} if self.interp_mode == 'nearest' else {'align_corners': False}
        return torch.nn.functional.interpolate(pred[None, None].to(torch.float32), size=tuple(target.shape), mode=self.interp_mode, **kw)[0, 0]

    def get_mask(self, target: torch.Tensor) -> torch.Tensor:
        mask = target > self.min
        if self.max: mask &= target < self.max
        if self.use_eigen_crop: mask &= self._get_nyud_mask(tuple(target.shape)).to(target.device)      # swapped in the reference (evaluator.py:179-180): kept
        if self.use_nyud_crop: mask &= self._get_eigen_mask(tuple(target.shape)).to(target.device)
        return mask

    @staticmethod
    def _get_eigen_mask(shape) -> torch.Tensor:
        h, w = shape
        crop = np.array([0.40810811*h, 0.99189189*h, 0.03594771*w, 0.96405229*w], dtype=int)
        mask = torch.zeros((h, w), dtype=torch.bool)
        mask[crop[0]:crop[1], crop[2]:crop[3]] = True
        return mask

    @staticmethod
    def _get_nyud_mask(shape) -> torch.Tensor:
        assert tuple(shape) == (480, 640)
        mask = torch.zeros(tuple(shape), dtype=torch.bool)
        mask[45:471, 41:601] = True
        return mask

    def align(self, pred: torch.Tensor, target: torch.Tensor, inv: bool = False):
        """Masked (n,) prediction and target -> (scale, shift) as floats; `inv`: in disparity space."""
        if inv: pred, target = to_inv(pred), to_inv(target)
        if self.align_mode == 'median': r, s = self._align_median(pred, target)
        elif self.align_mode == 'lsqr': r, s = self._align_lsqr(pred, target)
        else: r, s = self._align_metric(self.align_mode)
        return float(r), float(s)

    @staticmethod
    def _align_metric(factor=None): return factor or 1, 0

    @staticmethod
    def _align_median(pred, target): return (median(target)/median(pred)).item(), 0

    @staticmethod
    def _align_lsqr(pred, target):
        """The 2x2 normal equations (evaluator.py:229-234) from float64 sums; a determinant <= 0 gives (0, 0)."""
        p, t = pred.double(), target.double()
        n, sp, spp, spt, st = float(p.numel()), p.sum().item(), (p*p).sum().item(), (p*t).sum().item(), t.sum().item()
        det = spp*n - sp*sp
        if det <= 0: return 0, 0
        return (n*spt - sp*st)/det, (spp*st - sp*spt)/det

    def scale(self, pred: torch.Tensor, scale: float, shift: float, inv: bool = False) -> torch.Tensor:
        """`scale*pred + shift` in the prediction's dtype, in disparity space if asked, then `clip(min, max)`."""
        if inv: pred = to_inv(pred)
        pred = scale*pred + shift
        if inv: pred = to_inv(pred)
        return pred.clamp(self.min, self.max)

    def add_cats(self, metrics, cats, subcats) -> None:
        for m, cat, subcat in zip(metrics, cats, subcats):
            if m: m['Cat'], m['SubCat'] = str(cat), str(subcat)

    @staticmethod
    def average(metrics) -> dict:
        keys = (k for k, v in metrics[0].items() if isinstance(v, float))
        return {k: float(np.mean([d[k] for d in metrics if k in d])) for k in keys}

