"""Evaluation entry point: `python -m slowtv_monodepth_amd.evaluate --preds preds.npz --targets targets.npz [--metrics eigen benchmark pointcloud]
[--align median|lsqr|<float>] [--interp ...] [--min ...] [--max ...] [--eigen-crop] [--nyud-crop] [--max-items N] --out metrics.json`.

`preds.npz` carries `preds` (n,h,w), as `predict.py` writes it; `targets.npz` carries `depth` (n,H,W) and optionally `K` (n,4,4), `cat`, `subcat`.  The
output holds the mean metrics and the per-item list.  `--synthetic-data N` stands in for `--targets`: the ground truth is `synthetic.make_batch`'s depth for
the N batches `predict.py --synthetic-data N` predicts (same seeds), made dense and cut by rectangular holes, so that predict followed by evaluate runs
end to end without a dataset."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from .evaluator import MonoDepthEvaluator
from .synthetic import depth_hints_field, kitti_K

__all__ = ['main', 'synthetic_targets']


def synthetic_targets(n: int, shape, seed: int = 42) -> dict:
    """-> {'depth' (n,H,W), 'K' (n,4,4)}: item i is `synthetic.depth_hints_field` (a dense, smooth 2 .. 60 m field with three rectangular holes and 10 % scattered
    ones) under seed + i, with KITTI-like intrinsics of the shape."""
    H, W = int(shape[0]), int(shape[1])
    depth = torch.cat([depth_hints_field(torch.Generator().manual_seed(seed + i), 2, H, W)[:1, 0] for i in range(n)])
    return {'depth': depth.numpy(), 'K': kitti_K(n, H, W).numpy()}


def _align(v: str):
    return v if v in ('median', 'lsqr') else float(v)


def main(argv=None):
    p = argparse.ArgumentParser(description='Offline depth evaluation (MI355X hot path).')
    p.add_argument('--preds', type=Path, required=True, help='npz with `preds` (n,h,w) scaleless disparities, as predict.py writes it')
    p.add_argument('--targets', type=Path, default=None, help='npz with `depth` (n,H,W) and optionally `K`, `cat`, `subcat`')
    p.add_argument('--synthetic-data', type=int, default=0, metavar='N', help='instead of --targets: N synthetic ground-truth maps per predicted item batch')
    p.add_argument('--shape', default=None, type=int, nargs=2, help='shape of the synthetic targets (default: the predictions\')')
    p.add_argument('--seed', '-s', default=42, type=int)
    p.add_argument('--metrics', nargs='+', default=['eigen', 'benchmark', 'pointcloud'], choices=['eigen', 'benchmark', 'pointcloud', 'ibims'])
    p.add_argument('--align', type=_align, default='median')
    p.add_argument('--interp', default='bilinear', choices=['nearest', 'bilinear', 'bicubic'])
    p.add_argument('--min', type=float, default=1e-3)
    p.add_argument('--max', type=float, default=None)
    p.add_argument('--eigen-crop', action='store_true')
    p.add_argument('--nyud-crop', action='store_true')
    p.add_argument('--max-items', type=int, default=None)
    p.add_argument('--device', default=None)
    p.add_argument('--out', type=Path, required=True)
    args = p.parse_args(argv)

    with np.load(args.preds, allow_pickle=False) as z: preds = z['preds']
    if args.synthetic_data > 0:
        n = min(len(preds), args.max_items) if args.max_items else len(preds)
        preds = preds[:n]
        data = synthetic_targets(n, args.shape or preds.shape[-2:], args.seed)
    elif args.targets is not None:
        with np.load(args.targets, allow_pickle=False) as z: data = {k: z[k] for k in z.files}
    else: raise SystemExit('nothing to evaluate against: pass --targets targets.npz or --synthetic-data N')
    ev = MonoDepthEvaluator(metrics=args.metrics, align_mode=args.align, interp_mode=args.interp, min=args.min, max=args.max,
                            use_eigen_crop=args.eigen_crop, use_nyud_crop=args.nyud_crop, device=args.device)
    mean, items = ev.run(preds, data, max_items=args.max_items)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps({'mean': mean, 'items': items}, indent=1))
    print(f'{args.out}: {len(items)} items scored', flush=True)


if __name__ == '__main__':
    main()
