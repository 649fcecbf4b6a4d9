"""Prediction entry point: `python -m slowtv_monodepth_amd.predict --ckpt last.ckpt [--cfg cfg.yaml ...] [--stereo-blend] --synthetic-data N --out preds.npz`.

Loads a checkpoint with the `ours` predictor and writes the disparities for N synthetic batches (`synthetic.make_batch`) as `preds` (n,h,w) to an `.npz`.
Datasets are out of scope here, as in `train.py`: a cfg that names a real dataset type is refused unless `--synthetic-data` says that synthetic images of
its shape are intended."""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

from . import io
from .registry import PRED_REG
from .synthetic import make_batch
from .train import dataset_types

__all__ = ['main']


def main(argv=None):
    p = argparse.ArgumentParser(description='Monocular depth predictions (MI355X hot path).')
    p.add_argument('--ckpt', type=Path, required=True, help='checkpoint in the reference\'s layout (this package\'s last.ckpt)')
    p.add_argument('--cfg', type=Path, nargs='*', default=None, help='YAML configs, for a checkpoint that carries none or a legacy one')
    p.add_argument('--stereo-blend', action='store_true', help='blend with the prediction for the mirrored image (flip & average)')
    p.add_argument('--synthetic-data', type=int, default=0, metavar='N', help='predict N synthetic batches')
    p.add_argument('--batch-size', type=int, default=None, help='default: the cfg\'s loader.batch_size')
    p.add_argument('--shape', default=[192, 640], type=int, nargs=2)
    p.add_argument('--seed', '-s', default=42, type=int)
    p.add_argument('--device', default=None)
    p.add_argument('--out', type=Path, required=True)
    args = p.parse_args(argv)

    import slowtv_monodepth_amd.predictors  # noqa: F401  (registers `ours`)
    pred = PRED_REG['ours']()
    net = pred.load_model(args.ckpt, args.cfg or None)
    cfg = io.load_merge_yaml(*args.cfg) if args.cfg else torch.load(args.ckpt, map_location='cpu', weights_only=False)['hyper_parameters']['cfg']
    named = dataset_types(cfg)
    if args.synthetic_data < 1:
        if named: raise SystemExit(f'the cfg names dataset type(s) {named}: this package trains on synthetic triplets only (datasets are out of scope); '
                                   'pass --synthetic-data to run the cfg on synthetic triplets of its shape, or drop the dataset `type`')
        raise SystemExit('nothing to predict: pass --synthetic-data N (datasets are out of scope)')
    b = args.batch_size or cfg.get('loader', {}).get('batch_size', 12)
    batches = (make_batch(b, args.shape[0], args.shape[1], seed=args.seed + i) for i in range(args.synthetic_data))
    preds = pred(net, batches, use_stereo_blend=args.stereo_blend, device=args.device)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    np.savez(args.out, preds=preds)
    print(f'{args.out}: preds {preds.shape} {preds.dtype}, min {preds.min():.6f} max {preds.max():.6f}', flush=True)


if __name__ == '__main__':
    main()
