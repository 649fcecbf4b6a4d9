"""Seeded inputs of the offline-evaluation fixture (`eval_reference.npz`), shared by tests/golden/make_golden_eval.py and the tests.

Every case has a prediction of the target's shape (the reference resizes with cv2, which the fixture never calls).  Only `torch.rand` and IEEE
arithmetic go into the inputs, so that they regenerate bit for bit; the fixture records their checksums and `eval_case` is refused when they differ."""
from __future__ import annotations

import numpy as np
import torch

__all__ = ['EVAL_CASES', 'eval_case', 'eval_expected', 'eval_kwargs']

# name: shape, align_mode, max, caller mask, the parity of the valid count the case is built to have (None: whatever comes), metric order, `only` = keep
# that many valid target pixels (None: all)
EVAL_CASES = [
    dict(name='median_even', shape=(24, 32), align='median', max=None, mask=False, parity=0, metrics=('eigen', 'benchmark', 'pointcloud'), only=None),
    dict(name='median_odd_max_mask', shape=(24, 32), align='median', max=5.0, mask=True, parity=1, metrics=('benchmark', 'eigen', 'pointcloud'), only=None),
    dict(name='lsqr_33x47', shape=(33, 47), align='lsqr', max=None, mask=False, parity=None, metrics=('eigen', 'benchmark', 'pointcloud'), only=None),
    dict(name='lsqr_max_mask', shape=(24, 32), align='lsqr', max=5.0, mask=True, parity=None, metrics=('benchmark', 'pointcloud'), only=None),
    dict(name='metric_1', shape=(24, 32), align=1, max=None, mask=False, parity=None, metrics=('eigen', 'pointcloud'), only=None),
    dict(name='metric_5.4_max', shape=(24, 32), align=5.4, max=5.0, mask=False, parity=None, metrics=('eigen', 'benchmark', 'pointcloud'), only=None),
    dict(name='empty', shape=(24, 32), align='median', max=None, mask=False, parity=None, metrics=('eigen', 'benchmark', 'pointcloud'), only=0),
    dict(name='one_pixel', shape=(24, 32), align='median', max=None, mask=False, parity=None, metrics=('eigen', 'benchmark', 'pointcloud'), only=1),
    dict(name='two_pixels', shape=(24, 32), align='median', max=None, mask=False, parity=None, metrics=('eigen', 'benchmark', 'pointcloud'), only=2),
]
MIN_DEPTH = 1e-3


def eval_kwargs(k: int) -> dict:
    """The evaluator's constructor arguments of case k."""
    c = EVAL_CASES[k]
    return dict(metrics=c['metrics'], align_mode=c['align'], interp_mode='bilinear', min=MIN_DEPTH, max=c['max'], use_eigen_crop=False, use_nyud_crop=False)


def eval_case(k: int, fixture: dict | None = None) -> dict:
    """-> dict(pred (h,w) disparity, target (h,w) depth with holes, K (4,4), mask (h,w) bool or None), numpy arrays.  An indoor-like scene: a slanted plane
    1.5 .. 6 m with 0.3 m of roughness; the prediction is the target's depth off by up to 1 %, in other units (x 1/(1.7 + k/10)), with a few zero
    disparities; the target has two rectangular holes and 10 % scattered ones.  With `fixture` the regenerated inputs are checked against its checksums."""
    c = EVAL_CASES[k]
    h, w = c['shape']
    gen = torch.Generator().manual_seed(77100 + k)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    depth = 1.5 + 3.0*(ys/h) + 1.5*(xs/w) + 0.3*torch.rand(h, w, generator=gen)
    units = 1.0 if c['align'] == 1 else (5.4 if c['align'] == 5.4 else 1.7 + k/10)
    pred_depth = depth*(1 + 0.02*(torch.rand(h, w, generator=gen) - 0.5))/units
    pred = 1/pred_depth
    pred[torch.rand(h, w, generator=gen) < 0.02] = 0                      # `pred > 0` removes these
    target = depth.clone()
    target[torch.rand(h, w, generator=gen) < 0.1] = 0
    target[h//6:h//6 + 4, w//5:w//5 + 7] = 0
    target[h - 5:h - 2, w//2:w//2 + 5] = 0
    mask = None
    if c['mask']:
        mask = torch.rand(h, w, generator=gen) < 0.8
    if c['only'] is not None:
        keep = torch.nonzero((target > MIN_DEPTH) & (pred > 0)).tolist()[3:3 + c['only']]
        t2 = torch.zeros_like(target)
        for y, x in keep: t2[y, x] = target[y, x]
        target = t2
    if c['parity'] is not None:
        valid = (target > MIN_DEPTH) & (pred > 0)
        if c['max']: valid &= target < c['max']
        if mask is not None: valid &= mask
        if int(valid.sum()) % 2 != c['parity']:
            y, x = torch.nonzero(valid).tolist()[0]
            target[y, x] = 0
    f = 20.5 + k
    K = np.array([[f, 0, w/2 - 0.25, 0], [0, f + 0.75, h/2 + 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    out = dict(pred=pred.numpy(), target=target.numpy(), K=K, mask=None if mask is None else mask.numpy())
    if fixture is not None:
        from exact_inputs import bit_checksum
        chk = sum(bit_checksum(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))) for v in out.values() if v is not None)
        assert chk == int(fixture['chk'][k]), f'eval case {k}: the regenerated inputs differ from what the reference was run on'
    return out


def eval_expected(fixture: dict, k: int):
    """-> (metrics {name: float} in the reference's key order ({} for an empty item), pred_nn, target_nn (float32 arrays), (np.median(pred), np.median(target)))
    of case k: the fixture stores the names as one '|'-joined string per case and every array flat over the cases."""
    names = [n for n in str(fixture[f'keys_{k}']).split('|') if n]
    v0 = int(sum(int(fixture['nvals'][j]) for j in range(k)))
    vals = fixture['values'][v0:v0 + len(names)]
    q0 = int(sum(int(fixture['nq'][j]) for j in range(k)))
    nq = int(fixture['nq'][k])
    return ({n: float(v) for n, v in zip(names, vals)}, np.asarray(fixture['pred_nn'][q0:q0 + nq]), np.asarray(fixture['target_nn'][q0:q0 + nq]),
            (fixture['medians'][k][0], fixture['medians'][k][1]))
