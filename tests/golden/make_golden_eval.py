#!/usr/bin/env python3
"""Golden vectors for offline evaluation, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are
reused here).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_eval.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/core/evaluator.py:50-94     MonoDepthEvaluator.__call__ (with align, scale, get_mask)
  * src/core/metrics.py:27-165      metrics_eigen, metrics_benchmark, metrics_pointcloud, _chamfer_dist (its per-query distances are recorded)

Every case's prediction has the target's shape, so the reference never calls cv2.  tests/golden/eval_reference.npz (read it with
eval_inputs.eval_expected): `chk` the bit checksums of the seeded inputs of every case of eval_inputs.EVAL_CASES; `keys_k` the reference's metric names of
case k in its dict's order, `values` the values, `pred_nn` / `target_nn` the nearest-neighbour distances of `_chamfer_dist`, each flat over the cases
(`nvals`, `nq` the lengths); `medians` np.median of the masked prediction and target.  The fixture holds data only; no reference source text is stored.

The generator REFUSES inputs on which a one-ulp difference could flip a count (a test cannot tell such a flip from a bug): a masked max(t/p, p/t) of the
aligned prediction within 1e-5 relative of a delta threshold, a neighbour distance within 1e-5 relative of 0.05 / 0.1 / 0.2, a precision or recall within
1e-5 of 1e-3.  It also checks that this package's plain path forms the reference's aligned depth bit for bit and its distances to 1e-6."""
import sys

import numpy as np
import torch

from make_golden import OUT, import_reference, save

ROOT = OUT.parents[1]
if str(ROOT) not in sys.path: sys.path.insert(0, str(ROOT))


def main():
    torch.set_num_threads(1)
    import_reference()
    import src.core.metrics as RM
    from src.core.evaluator import MonoDepthEvaluator as RefEvaluator
    from eval_inputs import EVAL_CASES, MIN_DEPTH, eval_case, eval_kwargs
    from exact_inputs import bit_checksum
    from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator, backproject, plain_chamfer

    seen = {}
    chamfer, pointcloud = RM._chamfer_dist, RM.metrics_pointcloud

    def spy_chamfer(pred, target):
        seen['nn'] = chamfer(pred, target)
        return seen['nn']

    def spy_pointcloud(pred, target, mask, K):
        seen['aligned'], seen['mask'] = pred.copy(), mask.copy()
        return pointcloud(pred, target, mask, K)
    RM._chamfer_dist = spy_chamfer
    sys.modules['src.core.evaluator'].metrics_pointcloud = spy_pointcloud

    rec = {'chk': [], 'nvals': [], 'nq': [], 'medians': [], 'meta_min': MIN_DEPTH}
    values, pred_nn, target_nn = [], [], []
    for k, c in enumerate(EVAL_CASES):
        ins = eval_case(k)
        rec['chk'].append(sum(bit_checksum(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))) for v in ins.values() if v is not None))
        kw = eval_kwargs(k)
        ev = RefEvaluator(**kw)
        align = ev.align

        def spy_align(p, t, inv=False):
            seen['med'] = (np.median(p), np.median(t))
            return align(p, t, inv=inv)
        ev.align = spy_align
        seen.clear()
        mask = None if ins['mask'] is None else ins['mask'].copy()
        ms = ev(ins['pred'].copy(), ins['target'].copy(), list(c['metrics']), K=ins['K'].copy(), mask=mask)
        rec[f'keys_{k}'] = '|'.join(ms)
        rec['nvals'].append(len(ms)); values += list(ms.values())
        if not ms:
            rec['nq'].append(0); rec['medians'].append((0.0, 0.0))
            print(f'eval[{k}] {c["name"]}: empty')
            continue
        rec['medians'].append(seen['med'])
        p_nn, t_nn = (np.atleast_1d(v) for v in seen['nn'])
        rec['nq'].append(len(p_nn)); pred_nn.append(p_nn); target_nn.append(t_nn)

        # the margins
        m, p, t = seen['mask'], seen['aligned'], ins['target']
        q = np.maximum(t[m]/p[m], p[m]/t[m]).astype(np.float64)
        for th in (1.05, 1.1, 1.25, 1.25**2, 1.25**3): assert np.abs(q/th - 1).min() > 1e-5, f'case {k}: a ratio within 1e-5 of the delta threshold {th}'
        for th in (0.05, 0.1, 0.2):
            for d in (p_nn, t_nn):
                assert np.abs(d.astype(np.float64)/th - 1).min() > 1e-5, f'case {k}: a neighbour distance within 1e-5 of {th}'
                assert abs((d < th).mean() - 1e-3) > 1e-5, f'case {k}: P or R within 1e-5 of 1e-3'

        # this package's plain path on the same inputs: the aligned depth bit for bit, the distances to 1e-6
        mine = MonoDepthEvaluator(**kw, device='cpu')
        x = torch.from_numpy(ins['pred'])
        x = (x > 0)/x.clamp(min=torch.finfo(torch.float32).eps)
        aligned = mine.scale(x, ms['Scale'], ms['Shift'], inv=c['align'] == 'lsqr').numpy()
        assert np.array_equal(aligned[m], p[m]), f'case {k}: the plain path does not form the reference\'s aligned depth'
        K_inv = torch.linalg.inv(torch.from_numpy(ins['K']))
        mm = torch.from_numpy(m).flatten()
        mine_nn = plain_chamfer(backproject(torch.from_numpy(aligned), K_inv)[mm], backproject(torch.from_numpy(t), K_inv)[mm])
        worst = max(float(np.abs(a.numpy() - b).max()/max(float(b.max()), 1e-30)) if (b == 0).any() else float(np.abs(a.numpy()/b - 1).max())
                    for a, b in zip(mine_nn, (p_nn, t_nn)))
        assert worst <= 1e-6, (k, worst)
        print(f'eval[{k}] {c["name"]}: n = {int(m.sum())}, {len(ms)} values, Scale {ms["Scale"]:.6f} Shift {ms["Shift"]:.6f}; plain distances within {worst:.2e}')
    rec['chk'] = np.array(rec['chk'], dtype=np.int64)
    rec['nvals'], rec['nq'] = np.array(rec['nvals'], dtype=np.int64), np.array(rec['nq'], dtype=np.int64)
    rec['medians'] = np.array(rec['medians'], dtype=np.float32)
    rec['values'] = np.array(values, dtype=np.float64)
    rec['pred_nn'], rec['target_nn'] = np.concatenate(pred_nn).astype(np.float32), np.concatenate(target_nn).astype(np.float32)
    save('eval_reference', rec)


if __name__ == '__main__':
    main()
