#!/usr/bin/env python3
"""Golden vectors for the image-logging operators, made by IMPORTING the reference (build container only; make_golden.py's import shim and writer).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_viz.py

Reference entry points driven here: src/tools/viz.py:20-50 `rgb_from_disp`, :54-74 `rgb_from_feat`.

tests/golden/viz_reference.npz, per case k of viz_inputs.DISP_CASES: `disp_in_k`, `disp_out_k` (float64, as the reference returns it), `disp_vmax_k` (float32
per item: np.percentile(d[d > 0], 95), 0 without a positive value).  Per case k of FEAT_CASES: `feat_in_k`, `feat_out_k` (float32), `feat_err_k` = the largest
error of the reference's result against viz_inputs.pca_fp64 of the same input, `feat_solver_k` the solver sklearn's 'auto' ran.  Data only.

Disparity inputs: one item without a positive value, one with a single one, one with NaNs and negatives, one constant, `invert=True` over zeros.  For every
input the colour index of the float32 sequence equals that of the same sequence in float64 (asserted; a value that disagrees is nudged), so an index is a
property of the input and not of a rounding.

Feature inputs: four factors with squared scales 1, 0.7, 0.45, 0.2 plus 1e-3 noise and channel offsets: the four leading eigenvalues are separated by at
least a tenth of the first (asserted).  Solvers (sklearn 1.7.2, `_fit`): c3 runs `covariance_eigh` (40 samples >= 10 x 3 channels); c16 and c64 run `full`
(max(shape) <= 500); c512 (15 samples, 512 channels) is past 500 with 3 < 0.8 x 15 components, so 'auto' picks `randomized`, which draws from numpy's
global generator: it is seeded here (np.random.seed(0)) so that the fixture is reproducible.  c512_n3 (3 samples, 512 channels: 3 >= 0.8 x 3) runs `full`
at its lower boundary of three samples; it has two non-zero eigenvalues, so only its first two components are recorded as comparable (`feat_err_k` is
taken over them; FEAT_CASES' third field)."""
import numpy as np
import torch

from make_golden import import_reference, save
from viz_inputs import DISP_CASES, FEAT_CASES, leading_eigenvalues, pca_fp64


def disp_input(k, shape):
    g = np.random.default_rng(100 + k)
    d = (0.02 + 0.9*g.random(shape)).astype(np.float32)
    name = DISP_CASES[k][0]
    if name == 'no_positive_and_single':
        d[0] = -d[0]; d[0, 0, 1, 2:5] = 0
        d[1] = 0; d[1, 0, 3, 4] = 0.625; d[1, 0, 0, 0] = -1
    elif name in ('nan_neg_const_zeros', 'invert_with_zeros'):
        d[0, 0, 2, 3:9] = np.nan; d[0, 0, 5:7, 1:4] = -0.5
        d[1] = 0.37
        d[2, 0, ::3, ::4] = 0
    return d


def colour_index(d, vmax, dtype):
    """The index `apply_cmap` + `Colormap.__call__` reach, evaluated in `dtype` (-1: bad)."""
    x = d.astype(dtype)
    v = dtype(vmax)
    with np.errstate(invalid='ignore'):
        x = np.clip(x, dtype(0), v)
        x = (x - dtype(0))/(v - dtype(0) + dtype(1e-5))
        x = x*dtype(256)
        x[x == 256] = 255
        idx = np.where(np.isnan(x), -1, np.clip(np.nan_to_num(x), 0, 255).astype(int))
    return idx


def feat_input(k, shape):
    b, C, h, w = shape
    g = np.random.default_rng(200 + k)
    n = b*h*w
    r = min(4, C, n - 1)
    Z = g.standard_normal((n, r))
    if n - 1 < 4: Z, _ = np.linalg.qr(Z - Z.mean(0))     # so few samples that centring afterwards would undo the scales: centre first (Q's columns stay centred)
    else: Z, _ = np.linalg.qr(Z); Z -= Z.mean(0)
    Wm, _ = np.linalg.qr(g.standard_normal((C, r)))
    s = np.sqrt(np.array([1.0, 0.7, 0.45, 0.2])[:r])*np.sqrt(n)
    X = (Z*s) @ Wm.T + 1e-3*g.standard_normal((n, C)) + g.standard_normal(C)
    return X.reshape(b, h, w, C).transpose(0, 3, 1, 2).astype(np.float32).copy()


def main():
    torch.set_num_threads(1)
    import_reference()
    from sklearn.decomposition import PCA
    from src.tools.geometry import to_inv
    from src.tools.viz import rgb_from_disp, rgb_from_feat
    rec = {}
    for k, (name, shape, invert) in enumerate(DISP_CASES):
        d = disp_input(k, shape)
        for _ in range(10):
            v = to_inv(torch.from_numpy(d)).numpy() if invert else d
            vmax = np.array([np.percentile(x[x > 0], 95) if (x > 0).any() else 0.0 for x in v[:, 0]], dtype=np.float32)
            bad = np.stack([colour_index(v[i], vmax[i], np.float32) != colour_index(v[i], vmax[i], np.float64) for i in range(len(v))])
            if not bad.any(): break
            d[bad] *= np.float32(1.003)
        assert not bad.any(), name
        out = rgb_from_disp(torch.from_numpy(d), invert=invert)
        rec[f'disp_in_{k}'] = d; rec[f'disp_out_{k}'] = out; rec[f'disp_vmax_{k}'] = vmax
        print(f'rgb_from_disp[{k}] {name}: vmax {vmax.tolist()} out {tuple(out.shape)} {out.dtype}')
    for k, (name, shape, ncomp) in enumerate(FEAT_CASES):
        x = feat_input(k, shape)
        ev = leading_eigenvalues(x)
        ev = ev[:min(ncomp + 1, shape[1])]
        assert np.all(-np.diff(ev) >= 0.1*ev[0]), (name, ev)
        X = x.transpose(0, 2, 3, 1).reshape(-1, shape[1])
        np.random.seed(0)
        solver = PCA(n_components=3).fit(X)._fit_svd_solver
        np.random.seed(0)
        with np.errstate(invalid='ignore', divide='ignore'): out = rgb_from_feat(torch.from_numpy(x))
        err = float(np.abs(out.numpy().astype(np.float64) - pca_fp64(x))[:, :ncomp].max())
        rec[f'feat_in_{k}'] = x; rec[f'feat_out_{k}'] = out; rec[f'feat_err_{k}'] = np.float64(err); rec[f'feat_solver_{k}'] = np.array(solver)
        print(f'rgb_from_feat[{k}] {name}: solver {solver}, eigenvalues {ev.round(3).tolist()}, reference fp32 error {err:.3e}')
    save('viz_reference', rec)


if __name__ == '__main__':
    main()
