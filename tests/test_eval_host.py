"""Offline evaluation on the CPU: the plain path of `MonoDepthEvaluator` against the REFERENCE's fixture (tests/golden/eval_reference.npz), `run`'s
bookkeeping, the reference's oddities that are kept (stated as such), `np.median`'s even-count rule, the command line, and the C symbols.

The bounds (shared with test_gpu_eval.py through `check_case`):
  * Scale under 'median': within one float32 ulp of the reference's; the delta values: 1e-6 relative (the counts are identical: the generator refused inputs
    with a ratio within 1e-5 of a threshold);
  * Chamfer: 2e-6 relative; F-Score / IoU: 1e-6 relative (identical counts under the generator's margins);
  * every other value, and Scale / Shift under 'lsqr': the error against `restate_fp64` — the same formulas in float64 from the same float32 inputs — is at
    most 4x the reference's own float32 error against it, with a floor of one float32 ulp of the value."""
import json
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, parity_note
from eval_inputs import EVAL_CASES, MIN_DEPTH, eval_case, eval_expected, eval_kwargs

NEW_SYMBOLS = ('smd_eval_metrics', 'smd_eval_pointcloud', 'smd_eval_metrics_workspace_bytes', 'smd_eval_pointcloud_workspace_bytes')
DELTAS = ('$\\delta_{.05}$', '$\\delta_{.1}$', '$\\delta_{.25}$', '$\\delta_{.25^2}$', '$\\delta_{.25^3}$')
POINTCLOUD = ('Chamfer', 'F-Score (5)', 'IoU (5)', 'F-Score (10)', 'IoU (10)', 'F-Score (20)', 'IoU (20)')


@pytest.fixture(scope='module')
def fixture(): return load_golden('eval_reference')


def ulp32(v: float) -> float: return float(np.spacing(np.float32(abs(v))))


def restate_fp64(ins: dict, kw: dict) -> dict:
    """evaluator.py:65-94 with metrics.py:39-105 in float64 from the float32 inputs (same shape: no resize): both groups' values under 'eigen/..' and
    'benchmark/..' names, Scale and Shift."""
    eps = float(np.finfo(np.float32).eps)
    inv = lambda x: (x > 0)/np.maximum(x, eps)
    d, t = ins['pred'].astype(np.float64), ins['target'].astype(np.float64)
    p = inv(d)
    m = (t > kw['min']) & (p > 0)
    if kw['max']: m &= t < kw['max']
    if ins['mask'] is not None: m &= ins['mask']
    pm, tm = p[m], t[m]
    if kw['align_mode'] == 'median': a, b = np.median(tm)/np.median(pm), 0.0
    elif kw['align_mode'] == 'lsqr':
        x, y = inv(pm), inv(tm)
        a, b = np.linalg.solve(np.array([[(x*x).sum(), x.sum()], [x.sum(), float(x.size)]]), np.array([(x*y).sum(), y.sum()]))
    else: a, b = float(kw['align_mode'] or 1), 0.0
    q = inv(a*inv(pm) + b) if kw['align_mode'] == 'lsqr' else a*pm + b
    q = np.clip(q, kw['min'], kw['max'])
    err, l = np.abs(q - tm), np.log(q) - np.log(tm)
    iv = 1000*np.abs(1/q - 1/tm)
    th = np.maximum(tm/q, q/tm)
    out = {'Scale': float(a), 'Shift': float(b),
           'eigen/AbsRel': (err/tm).mean(), 'eigen/SqRel': (err**2/tm).mean(), 'eigen/RMSE': np.sqrt((err**2).mean()), 'eigen/LogRMSE': np.sqrt((l**2).mean()),
           'benchmark/MAE': err.mean(), 'benchmark/RMSE': np.sqrt((err**2).mean()), 'benchmark/InvMAE': iv.mean(), 'benchmark/InvRMSE': np.sqrt((iv**2).mean()),
           'benchmark/LogMAE': np.abs(100*l).mean(), 'benchmark/LogRMSE': np.sqrt(((100*l)**2).mean()),
           'benchmark/LogSI': np.sqrt(((100*l)**2).mean() - (100*l).mean()**2), 'benchmark/AbsRel': (100*err/tm).mean(), 'benchmark/SqRel': (100*err**2/tm**2).mean()}
    for name, v in zip(DELTAS, (1.05, 1.1, 1.25, 1.25**2, 1.25**3)): out[f'eigen/{name}'] = 100*(th < v).mean()
    return {k: float(v) for k, v in out.items()}


def owners(metrics) -> dict:
    """Which group's value a merged key holds after `ms |= ...` in the caller's order: the last group that has it."""
    from slowtv_monodepth_amd.eval_metrics import BENCHMARK_KEYS, EIGEN_KEYS
    own = {}
    for m in metrics:
        for k in {'eigen': EIGEN_KEYS, 'benchmark': BENCHMARK_KEYS}.get(m, ()): own[k] = m
    return own


def check_case(k: int, got: dict, fixture: dict, tag: str, lines=None) -> list:
    """Compare one item's metric dict with the reference's under the bounds of the module docstring -> the list of misses (empty: pass).  Every quantity's
    error and the reference's own go to the parity log (and to `lines`)."""
    ref, _, _, _ = eval_expected(fixture, k)
    if list(got) != list(ref): return [f'case {k}: keys {list(got)} != {list(ref)}']
    if not ref: return []
    c, kw = EVAL_CASES[k], eval_kwargs(k)
    r64, own, bad = restate_fp64(eval_case(k, fixture), kw), owners(c['metrics']), []
    for name, v in got.items():
        r = ref[name]
        if name in POINTCLOUD or name in DELTAS or (name == 'Scale' and c['align'] == 'median'):
            tol = ulp32(r) if name == 'Scale' else (2e-6 if name == 'Chamfer' else 1e-6)*abs(r)
            e_mine, e_ref = abs(v - r), 0.0
        else:
            exact = r64[name if name in ('Scale', 'Shift') else f'{own[name]}/{name}']
            e_mine, e_ref = abs(v - exact), abs(r - exact)
            tol = max(4*e_ref, ulp32(exact))
        line = f'eval_parity {tag} case {k} {c["name"]:<20} {name:<18} value {r:.9g} error {e_mine:.3e} reference\'s {e_ref:.3e} bound {tol:.3e}'
        parity_note(line)
        if lines is not None: lines.append(line)
        if not e_mine <= tol: bad.append(line)
    return bad


def _evaluator(k, **over):
    from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator
    return MonoDepthEvaluator(**{**eval_kwargs(k), **over}, device='cpu')


@pytest.mark.parametrize('k', range(len(EVAL_CASES)), ids=[c['name'] for c in EVAL_CASES])
def test_the_plain_path_matches_the_reference_fixture(fixture, k):
    """Same keys in the same merge order, values within the bounds; the empty item returns {}; the caller's mask is not touched."""
    ins = eval_case(k, fixture)
    mask = None if ins['mask'] is None else ins['mask'].copy()
    got = _evaluator(k)(ins['pred'], ins['target'], list(EVAL_CASES[k]['metrics']), K=ins['K'], mask=mask)
    if EVAL_CASES[k]['name'] == 'empty': assert got == {}
    if mask is not None: assert np.array_equal(mask, ins['mask'])
    assert check_case(k, got, fixture, 'plain') == []


def test_the_plain_nearest_neighbours_match_the_reference(fixture):
    """Per-query distances of both directions against `_chamfer_dist`'s, <= 1e-6 relative (exact zeros stay zeros)."""
    from slowtv_monodepth_amd.evaluator import backproject, plain_chamfer
    for k, c in enumerate(EVAL_CASES):
        ref, p_nn, t_nn, _ = eval_expected(fixture, k)
        if not ref: continue
        depth, mask, ins = aligned_depth(k, fixture)
        K_inv = torch.linalg.inv(torch.from_numpy(ins['K']))
        m = torch.from_numpy(mask).flatten()
        got = plain_chamfer(backproject(torch.from_numpy(depth), K_inv)[m], backproject(torch.from_numpy(ins['target']), K_inv)[m])
        for a, b in zip(got, (p_nn, t_nn)): assert np.all(np.abs(a.numpy() - b) <= 1e-6*b)


def aligned_depth(k, fixture):
    """-> (the reference's aligned depth, its mask, the inputs) of case k, formed from the fixture's Scale and Shift by the plain `scale` (the generator checked
    that this gives the reference's bits)."""
    ins, kw = eval_case(k, fixture), eval_kwargs(k)
    ref, *_ = eval_expected(fixture, k)
    ev = _evaluator(k)
    x = torch.from_numpy(ins['pred'])
    x = (x > 0)/x.clamp(min=torch.finfo(torch.float32).eps)
    t = torch.from_numpy(ins['target'])
    mask = ev.get_mask(t) & (x > 0)
    if ins['mask'] is not None: mask &= torch.from_numpy(ins['mask'])
    return ev.scale(x, ref['Scale'], ref['Shift'], inv=kw['align_mode'] == 'lsqr').numpy(), mask.numpy(), ins


def _dataset(ks, fixture):
    items = [eval_case(k, fixture) for k in ks]
    return [i['pred'] for i in items], {'depth': [i['target'] for i in items], 'K': [i['K'] for i in items]}


def test_run_averages_without_the_empty_items_and_appends_categories(fixture, capsys):
    ks = [0, 6, 4]                                     # 6 is the empty item
    preds, data = _dataset(ks, fixture)
    data['cat'], data['subcat'] = ['a', 'b', 'c'], ['x', 'y', 'z']
    ev = _evaluator(0, metrics=('eigen', 'pointcloud'))
    mean, items = ev.run(preds, data, nproc=3, chunks=2)
    assert len(items) == 2 and [m['Cat'] for m in items] == ['a', 'c'] and [m['SubCat'] for m in items] == ['x', 'z']
    assert 'Cat' not in mean and mean['AbsRel'] == np.mean([m['AbsRel'] for m in items]) and 'Chamfer' in mean
    assert 'AbsRel' in capsys.readouterr().out        # `summarize` prints a plain table
    one, items1 = ev.run(preds, data, max_items=1)
    assert len(items1) == 1 and one['RMSE'] == items[0]['RMSE']


def test_run_refuses_what_the_reference_refuses(fixture):
    preds, data = _dataset([0, 4], fixture)
    with pytest.raises(ValueError, match='Non-matching preds and targets'): _evaluator(0).run(preds[:1], data)
    with pytest.raises(ValueError, match='Missing intrinsics'): _evaluator(0).run(preds, {'depth': data['depth']})
    with pytest.raises(ValueError, match='Missing edge masks'): _evaluator(0, metrics=('eigen', 'ibims')).run(preds, data)
    edge = [np.ones_like(t, dtype=bool) for t in data['depth']]
    with pytest.raises(NotImplementedError, match='ibims'): _evaluator(0, metrics=('eigen', 'ibims')).run(preds, {**data, 'edge': edge})
    with pytest.raises(NotImplementedError, match='ibims'): _evaluator(0)(preds[0], data['depth'][0], ['ibims'])
    # edge masks without 'ibims' are evaluated as the reference does: a second pass with the edges as masks, reported as '<name>-Edges'; the masks stay as they were
    mean, items = _evaluator(0, metrics=('eigen',)).run(preds, {**data, 'edge': edge})
    assert 'AbsRel-Edges' in items[0] and items[0]['AbsRel-Edges'] == items[0]['AbsRel'] and all(e.all() for e in edge)


def test_the_crop_flags_are_swapped_as_in_the_reference():
    """evaluator.py:179-180: `use_eigen_crop` applies the NYU-D rectangle (which asserts 480x640), `use_nyud_crop` the Eigen rectangle.  Kept, and stated."""
    from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator
    t = torch.ones(480, 640)
    m = MonoDepthEvaluator(use_eigen_crop=True, device='cpu').get_mask(t)
    assert m[45:471, 41:601].all() and int(m.sum()) == 426*560
    with pytest.raises(AssertionError): MonoDepthEvaluator(use_eigen_crop=True, device='cpu').get_mask(torch.ones(24, 32))
    ev = MonoDepthEvaluator(use_nyud_crop=True, device='cpu')
    m = ev.get_mask(torch.ones(24, 32))
    c = np.array([0.40810811*24, 0.99189189*24, 0.03594771*32, 0.96405229*32], dtype=int)
    assert int(m.sum()) == (c[1] - c[0])*(c[3] - c[2]) and m[c[0]:c[1], c[2]:c[3]].all()
    assert ev._crop((24, 32)) == tuple(int(v) for v in c) and MonoDepthEvaluator(use_eigen_crop=True, use_nyud_crop=True, device='cpu')._crop((480, 640)) == (195, 471, 41, 601)
    # 480x640 with a little content: the evaluator scores only what lies inside the NYU-D rectangle
    target, pred = torch.zeros(480, 640), torch.ones(480, 640)
    target[40:50, 36:46] = 2.0
    got = MonoDepthEvaluator(align_mode=1, use_eigen_crop=True, device='cpu')(pred, target, ['benchmark'])
    assert got['MAE'] == 1.0 and MonoDepthEvaluator(align_mode=1, use_eigen_crop=True, device='cpu').get_mask(target).sum() == 25


@pytest.mark.parametrize('n', [1, 2, 7, 8, 451, 642])
def test_the_even_count_median_is_np_medians(n):
    from slowtv_monodepth_amd.evaluator import median
    x = (0.5 + 40*torch.rand(n, generator=torch.Generator().manual_seed(n))).float()
    assert median(x).numpy().tobytes() == np.median(x.numpy()).tobytes() and median(x).dtype == torch.float32


def test_a_subclass_that_overrides_a_step_is_honoured(fixture):
    from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator

    class Halved(MonoDepthEvaluator):
        def align(self, pred, target, inv=False): return 0.5, 0.0
    ins = eval_case(4, fixture)
    ev = Halved(**eval_kwargs(4), device='cpu')
    assert not ev._fused(torch.from_numpy(ins['pred']), torch.from_numpy(ins['target']))
    assert ev(ins['pred'], ins['target'], ['eigen'])['Scale'] == 0.5


def test_the_command_line_round_trip(tmp_path, capsys):
    """predict's output format -> evaluate --synthetic-data 2 at 64x96 on the CPU -> metrics.json with the mean and the per-item list."""
    from slowtv_monodepth_amd import evaluate
    data = evaluate.synthetic_targets(2, (64, 96), seed=42)
    from slowtv_monodepth_amd.synthetic import lidar_depth
    dense = torch.cat([lidar_depth(torch.Generator().manual_seed(42 + i), 2, 64, 96, density=2.0)[:1, 0] for i in range(2)])   # the targets' field without its holes
    assert torch.equal(torch.where(torch.from_numpy(data['depth']) > 0, dense, torch.zeros(())), torch.from_numpy(data['depth']))
    preds = (1/(3.0*dense)).numpy()[:, ::2, ::2]       # a perfect prediction in other units, at half size
    np.savez(tmp_path/'preds.npz', preds=preds)
    evaluate.main(['--preds', str(tmp_path/'preds.npz'), '--synthetic-data', '2', '--shape', '64', '96', '--device', 'cpu', '--max', '80', '--out', str(tmp_path/'m.json')])
    out = json.loads((tmp_path/'m.json').read_text())
    assert len(out['items']) == 2 and set(out['mean']) == set(k for k, v in out['items'][0].items() if isinstance(v, float))
    assert 'Chamfer' in out['mean'] and out['mean']['AbsRel'] < 5 and 0.3 < out['mean']['Scale'] < 0.37     # the prediction's depth is 3x the target's
    np.savez(tmp_path/'targets.npz', **data)
    evaluate.main(['--preds', str(tmp_path/'preds.npz'), '--targets', str(tmp_path/'targets.npz'), '--device', 'cpu', '--max', '80', '--out', str(tmp_path/'m2.json')])
    assert json.loads((tmp_path/'m2.json').read_text()) == out
    with pytest.raises(SystemExit): evaluate.main(['--preds', str(tmp_path/'preds.npz'), '--out', str(tmp_path/'m3.json')])


def test_the_new_symbols_are_declared_in_all_four_places():
    from slowtv_monodepth_amd import _lib, functional
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    csrc = ROOT/'slowtv_monodepth_amd'/'csrc'
    api, kernels = (csrc/'smd_api.hip').read_text(), (csrc/'smd_kernels.h').read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in the header'
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', api), f'{name} is not defined in smd_api.hip'
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name)
    assert 'launch_eval_metrics' in kernels and 'launch_eval_pointcloud' in kernels
    assert 'evaluator.py:65-94' in header and 'metrics.py:111-165' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_eval.hip' in (csrc/'Makefile').read_text() and 'getenv' not in (csrc/'smd_eval.hip').read_text()
    assert not any('eval' in n for n in functional.__all__)       # (the hostile-memory case table is `__all__`; these operators' cases live in test_gpu_eval.py)


def test_the_abi_refuses_bad_arguments_without_a_gpu():
    from slowtv_monodepth_amd import _lib
    p = 4096                                           # never dereferenced: every call below is refused first
    def metrics(b=1, h=4, w=4, H=4, W=4, lo=1e-3, hi=0.0, mode=1, flags=3, ws=1 << 30, disp=p):
        return _lib.call('smd_eval_metrics', disp, p, None, b, h, w, H, W, 0, H, 0, W, lo, hi, mode, 1.0, flags, p, p, p, p, None, None, None, p, ws, None)
    for kw in (dict(disp=None), dict(b=0), dict(lo=-1.0), dict(hi=1e-4), dict(mode=3), dict(flags=0), dict(flags=8 | 1)):
        with pytest.raises(ValueError): metrics(**kw)
    with pytest.raises(_lib.HotpathError): metrics(ws=16)
    assert _lib.lib.smd_eval_metrics_workspace_bytes(70000, 4, 4) == 0 and _lib.lib.smd_eval_pointcloud_workspace_bytes(1, 1 << 15, 1 << 15) == 0
    with pytest.raises(ValueError): _lib.call('smd_eval_pointcloud', p, p, p, p, p, 1, 1 << 15, 1 << 15, p, p, p, p, 1 << 30, None)
    with pytest.raises(ValueError): _lib.call('smd_eval_pointcloud', p, p, None, p, p, 1, 4, 4, p, p, p, p, 1 << 30, None)
