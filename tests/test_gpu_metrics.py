"""`functional.depth_metrics` (smd_depth_metrics) and `MonoDepthModule.compute_metrics` / `validation_step` on the GPU.

Exact outputs: `counts`, `med_t` (it does not depend on the resample) and, at equal sizes, `med_p` — bit-equal to `torch.nanmedian` of the masked tensors.
Outputs held to a tolerance: `med_p` under a resample and the five values.  The tolerance is not a constant: for each case the ATen fp32 sequence
(`interpolate`, `nanmedian`, the metric classes) is evaluated on the same device, its relative error against the fp64 restatement below is taken per OUTPUT
NUMBER (`med_p` and each of the five metrics, of each sample), and the kernel's same number is held to 4 x that error, floor 1e-6 relative — four times
because the kernel's summation order differs from ATen's and both are a few ulp from fp64.  Measured errors: profiles/val_metrics_times.txt."""
import copy

import numpy as np
import pytest
import torch

from conftest import parity_note
from metrics_cases import CASES, make_case

from slowtv_monodepth_amd import _lib, functional as F, metrics as M
from slowtv_monodepth_amd.synthetic import make_batch
from slowtv_monodepth_amd.trainer import MonoDepthModule

pytestmark = pytest.mark.gpu
NAMES = ['MAE', 'RMSE', 'LogSI', 'AbsRel', 'Acc']


def restate(pred, target, min_depth=None, max_depth=None):
    """The metrics in fp64 with numpy, from their definition: -> values (b,5), medians (b,2), counts (b), and the smallest |q - 1.25| per sample.
    The inputs and the two range bounds are fp32 numbers (the operator is fp32); everything computed from them is fp64."""
    lo, hi = float(np.float32(min_depth or 0.1)), float(np.float32(max_depth or 100))
    p, t = pred.double().cpu().numpy()[:, 0], target.double().cpu().numpy()[:, 0]
    b, h, w = p.shape
    H, W = t.shape[1:]
    if (h, w) == (H, W): p0 = p
    else:
        def taps(n_in, n_out):
            src = np.maximum((np.arange(n_out) + 0.5)*(n_in/n_out) - 0.5, 0.0)
            i0 = np.minimum(np.floor(src).astype(int), n_in - 1)
            return i0, np.minimum(i0 + 1, n_in - 1), src - i0
        y0, y1, fy = taps(h, H); x0, x1, fx = taps(w, W)
        fy, fx = fy[None, :, None], fx[None, None, :]
        top = (1 - fx)*p[:, y0][:, :, x0] + fx*p[:, y0][:, :, x1]
        bot = (1 - fx)*p[:, y1][:, :, x0] + fx*p[:, y1][:, :, x1]
        p0 = (1 - fy)*top + fy*bot
    p0 = np.clip(p0, lo, hi)
    values, medians, counts, margin = np.full((b, 5), np.nan), np.full((b, 2), np.nan), np.zeros(b, dtype=np.int64), np.full(b, np.inf)
    for i in range(b):
        with np.errstate(invalid='ignore'): m = (t[i] > lo) & (t[i] < hi)
        n = counts[i] = int(m.sum())
        if n == 0: continue
        pv, tv = p0[i][m], t[i][m]
        medians[i] = np.sort(pv)[(n - 1)//2], np.sort(tv)[(n - 1)//2]
        pa = np.clip(pv*(medians[i, 1]/medians[i, 0]), lo, hi)
        d, e, q = pa - tv, np.log(pa) - np.log(tv), np.maximum(tv/pa, pa/tv)
        values[i] = (np.abs(d).mean(), np.sqrt((d*d).mean()), 100*np.sqrt((e*e).mean() - e.mean()**2), 100*(np.abs(d)/tv).mean(), 100*(q < 1.25).sum()/q.sum())
        margin[i] = np.abs(q - 1.25).min()
    return values, medians, counts, margin


def aten_sequence(pred, target, min_depth=None, max_depth=None):
    """The reference's sequence in fp32 on ATen, per sample: -> values (b,5), medians (b,2) (masked `nanmedian`s)."""
    lo, hi = min_depth or 0.1, max_depth or 100
    p = torch.nn.functional.interpolate(pred, size=target.shape[-2:], mode='bilinear', align_corners=False).clamp(lo, hi)
    mask = (target > lo) & (target < hi)
    nan = target.new_tensor(float('nan'))
    t, p = target.where(mask, nan).flatten(1), p.where(mask, nan).flatten(1)
    mt, mp = t.nanmedian(dim=1, keepdim=True).values, p.nanmedian(dim=1, keepdim=True).values
    p, t = (p*(mt/mp)).clamp(lo, hi), t.clamp(lo, hi)
    ms = [M.MAE(), M.RMSE(), M.ScaleInvariant(mode='log'), M.AbsRel(), M.DeltaAcc(delta=1.25)]
    values = torch.stack([m.sf*m._compute(m._preprocess(p), m._preprocess(t)) for m in ms], dim=1)
    return values, torch.cat([mp, mt], dim=1)


def _bits(ts): return [t.cpu().contiguous().view(torch.int32) for t in ts]


_cache = {}


def case_results(name):
    """Inputs, the kernel's outputs, the ATen sequence and the fp64 restatement of a case: computed once, shared by the tests, never modified."""
    if name not in _cache:
        pred, target, lo, hi = make_case(name)
        pd, td = pred.cuda(), target.cuda()
        out = F.depth_metrics(pd, td, lo, hi)
        aten = aten_sequence(pd, td, lo, hi)
        torch.cuda.synchronize()
        _cache[name] = dict(pred=pd, target=td, lo=lo, hi=hi, out=tuple(o.cpu() for o in out), aten=tuple(o.cpu() for o in aten), ref=restate(pred, target, lo, hi))
    return _cache[name]


def rel_err(got, ref):
    """|got - ref|/|ref| per number; where ref is 0 the error is 0 for an exact 0 and infinite otherwise."""
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.abs(got - ref)/np.abs(ref)
    return np.where(np.abs(got - ref) == 0, 0.0, e)


def check_against_aten(tag, got, aten, ref):
    """Hold every number of `got` to 4 x the ATen sequence's relative error on that number (floor 1e-6); print both errors first."""
    e_aten, e_hip = rel_err(aten, ref), rel_err(got, ref)
    parity_note(f'{tag} largest rel. error vs fp64 per column: ATen ' + ' '.join(f'{v:.2e}' for v in e_aten.max(axis=0)) + ' | HIP ' + ' '.join(f'{v:.2e}' for v in e_hip.max(axis=0)))
    bound = np.maximum(4*e_aten, 1e-6)
    assert (e_hip <= bound).all(), (tag, e_hip, bound)


@pytest.mark.parametrize('case', CASES)
def test_depth_metrics_against_the_fp64_restatement(case):
    c = case_results(case)
    values, medians, counts = (o.numpy() for o in c['out'])
    av, am = (o.numpy() for o in c['aten'])
    rv, rm, rc, margin = c['ref']
    assert counts.dtype == np.int32 and counts.tolist() == rc.tolist()
    ok = rc > 0
    assert np.isnan(values[~ok]).all() and np.isnan(medians[~ok]).all()                  # n = 0: NaN in all five (and no median)
    assert (margin[ok] > 2e-6).all(), 'a ratio sits on the 1.25 threshold (fp32 ratios are within a few ulp = 1e-6 of the fp64 ones): pick another seed'
    assert (medians[ok, 1].view(np.uint32) == am[ok, 1].view(np.uint32)).all()              # med_t: bit-equal to torch.nanmedian
    assert (medians[ok, 1] == rm[ok, 1].astype(np.float32)).all()
    if c['pred'].shape[-2:] == c['target'].shape[-2:]:                                      # equal sizes: the resize returns its input, med_p is exact too
        assert (medians[ok, 0].view(np.uint32) == am[ok, 0].view(np.uint32)).all()
        assert (medians[ok, 0] == rm[ok, 0].astype(np.float32)).all()
    got = np.concatenate([medians[ok, :1], values[ok]], axis=1).astype(np.float64)
    aten = np.concatenate([am[ok, :1], av[ok]], axis=1).astype(np.float64)
    ref = np.concatenate([rm[ok, :1], rv[ok]], axis=1)
    check_against_aten(f'depth_metrics[{case}] (med_p, ' + ', '.join(NAMES) + ')', got, aten, ref)
    if case == 'equal': assert rc[0] % 2 == 1 and rc[1] % 2 == 0 and rc[2] == 0
    if case == 'tiny': assert rc.tolist() == [1, 2]
    if case == 'ties':
        assert all(len(np.unique(t[t > 0])) == 4 for t in c['target'].cpu().numpy()) and (medians[:, 0] == 100).all()
    if case == 'multi': assert _lib.lib.smd_depth_metrics_workspace_bytes(2, 96, 320) > 0 and 96*320 > 4096      # more than one block per sample


def test_non_contiguous_prediction_and_cpu_device_mix():
    c = case_results('up')
    wide = torch.zeros(2, 1, 6, 20, device='cuda')
    wide[..., ::2] = c['pred']
    out = F.depth_metrics(wide[..., ::2], c['target'], c['lo'], c['hi'])                    # made contiguous, as every operator's operands are
    for a, b in zip(_bits(out), _bits(c['out'])): assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match='same device'): F.depth_metrics(c['pred'].cpu(), c['target'])
    with pytest.raises(TypeError, match='float32'): F.depth_metrics(c['pred'].double(), c['target'].double())


def test_two_calls_and_a_dirty_workspace_agree_bit_for_bit(monkeypatch, knobs):
    c = case_results('multi')
    again = F.depth_metrics(c['pred'], c['target'])
    for a, b in zip(_bits(again), _bits(c['out'])): assert torch.equal(a, b)
    # a reused workspace full of garbage: the call zeroes what it accumulates into
    from slowtv_monodepth_amd import metric_ops
    nbytes = _lib.lib.smd_depth_metrics_workspace_bytes(2, 96, 320)
    dirty = torch.full((nbytes,), 0xA5, device='cuda', dtype=torch.uint8)
    monkeypatch.setattr(metric_ops, '_workspace', lambda device, query, *args, floor=0: (dirty, query(*args)))
    third = F.depth_metrics(c['pred'], c['target'])
    fourth = F.depth_metrics(c['pred'], c['target'])                                        # ... now dirtied by the call before it
    for out in (third, fourth):
        for a, b in zip(_bits(out), _bits(c['out'])): assert torch.equal(a, b)
    # the recomputing variant computes the same bits as the default, which stores the resampled prediction in its first pass
    for case in ('multi', 'down', 'equal'):
        cc = case_results(case)
        knobs('metrics_store_pred', 0)
        recomputed = F.depth_metrics(cc['pred'], cc['target'], cc['lo'], cc['hi'])
        knobs('metrics_store_pred', 1)
        for a, b in zip(_bits(recomputed), _bits(cc['out'])): assert torch.equal(a, b), case


def test_batch_of_64_samples():
    pred, target, _, _ = make_case('up')
    pred, target = pred.repeat(32, 1, 1, 1).cuda(), target.repeat(32, 1, 1, 1).cuda()
    values, medians, counts = F.depth_metrics(pred, target)
    ref = case_results('up')['out']
    for a, b in zip(_bits((values, medians, counts)), _bits(ref)): assert torch.equal(a, b.repeat(32, *([1]*(b.ndim - 1))))


_CFG = {'net': {'depth': {'enc_name': 'resnet18', 'pretrained': False}, 'pose': {'enc_name': 'resnet18'}},
        'loss': {'img_recon': {'weight': 1, 'use_min': True, 'use_automask': True}, 'disp_smooth': {'weight': 0.001, 'use_edges': True}},
        'optimizer': {'type': 'adamw', 'lr': 1e-4}, 'trainer': {'min_depth': 0.1, 'max_depth': 100}}


@pytest.fixture(scope='module')
def module():
    torch.manual_seed(0)
    return MonoDepthModule(copy.deepcopy(_CFG)).cuda().eval()


def test_nothing_synchronises(module):
    c = case_results('multi')
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = F.depth_metrics(c['pred'], c['target'])
        met = module.compute_metrics(c['pred'], c['target'])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b in zip(_bits(out), _bits(c['out'])): assert torch.equal(a, b)
    assert list(met) == NAMES
    for k, name in enumerate(NAMES):
        assert met[name].is_cuda and torch.equal(met[name].cpu(), c['out'][0][:, k].sum()/2)
        assert int(module.metrics[name].total) == 2
    for m in module.metrics.values(): m.reset()


def test_validation_step_fused_and_generic_paths_agree(module):
    """The network cannot run below 64 rows (its last stage reflection-pads a feature map of h/32 rows), so the step runs at 64x96 with a 37x121 target."""
    batch = make_batch(2, 64, 96, (-1, 1), seed=3, device='cuda', depth_shape=(37, 121))
    with torch.no_grad():
        loss, ld, fwd, met = module.validation_step(tuple(dict(d) for d in batch))
        assert 'single node' in module.backend.last_path                                    # the fused loss path ran: `depth_up` is the stack it handed back
        depth = fwd['depth_up'][0]
        generic = module.compute_metrics(depth, batch[1]['depth'], fused=False)
        # ... and with the handlers' path (separate autograd nodes) the same metrics come out
        module.want_aux = True
        try: _, _, fwd2, met2 = module.validation_step(tuple(dict(d) for d in batch))
        finally: module.want_aux = False
        assert 'handlers' in module.backend.last_path
    assert list(met) == NAMES and all(not v.requires_grad for v in met.values()) and all(p.grad is None for p in module.parameters())
    target = batch[1]['depth']
    for tag, d, got in (('fused loss path', depth, met), ('handlers path', fwd2['depth_up'][0], met2)):
        rv, _, rc, margin = restate(d, target, 0.1, 100)
        assert (rc > 0).all() and (margin > 2e-6).all()
        gen = generic if d is depth else module.compute_metrics(d, target, fused=False)
        stack = lambda m: np.array([[float(m[k]) for k in NAMES]], dtype=np.float64)
        check_against_aten(f'validation_step, {tag} (' + ', '.join(NAMES) + ')', stack(got), stack(gen), rv.mean(axis=0, keepdims=True))
    torch.testing.assert_close(fwd2['depth_up'][0], depth, rtol=1e-5, atol=0)                 # the two paths hand the metrics the same depth map
    assert all(int(m.total) >= 6 for m in module.metrics.values())                          # every call went through the states
    for m in module.metrics.values(): m.reset()
