"""Time the fused validation metrics (`functional.depth_metrics`, both variants of the knob metrics_store_pred) against the ATen sequence of the generic
path, at the validation workload of the reference: b = 12, prediction 192x640, LiDAR target 375x1242 at 5 % density.

HIP events around blocks of calls; the three candidates alternate within one process, round after round, after a warm-up of each.  Also reported: the
number of kernels per call (torch profiler, one call each, outside the timed rounds), the bytes the fused call has to move (the target once per pass,
the prediction's taps at the valid pixels) over its time as a fraction of the read ceiling measured by the library's own STREAM-style kernel, and the
errors of both against an fp64 evaluation.  Appends nothing: prints one report (redirect it to profiles/val_metrics_times.txt).

    python scripts/dev/val_metrics_times.py [--rounds 7] [--calls 50]"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from slowtv_monodepth_amd import _lib, functional as F, metrics as M   # noqa: E402
from slowtv_monodepth_amd.synthetic import lidar_depth                  # noqa: E402


def aten_sequence(pred, target, lo=0.1, hi=100.):
    """What `MonoDepthModule.compute_metrics(fused=False)` runs, returning the five batch values."""
    p = torch.nn.functional.interpolate(pred, size=target.shape[-2:], mode='bilinear', align_corners=False).clamp(lo, hi)
    mask = (target > lo) & (target < hi)
    nan = target.new_tensor(float('nan'))
    t, p = target.where(mask, nan).flatten(1), p.where(mask, nan).flatten(1)
    r = t.nanmedian(dim=1, keepdim=True).values/p.nanmedian(dim=1, keepdim=True).values
    p, t = (p*r).clamp(lo, hi), t.clamp(lo, hi)
    ms = [M.MAE(), M.RMSE(), M.ScaleInvariant(mode='log'), M.AbsRel(), M.DeltaAcc(delta=1.25)]
    return torch.stack([m.sf*m._compute(m._preprocess(p), m._preprocess(t)).sum()/p.shape[0] for m in ms])


def timed(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e)*1e3/calls     # us per call


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:   # the count is a convenience: the times stand without it
        return f'not measured ({type(exc).__name__})'


def read_ceiling(nbytes=1 << 28, reps=10):
    src = torch.empty(nbytes, device='cuda', dtype=torch.uint8).fill_(1); dst = torch.empty_like(src)
    st, best = torch.cuda.current_stream().cuda_stream, 0.0
    for mode in (1, 3, 5):
        for _ in range(2): _lib.lib.smd_debug_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, mode, st)
        us = timed(lambda: _lib.lib.smd_debug_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, mode, st), reps)
        best = max(best, nbytes/(us*1e-6)/1e9)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7); ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--b', type=int, default=12); ap.add_argument('--density', type=float, default=0.05)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    gen = torch.Generator(device='cuda').manual_seed(0)
    b, (h, w), (H, W) = a.b, (192, 640), (375, 1242)
    target = lidar_depth(gen, b, H, W, device='cuda', density=a.density)
    pred = torch.nn.functional.interpolate(lidar_depth(gen, b, H, W, device='cuda', density=1.0), size=(h, w), mode='area')*0.4 \
        * torch.exp(0.2*torch.randn(b, 1, h, w, device='cuda', generator=gen))

    def fused(store):
        def run(): return F.depth_metrics(pred, target, 0.1, 100.)[0]
        def pinned():
            _lib.set_knob('metrics_store_pred', store)
            return run()
        return pinned
    cands = {'fused, recompute (metrics_store_pred=0)': fused(0), 'fused, stored (metrics_store_pred=1)': fused(1), 'ATen sequence': lambda: aten_sequence(pred, target)}
    for fn in cands.values():
        for _ in range(5): fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items(): times[k].append(timed(fn, a.calls))
    n_valid = int(((target > 0.1) & (target < 100)).sum())
    print(f'validation metrics, b={b}, prediction {h}x{w}, target {H}x{W}, {n_valid/(b*H*W)*100:.2f} % valid ({n_valid} pixels); {a.rounds} alternated rounds of {a.calls} calls, us per call')
    for k, v in times.items(): print(f'  {k:42s} median {sorted(v)[len(v)//2]:9.1f}   min {min(v):9.1f}   max {max(v):9.1f}')
    med = {k: sorted(v)[len(v)//2] for k, v in times.items()}
    print(f'  ATen / fused (recompute): {med["ATen sequence"]/med["fused, recompute (metrics_store_pred=0)"]:.1f}x')
    print('kernels per call: ' + ', '.join(f'{k}: {kernel_count(fn)}' for k, fn in cands.items()) + '   (fused, by construction: 1 memset + 4 passes + 1 finish)')
    need = 4*b*H*W*4 + 4*n_valid*4*4          # the target once per pass + four 4-byte taps per valid pixel and pass (upper bound: neighbours share lines)
    ceil = read_ceiling()
    t0 = med['fused, recompute (metrics_store_pred=0)']
    print(f'bytes the recomputing form must move: {need/1e6:.1f} MB -> {need/(t0*1e-6)/1e9:.0f} GB/s = {need/(t0*1e-6)/1e9/ceil:.3f} of the measured read ceiling ({ceil:.0f} GB/s)')
    # errors against fp64 (same sequence evaluated in double on the device)
    _lib.set_knob('metrics_store_pred', 0)
    ref = aten_sequence(pred.double(), target.double()).cpu()
    got = F.depth_metrics(pred, target, 0.1, 100.)[0].double().mean(dim=0).cpu()
    at = aten_sequence(pred, target).double().cpu()
    print('relative error of the batch values vs fp64 (MAE RMSE LogSI AbsRel Acc): fused ' + ' '.join(f'{abs(x - y)/abs(y):.1e}' for x, y in zip(got.tolist(), ref.tolist()))
          + ' | ATen fp32 ' + ' '.join(f'{abs(x - y)/abs(y):.1e}' for x, y in zip(at.tolist(), ref.tolist())))
    _lib.reset_knobs()


if __name__ == '__main__':
    main()
