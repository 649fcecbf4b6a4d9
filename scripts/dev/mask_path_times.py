#!/usr/bin/env python3
"""Times of the predictive-mask path at cfg 2's shapes (b = 12, mask heads 16/32/64/128 -> 2 at 192x640 ... 24x80): `conv3x3_headn` forward and both backward
operators against what the decoder ran for such a head before (`act(F.conv2d(xp, w, bias))`, i.e. MIOpen + the activation's ATen kernels), and
`upsample_stack` / `scale_mean` against the ATen sequence of the reference (per-scale `F.interpolate` + `torch.stack`; per-scale BCE / mean + stack + mean).
HIP events, 10 warm-up and 30 timed iterations per number, operators timed one by one through autograd (`torch.autograd.grad` with only that input
requiring a gradient).  (GPU box.)   python scripts/dev/mask_path_times.py [--out profiles/mask_path_times.txt] [--step]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch, torch.nn.functional as TF
from slowtv_monodepth_amd import miopen_tuning  # noqa: F401  (same find-db settings as the bench)
from slowtv_monodepth_amd import functional as HF

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--step', action='store_true', help='also time a training step of cfg/kitti_sfm_learner.yaml next to cfg/kitti_resnet18.yaml (b = 12, 192x640)')
args = ap.parse_args()
lines = []
def say(s=''):
    print(s, flush=True); lines.append(s)

def timeit(fn, n=30, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e)/n*1e3

b, n = 12, 2
say(f'{torch.cuda.get_device_name(0)}; b = {b}, n = {n} mask channels; microseconds per call (mean of 30 after 10 warm-up)')
say(f'{"head":18s} {"act":8s} | {"ATen/MIOpen fwd":>15s} {"bwd data":>9s} {"bwd wgt":>9s} {"sum":>8s} | {"headn fwd":>9s} {"bwd data":>9s} {"bwd wgt":>9s} {"sum":>8s} | ratio')
for act in ('sigmoid', 'relu'):
    for C, h, w in [(16, 192, 640), (32, 96, 320), (64, 48, 160), (128, 24, 80)]:
        xp = torch.randn(b, C, h + 2, w + 2, device='cuda'); wt = torch.randn(n, C, 3, 3, device='cuda')/(3*C**0.5); bs = torch.zeros(n, device='cuda')
        g = torch.randn(b, n, h, w, device='cuda')
        ref = lambda x_, w_, b_: (torch.sigmoid if act == 'sigmoid' else torch.relu)(TF.conv2d(x_, w_, b_))
        new = lambda x_, w_, b_: HF.conv3x3_headn(x_, w_, b_, act)
        res = []
        for fn in (ref, new):
            with torch.no_grad(): f = timeit(lambda: fn(xp, wt, bs))
            xg = xp.clone().requires_grad_(True); y = fn(xg, wt, bs)
            bd = timeit(lambda: torch.autograd.grad(y, xg, g, retain_graph=True))
            wg, bg = wt.clone().requires_grad_(True), bs.clone().requires_grad_(True); y = fn(xp, wg, bg)
            bw = timeit(lambda: torch.autograd.grad(y, (wg, bg), g, retain_graph=True))
            res.append((f, bd, bw, f + bd + bw))
        say(f'{C:3d} -> {n} {h:3d}x{w:<6d} {act:8s} | ' + ' | '.join(f'{r[0]:{15 if i == 0 else 9}.1f} {r[1]:9.1f} {r[2]:9.1f} {r[3]:8.1f}' for i, r in enumerate(res))
            + f' | {res[0][3]/res[1][3]:.2f}x')
say('(the backward times of the ATen column include the activation\'s backward kernel, those of headn recompute it from the saved output)')
say()
sizes, size = [(192, 640), (96, 320), (48, 160), (24, 80)], (192, 640)
xs = [torch.rand(b, n, hs, ws, device='cuda', requires_grad=True) for hs, ws in sizes]
g = torch.randn(4, b, n, *size, device='cuda')
ref = lambda: torch.stack([TF.interpolate(x, size=size, mode='bilinear', align_corners=False) for x in xs])
new = lambda: HF.upsample_stack(xs, size)
for nm, fn in (('ATen interpolate x4 + stack', ref), ('upsample_stack', new)):
    with torch.no_grad(): f = timeit(fn)
    y = fn(); bw = timeit(lambda: torch.autograd.grad(y, xs, g, retain_graph=True))
    say(f'{nm:30s} fwd {f:8.1f}  bwd {bw:8.1f}')
say()
for mode in ('bce_ones', 'identity'):
    ms = [torch.sigmoid(torch.randn(b, n if mode == 'bce_ones' else 1, hs, ws, device='cuda')).requires_grad_(True) for hs, ws in sizes]
    if mode == 'bce_ones': ref = lambda: torch.stack([TF.binary_cross_entropy(m, torch.ones_like(m)) for m in ms]).mean()
    else: ref = lambda: torch.stack([m.mean() for m in ms]).mean()
    new = lambda: HF.scale_mean(ms, mode)
    for nm, fn in ((f'ATen per scale ({mode})', ref), (f'scale_mean ({mode})', new)):
        with torch.no_grad(): f = timeit(fn)
        y = fn(); bw = timeit(lambda: torch.autograd.grad(y, ms, retain_graph=True))
        say(f'{nm:30s} fwd {f:8.1f}  bwd {bw:8.1f}')
if args.step:
    import copy, yaml
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    say()
    batch = make_batch(12, 192, 640, (-1, 1), seed=42, device='cuda')
    for name in ('kitti_resnet18', 'kitti_sfm_learner'):
        cfg = yaml.safe_load(open(os.path.join(root, 'cfg', name + '.yaml')))
        m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
        opt = m.configure_optimizers()['optimizer']
        def step():
            opt.zero_grad(set_to_none=True)
            loss, _, _ = m.step(batch); loss.backward(); opt.step()
        t = timeit(step, n=20, warm=15)
        say(f'training step cfg/{name}.yaml (b = 12, 192x640, fp32, eager): {t/1e3:.2f} ms')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
