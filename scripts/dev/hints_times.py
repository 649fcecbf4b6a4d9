#!/usr/bin/env python3
"""Times and peak memory of the fused Depth-Hints handler against the plain one of the same commit (profiles/hints_times.txt).

    python scripts/dev/hints_times.py [--out profiles/hints_times.txt]

`handlers.depth_regr_fused` against `handlers.depth_regr` (the parent commit's code, unchanged) at b = 12, 192 x 640, n = 3 supports, S = 4 scales, log_l1 + automask:
forward alone and forward + backward, peak memory above the inputs; then smaller shapes, to see whether any loses (a shape that did would be routed to the plain
handler by a static rule in hints.py); then the step time of cfg/kitti_depth_hints.yaml at its batch size with the fused handler and with the plain one.  The two
candidates alternate in one process (scripts/dev/cadepth_times.py's timing helper)."""
import argparse
import copy
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from cadepth_times import time_pair                                     # noqa: E402
from slowtv_monodepth_amd import handlers, io                          # noqa: E402
from slowtv_monodepth_amd import functional as F                       # noqa: E402
from slowtv_monodepth_amd.losses import ReconstructionLoss, RegressionLoss   # noqa: E402
from slowtv_monodepth_amd.synthetic import make_batch                  # noqa: E402


def peak_mb(run):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base)/2**20


def case(b, h, w, n, S, seed=0):
    gen = torch.Generator().manual_seed(seed)
    _, y, _ = make_batch(b, h, w, tuple([-1, 1, 0][:n]), seed=seed, device='cuda', depth_hints=True)
    depth = (1.0 + 20*torch.rand(S, b, 1, h, w, generator=gen)).cuda()
    aa, t = 0.005*torch.randn(n*b, 3, generator=gen), 0.03*torch.randn(n*b, 3, generator=gen)
    Ts = F.pose_matrices(aa.cuda(), t.cuda()).unflatten(0, (n, b))
    return depth, y['depth_hints'], y['imgs'], y['supp_imgs'], Ts, y['K']


def runner(fn, crit, photo, depth, rest, backward):
    leaf = depth.clone().requires_grad_(True)

    def run():
        if not backward:
            with torch.no_grad(): fn(crit, None, photo, {s: leaf[s] for s in range(leaf.shape[0])}, *rest)
            return
        leaf.grad = None
        fn(crit, None, photo, {s: leaf[s] for s in range(leaf.shape[0])}, *rest)[0].backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], fused and plain handler alternating; peak MB of one call above the inputs',
             f'# {"handlers.depth_regr, log_l1 + automask":52} {"fused":>26} {"plain":>26}  plain/fused  {"fused MB":>8} {"plain MB":>8}']
    crit, photo = RegressionLoss('log_l1', use_automask=True), ReconstructionLoss('ssim', use_min=True, use_automask=True).compute_photo
    for (b, h, w, n, S) in ((12, 192, 640, 3, 4), (12, 192, 640, 2, 4), (4, 96, 320, 3, 4), (2, 64, 96, 3, 4), (1, 24, 32, 1, 1)):
        depth, *rest = case(b, h, w, n, S)
        for backward in (False, True):
            cands = {'fused': runner(handlers.depth_regr_fused, crit, photo, depth, rest, backward), 'plain': runner(handlers.depth_regr, crit, photo, depth, rest, backward)}
            res = time_pair(cands, args.window, args.rounds, warmup=3)
            f, p = res['fused'], res['plain']
            name = f'b={b} {h}x{w} n={n} S={S} ' + ('forward + backward' if backward else 'forward')
            lines.append(f'{name:54} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(cands["fused"]):8.1f} {peak_mb(cands["plain"]):8.1f}')
            print(lines[-1], flush=True)
        del depth, rest, cands
        torch.cuda.empty_cache()
    # the training step of the example configuration, fused against plain handler (same weights, same batch)
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule

    class Plain(HipLossBackend):
        def depth_regr(self, crit, synth, photo, depths, targets, imgs, supp_imgs, Ts, Ks):
            return handlers.depth_regr(crit, synth, photo, depths, targets.float(), imgs, supp_imgs, Ts.float(), Ks.float())
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_depth_hints.yaml')
    b = cfg['loader']['batch_size']
    batch = make_batch(b, 192, 640, [-1, 1, 0], seed=1, device='cuda', depth_hints=True)
    steps = {}
    for tag, backend in (('fused', None), ('plain', Plain())):
        torch.manual_seed(0)
        m = MonoDepthModule(copy.deepcopy(cfg), loss_backend=backend).cuda()
        opt = m.configure_optimizers()['optimizer']

        def step(m=m, opt=opt):
            loss, _, _ = m.step(tuple(dict(d) for d in batch))
            loss.backward(); opt.step(); opt.zero_grad(set_to_none=True)
        steps[tag] = step
    res = time_pair(steps, max(args.window, 1.0), args.rounds, warmup=5)
    f, p = res['fused'], res['plain']
    lines.append(f'# training step of cfg/kitti_depth_hints.yaml, b = {b}, 192 x 640, supports [-1, 1, 0], fp32, ms per step (forward + backward + AdamW)')
    lines.append(f'{"step":54} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(steps["fused"]):8.1f} {peak_mb(steps["plain"]):8.1f}')
    print(lines[-1], flush=True)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
