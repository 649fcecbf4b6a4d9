#!/usr/bin/env python3
"""Times and peak memory of the fused feature-metric reconstruction handler against the plain one of the same commit (profiles/featrecon_times.txt).

    python scripts/dev/featrecon_times.py [--out profiles/featrecon_times.txt]

`handlers.feat_recon_fused` (without the warp, as training runs it) against `handlers.feat_recon` (the parent commit's code, unchanged), l2 + min + automask, C = 64
features at 1/4 resolution: cfg/kitti_featdepth.yaml's shape (b = 6, n = 3, 48 x 160 -> 192 x 640), b = 12 with n = 2, and the smallest shape (b = 1, n = 1,
6 x 8 -> 24 x 32): forward alone and forward + backward, peak memory above the inputs; a shape that lost would be routed to the plain handler by a static rule in
featrecon.py.  Then the step time of cfg/kitti_featdepth.yaml at its batch size with the fused handler and with the plain one.  The two candidates alternate in
one process (scripts/dev/cadepth_times.py's timing helper)."""
import argparse
import copy
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from cadepth_times import time_pair                                     # noqa: E402
from hints_times import peak_mb                                         # noqa: E402
from slowtv_monodepth_amd import handlers, io                          # noqa: E402
from slowtv_monodepth_amd import functional as F                       # noqa: E402
from slowtv_monodepth_amd.losses import ReconstructionLoss             # noqa: E402
from slowtv_monodepth_amd.synthetic import kitti_K, make_batch         # noqa: E402


def case(b, n, C, hf, wf, H, W, seed=0):
    gen = torch.Generator().manual_seed(seed)
    depth = (1.0 + 20*torch.rand(b, 1, H, W, generator=gen)).cuda()
    feats = torch.randn(b, C, hf, wf, generator=gen).cuda()
    supp = (0.5*torch.randn(n, b, C, hf, wf, generator=gen)).cuda() + 0.5*feats[None]
    aa, t = 0.005*torch.randn(n*b, 3, generator=gen), 0.03*torch.randn(n*b, 3, generator=gen)
    Ts = F.pose_matrices(aa.cuda(), t.cuda()).unflatten(0, (n, b))
    return depth, feats, supp, Ts, kitti_K(b, H, W).cuda()


def runner(fn, crit, depth, feats, supp, Ts, K, backward, **kw):
    leaf, T = depth.clone().requires_grad_(True), Ts.clone().requires_grad_(True)

    def run():
        if not backward:
            with torch.no_grad(): fn(crit, None, {0: leaf}, None, feats, supp, T, K, **kw)
            return
        leaf.grad = T.grad = None
        fn(crit, None, {0: leaf}, None, feats, supp, T, K, **kw)[0].backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], fused and plain handler alternating; peak MB of one call above the inputs',
             f'# {"handlers.feat_recon, l2 + min + automask, C = 64":52} {"fused":>26} {"plain":>26}  plain/fused  {"fused MB":>8} {"plain MB":>8}']
    crit = ReconstructionLoss('l2', use_min=True, use_automask=True)
    for (b, n, hf, wf, H, W) in ((6, 3, 48, 160, 192, 640), (12, 2, 48, 160, 192, 640), (1, 1, 6, 8, 24, 32)):
        ops = case(b, n, 64, hf, wf, H, W)
        for backward in (False, True):
            cands = {'fused': runner(handlers.feat_recon_fused, crit, *ops, backward, want_warp=False), 'plain': runner(handlers.feat_recon, crit, *ops, backward)}
            res = time_pair(cands, args.window, args.rounds, warmup=3)
            f, p = res['fused'], res['plain']
            name = f'b={b} n={n} {hf}x{wf} -> {H}x{W} ' + ('forward + backward' if backward else 'forward')
            lines.append(f'{name:54} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(cands["fused"]):8.1f} {peak_mb(cands["plain"]):8.1f}')
            print(lines[-1], flush=True)
        del ops, cands
        torch.cuda.empty_cache()
    # the training step of the example configuration, fused against plain handler (same weights, same batch)
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule

    class Plain(HipLossBackend):
        def feat_recon(self, crit, synth, depths, masks, feats, supp_feats, Ts, Ks):
            return handlers.feat_recon(crit, synth, depths, masks, feats, supp_feats, Ts.float(), Ks.float())
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_featdepth.yaml')
    b = cfg['loader']['batch_size']
    batch = make_batch(b, 192, 640, [-1, 1], seed=1, device='cuda')
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
    lines.append(f'# training step of cfg/kitti_featdepth.yaml, b = {b}, 192 x 640, supports [-1, 1], fp32, ms per step (forward + backward + AdamW)')
    lines.append(f'{"step":54} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(steps["fused"]):8.1f} {peak_mb(steps["plain"]):8.1f}')
    print(lines[-1], flush=True)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
