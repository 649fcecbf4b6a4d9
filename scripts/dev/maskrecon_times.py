#!/usr/bin/env python3
"""Times and peak memory of the fused masked image-reconstruction handler against the plain one of the same commit (profiles/maskrecon_times.txt).

    python scripts/dev/maskrecon_times.py [--out profiles/maskrecon_times.txt]

`handlers.image_recon_masked_fused` (without the warp, as training runs it) against `handlers.image_recon` (the un-fused operators, unchanged), ssim + min +
automask, both mask kinds: the workload's shape (b = 12, n = 2, S = 4, 192 x 640) and the smallest one (b = 1, n = 1, S = 1, 24 x 32): forward alone and
forward + backward, peak memory above the inputs; a shape that lost would be routed to the plain handler by a static rule in maskrecon.py.  Then the step time of
cfg/kitti_sfm_learner.yaml at b = 12 with either route: the median and range of three alternated runs.  The two candidates alternate in one process
(scripts/dev/cadepth_times.py's timing helper)."""
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


def case(b, n, S, h, w, kind, seed=0):
    gen = torch.Generator().manual_seed(seed)
    _, y, _ = make_batch(b, h, w, list(range(-(n//2), 0)) + list(range(1, n - n//2 + 1)), seed=seed, device='cuda')
    depth = (1.0 + 20*torch.rand(S, b, 1, h, w, generator=gen)).cuda()
    mask = (torch.rand(S, b, n, h, w, generator=gen) if kind == 'explainability' else 0.3*torch.randn(S, b, n, h, w, generator=gen)).cuda()
    aa, t = 0.005*torch.randn(n*b, 3, generator=gen), 0.03*torch.randn(n*b, 3, generator=gen)
    Ts = F.pose_matrices(aa.cuda(), t.cuda()).unflatten(0, (n, b))
    return depth, mask, y['imgs'], y['supp_imgs'][:n], Ts, kitti_K(b, h, w).cuda()


def runner(fn, crit, depth, mask, imgs, supp, Ts, K, backward):
    d, m, T = depth.clone().requires_grad_(True), mask.clone().requires_grad_(True), Ts.clone().requires_grad_(True)
    S = depth.shape[0]

    def call():
        return fn(crit, None, handlers.ScaleDict.from_stack(range(S), d), handlers.ScaleDict.from_stack(range(S), m), imgs, supp, T, K, want_warp=False)[0]

    def run():
        if not backward:
            with torch.no_grad(): call()
            return
        d.grad = m.grad = T.grad = None
        call().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], fused and plain handler alternating; peak MB of one call above the inputs',
             f'# {"handlers.image_recon with masks, ssim + min + automask":62} {"fused":>26} {"plain":>26}  plain/fused  {"fused MB":>8} {"plain MB":>8}']
    for kind in ('explainability', 'uncertainty'):
        crit = ReconstructionLoss('ssim', use_min=True, use_automask=True, mask_name=kind)
        for (b, n, S, h, w) in ((12, 2, 4, 192, 640), (1, 1, 1, 24, 32)):
            ops = case(b, n, S, h, w, kind)
            for backward in (False, True):
                cands = {'fused': runner(handlers.image_recon_masked_fused, crit, *ops, backward), 'plain': runner(handlers.image_recon, crit, *ops, backward)}
                res = time_pair(cands, args.window, args.rounds, warmup=3)
                f, p = res['fused'], res['plain']
                name = f'{kind[:6]} b={b} n={n} S={S} {h}x{w} ' + ('forward + backward' if backward else 'forward')
                lines.append(f'{name:64} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(cands["fused"]):8.1f} {peak_mb(cands["plain"]):8.1f}')
                print(lines[-1], flush=True)
            del ops, cands
            torch.cuda.empty_cache()
    # the training step of the example configuration with either route (same weights, same batch): three alternated runs
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule

    class Plain(HipLossBackend):
        def image_recon(self, crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks, want_warp=True, K_inv=None, prepared=None):
            return handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts.float(), Ks.float(), K_inv=K_inv, want_warp=want_warp, prepared=prepared)
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_sfm_learner.yaml')
    b = 12
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
    res = time_pair(steps, max(args.window, 1.0), 3, warmup=5)
    f, p = res['fused'], res['plain']
    lines.append(f'# training step of cfg/kitti_sfm_learner.yaml, b = {b}, 192 x 640, supports [-1, 1], fp32, ms per step (forward + backward + AdamW), median of 3 alternated runs [min .. max]')
    lines.append(f'{"step":64} {f[0]:8.3f} [{f[1]:6.3f} ..{f[2]:7.3f}] {p[0]:8.3f} [{p[1]:6.3f} ..{p[2]:7.3f}]  {p[0]/f[0]:8.2f}    {peak_mb(steps["fused"]):8.1f} {peak_mb(steps["plain"]):8.1f}')
    print(lines[-1], flush=True)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
