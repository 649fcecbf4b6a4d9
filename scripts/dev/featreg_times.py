#!/usr/bin/env python3
"""Times and peak memory of the fused feature regularisers against the two plain regularisers on ATen of the same commit (profiles/featdepth_times.txt).

    python scripts/dev/featreg_times.py [--out profiles/featdepth_times.txt]

At b = 6 with three supports (24 images) the five ResNet-18 feature shapes of a 192 x 640 input: `featreg.feat_regs` computing BOTH losses (with edges) against
`FeatPeakReg(True)` + `FeatSmoothReg(True)`, forward alone and forward + backward; then the whole `feat_peaky` + `feat_smooth` loss of a step (`handlers.feat_smooth_pair`
against two `handlers.feat_smooth` calls on the plain regularisers: b = 6 targets and 3 x 6 supports, five scales, image resize included).  The two candidates
alternate in one process, as in scripts/dev/cadepth_times.py (whose timing helper is used).  Peak memory is `torch.cuda.max_memory_allocated` over one call,
above what was allocated before it."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from cadepth_times import time_pair                                     # noqa: E402
from slowtv_monodepth_amd import handlers                              # noqa: E402
from slowtv_monodepth_amd.featreg import feat_regs                     # noqa: E402
from slowtv_monodepth_amd.regularizers import FeatPeakReg, FeatSmoothReg   # noqa: E402

SHAPES = [(64, 96, 320), (64, 48, 160), (128, 24, 80), (256, 12, 40), (512, 6, 20)]


def peak_mb(run):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base)/2**20


def runner(fn, leaves, backward):
    def run():
        if not backward:
            with torch.no_grad(): fn()
            return
        for t in leaves: t.grad = None
        lp, ls = fn()
        (lp + ls).backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], kernel and ATen alternating; peak MB of one call',
             f'# {"operator":44} {"hip":>26} {"aten":>26}  aten/hip  {"hip MB":>8} {"aten MB":>8}']
    g = torch.Generator().manual_seed(0)
    peaky, smooth = FeatPeakReg(True), FeatSmoothReg(True)

    def report(name, cands):
        res = time_pair(cands, args.window, args.rounds, warmup=3)
        h, a = res['hip'], res['aten']
        lines.append(f'{name:46} {h[0]:8.3f} [{h[1]:6.3f} ..{h[2]:7.3f}] {a[0]:8.3f} [{a[1]:6.3f} ..{a[2]:7.3f}]  {a[0]/h[0]:6.2f}  {peak_mb(cands["hip"]):8.1f} {peak_mb(cands["aten"]):8.1f}')
        print(lines[-1], flush=True)

    for c, h, w in SHAPES:
        feat = torch.randn(24, c, h, w, generator=g).cuda().requires_grad_(True)
        img = torch.rand(24, 3, h, w, generator=g).cuda()
        for what, backward in (('fwd', False), ('fwd+bwd', True)):
            report(f'feat_regs 24x{c}x{h}x{w} {what}', {'hip': runner(lambda: feat_regs(feat, img, True, True), [feat], backward),
                                                      'aten': runner(lambda: (peaky(feat, img)[0], smooth(feat, img)[0]), [feat], backward)})
        del feat, img
    feats = [torch.randn(6, c, h, w, generator=g).cuda().requires_grad_(True) for c, h, w in SHAPES]
    supp = [torch.randn(3, 6, c, h, w, generator=g).cuda().requires_grad_(True) for c, h, w in SHAPES]
    imgs, supp_imgs = torch.rand(6, 3, 192, 640, generator=g).cuda(), torch.rand(3, 6, 3, 192, 640, generator=g).cuda()
    fused = lambda: handlers.feat_smooth_pair(peaky, smooth, feats, imgs, supp, supp_imgs)

    def plain():
        keep = handlers._fused_feat_regs
        handlers._fused_feat_regs = lambda *a: False
        try: return handlers.feat_smooth(peaky, feats, imgs, supp, supp_imgs)[0], handlers.feat_smooth(smooth, feats, imgs, supp, supp_imgs)[0]
        finally: handlers._fused_feat_regs = keep
    for what, backward in (('fwd', False), ('fwd+bwd', True)):
        report(f'feat_peaky + feat_smooth of a step (b=6, n=3) {what}', {'hip': runner(fused, feats + supp, backward), 'aten': runner(plain, feats + supp, backward)})
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
