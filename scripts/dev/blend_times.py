#!/usr/bin/env python3
"""Times of the flip-and-blend kernel against the plain ATen sequence of the same commit, and its bit parity with the reference fixture
(profiles/blend_stereo_times.txt).

    python scripts/dev/blend_times.py [--out profiles/blend_stereo_times.txt]

`functional.flip_blend` at b = 12, 1 x 192 x 640 and `functional.flip_blend_pyramid` on the four levels 192 x 640 .. 24 x 80, each with and without the
disparity scaling, against `blend.plain_flip_blend` (ATen's `flip` + the blend + `to_scaled`; per level for the pyramid), forward alone and forward +
backward.  The two candidates alternate in one process, as in scripts/dev/cadepth_times.py (whose timing helpers are used).  Then, for every case of
tests/golden/blend_stereo.npz, how many output and gradient elements of the kernel are bit-equal to the reference's."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT/'tests'/'golden'))
sys.path.insert(0, str(ROOT/'tests'))
from cadepth_times import time_pair                                     # noqa: E402
from slowtv_monodepth_amd import functional as HF                      # noqa: E402
from slowtv_monodepth_amd.blend import plain_flip_blend                # noqa: E402


def candidates(ls, rs, gs, kw, backward):
    """-> {'hip': run, 'aten': run} over the levels `ls` / `rs` (lists; one level: `flip_blend`, more: `flip_blend_pyramid` against per-level ATen)."""
    def hip():
        if len(ls) == 1: return [HF.flip_blend(ls[0], rs[0], **kw)]
        return list(HF.flip_blend_pyramid(dict(enumerate(ls)), dict(enumerate(rs)), **kw).values())

    def aten(): return [plain_flip_blend(l, r, **kw) for l, r in zip(ls, rs)]

    def runner(fn):
        def run():
            if not backward:
                with torch.no_grad(): fn()
                return
            for t in (*ls, *rs): t.grad = None
            torch.autograd.backward(fn(), gs)
        return run
    return {'hip': runner(hip), 'aten': runner(aten)}


def parity(lines):
    from blend_inputs import BLEND_CASES, BLEND_RANGE, BLEND_SCALED, blend_case, blend_expected
    from conftest import load_golden
    g = load_golden('blend_stereo')
    for scaled in (False, True):
        kw = dict(min_depth=BLEND_RANGE[0], max_depth=BLEND_RANGE[1]) if scaled else {}
        same, total, worst = 0, 0, 0.0
        for k in (BLEND_SCALED if scaled else range(len(BLEND_CASES))):
            ins = blend_case(k)
            l, r_raw = ins['l'].cuda().requires_grad_(True), ins['r'].flip(-1).contiguous().cuda().requires_grad_(True)
            out = HF.flip_blend(l, r_raw, **kw)
            out.backward(ins['g'].cuda())
            for mine, ref in zip((out.detach().cpu(), l.grad.cpu(), r_raw.grad.flip(-1).cpu()), blend_expected(g, k, scaled)):
                same += int((mine == ref).sum()); total += ref.numel(); worst = max(worst, (mine.double() - ref.double()).abs().max().item())
        lines.append(f'# reference fixture ({"scaled" if scaled else "plain"}, outputs and both gradients): {same} of {total} elements bit-equal, max |difference| {worst:.3e}')
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], kernel and ATen alternating',
             f'# {"operator":58} {"hip":>26} {"aten":>26}  aten/hip']
    g = torch.Generator().manual_seed(0)
    b, levels = 12, [(192, 640), (96, 320), (48, 160), (24, 80)]
    leaf = lambda h, w: torch.rand(b, 1, h, w, generator=g).cuda().requires_grad_(True)
    ls, rs = [leaf(h, w) for h, w in levels], [leaf(h, w) for h, w in levels]
    gs = [torch.randn(b, 1, h, w, generator=g).cuda() for h, w in levels]
    for name, n in (('flip_blend 12x1x192x640', 1), ('flip_blend_pyramid 12x1x(192x640 .. 24x80)', 4)):
        for tag, kw in (('', {}), (' scaled', dict(min_depth=0.1, max_depth=100))):
            for what, backward in (('fwd', False), ('fwd+bwd', True)):
                res = time_pair(candidates(ls[:n], rs[:n], gs[:n], kw, backward), args.window, args.rounds, warmup=3)
                h, a = res['hip'], res['aten']
                lines.append(f'{name + tag + " " + what:60} {h[0]:8.3f} [{h[1]:6.3f} ..{h[2]:7.3f}] {a[0]:8.3f} [{a[1]:6.3f} ..{a[2]:7.3f}]  {a[0]/h[0]:6.2f}')
                print(lines[-1], flush=True)
    parity(lines)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
