#!/usr/bin/env python3
"""Times of the offline-evaluation operators against the plain path on the same GPU -> profiles/eval_times.txt (or --out).

    python scripts/dev/eval_times.py [--out profiles/eval_times.txt] [--skip-plain-dense]

Method: every figure is the median of `reps` event-timed calls after `warm` untimed ones, inputs resident on the device, nothing else on the GPU; the plain
path's times include its synchronising steps (boolean indexing, `.item()`), which are part of what it costs.  Cases: the align-and-score operator at b = 12,
192x640 -> 375x1242 (5 % dense LiDAR targets, then dense ones); the point-cloud operator at about 2*10^4 points (375x1242 at 4.3 % density) and at 480x640
dense; both at the smallest tested shape (24x32).  If sklearn imports, the kd-tree's CPU time at the sparse case is recorded for information."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from slowtv_monodepth_amd import eval_metrics as E  # noqa: E402
from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator, backproject, plain_chamfer, plain_evaluate  # noqa: E402
from slowtv_monodepth_amd.synthetic import kitti_K, lidar_depth  # noqa: E402


def timed(fn, warm=3, reps=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def inputs(b, shape, Shape, density, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    t = lidar_depth(g, b, *Shape, device='cuda', density=density)
    dense = lidar_depth(torch.Generator(device='cuda').manual_seed(seed), b, *Shape, device='cuda', density=2.0)
    d = torch.nn.functional.interpolate(1/(1.7*dense*(1 + 0.02*(torch.rand(dense.shape, generator=g, device='cuda') - 0.5))), size=shape, mode='bilinear', align_corners=False)
    return d.contiguous(), t.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', type=Path, default=ROOT/'profiles'/'eval_times.txt')
    ap.add_argument('--skip-plain-dense', action='store_true', help='do not time the plain nearest-neighbour search at 480x640 dense (seconds per call)')
    args = ap.parse_args()
    lines = [f'# scripts/dev/eval_times.py on {torch.cuda.get_device_name(0)}: median (min .. max) in ms of 10 event-timed calls after 3 warm-up calls']

    def note(s): lines.append(s); print(s, flush=True)

    # ---- align and score
    for name, b, shape, Shape, density in (('b = 12, 192x640 -> 375x1242, 5 % dense target', 12, (192, 640), (375, 1242), 0.05),
                                           ('b = 12, 192x640 -> 375x1242, dense target', 12, (192, 640), (375, 1242), 2.0),
                                           ('b = 1, 24x32 -> 24x32, dense target', 1, (24, 32), (24, 32), 2.0)):
        d, t = inputs(b, shape, Shape, density)
        for mode in ('median', 'lsqr'):
            ev = MonoDepthEvaluator(metrics=('eigen', 'benchmark'), align_mode=mode, max=80.0, device='cuda')
            f = timed(lambda: E.eval_metrics(d, t, max_depth=80.0, align=mode))
            p = timed(lambda: [plain_evaluate(ev, d[i, 0], t[i, 0], ['eigen', 'benchmark']) for i in range(b)], warm=1, reps=5)
            note(f'align-and-score  {name:<48} {mode:<6} fused {f[0]:9.3f} ({f[1]:.3f} .. {f[2]:.3f})   plain {p[0]:9.3f} ({p[1]:.3f} .. {p[2]:.3f})   x{p[0]/f[0]:.1f}')

    # ---- point clouds
    for name, Shape, density, plain in (('375x1242 at 4.3 % density (about 2*10^4 points)', (375, 1242), 0.043, True),
                                        ('480x640 dense (3*10^5 points)', (480, 640), 2.0, not args.skip_plain_dense),
                                        ('24x32 dense (768 points)', (24, 32), 2.0, True)):
        d, t = inputs(1, Shape, Shape, density)
        r = E.eval_metrics(d, t, max_depth=80.0, align='median', want_depth=True, want_valid=True)
        K_inv = torch.linalg.inv(kitti_K(1, *Shape)).cuda()
        n = int(r['counts'][0])
        f = timed(lambda: E.eval_pointcloud(r['depth'], t, r['valid'], K_inv), warm=2, reps=5 if n > 100000 else 10)
        pairs = 2*((n + 1)//2)*n
        line = f'point cloud      {name:<48} n = {n:<7} fused {f[0]:9.3f} ({f[1]:.3f} .. {f[2]:.3f})   {pairs/f[0]/1e6:8.1f} G pairs/s'
        if plain:
            m = r['valid'][0, 0].bool().flatten()
            P, T = backproject(r['depth'][0, 0], K_inv[0])[m], backproject(t[0, 0], K_inv[0])[m]
            p = timed(lambda: plain_chamfer(P, T), warm=0 if n > 100000 else 1, reps=1 if n > 100000 else 3)
            line += f'   plain (chunked float64 cdist) {p[0]:10.3f} ({p[1]:.3f} .. {p[2]:.3f})   x{p[0]/f[0]:.1f}'
            if n < 50000:
                try:
                    import sklearn.neighbors as skln
                    Pc, Tc = P.cpu().numpy(), T.cpu().numpy()
                    t0 = time.perf_counter()
                    for q, db in ((Pc, Tc), (Tc, Pc)): skln.NearestNeighbors(n_neighbors=1, algorithm='kd_tree', n_jobs=1).fit(db).kneighbors(q[::2])
                    line += f'   [sklearn kd-tree on the CPU, for information: {1e3*(time.perf_counter() - t0):.1f}]'
                except ImportError: pass
        note(line)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
