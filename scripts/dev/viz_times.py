#!/usr/bin/env python3
"""Times of the image-logging operators against the plain path on the same machine -> profiles/viz_times.txt (or --out).

    python scripts/dev/viz_times.py [--out profiles/viz_times.txt] [--skip-log-step]

Method: fused and plain are ALTERNATED call by call in one process (fused, plain, fused, plain, ...) after warm-up calls of each, inputs resident on the
device, nothing else on the GPU; a figure is the median (min .. max) of the wall-clock times of `reps` calls, each ended by a device synchronisation — wall
clock and not events, because the plain path works on the host (its copy of the tensor to the host is part of what it costs) and the fused `rgb_from_feat`
copies the C x C matrix down.  The plain path is this package's restatement of the reference's host sequence (numpy + matplotlib / sklearn).
Cases: `rgb_from_disp` at b = 12 at the four pyramid levels of 192x640; `rgb_from_feat` at (12,64,96,320), (12,512,6,20) and (6,64,192,640); `make_grid`
of six 192x640 images; the smallest shapes the tests use; a whole `log_step` of cfg/kitti_resnet18.yaml and cfg/kitti_featdepth.yaml at b = 12, 192x640."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from slowtv_monodepth_amd import io, viz  # noqa: E402
from slowtv_monodepth_amd.heavy_logger import HeavyLogger, RecordingWriter  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3*(time.perf_counter() - t0)


def alternated(fused, plain, warm=3, reps=21):
    for _ in range(warm): fused(); plain()
    f, p = [], []
    for _ in range(reps): f.append(wall(fused)); p.append(wall(plain))
    s = lambda ts: (statistics.median(ts), min(ts), max(ts))
    return s(f), s(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', type=Path, default=ROOT/'profiles'/'viz_times.txt')
    ap.add_argument('--skip-log-step', action='store_true')
    args = ap.parse_args()
    lines = [f'# scripts/dev/viz_times.py on {torch.cuda.get_device_name(0)}: wall-clock ms, median (min .. max), fused and plain alternated call by call after warm-up']

    def note(name, f, p):
        s = f'{name:<58} fused {f[0]:10.3f} ({f[1]:.3f} .. {f[2]:.3f})   plain {p[0]:10.3f} ({p[1]:.3f} .. {p[2]:.3f})   x{p[0]/f[0]:.1f}'
        lines.append(s); print(s, flush=True)

    g = torch.Generator(device='cuda').manual_seed(0)
    rand = lambda *s: torch.rand(*s, device='cuda', generator=g)
    for shape in ((12, 1, 192, 640), (12, 1, 96, 320), (12, 1, 48, 160), (12, 1, 24, 80), (1, 1, 1, 3)):
        d = 0.01 + rand(*shape)
        note(f'rgb_from_disp {shape}', *alternated(lambda: viz.rgb_from_disp(d), lambda: viz.plain_rgb_from_disp(d)))
        if shape[2] == 192:
            # where does the spread of the alternated figure come from?  the same call back to back (no host phase between two calls), and alternated
            # with a caller's vmax (no select: no histogram, no memset)
            ts = sorted(wall(lambda: viz.rgb_from_disp(d)) for _ in range(50))
            lines.append(f'    the fused call back to back, 50 calls: median {ts[25]:.3f} (min {ts[0]:.3f}, 90th percentile {ts[45]:.3f}, max {ts[-1]:.3f})'); print(lines[-1], flush=True)
            ts = sorted(wall(lambda: time.sleep(0.04) or viz.rgb_from_disp(d)) - 40.0 for _ in range(21))
            lines.append(f'    the fused call after 40 ms of host sleep (sleep subtracted), 21 calls: median {ts[10]:.3f} (min {ts[0]:.3f}, max {ts[-1]:.3f})'); print(lines[-1], flush=True)
            note(f'rgb_from_disp {shape}, vmax=0.9 (no select)', *alternated(lambda: viz.rgb_from_disp(d, vmax=0.9), lambda: viz.plain_rgb_from_disp(d, vmax=0.9)))
    for shape, reps in (((12, 64, 96, 320), 7), ((12, 512, 6, 20), 11), ((6, 64, 192, 640), 5), ((2, 3, 4, 5), 21)):
        f = rand(*shape)*torch.linspace(0.2, 2.0, shape[1], device='cuda').view(1, -1, 1, 1)
        note(f'rgb_from_feat {shape}', *alternated(lambda: viz.fused_rgb_from_feat(f), lambda: viz.plain_rgb_from_feat(f), warm=1, reps=reps))
    for shape in ((12, 3, 192, 640), (5, 1, 5, 7)):
        x = rand(*shape)
        note(f'make_grid(normalize=True) {shape}', *alternated(lambda: viz.make_grid(x, normalize=True), lambda: viz.plain_make_grid(x.cpu(), normalize=True)))
    if not args.skip_log_step:
        from slowtv_monodepth_amd.synthetic import make_batch
        from slowtv_monodepth_amd.train import dataset_supp_idxs
        from slowtv_monodepth_amd.trainer import MonoDepthModule
        for name in ('kitti_resnet18', 'kitti_featdepth'):
            try:
                cfg = io.load_merge_yaml(ROOT/'cfg'/f'{name}.yaml')
                cfg.setdefault('trainer', {})['log_images'] = True
                torch.manual_seed(0)
                module = MonoDepthModule(cfg).cuda()
                batch = make_batch(12, 192, 640, dataset_supp_idxs(cfg), seed=1, device='cuda', depth_hints='depth_regr' in cfg.get('loss', {}))
                fused, plain = HeavyLogger(writer=RecordingWriter()), HeavyLogger(writer=RecordingWriter(), plain=True)
                def run(lg):
                    lg.writer.images.clear(); lg.writer.texts.clear()
                    lg.log_step(module, batch, 'train', 0)
                    for _, v, _ in lg.writer.images: v.cpu()               # the host sees every finished grid
                note(f'log_step cfg/{name}.yaml b = 12, 192x640 ', *alternated(lambda: run(fused), lambda: run(plain), warm=1, reps=5))
                lines[-1] += f'   [{len(fused.writer.images)} grids]'
            except Exception as e:       # (recorded, not hidden: the operators' lines above stand on their own)
                lines.append(f'log_step cfg/{name}.yaml: failed with {e!r}'); print(lines[-1], flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
