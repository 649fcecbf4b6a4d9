#!/usr/bin/env python3
"""Times and peak memory of the DDVNet head and decoder against the plain ATen path of the same commit (profiles/ddvnet_times.txt).

    python scripts/dev/ddvnet_times.py [--out profiles/ddvnet_times.txt]

The four heads at b = 12, 192 x 640: `functional.ddv_head` against the decoder's plain sequence (conv2d on the same padded tensor, softmax, multiply by the
bins, sum), forward alone and forward + backward; then the whole decoder, glued against `plain_path()`.  Every ATen candidate is first timed by itself, before the kernel path has run
in the process (column `aten alone`); then the two candidates alternate in one process, as in scripts/dev/cadepth_times.py (whose timing helpers are used); peak memory is `max_memory_allocated` over one call, above what was allocated before it."""
import argparse
import contextlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from cadepth_times import fwd_bwd, fwd_only, time_pair                  # noqa: E402
from slowtv_monodepth_amd import functional as HF                      # noqa: E402
from slowtv_monodepth_amd.networks.decoders import DDVNetDecoder       # noqa: E402

BINS = 128


def head_aten(xp, weight, bias):
    logits = torch.conv2d(xp, weight, bias)
    bins = (torch.arange(BINS, device=xp.device)/BINS).view(1, BINS, 1, 1)
    return (logits.softmax(dim=1)*bins).sum(dim=1, keepdim=True)


def peak_mb(run):
    run(); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run(); torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base)/2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], kernel and ATen alternating; peak MiB above the operands',
             '# aten alone: the same ATen call timed BEFORE the kernel path ran in the process (ddv_head\'s backward calls MIOpen in its deterministic mode where MIOpen serves an',
             '# operator; in a process where that call came first, ATen\'s own backward of the same problem was measured at 33 ms instead of 6.2 ms at scale 0: it then runs the solver',
             '# MIOpen found for the deterministic request.  Here ATen comes first and keeps its own solver in the alternating column too.)',
             f'# {"operator":44} {"hip":>26} {"aten":>26}  aten/hip   peak MiB hip / aten   aten alone  alone/hip']
    jobs = []     # (name, {'hip': fn, 'aten': fn})

    g = torch.Generator().manual_seed(0)
    kw = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32])
    torch.manual_seed(0)
    dec = DDVNetDecoder(**kw).cuda().train()
    feats = [torch.randn(12, c, 192//s, 640//s, generator=g).cuda().requires_grad_(True) for c, s in zip(kw['num_ch_enc'], kw['enc_sc'])]
    gouts = {i: torch.randn(12, 1, 192 >> i, 640 >> i, generator=g).cuda() for i in range(4)}

    def decoder(glued, backward):
        def run():
            with contextlib.nullcontext() if glued else dec.plain_path():
                if not backward:
                    with torch.no_grad(): dec(feats)
                    return
                dec.zero_grad(set_to_none=True)
                for f in feats: f.grad = None
                out = dec(feats)
                sum((out[i]*gouts[i]).sum() for i in out).backward()
            dec.logits = {}
        return run
    for shape in [(12, 16, 192, 640), (12, 32, 96, 320), (12, 64, 48, 160), (12, 128, 24, 80)]:
        B, C, h, w = shape
        xp = torch.randn(B, C, h + 2, w + 2, generator=g).cuda().requires_grad_(True)
        weight = (torch.randn(BINS, C, 3, 3, generator=g)/float(9*C)**0.5).cuda().requires_grad_(True)
        bias = (0.1*torch.randn(BINS, generator=g)).cuda().requires_grad_(True)
        gout = torch.randn(B, 1, h, w, generator=g).cuda()
        tag = 'x'.join(map(str, shape))
        ins = [xp, weight, bias]
        jobs.append((f'ddv_head {tag} fwd', {'hip': fwd_only(HF.ddv_head, ins), 'aten': fwd_only(head_aten, ins)}))
        jobs.append((f'ddv_head {tag} fwd+bwd', {'hip': fwd_bwd(HF.ddv_head, ins, gout), 'aten': fwd_bwd(head_aten, ins, gout)}))
    jobs.append(('DDVNetDecoder 12x192x640 resnet18 fwd', {'hip': decoder(True, False), 'aten': decoder(False, False)}))
    jobs.append(('DDVNetDecoder 12x192x640 resnet18 fwd+bwd', {'hip': decoder(True, True), 'aten': decoder(False, True)}))
    # first every ATen candidate by itself, before anything of the kernel path has run; then the alternating pairs
    alone = {name: time_pair({'aten': c['aten']}, args.window, args.rounds, warmup=3)['aten'] for name, c in jobs}
    for name, cands in jobs:
        res = time_pair(cands, args.window, args.rounds, warmup=3)
        mem = {k: peak_mb(fn) for k, fn in cands.items()}
        h, a, a0 = res['hip'], res['aten'], alone[name]
        lines.append(f'{name:46} {h[0]:8.3f} [{h[1]:6.3f} ..{h[2]:7.3f}] {a[0]:8.3f} [{a[1]:6.3f} ..{a[2]:7.3f}]  {a[0]/h[0]:6.2f}   {mem["hip"]:8.1f} / {mem["aten"]:8.1f}     {a0[0]:8.3f}     {a0[0]/h[0]:6.2f}')
        print(lines[-1], flush=True)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
