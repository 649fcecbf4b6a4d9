#!/usr/bin/env python3
"""Times and peak memory of the DiffNet glue and decoder against the plain ATen path of the same commit (profiles/diffnet_times.txt).

    python scripts/dev/diffnet_times.py [--out profiles/diffnet_times.txt]

The four attention stages of a ResNet-18 trunk at b = 12, 192 x 640 (768 / 384 / 192 / 128 channels at strides 16 / 8 / 4 / 2): `functional.up_cat_gate_pad`
against the ATen sequence it replaces (bias + ReLU, interpolate, cat, mean, the two Linear layers, sigmoid, multiply, reflection pad), forward alone and
forward + backward; then the whole decoder, glued against `plain_path()`.  The two candidates alternate in one process, as in scripts/dev/cadepth_times.py
(whose timing helpers are used); peak memory is `max_memory_allocated` over one call, above what was allocated before it."""
import argparse
import contextlib
import sys
from pathlib import Path

import torch
import torch.nn.functional as TF

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from cadepth_times import fwd_bwd, fwd_only, time_pair                  # noqa: E402
from ddvnet_times import peak_mb                                        # noqa: E402
from slowtv_monodepth_amd import functional as HF                      # noqa: E402
from slowtv_monodepth_amd.networks.decoders import DiffNetDecoder      # noqa: E402


def fuse_aten(a, bias, skip, w1, w2):
    src = torch.cat((TF.interpolate(TF.relu(a + bias.view(1, -1, 1, 1)), scale_factor=2, mode='nearest'), skip), 1)
    gate = TF.linear(TF.relu(TF.linear(src.mean((2, 3)), w1)), w2).sigmoid()
    return TF.pad(src*gate[..., None, None], (1, 1, 1, 1), mode='reflect')


def fuse_hip(a, bias, skip, w1, w2):
    return HF.up_cat_gate_pad(a, skip, w1, w2, bias, 'relu')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], kernel and ATen alternating; peak MiB above the operands',
             f'# {"operator":50} {"hip":>26} {"aten":>26}  aten/hip   peak MiB hip / aten']
    jobs = []     # (name, {'hip': fn, 'aten': fn})

    g = torch.Generator().manual_seed(0)
    kw = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32])
    torch.manual_seed(0)
    dec = DiffNetDecoder(**kw).cuda().train()
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
        return run
    # (B, Ca, Cs, h, w): stages 4 .. 1 of the ResNet-18 decoder
    for B, Ca, Cs, h, w in [(12, 512, 256, 6, 20), (12, 256, 128, 12, 40), (12, 128, 64, 24, 80), (12, 64, 64, 48, 160)]:
        C = Ca + Cs
        R = C//16
        a = torch.randn(B, Ca, h, w, generator=g).cuda().requires_grad_(True)
        bias = (0.1*torch.randn(Ca, generator=g)).cuda().requires_grad_(True)
        skip = torch.randn(B, Cs, 2*h, 2*w, generator=g).cuda().requires_grad_(True)
        w1 = (torch.randn(R, C, generator=g)/float(C)**0.5).cuda().requires_grad_(True)
        w2 = (torch.randn(C, R, generator=g)/float(R)**0.5).cuda().requires_grad_(True)
        gout = torch.randn(B, C, 2*h + 2, 2*w + 2, generator=g).cuda()
        ins = [a, bias, skip, w1, w2]
        tag = f'{B}x({Ca}+{Cs})x{2*h}x{2*w}'
        jobs.append((f'up_cat_gate_pad {tag} fwd', {'hip': fwd_only(fuse_hip, ins), 'aten': fwd_only(fuse_aten, ins)}))
        jobs.append((f'up_cat_gate_pad {tag} fwd+bwd', {'hip': fwd_bwd(fuse_hip, ins, gout), 'aten': fwd_bwd(fuse_aten, ins, gout)}))
    jobs.append(('DiffNetDecoder 12x192x640 resnet18 fwd', {'hip': decoder(True, False), 'aten': decoder(False, False)}))
    jobs.append(('DiffNetDecoder 12x192x640 resnet18 fwd+bwd', {'hip': decoder(True, True), 'aten': decoder(False, True)}))
    for name, cands in jobs:
        res = time_pair(cands, args.window, args.rounds, warmup=3)
        mem = {k: peak_mb(fn) for k, fn in cands.items()}
        h, a = res['hip'], res['aten']
        lines.append(f'{name:52} {h[0]:8.3f} [{h[1]:6.3f} ..{h[2]:7.3f}] {a[0]:8.3f} [{a[1]:6.3f} ..{a[2]:7.3f}]  {a[0]/h[0]:6.2f}   {mem["hip"]:8.1f} / {mem["aten"]:8.1f}')
        print(lines[-1], flush=True)
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
