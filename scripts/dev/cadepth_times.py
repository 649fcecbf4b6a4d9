#!/usr/bin/env python3
"""Times of the CADepth operators and decoder against the plain ATen path of the same commit (profiles/cadepth_times.txt).

    python scripts/dev/cadepth_times.py [--out profiles/cadepth_times.txt]

Per operating point the two candidates alternate in one process (kernel, ATen, kernel, ATen, ...): warm-up calls, then `--rounds` rounds between two events,
each of as many calls as fill `--window` seconds; the table holds the median round and the spread of the rounds.  Forward + backward are timed together and
the forward alone.  The decoder rows time the decoder as it ships, with its static routing of the two operators, against its own plain path."""
import argparse
import contextlib
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from slowtv_monodepth_amd import functional as HF                      # noqa: E402
from slowtv_monodepth_amd.networks.decoders import CaDepthDecoder      # noqa: E402


def sp_aten(x):
    b, c, h, w = x.shape
    v = x.view(b, c, -1)
    a = v @ v.transpose(1, 2)
    return x + (torch.softmax(a.amax(-1, keepdim=True) - a, -1) @ v).view_as(x)


def se_aten(x, w1, b1, w2, b2):
    c = x.shape[1]
    a = torch.sigmoid(torch.conv2d(torch.relu(torch.conv2d(x.mean((2, 3), keepdim=True), w1.view(c, c, 1, 1), b1)), w2.view(c, c, 1, 1), b2))
    return x + x*a


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)/iters


def time_pair(cands, window, rounds, warmup=5):
    """cands: {name: callable}; -> {name: (median ms per call, min, max)} with the candidates alternating round by round, each round `window` seconds long."""
    iters = {}
    for k, fn in cands.items():
        for _ in range(warmup): fn()
        torch.cuda.synchronize()
        iters[k] = max(5, int(window*1e3/_window(fn, 10)) + 1)
    ms = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items(): ms[k].append(_window(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def fwd_bwd(fn, ins, gout):
    def run():
        for t in ins: t.grad = None
        fn(*ins).backward(gout)
    return run


def fwd_only(fn, ins):
    def run():
        with torch.no_grad(): fn(*ins)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None); ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.window} s each [min .. max], kernel and ATen alternating',
             f'# {"operator":44} {"hip":>26} {"aten":>26}  aten/hip']

    def row(name, res):
        h, a = res['hip'], res['aten']
        lines.append(f'{name:46} {h[0]:8.3f} [{h[1]:6.3f} ..{h[2]:7.3f}] {a[0]:8.3f} [{a[1]:6.3f} ..{a[2]:7.3f}]  {a[0]/h[0]:6.2f}')
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(0)
    # the two operating points, then the points the decoder's routing rule on C rests on: fewer channels, and C = 512 at a smaller batch
    for shape in [(12, 512, 6, 20), (12, 1024, 6, 20), (12, 256, 6, 20), (12, 128, 6, 20), (4, 512, 6, 20)]:
        x = (torch.relu(torch.randn(shape, generator=g)) + 0.1).cuda().requires_grad_(True)
        gout = torch.randn(shape, generator=g).cuda()
        tag = 'x'.join(map(str, shape))
        row(f'channel_attention {tag} fwd', time_pair({'hip': fwd_only(HF.channel_attention, [x]), 'aten': fwd_only(sp_aten, [x])}, args.window, args.rounds))
        row(f'channel_attention {tag} fwd+bwd', time_pair({'hip': fwd_bwd(HF.channel_attention, [x], gout), 'aten': fwd_bwd(sp_aten, [x], gout)}, args.window, args.rounds))
    for shape in [(12, 512, 12, 40), (12, 256, 24, 80), (12, 128, 48, 160), (12, 96, 96, 320), (12, 16, 192, 640)]:
        c = shape[1]
        x = torch.relu(torch.randn(shape, generator=g)).cuda().requires_grad_(True)
        ws = [(torch.randn(c, c, generator=g)/c**0.5).cuda().requires_grad_(True), (0.1*torch.randn(c, generator=g)).cuda().requires_grad_(True),
              (torch.randn(c, c, generator=g)/c**0.5).cuda().requires_grad_(True), (0.1*torch.randn(c, generator=g)).cuda().requires_grad_(True)]
        gout = torch.randn(shape, generator=g).cuda()
        tag = 'x'.join(map(str, shape))
        row(f'se_gate {tag} fwd', time_pair({'hip': fwd_only(HF.se_gate, [x] + ws), 'aten': fwd_only(se_aten, [x] + ws)}, args.window, args.rounds))
        row(f'se_gate {tag} fwd+bwd', time_pair({'hip': fwd_bwd(HF.se_gate, [x] + ws, gout), 'aten': fwd_bwd(se_aten, [x] + ws, gout)}, args.window, args.rounds))
        del x, ws, gout
    # the whole decoder, b = 12 at 192 x 640 with ResNet-18 channel counts, train mode
    kw = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32])
    torch.manual_seed(0)
    dec = CaDepthDecoder(**kw).cuda().train()
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
    row('CaDepthDecoder 12x192x640 resnet18 fwd', time_pair({'hip': decoder(True, False), 'aten': decoder(False, False)}, args.window, args.rounds, warmup=3))
    row('CaDepthDecoder 12x192x640 resnet18 fwd+bwd', time_pair({'hip': decoder(True, True), 'aten': decoder(False, True)}, args.window, args.rounds, warmup=3))
    if args.out: Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
