#!/usr/bin/env python
"""profiles/norm_sweep_times.txt: kernel durations of every k_bn_* and k_ln_cf_* kernel at the encoder shapes of cfg 2 (ResNet-18, 192x640, b = 12) and cfg 5
(ConvNeXt-B, 384x640, b = 12), and of one representative launch of each other kernel whose block sum moved to smd_common.h.  One process per library
(SMD_HOTPATH_LIB names the one to load), each under a kernel trace, the parent's build and this tree's alternately:

    SMD_HOTPATH_LIB=<lib> rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/dev/norm_sweep_times.py run
    python scripts/dev/norm_sweep_times.py table parent1=<csv> this1=<csv> parent2=<csv> this2=<csv> parent3=<csv> this3=<csv>

`table` prints the median duration per (kernel, grid) of every trace.  A kernel is NAMED when this tree is above the parent in every alternation (this_i >
parent_i for all i), with its smallest delta, and whether it is also above the parent's slowest run.
"""
import csv
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

BN_SHAPES = [(12, 64, 96, 320), (12, 64, 48, 160), (12, 128, 24, 80), (12, 256, 12, 40), (12, 512, 6, 20)]      # stem, layer1..4 of cfg 2's encoders
LN_SHAPES = [(12, 128, 96, 160), (12, 256, 48, 80), (12, 512, 24, 40), (12, 1024, 12, 20)]                       # the four stages of cfg 5's depth encoder
KERNELS = ('k_bn_', 'k_ln_cf_', 'k_dwconv7_wrw', 'k_se_pool', 'k_scale_mean_fwd', 'k_view_synth_bwd', 'k_recon_reduce_fwd', 'k_smooth_lap_main', 'k_elu_pad_bwd',
           'k_elu_up_cat_pad_bwd_a', 'k_sum_partials')
CALLS = 30


def run(calls=CALLS):
    import torch
    import slowtv_monodepth_amd.functional as F
    g = torch.Generator(device='cuda').manual_seed(0)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)

    def repeat(fn, *leaves):
        for _ in range(calls):
            fn()
            for t in leaves: t.grad = None
        torch.cuda.synchronize()

    for shape in BN_SHAPES:
        C = shape[1]
        for res in (False, True):
            x, r, w, b, gy = rn(*shape).requires_grad_(), (rn(*shape).requires_grad_() if res else None), rn(C).requires_grad_(), rn(C).requires_grad_(), rn(*shape)
            rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
            repeat(lambda: F.batch_norm_act(x, w, b, rm, rv, residual=r, momentum=0.1, eps=1e-5, relu=True).backward(gy), x, w, b, *([r] if res else []))
    for shape in LN_SHAPES:
        C = shape[1]
        x, w, b, gy = rn(*shape).requires_grad_(), rn(C).requires_grad_(), rn(C).requires_grad_(), rn(*shape).bfloat16()
        repeat(lambda: F.layer_norm_cf(x, w, b, 1e-6, out_dtype=torch.bfloat16).backward(gy), x, w, b)
    x, w, b, gy = rn(12, 128, 96, 160).requires_grad_(), rn(128, 1, 7, 7).requires_grad_(), rn(128).requires_grad_(), rn(12, 128, 96, 160)
    repeat(lambda: F.dwconv7x7(x, w, b).backward(gy), x, w, b)
    x, w1, b1, w2, b2 = rn(12, 64, 48, 160).requires_grad_(), rn(64, 64).requires_grad_(), rn(64).requires_grad_(), rn(64, 64).requires_grad_(), rn(64).requires_grad_()
    gy = rn(12, 64, 48, 160)
    repeat(lambda: F.se_gate(x, w1, b1, w2, b2).backward(gy), x, w1, b1, w2, b2)
    ms = [torch.rand(12, 2, 192 >> s, 640 >> s, device='cuda', generator=g).clamp_(0.01, 0.99).requires_grad_() for s in range(4)]
    repeat(lambda: F.scale_mean(ms, 'bce_ones').backward(), *ms)
    inp, depth = torch.rand(12, 3, 192, 640, device='cuda', generator=g).requires_grad_(), (1 + 9*torch.rand(12, 1, 192, 640, device='cuda', generator=g)).requires_grad_()
    T = torch.eye(4, device='cuda').repeat(12, 1, 1); T[:, 0, 3] = 0.1
    K = torch.tensor([[0.58*640, 0, 320, 0], [0, 1.92*192, 96, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda').repeat(12, 1, 1)
    gw = rn(12, 3, 192, 640)
    def vs():
        out = F.view_synth(inp, depth, T, K)
        (out[0] if isinstance(out, (tuple, list)) else out).backward(gw)
    repeat(vs, inp, depth)
    ew = torch.rand(2, 12, 192, 640, device='cuda', generator=g).requires_grad_()
    repeat(lambda: F.recon_reduce(ew, None, use_min=True)[0].backward(), ew)
    imgs = torch.rand(12, 3, 192, 640, device='cuda', generator=g)
    d = {s: torch.rand(12, 1, 192 >> s, 640 >> s, device='cuda', generator=g).requires_grad_() for s in range(4)}
    repeat(lambda: F.disp_smooth_fused(d, imgs, use_edges=True, want_aux=False, use_laplacian=True)[0].backward(), *d.values())
    x, b, gy = rn(12, 64, 48, 160).requires_grad_(), rn(64).requires_grad_(), rn(12, 64, 50, 162)
    repeat(lambda: F.elu_pad(x, b).backward(gy), x, b)
    a, skip, b, gy = rn(12, 64, 24, 80).requires_grad_(), rn(12, 64, 48, 160).requires_grad_(), rn(64).requires_grad_(), rn(12, 128, 50, 162)
    repeat(lambda: F.elu_up_cat_pad(a, skip, b).backward(gy), a, skip, b)


def medians(path):
    d = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r'^(void )?smd::|\(.*$', '', r['Kernel_Name']).replace('__hip_bfloat16', 'bf16')
        if name.startswith(KERNELS):
            d.setdefault((name, '%sx%sx%s' % (r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z'])), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp']))/1e3)
    return {k: (statistics.median(v), len(v)) for k, v in d.items()}


def table(args):
    runs = [a.split('=', 1) for a in args]
    data = [medians(p) for _, p in runs]
    print('%-34s %16s %5s | %s  us (median) | verdict' % ('kernel', 'grid (threads)', 'calls', ' '.join('%8s' % n for n, _ in runs)))
    named = 0
    for key in sorted(data[0]):
        if not all(key in d for d in data): continue
        t = [d[key][0] for d in data]
        par = [v for (n, _), v in zip(runs, t) if n.startswith('parent')]
        new = [v for (n, _), v in zip(runs, t) if not n.startswith('parent')]
        if all(b > a for a, b in zip(par, new)):
            named += 1
            verdict = 'ABOVE the parent in every alternation: at least +%.2f us (%.1f %%); %s' % (
                min(b - a for a, b in zip(par, new)), 100*min((b - a)/a for a, b in zip(par, new)),
                'also above the parent\'s slowest run' if min(new) > max(par) else 'inside the parent\'s own spread (%.2f .. %.2f)' % (min(par), max(par)))
        elif all(b < a for a, b in zip(par, new)): verdict = 'below the parent in every alternation'
        else: verdict = 'mixed'
        print('%-34s %16s %5d | %s | %s' % (key[0], key[1], data[0][key][1], ' '.join('%8.2f' % v for v in t), verdict))
    print('%d kernel(s) above the parent in every alternation' % named)


if __name__ == '__main__':
    run() if sys.argv[1] == 'run' else table(sys.argv[2:])
