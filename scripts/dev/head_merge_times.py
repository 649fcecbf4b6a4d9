#!/usr/bin/env python
"""Section 1 of profiles/head_merge_times.txt: kernel durations of the output heads at cfg 2's four head shapes (b = 12), fp32 and bf16 activations: n = 1 through
conv3x3_head and n = 2 through conv3x3_headn with a sigmoid, then n = 1 through conv3x3_headn with relu (the uncertainty mask's head).  One process per library (SMD_HOTPATH_LIB names the one to load), each under a kernel trace:

    SMD_HOTPATH_LIB=<lib> rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/dev/head_merge_times.py run
    python scripts/dev/head_merge_times.py table parent1=<csv> this1=<csv> parent2=<csv> this2=<csv>

`table` prints the median duration per (kernel, grid) of every trace and compares the slower run of this tree with the slower run of the parent.
"""
import csv
import re
import statistics
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

SHAPES = [(16, 192, 640), (32, 96, 320), (64, 48, 160), (128, 24, 80)]


CALLS = 200


def run(calls=CALLS):
    import torch
    import slowtv_monodepth_amd.functional as F
    g = torch.Generator(device='cuda').manual_seed(0)
    for n, op, act in ((1, F.conv3x3_head, 'sigmoid'), (2, F.conv3x3_headn, 'sigmoid'), (1, F.conv3x3_headn, 'relu')):
        for dt in (torch.float32, torch.bfloat16):
            for C, h, w in SHAPES:
                xp = torch.randn(12, C, h + 2, w + 2, device='cuda', generator=g).to(dt).requires_grad_()
                wt = (0.1*torch.randn(n, C, 3, 3, device='cuda', generator=g)).requires_grad_()
                b = torch.zeros(n, device='cuda', requires_grad=True)
                gy = torch.randn(12, n, h, w, device='cuda', generator=g)
                for _ in range(calls):
                    op(xp, wt, b, act).backward(gy)
                    xp.grad = wt.grad = b.grad = None
                torch.cuda.synchronize()


def successor(name):
    name = re.sub(r'^(void )?smd::|\(.*$', '', name).replace('k_headn_', 'k_head_')
    m = re.match(r'(k_head_\w+)<(.*)>$', name)
    if not m:
        return name
    args = m.group(2).split(', ')
    return '%s<%s>' % (m.group(1), ', '.join((['1'] if len(args) < (5 if m.group(1) == 'k_head_fwd' else 3) else []) + args))


def medians(path):
    d, seen = {}, {}
    for r in csv.DictReader(open(path)):
        if 'k_head' in r['Kernel_Name']:
            key = (successor(r['Kernel_Name']), '%sx%sx%s' % (r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z']))
            seen[key] = seen.get(key, 0) + 1
            per = CALLS*(2 if 'finalize' in key[0] else 1)     # (the finalize has one name for fp32 and bf16 rows alike: two cases per block)
            key += ((seen[key] - 1)//per,)                      # the same kernel and grid serve several cases of `run`, CALLS launches each, one after the other
            d.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp']))/1e3)
    return {k: (statistics.median(v), len(v)) for k, v in d.items()}


def table(args):
    runs = [a.split('=', 1) for a in args]
    data = [medians(p) for _, p in runs]
    print('%-50s %14s %5s | %s  us (median) | verdict' % ('kernel of this tree', 'grid (threads)', 'calls', ' '.join('%8s' % n for n, _ in runs)))
    for key in data[0]:
        t = [d[key][0] for d in data]
        par = [v for (n, _), v in zip(runs, t) if n.startswith('parent')]
        new = [v for (n, _), v in zip(runs, t) if not n.startswith('parent')]
        if min(new) > max(par):
            verdict = 'every run above every parent run: +%.2f us (%.1f %%) over the parent\'s slowest' % (min(new) - max(par), 100*(min(new) - max(par))/max(par))
        elif max(new) > max(par):
            verdict = 'overlaps; slowest run +%.2f us above the parent\'s slowest' % (max(new) - max(par))
        else:
            verdict = 'within the parent\'s spread' if max(new) >= min(par) else 'below the parent\'s spread'
        print('%-50s %14s %5d | %s | %s' % (key[0].replace('__hip_bfloat16', 'bf16') + (' (relu)' if key[2] else ''), key[1], data[0][key][1], ' '.join('%8.2f' % v for v in t), verdict))


if __name__ == '__main__':
    run() if sys.argv[1] == 'run' else table(sys.argv[2:])
