#!/usr/bin/env python
"""Bit-for-bit comparison of the output heads between two builds of the library (SMD_HOTPATH_LIB names the one to load):

    SMD_HOTPATH_LIB=<parent's lib> python scripts/dev/head_merge_dump.py dump a.json
    python scripts/dev/head_merge_dump.py dump b.json
    python scripts/dev/head_merge_dump.py cmp a.json b.json          -> "k of k equal"

y, g_xp, g_w and g_b of conv3x3_head (n = 1; sigmoid, none) and conv3x3_headn (n = 1..4; sigmoid, none, relu) with fp32 and bf16 activations, at the shapes of
test_head_entries_agree (plus an odd width on the unsplit path) and cfg 2's four head shapes; an array is recorded as the SHA-256 of its bytes.
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

SHAPES = [(2, 4, 9, 70), (2, 4, 9, 71), (2, 8, 342, 130), (1, 16, 6, 8), (1, 8, 5, 7), (12, 16, 192, 640), (12, 32, 96, 320), (12, 64, 48, 160), (12, 128, 24, 80)]


def dump(path):
    import torch
    import slowtv_monodepth_amd.functional as F
    out = {}
    for name, op, ns, acts in (('head', F.conv3x3_head, (1,), ('sigmoid', None)), ('headn', F.conv3x3_headn, (1, 2, 3, 4), ('sigmoid', None, 'relu'))):
        for n in ns:
            for act in acts:
                for dt in (torch.float32, torch.bfloat16):
                    for B, C, h, w in SHAPES:
                        g = torch.Generator(device='cuda').manual_seed(1000*n + C + h)
                        xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=g).to(dt).requires_grad_()
                        wt = (0.2*torch.randn(n, C, 3, 3, device='cuda', generator=g)).requires_grad_()
                        b = (0.1*torch.randn(n, device='cuda', generator=g)).requires_grad_()
                        y = op(xp, wt, b, act)
                        y.backward(torch.randn(B, n, h, w, device='cuda', generator=g))
                        for k, t in (('y', y.detach()), ('g_xp', xp.grad), ('g_w', wt.grad), ('g_b', b.grad)):
                            out['%s n=%d %s %s %s %s' % (name, n, act, dt, (B, C, h, w), k)] = hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
    json.dump(out, open(path, 'w'), indent=0)
    print('%d arrays' % len(out))


def cmp(a, b):
    a, b = json.load(open(a)), json.load(open(b))
    assert a.keys() == b.keys()
    bad = [k for k in a if a[k] != b[k]]
    for k in bad:
        print('differs:', k)
    print('%d of %d equal' % (len(a) - len(bad), len(a)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == 'dump' else cmp(sys.argv[2], sys.argv[3]))
