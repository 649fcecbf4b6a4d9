#!/usr/bin/env python
"""Bit-for-bit comparison of every operator whose kernels use the shared channel sweep (smd_norm_dev.h) or the block-sum family (smd_common.h) between two
builds of the library (SMD_HOTPATH_LIB names the one to load):

    SMD_HOTPATH_LIB=<parent's lib> python scripts/dev/norm_sweep_dump.py dump a.json
    python scripts/dev/norm_sweep_dump.py dump b.json
    python scripts/dev/norm_sweep_dump.py cmp a.json b.json          -> "k of k equal"

What runs, forward and every gradient: the value-edge table (tests/value_edges.py) of batch_norm_act, layer_norm_cf, dwconv7x7 and the ELU glue; every entry
of the gradient-subset table (tests/grad_subsets.py) but the convolutions', with all its operands as leaves (each of them ends in the one-block sum of smd_misc.hip; among them se_gate,
the mask regularisers, photo_error, recon_reduce, view_synth and the smoothness); BatchNorm at the shapes where the sweep changes its path, with and without
residual / ReLU / a requested g_residual; LayerNorm at C = 1, C % 4 != 0, pixels % 64 != 0, two chunks of the gamma / beta reduction, fp32 and bf16; the
second-order smoothness; crop_resize.  An array is recorded as the SHA-256 of its bytes.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

# small scalar / small f4 / chunked scalar / chunked f4; N*HW = 16384 (last single launch: kept + re-read values), the same in 1-float steps, 16388 (first
# chunked); HW = 8196 with N = 3 (sample boundaries inside a chunk); above 128*8192 values per channel (chunks longer than a thread's registers)
BN_SHAPES = [(2, 3, 5, 7), (4, 8, 6, 20), (3, 2, 77, 71), (12, 64, 24, 80), (1, 2, 128, 128), (1, 2, 101, 101), (1, 2, 4097, 4), (3, 2, 4, 2049), (1, 2, 1023, 1027),
             (1, 2, 1024, 1028)]
LN_SHAPES = [(2, 1, 3, 3), (1, 7, 33, 65), (2, 96, 6, 20), (1, 5, 91, 91), (2, 1030, 5, 7)]
EDGE_OPS = ('batch_norm_act', 'layer_norm_cf', 'dwconv7x7', 'elu_pad', 'elu_up_cat_pad')


def dump(path):
    import torch
    import slowtv_monodepth_amd.functional as F
    import grad_subsets as G
    import value_edges as V
    out = {}

    def put(key, t):
        if not torch.is_tensor(t): return
        assert key not in out, key
        out[key] = hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    for c in V.CASES:
        if c.op in EDGE_OPS:
            ops = c.operands(torch.Generator().manual_seed(len(c.name)*7919 + 17))
            for k, v in c.run(F, {k: v.cuda() for k, v in ops.items()}).items(): put('edge %s %s' % (c.name, k), v)
    for e in G.TABLE:
        if e.wrapper.startswith('conv'): continue      # not touched, and no yardstick: conv3x3_same's bits differ between two processes of ONE build
        o = e.operands(torch.Generator().manual_seed(len(e.name)*7919 + 31), frozenset())
        try: res = G.run_entry(e, F, {k: v.cuda() for k, v in o.items()}, frozenset(e.diff))
        except (ValueError, TypeError, KeyError) as err:      # an entry this plain run does not serve is named, not hidden
            print('not run: %s: %r' % (e.name, err))
            continue
        for k, v in res.items():
            if k not in e.loose: put('subset %s %s' % (e.name, k), v)      # (loose: sums of float atomics, whose bits differ from run to run of ONE build)
    for shape in BN_SHAPES:
        C = shape[1]
        g = torch.Generator(device='cuda').manual_seed(sum(shape))
        x0 = 2*torch.randn(*shape, device='cuda', generator=g) + 3*torch.randn(1, C, 1, 1, device='cuda', generator=g)
        r0, gy = torch.randn(*shape, device='cuda', generator=g), torch.randn(*shape, device='cuda', generator=g)
        w0, b0 = torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)
        for relu in (False, True):
            for res in ('none', 'leaf', 'constant'):      # constant: a residual that asks for no gradient
                x, w, b = x0.clone().requires_grad_(), w0.clone().requires_grad_(), b0.clone().requires_grad_()
                r = None if res == 'none' else r0.clone().requires_grad_(res == 'leaf')
                rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
                y = F.batch_norm_act(x, w, b, rm, rv, residual=r, momentum=0.1, eps=1e-5, relu=relu)
                y.backward(gy)
                for k, t in (('y', y), ('g_x', x.grad), ('g_w', w.grad), ('g_b', b.grad), ('g_r', r.grad if res == 'leaf' else None), ('rm', rm), ('rv', rv)):
                    put('bn %s relu=%d res=%s %s' % (shape, relu, res, k), t)
    for shape in LN_SHAPES:
        C = shape[1]
        g = torch.Generator(device='cuda').manual_seed(sum(shape))
        x0 = 2*torch.randn(*shape, device='cuda', generator=g) + 3*torch.randn(shape[0], 1, *shape[2:], device='cuda', generator=g)
        w0, b0, gy = torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g), torch.randn(*shape, device='cuda', generator=g)
        for dt in (torch.float32, torch.bfloat16):
            x, w, b = x0.clone().requires_grad_(), w0.clone().requires_grad_(), b0.clone().requires_grad_()
            y = F.layer_norm_cf(x, w, b, 1e-6, out_dtype=dt)
            y.backward(gy.to(dt))
            for k, t in (('y', y), ('g_x', x.grad), ('g_w', w.grad), ('g_b', b.grad)): put('ln %s %s %s' % (shape, dt, k), t)
    g = torch.Generator(device='cuda').manual_seed(5)
    imgs = torch.rand(2, 3, 40, 72, device='cuda', generator=g)
    for edges in (False, True):
        d = {s: (0.05 + 0.9*torch.rand(2, 1, 40 >> s, 72 >> s, device='cuda', generator=g)).requires_grad_() for s in range(3)}
        loss, dg, ig = F.disp_smooth_fused(d, imgs, use_edges=edges, want_aux=True, use_laplacian=True)
        loss.backward()
        for k, t in [('loss', loss), ('disp_grad', dg), ('image_grad', ig)] + [('g_d%d' % s, v.grad) for s, v in d.items()]: put('laplacian edges=%d %s' % (edges, k), t)
    K = torch.eye(4, device='cuda').repeat(2, 1, 1)
    outs, Ko = F.crop_resize([imgs, imgs[:, :1].contiguous()], (30, 60), (19, 45), K)
    for i, t in enumerate(outs + [Ko]): put('crop_resize %d' % i, t)
    torch.cuda.synchronize()
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
