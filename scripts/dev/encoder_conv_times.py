#!/usr/bin/env python3
"""The ResNet encoders' 3x3 stride-1 zero-padded convolutions (C = CO, cfg 2: 640 x 192, depth net b = 12, pose net b = 24): MIOpen's fp32 forward / data
gradient / weight gradient (whatever the library runs inside the call, its layout transposes included) against the split-bf16 MFMA kernels with the padding
inside them (`smd_conv3x3z_mfma_*`, raw C calls; the forward also with the weight pack every call pays).  HIP events, 20 calls each, the two sides
interleaved per operator.  Then the decoder's coarse wide layers in their padded form (`smd_conv3x3_mfma_*`: input already padded, the data gradient
on the padded input) against MIOpen's unpadded conv2d of the same padded tensor.  `--stem`: the 7x7 stride-2 stems instead (`smd_conv7x7s2_*`).  (GPU box.)
usage: encoder_conv_times.py [--hw 192x640] [--b 12 24] [--stem]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from slowtv_monodepth_amd import miopen_tuning  # noqa: F401
from slowtv_monodepth_amd import _lib
from slowtv_monodepth_amd._lib import call

ap = argparse.ArgumentParser()
ap.add_argument('--hw', default='192x640'); ap.add_argument('--b', type=int, nargs='*', default=[12, 24])
ap.add_argument('--stem', action='store_true', help='only the 7x7 stride-2 stems (smd_conv7x7s2_*)')
args = ap.parse_args()
H, W = map(int, args.hw.split('x'))


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e)/n*1e3


def stream(): return torch.cuda.current_stream().cuda_stream


def stems():
    """The stems conv2d(x, w (64,C,7,7), stride 2, padding 3): depth net C = 3 / b = 12, pose net C = 6 / b = 24 at the cfg 2 image, the pose net at
    384 x 640 (cfg 4).  Floors: bytes of x + y at 4 TB/s; six bf16 MFMAs per fp32 product at 2.5 PFLOP/s on K padded (c, ky, 8)."""
    print('# stems 7x7 s2 p3 -> 64; us per call (HIP events, 20 calls, MIOpen and the kernel interleaved per operator); floors: bytes at 4 TB/s | MFMA at peak')
    print(f'{"C":>2s} {"HxW":>8s} {"b":>3s} | {"MIOpen fwd":>10s} {"wgt":>7s} | {"MFMA fwd+pack":>13s} {"wgt":>7s} | {"ratio fwd":>9s} {"wgt":>5s} | {"floor B":>7s} {"floor M":>7s} | ws MB')
    for C, B, (h, w) in ((3, 12, (H, W)), (6, 24, (H, W)), (6, 24, (384, 640))):
        gen = torch.Generator(device='cuda').manual_seed(C + B)
        ho, wo = (h - 1)//2 + 1, (w - 1)//2 + 1
        x = torch.randn(B, C, h, w, device='cuda', generator=gen)
        wt = torch.randn(64, C, 7, 7, device='cuda', generator=gen)/(7*C**0.5)
        gy = torch.randn(B, 64, ho, wo, device='cuda', generator=gen)
        wp = torch.empty(_lib.lib.smd_conv7x7s2_packed_bytes(C, 64), device='cuda', dtype=torch.uint8)
        y = torch.empty_like(gy); gw = torch.empty_like(wt)
        nws = _lib.lib.smd_conv7x7s2_workspace_bytes(B, C, 64, h, w); ws = torch.empty(max(nws, 256), device='cuda', dtype=torch.uint8)

        def fwd():
            call('smd_conv7x7s2_pack', wt.data_ptr(), wp.data_ptr(), C, 64, stream())
            call('smd_conv7x7s2_fwd', x.data_ptr(), wp.data_ptr(), y.data_ptr(), B, C, 64, h, w, stream())
        t = {k: [] for k in ('tf', 'kf', 'tw', 'kw')}
        for _ in range(3):                                   # interleaved
            t['tf'].append(timeit(lambda: torch.conv2d(x, wt, None, 2, 3))); t['kf'].append(timeit(fwd))
            t['tw'].append(timeit(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1, [False, True, False])))
            t['kw'].append(timeit(lambda: call('smd_conv7x7s2_bwd_weight', x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), nws, B, C, 64, h, w, stream())))
        m = {k: sorted(v)[1] for k, v in t.items()}
        fb = (x.numel() + y.numel())*4/4e12*1e6
        fm = 6*2*64*(8*2*((7*C + 1)//2))*B*ho*wo/2.5e15*1e6
        print(f'{C:2d} {h:3d}x{w:<4d} {B:3d} | {m["tf"]:10.1f} {m["tw"]:7.1f} | {m["kf"]:13.1f} {m["kw"]:7.1f} | {m["tf"]/m["kf"]:9.2f} {m["tw"]/m["kw"]:5.2f} | '
              f'{fb:7.1f} {fm:7.1f} | {nws/2**20:.0f}', flush=True)


if args.stem:
    stems(); sys.exit(0)

print(f'# image {H}x{W}; us per call (HIP events, 20 calls); ratio = MIOpen / MFMA (> 1: the MFMA kernel is faster); fwd+pack = the forward as production pays it')
print(f'{"stage":7s} {"C":>4s} {"hxw":>7s} {"b":>3s} | {"MIOpen fwd":>10s} {"data":>7s} {"wgt":>7s} | {"MFMA fwd+pack":>13s} {"data":>7s} {"wgt":>7s} | '
      f'{"ratio fwd":>9s} {"data":>5s} {"wgt":>5s} | ws MB')
for stage, C, div in (('layer1', 64, 4), ('layer2', 128, 8), ('layer3', 256, 16), ('layer4', 512, 32)):
    h, w = H//div, W//div
    for B in args.b:
        gen = torch.Generator(device='cuda').manual_seed(C + B)
        x = torch.randn(B, C, h, w, device='cuda', generator=gen)
        wt = torch.randn(C, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
        gy = torch.randn(B, C, h, w, device='cuda', generator=gen)
        t_f = timeit(lambda: torch.conv2d(x, wt, None, 1, 1))
        t_d = timeit(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False]))
        t_w = timeit(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False]))
        nb = _lib.lib.smd_conv3x3_mfma_packed_bytes(C, C, 3)
        wf = torch.empty(nb, device='cuda', dtype=torch.uint8); wb = torch.empty(nb, device='cuda', dtype=torch.uint8)
        y = torch.empty_like(gy); gx = torch.empty_like(x); gw = torch.empty_like(wt)
        nws = _lib.lib.smd_conv3x3z_mfma_workspace_bytes(B, C, C, h, w); ws = torch.empty(max(nws, 256), device='cuda', dtype=torch.uint8)

        def fwd():
            call('smd_conv3x3_mfma_pack', wt.data_ptr(), wf.data_ptr(), wb.data_ptr(), C, C, 3, stream())
            call('smd_conv3x3z_mfma_fwd', x.data_ptr(), wf.data_ptr(), y.data_ptr(), ws.data_ptr(), nws, B, C, C, h, w, 3, stream())
        k_f = timeit(fwd)
        k_d = timeit(lambda: call('smd_conv3x3z_mfma_bwd_data', gy.data_ptr(), wb.data_ptr(), gx.data_ptr(), ws.data_ptr(), nws, B, C, C, h, w, 3, stream()))
        k_w = timeit(lambda: call('smd_conv3x3z_mfma_bwd_weight', x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), nws, B, C, C, h, w, 3, stream()))
        print(f'{stage:7s} {C:4d} {h:3d}x{w:<3d} {B:3d} | {t_f:10.1f} {t_d:7.1f} {t_w:7.1f} | {k_f:13.1f} {k_d:7.1f} {k_w:7.1f} | '
              f'{t_f/k_f:9.2f} {t_d/k_d:5.2f} {t_w/k_w:5.2f} | {nws/2**20:.0f}', flush=True)

print('# decoder coarse layers, padded form (xp = B x C x (h + 2) x (w + 2)); same columns')
for stage, C, CO, div in (('dec4', 512, 256, 32), ('dec4', 512, 256, 16), ('dec3', 256, 128, 16), ('dec3', 256, 128, 8)):
    h, w = H//div, W//div
    for B in args.b:
        gen = torch.Generator(device='cuda').manual_seed(C + CO + B + h)
        xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen)
        wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
        gy = torch.randn(B, CO, h, w, device='cuda', generator=gen)
        t_f = timeit(lambda: torch.conv2d(xp, wt))
        t_d = timeit(lambda: torch.ops.aten.convolution_backward(gy, xp, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False]))
        t_w = timeit(lambda: torch.ops.aten.convolution_backward(gy, xp, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False]))
        nb = _lib.lib.smd_conv3x3_mfma_packed_bytes(C, CO, 3)
        wf = torch.empty(nb, device='cuda', dtype=torch.uint8); wb = torch.empty(nb, device='cuda', dtype=torch.uint8)
        y = torch.empty_like(gy); gx = torch.empty_like(xp); gw = torch.empty_like(wt)
        nws = _lib.lib.smd_conv3x3_mfma_workspace_bytes(B, C, CO, h, w); ws = torch.empty(max(nws, 256), device='cuda', dtype=torch.uint8)

        def fwd():
            call('smd_conv3x3_mfma_pack', wt.data_ptr(), wf.data_ptr(), wb.data_ptr(), C, CO, 3, stream())
            call('smd_conv3x3_mfma_fwd', xp.data_ptr(), wf.data_ptr(), y.data_ptr(), ws.data_ptr(), nws, B, C, CO, h, w, 3, stream())
        k_f = timeit(fwd)
        k_d = timeit(lambda: call('smd_conv3x3_mfma_bwd_data', gy.data_ptr(), wb.data_ptr(), gx.data_ptr(), ws.data_ptr(), nws, B, C, CO, h, w, 3, stream()))
        k_w = timeit(lambda: call('smd_conv3x3_mfma_bwd_weight', xp.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), nws, B, C, CO, h, w, 3, stream()))
        print(f'{stage:7s} {C:4d} {h:3d}x{w:<3d} {B:3d} | {t_f:10.1f} {t_d:7.1f} {t_w:7.1f} | {k_f:13.1f} {k_d:7.1f} {k_w:7.1f} | '
              f'{t_f/k_f:9.2f} {t_d/k_d:5.2f} {t_w/k_w:5.2f} | {nws/2**20:.0f}', flush=True)
