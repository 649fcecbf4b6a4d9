#!/usr/bin/env python3
"""The ResNet encoders' 3x3 stride-1 zero-padded convolutions (C = CO, cfg 2: 640 x 192, depth net b = 12, pose net b = 24): MIOpen's fp32 forward / data
gradient / weight gradient (whatever the library runs inside the call, its layout transposes included) against the split-bf16 MFMA kernels with the padding
inside them (`smd_conv3x3z_mfma_*`, raw C calls; the forward also with the weight pack every call pays).  HIP events, 20 calls each, the two sides
interleaved per operator.  Then the decoder's coarse wide layers in their padded form (`smd_conv3x3_mfma_*`: input already padded, the data gradient
on the padded input) against MIOpen's unpadded conv2d of the same padded tensor.  (GPU box.)
usage: encoder_conv_times.py [--hw 192x640] [--b 12 24]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from slowtv_monodepth_amd import miopen_tuning  # noqa: F401
from slowtv_monodepth_amd import _lib
from slowtv_monodepth_amd._lib import call

ap = argparse.ArgumentParser()
ap.add_argument('--hw', default='192x640'); ap.add_argument('--b', type=int, nargs='*', default=[12, 24])
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
