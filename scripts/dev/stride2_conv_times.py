#!/usr/bin/env python3
"""The ResNet encoders' 3x3 stride-2 transition convolutions (`conv1` of the first BasicBlock of layer2 / layer3 / layer4; cfg 2: 640 x 192, depth net b = 12,
pose net b = 24): MIOpen's fp32 forward / data gradient / weight gradient (whatever the library runs inside the call: layout transposes and the zeroing of its
atomically added weight gradient included; the data gradient alone: `convolution_backward` with mask [True, False, False]) against the split-bf16 MFMA kernels
(`smd_conv3x3s2_mfma_*`, `smd_conv3x3s2d_mfma_bwd_data`, raw C calls; the forward with the weight pack every call pays, which leaves the data gradient's image too).
HIP events, 20 calls each, MIOpen and the kernel interleaved three times per operator, the middle one reported.  (GPU box.)
usage: stride2_conv_times.py [--hw 192x640] [--b 12 24]"""
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


print(f'# image {H}x{W}; 3x3 s2 p1, hxw = the layer\'s INPUT; us per call (HIP events, 20 calls, MIOpen and the kernel interleaved); ratio = MIOpen / MFMA;')
print('# a route needs ratio >= 1.031 (the A/B margin `_AB_MARGIN` = 0.97: the kernel at least 3 % ahead), else the shape stays MIOpen\'s')
print(f'{"stage":7s} {"C":>4s} {"CO":>4s} {"hxw":>7s} {"b":>3s} | {"MIOpen fwd":>10s} {"data":>7s} {"wgt":>7s} | {"MFMA fwd+pack":>13s} {"data":>7s} {"wgt":>7s} | {"ratio fwd":>9s} {"data":>5s} {"wgt":>5s} | ws MB')
for stage, C, div in (('layer2', 64, 4), ('layer3', 128, 8), ('layer4', 256, 16)):
    h, w, CO = H//div, W//div, 2*C
    ho, wo = (h - 1)//2 + 1, (w - 1)//2 + 1
    for B in args.b:
        gen = torch.Generator(device='cuda').manual_seed(C + B)
        x = torch.randn(B, C, h, w, device='cuda', generator=gen)
        wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
        gy = torch.randn(B, CO, ho, wo, device='cuda', generator=gen)
        wf = torch.empty(_lib.lib.smd_conv3x3_mfma_packed_bytes(C, CO, 3), device='cuda', dtype=torch.uint8); wb = torch.empty_like(wf)
        y = torch.empty_like(gy); gw = torch.empty_like(wt); gx = torch.empty_like(x)
        nwd = _lib.lib.smd_conv3x3s2d_mfma_workspace_bytes(B, C, CO, h, w); wsd = torch.empty(max(nwd, 256), device='cuda', dtype=torch.uint8)
        nws = _lib.lib.smd_conv3x3s2_mfma_workspace_bytes(B, C, CO, h, w); ws = torch.empty(max(nws, 256), device='cuda', dtype=torch.uint8)

        def fwd():
            call('smd_conv3x3_mfma_pack', wt.data_ptr(), wf.data_ptr(), wb.data_ptr(), C, CO, 3, stream())
            call('smd_conv3x3s2_mfma_fwd', x.data_ptr(), wf.data_ptr(), y.data_ptr(), ws.data_ptr(), nws, B, C, CO, h, w, stream())
        t = {k: [] for k in ('tf', 'kf', 'td', 'kd', 'tw', 'kw')}
        for _ in range(3):
            t['tf'].append(timeit(lambda: torch.conv2d(x, wt, None, 2, 1))); t['kf'].append(timeit(fwd))
            t['td'].append(timeit(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])))
            t['kd'].append(timeit(lambda: call('smd_conv3x3s2d_mfma_bwd_data', gy.data_ptr(), wb.data_ptr(), gx.data_ptr(), wsd.data_ptr(), nwd, B, C, CO, h, w, stream())))
            t['tw'].append(timeit(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])))
            t['kw'].append(timeit(lambda: call('smd_conv3x3s2_mfma_bwd_weight', x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), nws, B, C, CO, h, w, stream())))
        m = {k: sorted(v)[1] for k, v in t.items()}
        print(f'{stage:7s} {C:4d} {CO:4d} {h:3d}x{w:<3d} {B:3d} | {m["tf"]:10.1f} {m["td"]:7.1f} {m["tw"]:7.1f} | {m["kf"]:13.1f} {m["kd"]:7.1f} {m["kw"]:7.1f} | {m["tf"]/m["kf"]:9.2f} {m["td"]/m["kd"]:5.2f} '
              f'{m["tw"]/m["kw"]:5.2f} | {max(nws, nwd)/2**20:.0f}', flush=True)
