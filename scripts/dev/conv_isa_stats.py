#!/usr/bin/env python3
"""Instruction mix of the decoder convolutions' inner loops, from the ISA hipcc generates (no GPU needed): MFMAs against LDS reads / writes, vector-memory
instructions and other vector instructions per K chunk (forward forms) / per row (weight gradients).  VERDICT r5 item 2 asked for the MFMA : LDS-read ratio.
usage: python scripts/dev/conv_isa_stats.py >> profiles/rNN_instruction_counts.txt"""
import re, shutil, subprocess, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
CSRC = ROOT/'slowtv_monodepth_amd'/'csrc'

FLAGS = ['-O3', '-std=c++17', '-fPIC', '-fno-slp-vectorize', '--offload-arch=gfx950']      # csrc/Makefile's CXXFLAGS

def isa(src):
    """-> {demangled kernel name without its argument list: (body lines, resource lines of the kernel's own 'Kernel info' block)}"""
    out = Path(tempfile.mkdtemp())/'k.s'
    subprocess.run(['/opt/rocm/bin/hipcc', *FLAGS, '-S', '--cuda-device-only', src, '-o', str(out)], check=True, stderr=subprocess.DEVNULL, cwd=CSRC)
    lines = out.read_text().split('\n')
    syms = [l.split()[1] for l in lines if l.strip().startswith('.amdhsa_kernel ')]
    filt = shutil.which('llvm-cxxfilt') or shutil.which('llvm-cxxfilt', path='/opt/rocm/lib/llvm/bin') or shutil.which('c++filt')
    if filt is None: raise SystemExit('conv_isa_stats.py needs a demangler: llvm-cxxfilt (ROCm) or c++filt (binutils) on the PATH')
    names = subprocess.run([filt], input='\n'.join(syms), capture_output=True, text=True, check=True).stdout.split('\n')
    kernels = {}
    for sym, name in zip(syms, names):
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ':'))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        info = next(i for i in range(end, len(lines)) if lines[i].startswith('; Kernel info'))
        res = {m.group(1): m.group(2) for l in lines[info:info + 30] if (m := re.match(r'; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)', l))}
        name = name.replace('(anonymous namespace)::', '').replace('smd::', '').replace('__hip_bfloat16', 'bf16')    # 'void k<args>(parameters)'
        kernels[name[len('void '):name.index('(')]] = (lines[start:end], res)
    return kernels

def kernel(kernels, key):
    """key: the kernel's name with its template arguments as the demangler prints them, e.g. 'k_conv_mfma<64, 3, 0, float, float, 1>'."""
    if key not in kernels: raise SystemExit(f'no kernel {key!r}; this source has: ' + ', '.join(sorted(kernels)))
    return kernels[key]

def count(body):
    c = {'mfma': 0, 'ds_read': 0, 'ds_write': 0, 'vmem_load': 0, 'vmem_store': 0, 'valu': 0, 'salu': 0, 'barrier': 0, 'waitcnt': 0}
    for l in body:
        t = l.strip().split(' ')[0] if l.strip() else ''
        if t.startswith('v_mfma'): c['mfma'] += 1
        elif t.startswith('ds_read') or t.startswith('ds_load'): c['ds_read'] += 1
        elif t.startswith('ds_write') or t.startswith('ds_store'): c['ds_write'] += 1
        elif t.startswith('global_load') or t.startswith('buffer_load'): c['vmem_load'] += 1
        elif t.startswith('global_store') or t.startswith('buffer_store'): c['vmem_store'] += 1
        elif t.startswith('v_'): c['valu'] += 1
        elif t == 's_barrier': c['barrier'] += 1
        elif t == 's_waitcnt': c['waitcnt'] += 1
        elif t.startswith('s_'): c['salu'] += 1
    return c

def main_loop(body):
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r'^(\.LBB\d+_\d+):', l))}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r's_c?branch\w*\s+(\.LBB\d+_\d+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i: loops.append((labels[m.group(1)], i))
    best = max(loops, key=lambda ab: sum(1 for l in body[ab[0]:ab[1]] if 'v_mfma' in l)) if loops else (0, len(body))
    return body[best[0]:best[1]]

def report(lines, key, what, unit):
    body, meta = kernel(lines, key)
    whole, loop = count(body), count(main_loop(body))
    if loop['mfma'] == 0: loop = whole                     # (no loop around the MFMAs: the kernel is one chunk)
    print(f'{what}')
    print(f'  main loop ({unit}): {loop["mfma"]} MFMA, {loop["ds_read"]} LDS reads, {loop["ds_write"]} LDS writes, {loop["vmem_load"]} vector-memory loads, {loop["valu"]} other vector, '
          f'{loop["salu"]} scalar, {loop["barrier"]} barriers, {loop["waitcnt"]} waits  ->  MFMA : LDS read = {loop["mfma"]/max(loop["ds_read"], 1):.2f}, other vector per MFMA = {loop["valu"]/max(loop["mfma"], 1):.2f}')
    print(f'  whole kernel: {whole["mfma"]} MFMA, {whole["vmem_load"]} loads, {whole["vmem_store"]} stores; {meta.get("NumVgprs")} VGPRs, {meta.get("NumAgprs")} AGPRs, {meta.get("TotalNumSgprs")} SGPRs, '
          f'{meta.get("ScratchSize")} bytes of scratch, {meta.get("LDSByteSize")} bytes of LDS, occupancy {meta.get("Occupancy")}\n')

print('\nDecoder convolutions, produced by scripts/dev/conv_isa_stats.py\n')
L = isa('smd_conv_mfma.hip')
report(L, 'k_conv_mfma<64, 3, 0, float, float, 1>', 'k_conv_mfma<64, 3, 0, float, float, 1>   (wide forward, fp32 tensors, three pieces: 4 rows x 64 columns x 32 output channels per block; a chunk = 16 channels x 9 taps)', 'one K chunk of one wave: 9 taps x 2 pixel tiles x 6 products = 108 MFMA')
report(L, 'k_conv_mfma<64, 3, 2, float, float, 1>', 'k_conv_mfma<64, 3, 2, float, float, 1>   (wide data gradient)', 'one K chunk')
report(L, 'k_conv_mfma<64, 3, 1, float, float, 1>', 'k_conv_mfma<64, 3, 1, float, float, 1>   (zero-padded "same" layer, forward and data gradient)', 'one K chunk')
report(L, 'k_conv_mfma<64, 1, 0, bf16, bf16, 1>', 'k_conv_mfma<64, 1, 0, bf16, bf16, 1>     (wide forward, bf16 tensors, one piece)', 'one K chunk: 18 MFMA')
report(L, 'k_conv16_mfma<1, 3, false, float, float>', 'k_conv16_mfma<1, 3, false, float, float> (thin forward 16 -> 16: 16x16x32 MFMA, two taps per K step, weights in registers; no loop — one chunk)', 'the whole tile: 5 K steps x 4 rows x 6 products = 120 MFMA')
G = isa('smd_conv_wgrad.hip')
report(G, 'k_wgrad_dma<WgradWide, 3, false>', 'k_wgrad_dma<WgradWide, 3, false>         (wide weight gradient, fp32 tensors: 32 output x 64 input channels per block, loop over INPUT rows, ring of four RAW rows by LDS-DMA, split at fragment read; the loop body is three rows)', 'three input rows of one wave (its K step of 16 columns, one tile of 32 input channels): 3 x 54 MFMA')
report(G, 'k_wgrad_dma<WgradWide, 3, true>', 'k_wgrad_dma<WgradWide, 3, true>          (the same on the unpadded input of a zero-padded layer)', 'three input rows of one wave')
report(G, 'k_wgrad_dma<WgradThin<1>, 3, false>', 'k_wgrad_dma<WgradThin<1>, 3, false>      (thin weight gradient 16 -> 16, fp32 tensors: the same on 16x16x32, strips of 64 columns)', 'three input rows of one wave')
report(G, 'k_wgrad_dma<WgradThin<2>, 3, false>', 'k_wgrad_dma<WgradThin<2>, 3, false>      (thin weight gradient 32 -> 16)', 'three input rows of one wave')
report(G, 'k_wgrad_staged<WgradWide, 1, bf16>', 'k_wgrad_staged<WgradWide, 1, bf16>       (wide weight gradient, bf16 tensors: rows staged through registers, split + filed after the row\'s MFMAs)', 'one input row of one wave: 9 MFMA')
T = isa('smd_conv_thin.hip')
report(T, 'k_thin_mfma<16, 1, false>', 'k_thin_mfma<16, 1, false>                (round 5, f32 MFMA 16x16x4: the comparison)', 'the whole tile')
