#!/usr/bin/env python
"""The table of profiles/head_merge_resources.txt: every k_head_* / k_headn_* instantiation of the commit before the output heads were merged next to its
successor in this tree.  No GPU: both csrc directories are cross-compiled for gfx950 with the library's flags plus `--cuda-device-only -S`.

    python scripts/dev/head_merge_resources.py PARENT_CSRC [THIS_CSRC]        (PARENT_CSRC: slowtv_monodepth_amd/csrc of a checkout of the parent commit)

Registers, scratch [bytes/lane] and LDS [bytes/block] are the code object's metadata, occupancy [waves/SIMD] the compiler's comment; the rest is counted in the
assembly text: vld/B and vst/B = vector memory loads / stores and the bytes per lane they move, vmw = waits that name vmcnt (static, all paths), insts = instructions.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = '-O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-arch=gfx950 --cuda-device-only -S'.split()
BYTES = {'ubyte': 1, 'sbyte': 1, 'ushort': 2, 'sshort': 2, 'short': 2, 'byte': 1, 'dword': 4, 'dwordx2': 8, 'dwordx3': 12, 'dwordx4': 16}


def kernels(csrc, files, keep=lambda sym: 'k_head' in sym):
    """{demangled kernel: (vgpr, sgpr, scratch, lds, occupancy, 'loads/bytes', 'stores/bytes', vmcnt waits, instructions, barriers)} of the kernels of
    `files` whose mangled name `keep` accepts."""
    out = {}
    for f in files:
        if not os.path.exists(os.path.join(csrc, f)):
            continue
        with tempfile.NamedTemporaryFile(suffix='.s') as t:
            subprocess.check_call([HIPCC] + FLAGS + [f, '-o', t.name], cwd=csrc)
            text = open(t.name).read()
        meta = {m.group(1): dict(re.findall(r'\.(\w+):\s+(\d+)', m.group(0)))
                for m in re.finditer(r'- \.agpr_count:.*?\.name:\s+(\S+).*?\.wavefront_size', text, re.S)}
        for m in re.finditer(r'^(_ZN3smd\w+):[^\n]*\n(.*?)^\.Lfunc_end', text, re.S | re.M):
            sym, body = m.group(1), m.group(2)
            if sym not in meta or not keep(sym):
                continue
            name = subprocess.check_output(['c++filt', sym], text=True).strip()
            name = re.sub(r'^void smd::|\(.*$', '', name).replace('__hip_bfloat16', 'bf16')
            insts = [l.split()[0] for l in body.split('\n') if re.match(r'^\s+[a-z]\w+', l) and not l.lstrip().startswith(('.', ';'))]
            ld = [i for i in insts if re.match(r'(global|flat|buffer)_load', i)]
            st = [i for i in insts if re.match(r'(global|flat|buffer)_store', i)]
            nb = lambda v: sum(next(BYTES[t] for t in i.split('_')[2:] if t in BYTES) for i in v)   # (global_load_short_d16_hi: the size is not last)
            occ = re.search(r'; Occupancy: (\d+)', text[m.end():])
            k = meta[sym]
            out[name] = (int(k['vgpr_count']), int(k['sgpr_count']), int(k['private_segment_fixed_size']), int(k['group_segment_fixed_size']), int(occ.group(1)),
                         '%d/%d' % (len(ld), nb(ld)), '%d/%d' % (len(st), nb(st)),
                         sum(1 for l in body.split('\n') if 's_waitcnt' in l and 'vmcnt' in l), len(insts), insts.count('s_barrier'))
    return out


def successor(name):
    name = name.replace('k_headn_', 'k_head_')
    m = re.match(r'(k_head_\w+)<(.*)>$', name)
    if not m:
        return name
    args = m.group(2).split(', ')
    want = 5 if m.group(1) == 'k_head_fwd' else 3
    return '%s<%s>' % (m.group(1), ', '.join((['1'] if len(args) < want else []) + args))


def main():
    parent_dir = sys.argv[1]
    this_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), '..', '..', 'slowtv_monodepth_amd', 'csrc')
    parent = kernels(parent_dir, ['smd_conv_head.hip', 'smd_conv_headn.hip'])
    this = kernels(this_dir, ['smd_conv_head.hip', 'smd_conv_headn.hip'])
    fmt = '%-44s %5d %4d %4d %5d %3d  %-8s %-6s %4d %5d'
    head = '%-44s %5s %4s %4s %5s %3s  %-8s %-6s %4s %5s' % ('%s', 'vgpr', 'sgpr', 'scr', 'lds', 'occ', 'vld/B', 'vst/B', 'vmw', 'insts')
    print('kernels: parent %d, this tree %d' % (len(parent), len(this)))
    print(head % 'parent kernel', ' |', head % 'successor')
    order = lambda n: (not n.startswith('k_head_fwd') and not n.startswith('k_headn_fwd'), 'data' not in n and 'fwd' not in n, 'finalize' in n, 'headn' in n, n)
    for name in sorted(parent, key=order):
        p, s = parent[name][:9], this[successor(name)][:9]
        print(fmt % ((name,) + p), ' |', fmt % ((successor(name),) + s))
        if p[5].split('/')[0] != s[5].split('/')[0] or p[6].split('/')[0] != s[6].split('/')[0]:
            print('    ^ load/store count differs')
        if abs(p[0] - s[0]) > 4:
            print('    ^ VGPRs move by more than 4')
        if s[4] < p[4]:
            print('    ^ occupancy drops')
        if s[2]:
            print('    ^ scratch')


if __name__ == '__main__':
    main()
