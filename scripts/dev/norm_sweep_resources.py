#!/usr/bin/env python
"""The table of profiles/norm_sweep_resources.txt: every kernel of the files that the shared channel sweep (smd_norm_dev.h) and the block-sum family
(smd_common.h) touched, the parent commit next to this tree.  No GPU: both csrc directories are cross-compiled as head_merge_resources.py does.

    python scripts/dev/norm_sweep_resources.py PARENT_CSRC [THIS_CSRC]        (PARENT_CSRC: slowtv_monodepth_amd/csrc of a checkout of the parent commit)

Columns as in head_merge_resources.py, plus bar = s_barrier instructions.  A kernel whose row is identical in both trees is printed once.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from head_merge_resources import kernels  # noqa: E402

FILES = ['smd_norm.hip', 'smd_layernorm.hip', 'smd_smooth.hip', 'smd_masks.hip', 'smd_attention.hip', 'smd_unfused.hip', 'smd_dwconv.hip', 'smd_misc.hip',
         'smd_decoder.hip']


def main():
    parent_dir = sys.argv[1]
    this_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), '..', '..', 'slowtv_monodepth_amd', 'csrc')
    fmt = '%-62s %4d %4d %3d %5d %3d  %-7s %-6s %3d %5d %3d'
    print('%-62s %4s %4s %3s %5s %3s  %-7s %-6s %3s %5s %3s' % ('kernel', 'vgpr', 'sgpr', 'scr', 'lds', 'occ', 'vld/B', 'vst/B', 'vmw', 'insts', 'bar'))
    bad = 0
    for f in FILES:
        parent, this = kernels(parent_dir, [f], keep=lambda s: True), kernels(this_dir, [f], keep=lambda s: True)
        same = sum(1 for n in parent if this.get(n) == parent[n])
        print('\n%s: kernels parent %d, this tree %d; %d identical in every column' % (f, len(parent), len(this), same))
        bad += len(this) > len(parent)
        for n in sorted(set(parent) | set(this)):
            p, s = parent.get(n), this.get(n)
            if p == s:
                print(fmt % ((n,) + p))
                continue
            if p: print(fmt % ((n + '  [parent]',) + p))
            if s: print(fmt % ((n + '  [this]',) + s))
            if p and s:
                notes = [('scratch appears', s[2] > 0 and p[2] == 0), ('occupancy drops', s[4] < p[4]), ('gains an s_barrier', s[9] > p[9])]
                for text, hit in notes:
                    if hit:
                        print('    ^ ' + text)
                        bad += 1
    print('\nconditions (no new scratch, no occupancy drop, no added s_barrier, no file with more kernels): %s' % ('all hold' if not bad else '%d VIOLATED' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
