#!/usr/bin/env python3
"""Per-kernel comparison of two trees' generated code (the method of profiles/experiments_prune_isa.txt and profiles/plain_stages_isa.txt).  No GPU needed.

    for f in slowtv_monodepth_amd/csrc/*.hip:      # in each tree, the Makefile's flags
      hipcc -O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-arch=gfx950 -Wall -Wno-unused-function --cuda-device-only -S $f -o <dir>/$(basename $f .hip).s
    python scripts/dev/isa_compare.py <parent dir> <new dir> [--full name-substring ...]

Per file: identical text after stripping .file / .ident lines and the per-translation-unit __hip_cuid_<hash> symbol, or per kernel (its text from its label to
.Lfunc_end with the compiler's per-function label numbers normalised, its .amdhsa_ block, its metadata entry): gone, new, identical, or the number of changed
lines, whether the multiset of instruction mnemonics is the same (a reordering / renumbering) and the metadata fields that moved.  --full prints the whole
unified diff of the kernels whose name contains one of the substrings."""
import argparse
import collections
import difflib
import re
import sys
from pathlib import Path

META = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size', '.vgpr_spill_count', '.sgpr_spill_count', '.kernarg_segment_size')


def strip(text):
    out = [ln for ln in text.splitlines() if not re.match(r'\s*\.(file|ident)\b', ln) and '__hip_cuid_' not in ln]
    return out


def kernels(lines):
    """-> {name: (body lines, amdhsa lines, metadata dict)}"""
    names = [m.group(1) for ln in lines if (m := re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln))]
    res = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(f'{name}:'))
        end = next(i for i in range(start, len(lines)) if re.match(r'\.Lfunc_end\d+:', lines[i]))
        h0 = lines.index(f'\t.amdhsa_kernel {name}')
        body = [re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', ln)) for ln in lines[start + 1:min(end, h0)]]
        body = [ln for ln in body if ln.strip() and not re.match(r'\s+\.(p2align|section|text|rodata)', ln)]
        h1 = next(i for i in range(h0, len(lines)) if lines[i].strip() == '.end_amdhsa_kernel')
        m0 = next(i for i, ln in enumerate(lines) if re.match(r'\s*\.name:\s+' + re.escape(name) + r'\s*$', ln))
        meta = {}
        i = next(i for i in range(m0, -1, -1) if re.match(r'  - \.', lines[i]))      # a kernel's entry opens at indent 2; the entries of its .args at indent 6
        for j in range(i, len(lines)):
            if j > i and (re.match(r'  - \.', lines[j]) or not lines[j].startswith(' ')): break
            if (m := re.match(r'\s*(?:- )?(\.\w+):\s+(\S+)\s*$', lines[j])) and m.group(1) in META: meta[m.group(1)] = m.group(2)
        res[name] = (body, lines[h0:h1], meta)
    return res


def mnemonics(body): return collections.Counter(ln.split()[0] for ln in body if not ln.strip().endswith(':'))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('old'); ap.add_argument('new'); ap.add_argument('--full', nargs='*', default=[])
    a = ap.parse_args()
    total = [0, 0]
    for f in sorted(Path(a.old).glob('*.s')):
        g = Path(a.new)/f.name
        lo, ln_ = strip(f.read_text()), strip(g.read_text())
        ko, kn = kernels(lo), kernels(ln_)
        total[0] += len(ko); total[1] += len(kn)
        if lo == ln_: print(f'{f.name}: identical text ({len(ko)} kernels)'); continue
        same = [k for k in ko if k in kn and ko[k] == kn[k]]
        diff = [k for k in ko if k in kn and ko[k] != kn[k]]
        print(f'{f.name}: {len(ko)} kernels before, {len(kn)} after; {len(ko.keys() - kn.keys())} gone, {len(kn.keys() - ko.keys())} new, {len(same)} identical (text, .amdhsa block, metadata), {len(diff)} differ')
        for k in ko.keys() - kn.keys(): print(f'    gone: {k}')
        for k in kn.keys() - ko.keys(): print(f'    new:  {k}  {kn[k][2]}')
        for k in diff:
            d = [x for x in difflib.unified_diff(ko[k][0], kn[k][0], lineterm='', n=2)][2:]
            changed = sum(1 for x in d if x[0] in '+-')
            mo, mn = mnemonics(ko[k][0]), mnemonics(kn[k][0])
            meta = {m: (ko[k][2].get(m), kn[k][2].get(m)) for m in META if ko[k][2].get(m) != kn[k][2].get(m)}
            delta = {m: mn[m] - mo[m] for m in mo.keys() | mn.keys() if mn[m] != mo[m]}
            print(f'    differs: {k}: {len(ko[k][0])} -> {len(kn[k][0])} instructions, {changed} changed lines; mnemonic counts {"equal" if not delta else delta}; metadata {"equal" if not meta else meta}'
                  + ('' if ko[k][1] == kn[k][1] else '; .amdhsa block differs'))
            if any(s in k for s in a.full):
                for x in d: print('        ' + x)
    print(f'Kernel counts: {total[0]} before, {total[1]} after')


if __name__ == '__main__':
    sys.exit(main())
