#!/usr/bin/env python3
"""tests/golden/conv_skeleton_rules.npz and conv_skeleton_calls.json: what the routed convolutions decided and launched at the commit BEFORE their three
rule tables became one and their three operators one skeleton (conv_skeleton_cases.py: the grid, the cases, the recorder).  To be run at that commit only,
never with the code under test.

    python tests/golden/make_golden_conv_skeleton.py rules      # no GPU: `static_rule` on every grid point, the booleans packed
    python tests/golden/make_golden_conv_skeleton.py calls      # on an MI355X: per case, route and gradient subset the launches in order; under 'mfma' the
                                                                # SHA-256 of the bits of the output and of the gradients the kernels write

Data only."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1])); sys.path.insert(0, str(HERE))
import conv_skeleton_cases as K      # noqa: E402


def rules(out):
    from slowtv_monodepth_amd import conv_routing as R
    pts = K.grid()
    served = np.array([R.static_rule(*p) for p in pts], dtype=bool)
    for op in K.NO_SUCH_OP:
        try: R.static_rule(op, 12, 64, 128, 48, 160)
        except KeyError: continue
        raise SystemExit(f'{op}: expected a KeyError')
    np.savez_compressed(out/'conv_skeleton_rules.npz', n=np.int64(len(pts)), served=np.packbits(served))
    print(f'{len(pts)} grid points, {int(served.sum())} served ->', out/'conv_skeleton_rules.npz')


def calls(out):
    from slowtv_monodepth_amd import conv_routing as R, functional as F
    names, seq, bits = {}, {}, {}
    for case in K.CASES:
        for mode in K.MODES:
            for subset in K.SUBSETS:
                log, res = K.record_case(F, R, case, mode, subset)
                seq.setdefault(case.name, {}).setdefault(mode, {})[subset] = [names.setdefault(c, len(names)) for c in log]
                if mode == 'mfma':
                    for k in case.bits:
                        if res[k] is None: continue
                        d = K.digest(res[k])
                        if bits.setdefault(case.name, {}).setdefault(k, d) != d: raise SystemExit(f'{case.name}: {k} depends on who asks for a gradient')
        print(case.name, {m: [len(v) for v in s.values()] for m, s in seq[case.name].items()}, flush=True)
    (out/'conv_skeleton_calls.json').write_text(json.dumps(dict(launches=list(names), sequences=seq, bits=bits), indent=None, separators=(',', ':')) + '\n')
    print(len(names), 'distinct launches ->', out/'conv_skeleton_calls.json')


if __name__ == '__main__':
    ap = argparse.ArgumentParser(); ap.add_argument('what', choices=['rules', 'calls']); ap.add_argument('--out', default=str(HERE))
    a = ap.parse_args()
    Path(a.out).mkdir(parents=True, exist_ok=True)
    {'rules': rules, 'calls': calls}[a.what](Path(a.out))
