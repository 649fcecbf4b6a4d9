#!/usr/bin/env python3
"""Golden vectors for the flip-and-blend post-process, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and
writer are reused here).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_blend.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/tools/geometry.py:94-129   blend_stereo
  * src/tools/geometry.py:63-76    to_scaled (its disparity output, behind the blend)

tests/golden/blend_stereo.npz (read it with blend_inputs.blend_expected): `chk` the bit checksums of the seeded inputs of every case of blend_inputs.BLEND_CASES
(`blend_case(k)`: l, r = the right disparity already flipped back, g = the incoming gradient); `out` = blend_stereo(l, r), `grad_l`, `grad_r` = autograd's
gradients of sum(out*g), each flattened and concatenated over the cases; `outs`, `grads_l`, `grads_r` the same behind to_scaled(.., min=0.1, max=100)[0] over the
cases of BLEND_SCALED.  The fixture holds data only (checksums + expected outputs); no reference source text is stored."""
import numpy as np
import torch

from make_golden import import_reference, save


def main():
    torch.set_num_threads(1)
    import_reference()
    from src.tools.geometry import blend_stereo, to_scaled
    from blend_inputs import BLEND_CASES, BLEND_RANGE, BLEND_SCALED, blend_case
    from exact_inputs import bit_checksum
    rec = {'meta_min_depth': BLEND_RANGE[0], 'meta_max_depth': float(BLEND_RANGE[1]), 'chk': []}
    flat = {n: [] for n in ('out', 'grad_l', 'grad_r', 'outs', 'grads_l', 'grads_r')}
    for k, shape in enumerate(BLEND_CASES):
        ins = blend_case(k)
        l, r, g = ins['l'], ins['r'], ins['g']
        rec['chk'].append(sum(bit_checksum(t) for t in ins.values()))
        for tag, scaled in (('', False), ('s', True)):
            if scaled and k not in BLEND_SCALED: continue
            ll, rr = l.clone().requires_grad_(True), r.clone().requires_grad_(True)
            out = blend_stereo(ll, rr)
            if scaled: out = to_scaled(out, min=BLEND_RANGE[0], max=BLEND_RANGE[1])[0]
            (out*g).sum().backward()
            for n, t in ((f'out{tag}', out.detach()), (f'grad{tag}_l', ll.grad), (f'grad{tag}_r', rr.grad)): flat[n].append(t.reshape(-1))
        print(f'blend_stereo[{k}] {shape}: out in [{flat["out"][-1].min().item():.4f}, {flat["out"][-1].max().item():.4f}]')
    rec['chk'] = np.array(rec['chk'], dtype=np.int64)
    rec.update({n: torch.cat(v) for n, v in flat.items()})
    save('blend_stereo', rec)


if __name__ == '__main__':
    main()
