#!/usr/bin/env python3
"""tests/golden/second_stage_bits.npz: the float32 loss bit patterns of the fused masked and the fused feature-metric reconstruction forwards on
second_stage_inputs.py's operands, recorded on an MI355X with the library of the commit BEFORE the two operators' private one-block fp64 second stages
were replaced by `launch_sum_partials_f64`.  A sum in a fixed order: the test asserts the same bits.  To be run with that older library only
(SMD_HOTPATH_LIB=<its libsmd_hotpath.so>), never with the code under test.

    python tests/golden/make_golden_second_stage.py [--out tests/golden/second_stage_bits.npz]

Keys: `mask_recon`, `feat_recon` (int32: the bits at the small shape), `in_mask_<name>` / `in_feat_<name>` (its operands, float32); `mask_recon_large`,
`feat_recon_large` (the bits at the large shape, whose operands are regenerated from their seed: the fp64 sum of each is kept, `chk_<...>`).  Data only."""
import argparse
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1])); sys.path.insert(0, str(HERE))
from second_stage_inputs import feat_inputs, loss_bits, mask_inputs      # noqa: E402

if __name__ == '__main__':
    ap = argparse.ArgumentParser(); ap.add_argument('--out', default=str(HERE/'second_stage_bits.npz'))
    out = Path(ap.parse_args().out)
    m, f = mask_inputs(), feat_inputs()
    bits = loss_bits(m, f)
    ml, fl = mask_inputs('large'), feat_inputs('large')
    bits.update({f'{k}_large': v for k, v in loss_bits(ml, fl).items()})
    chk = {f'chk_{tag}_{k}': np.float64(v.double().sum().item()) for tag, d in (('mask', ml), ('feat', fl)) for k, v in d.items()}
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **{k: np.int32(v) for k, v in bits.items()}, **chk, **{f'in_mask_{k}': v.numpy() for k, v in m.items()}, **{f'in_feat_{k}': v.numpy() for k, v in f.items()})
    print({k: hex(v & 0xffffffff) for k, v in bits.items()}, '->', out)
