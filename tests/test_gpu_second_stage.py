"""The one-block fp64 second stage (`launch_sum_partials_f64`, csrc/smd_misc.hip) behind the fused masked and the fused feature-metric reconstruction forwards: a
sum in a fixed order (at the large shape more block sums than threads: the strided loop and the waves' order take part), so the losses carry the bit patterns that the two operators' former private second stages gave on the same operands
(tests/golden/second_stage_bits.npz, recorded by tests/golden/make_golden_second_stage.py with the library of the commit before the change)."""
import pytest
import torch

from conftest import load_golden
from second_stage_inputs import feat_inputs, loss_bits, mask_inputs

pytestmark = pytest.mark.gpu


def test_losses_keep_the_recorded_bits():
    if not torch.cuda.is_available(): pytest.skip('no GPU')
    g = load_golden('second_stage_bits')
    m, f = mask_inputs(), feat_inputs()
    for k, v in m.items(): assert torch.equal(v, g[f'in_mask_{k}']), f'mask operand {k} is not the recorded one'
    for k, v in f.items(): assert torch.equal(v, g[f'in_feat_{k}']), f'feat operand {k} is not the recorded one'
    ml, fl = mask_inputs('large'), feat_inputs('large')
    for tag, d in (('mask', ml), ('feat', fl)):
        for k, v in d.items(): assert v.double().sum().item() == float(g[f'chk_{tag}_{k}']), f'large {tag} operand {k} is not the recorded one'
    got = {**loss_bits(m, f), **{f'{k}_large': v for k, v in loss_bits(ml, fl).items()}}
    for k in ('mask_recon', 'feat_recon', 'mask_recon_large', 'feat_recon_large'):
        print(f'{k}: {got[k] & 0xffffffff:#010x} recorded {int(g[k]) & 0xffffffff:#010x}')
        assert got[k] == int(g[k]), f'{k}: the loss moved ({got[k] & 0xffffffff:#010x} against {int(g[k]) & 0xffffffff:#010x})'
