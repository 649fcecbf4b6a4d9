"""The value-edge table (value_edges.py) on the kernels: every case against its fp64 reference at the operator's own bound, finite wherever the reference is
(an identical non-finite pattern where it is not), and bit-equal between two runs."""
import pytest
import torch

import value_edges as V
from hostile_memory import assert_finite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def _run(F, c, ops):
    out = c.run(F, {k: v.cuda() for k, v in ops.items()})
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items() if v is not None}


@pytest.mark.parametrize('c', V.CASES, ids=[c.name for c in V.CASES])
def test_value_edges(F, c):
    ops = c.operands(torch.Generator().manual_seed(len(c.name)*7919 + 17))
    ref = {k: v.detach() for k, v in c.ref({k: v.clone() for k, v in ops.items()}, V.F64).items() if v is not None}
    yard = V.yardstick(c, ops)      # ATen's fp32 sequence on the CPU, for the bounds that are measured against it (never the kernel's own output)
    A, B = _run(F, c, ops), _run(F, c, ops)
    for k, e in V.errors(c, A, ref, ops, yard).items():
        bound = c.tol.get(k, c.tol.get('*'))
        what = f'{bound[0]} bound' if bound[0] == 'elem' else bound
        if bound[0] in V.YARD_KINDS: what = f'{bound}, torch fp32 {V.excess(yard[k], ref[k], ("rel", 1.0)):.2e} of the maximum'
        print(f'{c.name}: {k}: {e:.3g} of its bound {what}')
    for k, v in A.items():
        if bool(ref[k].isfinite().all()): assert_finite(v, f'{c.name}: {k}')
        else: assert V.same_pattern(v.double(), ref[k].double().reshape(v.shape)), f'{c.name}: {k}: the non-finite elements are not where the reference has them'
    V.judge(c, A, ref, ops, yard)
    assert set(A) == set(B)
    for k, v in A.items():
        bits = torch.int32 if v.dtype == torch.float32 else torch.int16      # (the bit patterns: NaNs and signed zeros included)
        assert torch.equal(v.view(bits), B[k].view(bits)), f'{c.name}: {k} differs between two runs'
