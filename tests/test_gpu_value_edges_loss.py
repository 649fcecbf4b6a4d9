"""The loss-path value-edge table (value_edges_loss.py) on the kernels, as test_gpu_value_edges.py runs the first table: every case against its fp64 reference at
the operator's own bound, finite wherever the reference is (an identical non-finite pattern where it is not), and bit-equal between two runs; the outputs
accumulated with float atomics (`LOOSE`: `view_synth`'s `g_input`, as test_gpu_hostile_memory.py notes) are held to their bound between the runs instead."""
import pytest
import torch

import value_edges as V
import value_edges_loss as L
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


@pytest.mark.parametrize('c', L.CASES, ids=[c.name for c in L.CASES])
def test_value_edges_loss(F, c):
    ops = c.operands(torch.Generator().manual_seed(len(c.name)*7919 + 17))
    ref = {k: v.detach() for k, v in c.ref({k: v.clone() for k, v in ops.items()}, V.F64).items() if v is not None}
    yard = V.yardstick(c, ops)      # the oracle's fp32 on the CPU, for the bounds that are measured against it (never the kernel's own output)
    A, B = _run(F, c, ops), _run(F, c, ops)
    for k, e in V.errors(c, A, ref, ops, yard).items():
        bound = c.tol.get(k, c.tol.get('*'))
        what = f'{bound}, oracle fp32 {V.excess(yard[k], ref[k], ("rel", 1.0), c.split.get(k)):.2e} of the maximum' if bound[0] in V.YARD_KINDS else bound
        print(f'{c.name}: {k}: {e:.3g} of its bound {what}')
    for k, v in A.items():
        if bool(ref[k].isfinite().all()): assert_finite(v, f'{c.name}: {k}')
        else: assert V.same_pattern(v.double(), ref[k].double().reshape(v.shape)), f'{c.name}: {k}: the non-finite elements are not where the reference has them'
    V.judge(c, A, ref, ops, yard)
    assert set(A) == set(B)
    for k, v in A.items():
        if k in L.LOOSE.get(c.name, ()): assert V.excess(B[k], v, c.tol.get(k, c.tol.get('*')), c.split.get(k)) <= 1.0, f'{c.name}: {k} differs between two runs by more than its bound'
        else:
            bits = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[v.element_size()]      # (the bit patterns: NaNs and signed zeros included)
            assert torch.equal(v.view(bits), B[k].view(bits)), f'{c.name}: {k} differs between two runs'


@pytest.mark.parametrize('w_ssim,C', L.SSIM_UNRESOLVED)
@pytest.mark.parametrize('h,w', L.PHOTO_SHAPES)
def test_ssim_at_contrast_2_12(F, w_ssim, C, h, w):
    """SSIM on near-1 images whose contrast is 2^-12: the variance 9 sxx - sx^2 is 1e-8 of its two terms, below one fp32 rounding of either, so the oracle's fp32
    is wrong by the error map's whole size and no fp32 evaluation can be held to the fp64 one (value_edges_loss._photo_tol).  What needs no yardstick still holds:
    finite, each channel's clamped SSIM error in [0, 1] (so the error map lies between its exact L1 part and that plus weight_ssim), and the bits of a second run."""
    gen = torch.Generator().manual_seed(h*100 + w + C)
    pred, target = (t.cuda() for t in L.PHOTO_VALUES['contrast_2^-12']((2, C, h, w), gen))
    ge = V._pattern((2, 1, h, w)).cuda()

    def run():
        p = pred.clone().requires_grad_(True)
        err = F.photo_error(p, target, 'ssim', w_ssim); err.backward(ge)
        torch.cuda.synchronize()
        return err.detach().cpu(), p.grad.cpu()
    (err, g), (err2, g2) = run(), run()
    assert_finite(err, 'err'); assert_finite(g, 'g_pred')
    l1 = (1 - w_ssim)*(pred - target).abs().mean(1, keepdim=True).cpu().double()      # (exact: differences of 0 or 2^-12)
    assert bool((err.double() >= l1*(1 - 1e-6)).all()) and bool((err.double() <= (w_ssim + l1)*(1 + 1e-6)).all()), 'the SSIM part leaves [0, weight_ssim]'
    assert torch.equal(err.view(torch.int32), err2.view(torch.int32)) and torch.equal(g.view(torch.int32), g2.view(torch.int32)), 'two runs differ'
