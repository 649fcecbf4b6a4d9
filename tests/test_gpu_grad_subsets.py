"""Every operator's backward with frozen operands, absent optional operands and awkward incoming gradients (the table and the checker: grad_subsets.py).

    Axis A  each subset of the differentiable operands asks for a gradient, in hostile memory (hostile_memory.py, shift 0, guards checked): forward outputs and
            every requested gradient bit-equal to the full run's, nothing for the operands left out, everything finite; the full run itself (outputs and EVERY
            gradient, the regression loss's g_target and the K_inv gradients included) held to the fp64 / oracle reference at the family's bound
    Axis B  each optional operand absent once, with the full set of gradients, held to the reference (present: Axis A's full run)
    Axis C  the incoming gradient as a stride-0 expanded tensor, as a channels-last-strided view, and with one of several outputs unused: every gradient
            bit-equal to the contiguous run with the same values

The exceptions to bit-equality are the `loose` gradients of the table (view_synth's g_input), held to the reference instead.  Pinned as the hostile-memory
module pins them: the routed convolutions to the MFMA kernels, the fused backward's row loop (`SMD_BWD_SKIP=0`).  Observed figures: profiles/grad_subsets.txt."""
import pytest
import torch

import grad_subsets as G
from conftest import parity_note
from hostile_memory import Arena, hostile

pytestmark = pytest.mark.gpu
IDS = [e.name for e in G.TABLE]


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


@pytest.fixture(autouse=True)
def _one_row_loop(monkeypatch): monkeypatch.setenv('SMD_BWD_SKIP', '0')


_shared = {}      # (entry, absent) -> (operands, reference, bounds): computed once, never modified


def _case(e, absent=frozenset()):
    key = (e.name, absent)
    if key not in _shared:
        o = e.operands(torch.Generator().manual_seed(len(e.name)*7919 + 31), absent)
        ref = G.run_reference(e, o)
        _shared[key] = (o, ref, G.bounds_of(e, o, ref, G.run_reference(e, o, torch.float32) if e.yard else None))
    return _shared[key]


def _friendly(e, F, o, subset, **kw):
    out = G.run_entry(e, F, {k: v.cuda() for k, v in o.items()}, subset, **kw)
    torch.cuda.synchronize()
    return out


def _hostile(e, F, o, subset):
    from slowtv_monodepth_amd import class_ops
    class_ops._mean_ws.clear()       # `scale_mean`'s persistent workspace: a fresh one (test_gpu_hostile_memory.py, module text)
    arena = Arena()
    ops = {k: arena.guarded(v.cuda()) for k, v in o.items()}
    with hostile(arena): out = G.run_entry(e, F, ops, subset)
    arena.check()
    return out


@pytest.mark.parametrize('e', G.TABLE, ids=IDS)
def test_each_gradient_subset_equals_the_full_backward(F, e):
    o, ref, bounds = _case(e)
    diff = [d for d in e.diff if d in o]
    full, figures = _friendly(e, F, o, frozenset(diff)), {}
    G.check_full(f'{e.name} (every operand asks)', full, ref, bounds, e.views, figures)
    subsets = G.subsets_of(diff, e.groups)
    hold = lambda what, k, g: G.check_full(f'{e.name}: {what}', {k: g}, {k: ref[k]}, bounds, e.views)
    G.check_subsets(lambda s: _hostile(e, F, o, s), full, subsets, diff, name=e.name, loose=e.loose, hold=hold)
    fresh = {k: f'{figures[k]:.2e}' for k in ('g_target', 'g_K_inv') if k in figures}
    parity_note(f'grad_subsets {e.name}: {len(subsets)} subsets, held to a bound instead of bit-equality: {sorted(e.loose) or "none"}' + (f', measured against the reference: {fresh}' if fresh else ''))


OPTIONAL = [(e, a) for e in G.TABLE for a in e.optional]


@pytest.mark.parametrize('e,absent', OPTIONAL, ids=[f'{e.name}-no_{a}' for e, a in OPTIONAL])
def test_optional_operand_absent(F, e, absent):
    o, ref, bounds = _case(e, frozenset([absent]))
    full, figures = _hostile(e, F, o, frozenset(e.diff)), {}
    G.check_full(f'{e.name} without {absent}', full, ref, bounds, e.views, figures)
    if 'g_K' in figures: parity_note(f'grad_subsets {e.name} without {absent}: g_K {figures["g_K"]:.2e} against the reference')


def _same_bits(e, what, got, want, diff):
    fails = []
    for d in diff:
        k = f'g_{d}'
        if k in e.loose: continue
        if got[k] is None or want[k] is None or not torch.equal(got[k], want[k]): fails.append(f'gradient of operand {d}')
    assert not fails, f'{e.name}, {what}: {fails} differ from the contiguous run with the same values'


@pytest.mark.parametrize('e', G.TABLE, ids=IDS)
def test_incoming_gradient_layouts(F, e):
    o, _, _ = _case(e)
    diff = [d for d in e.diff if d in o]
    full = frozenset(diff)
    probe = _friendly(e, F, o, full)
    ones = {n: torch.ones_like(probe[n]) for n in e.outputs}
    want = _friendly(e, F, o, full, gy=ones)
    got = _friendly(e, F, o, full, gy={n: torch.ones((), device='cuda').expand_as(probe[n]) for n in e.outputs})
    _same_bits(e, 'stride-0 expanded gradient', got, want, diff)
    strided = {n: o[f'gy_{n}'].cuda().contiguous(memory_format=torch.channels_last) for n in e.outputs if probe[n].ndim == 4}
    if strided:
        assert all(not g.is_contiguous() or 1 in g.shape for g in strided.values())
        _same_bits(e, 'channels-last-strided gradient', _friendly(e, F, o, full, gy=strided), probe, diff)
    if len(e.outputs) > 1:
        for n in e.outputs:      # the other outputs unused, against an explicit zero gradient for them
            others = [m for m in e.outputs if m != n]
            want = _friendly(e, F, o, full, gy={m: torch.zeros_like(probe[m]) for m in others})
            _same_bits(e, f'{n} only', _friendly(e, F, o, full, unused=others), want, diff)


def test_outputs_that_carry_no_gradient(F):
    """`se_gate(return_gate=True)`: the gate is detached, the gradients are those of `se_gate` without it.  `disp_to_depth(want_disp_up=True)`: `disp_up` is not
    differentiable, the gradients are those of the call without it."""
    e = G.BY_NAME['se_gate(2, 12, 5, 7)']
    o, _, _ = _case(e)
    full = frozenset(e.diff)
    with_gate = _friendly(e, F, o, full)
    assert not with_gate['gate'].requires_grad
    L = {k: v.cuda().requires_grad_(k in full) for k, v in o.items() if v.is_floating_point()}
    F.se_gate(L['x'], L['w1'], L['b1'], L['w2'], L['b2']).backward(L['gy_y'])
    for d in e.diff: assert torch.equal(L[d].grad, with_gate[f'g_{d}']), d
    e = G.BY_NAME['disp_to_depth']
    o, _, _ = _case(e)
    both = _friendly(e, F, o, frozenset(e.diff))
    assert not both['disp_up'].requires_grad
    L = {k: v.cuda().requires_grad_(k in e.diff) for k, v in o.items()}
    dep, none = F.disp_to_depth([L[k] for k in G.DS], (G.RH, G.RW), 0.1, 100)
    assert none is None
    dep.backward(L['gy_depth_up'])
    for d in e.diff: assert torch.equal(L[d].grad, both[f'g_{d}']), d
