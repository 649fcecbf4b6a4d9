"""grad_subsets.py on the CPU: the table names every `torch.autograd.Function` of the package, and the checker rejects what it claims to reject.  The wrong
Functions below are wrong in VALUE only (a lost term, an unfilled scratch tensor, an output that depends on who asks); nothing is made to fault."""
import pytest
import torch

import grad_subsets as G
from hostile_memory import Arena, hostile


def test_every_function_of_the_package_is_in_the_table():
    fns = G.functions_of_the_package()
    assert len(fns) >= 30, sorted(fns)
    in_table = {e.fn.__name__ for e in G.TABLE}
    missing = [n for n in sorted(fns) if n not in in_table]
    assert not missing, f'no entry in grad_subsets.TABLE for {missing}: add the operands, the reference and the bounds of the new Function'
    for e in G.TABLE: assert fns.get(e.fn.__name__) is e.fn, f'{e.name}: {e.fn.__name__} is not a Function of a *_ops.py module'
    for n, why in G.EXEMPT.items():
        assert n in fns and why and n in in_table, f'{n}: exempt from the subset axis, but it must stay in the table for the gradient-layout axis'
        for e in G.TABLE:
            if e.fn.__name__ == n: assert len(e.diff) == 1 and not e.optional, f'{e.name}: only a Function with one differentiable operand and no optional one may be exempt'


def test_removing_an_entry_is_noticed(monkeypatch):
    victim = G.BY_NAME['disp_smooth_fused']
    monkeypatch.setattr(G, 'TABLE', [e for e in G.TABLE if e is not victim])
    with pytest.raises(AssertionError, match='_DispSmooth'): test_every_function_of_the_package_is_in_the_table()


def test_table_entries_are_well_formed():
    from slowtv_monodepth_amd import functional
    for e in G.TABLE:
        assert hasattr(functional, e.wrapper), e.name
        o = e.operands(torch.Generator().manual_seed(1))
        assert all(d in o for d in e.diff) and all(f'gy_{n}' in o for n in e.outputs), e.name
        assert all(g <= set(e.diff) for g in e.groups), e.name
        for k, why in e.loose.items(): assert k[2:] in e.diff and 'k_' in why, f'{e.name}: an exception to bit-equality names the kernel and the reason'
        subs = G.subsets_of(e.diff, e.groups)
        assert len(set(subs)) == len(subs) and frozenset(e.diff) in subs and all(frozenset([d]) in subs for d in e.diff), e.name
        if len(e.diff) <= 3: assert len(subs) == 2**len(e.diff) - 1
        else: assert all(frozenset(e.diff) - {d} in subs for d in e.diff)
    assert [k for e in G.TABLE for k in e.loose] == ['g_inp'], 'view_synth\'s g_input is the one exception to bit-equality'


def test_references_run_in_fp64_with_and_without_the_optional_operands():
    for e in G.TABLE:
        for absent in [frozenset()] + [frozenset([a]) for a in e.optional]:
            o = e.operands(torch.Generator().manual_seed(3), absent)
            r = G.run_reference(e, o)
            for k, v in r.items(): assert v is not None and (not v.is_floating_point() or (v.dtype == torch.float64 and torch.isfinite(v).all())), (e.name, sorted(absent), k)
            assert all(f'g_{d}' in r for d in e.diff if d in o), e.name


# ---- small Functions, y = x*w + b.sum(): one correct, three wrong ---------------------------------------------------------------------------------------------------
class _Good(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w): ctx.save_for_backward(x, w); return x*w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g_x = torch.empty_like(x); g_x.copy_(g*w)
        g_w = None
        if ctx.needs_input_grad[1]: g_w = torch.empty_like(w); g_w.copy_(g*x)
        return (g_x if ctx.needs_input_grad[0] else None), g_w


class _LosesATerm(_Good):
    """g_x = g*w + g: the second term is added only inside the branch that also writes the weight gradient."""
    @staticmethod
    def forward(ctx, x, w): ctx.save_for_backward(x, w); return x*w + x

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g_x = g*w
        if ctx.needs_input_grad[1]: g_x = g_x + g
        return g_x, (g*x if ctx.needs_input_grad[1] else None)


class _UnfilledScratch(_Good):
    """Returns the weight gradient from an `empty` tensor it fills only when x asks too."""
    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g_w = torch.empty_like(w)
        if ctx.needs_input_grad[0]: g_w.copy_(g*x)
        return (g*w if ctx.needs_input_grad[0] else None), g_w


class _ForwardDepends(_Good):
    @staticmethod
    def forward(ctx, x, w): ctx.save_for_backward(x, w); return x*w*(1 + 1e-6) if ctx.needs_input_grad[1] else x*w


def _check(fn):
    gen = torch.Generator().manual_seed(0)
    ops = dict(x=torch.randn(4, 5, generator=gen), w=torch.randn(4, 5, generator=gen), gy=torch.randn(4, 5, generator=gen))

    def run(subset):
        arena = Arena()
        o = {k: arena.guarded(v) for k, v in ops.items()}
        L = {k: o[k].requires_grad_(True) for k in ('x', 'w') if k in subset}
        with hostile(arena, device_types=('cpu',)):
            y = fn.apply(L.get('x', o['x']), L.get('w', o['w'])); y.backward(o['gy'])
        arena.check()
        return dict(y=y.detach(), g_x=L['x'].grad if 'x' in L else None, g_w=L['w'].grad if 'w' in L else None)
    full = run(frozenset(['x', 'w']))
    G.check_subsets(run, full, G.subsets_of(['x', 'w']), ['x', 'w'], name=fn.__name__)


def test_checker_passes_a_correct_function(): _check(_Good)


@pytest.mark.parametrize('fn,message', [(_LosesATerm, r'gradient of operand x \(subset \{x\}\) differs from the full backward'),
                                        (_UnfilledScratch, r'gradient of operand w \(subset \{w\}\): .* not finite'),
                                        (_ForwardDepends, r'output y \(subset \{x\}\) differs from the full backward')], ids=lambda v: getattr(v, '__name__', None))
def test_checker_rejects_a_wrong_function(fn, message):
    with pytest.raises(AssertionError, match=message): _check(fn)


def test_checker_rejects_a_gradient_nobody_asked_for_and_a_missing_one():
    full = dict(y=torch.ones(2), g_x=torch.ones(2), g_w=torch.ones(2))
    with pytest.raises(AssertionError, match=r'operand w got a gradient nobody asked for \(subset \{x\}\)'):
        G.check_subsets(lambda s: dict(full), full, [frozenset(['x'])], ['x', 'w'])
    with pytest.raises(AssertionError, match=r'operand x: no gradient although asked for \(subset \{x\}\)'):
        G.check_subsets(lambda s: dict(y=full['y'], g_x=None, g_w=None), full, [frozenset(['x'])], ['x', 'w'])


def test_full_run_is_held_to_the_reference():
    ref = dict(y=torch.ones(3, dtype=torch.float64), g_x=torch.full((3,), 2.0, dtype=torch.float64))
    G.check_full('ok', dict(y=torch.ones(3), g_x=torch.full((3,), 2.0)), ref, {'y': G.EQUAL, 'g_x': G.TOL_CONV_F32})
    with pytest.raises(AssertionError, match='g_x: .* against the reference'):
        G.check_full('negated', dict(y=torch.ones(3), g_x=torch.full((3,), -2.0)), ref, {'y': G.EQUAL, 'g_x': G.TOL_CONV_F32})
