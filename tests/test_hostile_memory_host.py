"""The hostile-memory harness (hostile_memory.py) on the CPU: it must catch what it claims to catch.  Small pure-torch `autograd.Function`s on CPU tensors
that are wrong on purpose - nothing here touches a GPU and nothing is made to fault: every "out-of-bounds" access stays inside the arena's own buffer - and a
correct one that must pass; the patch's pass-through rules; and the completeness of the GPU module's case table."""
import pytest
import torch

import hostile_memory as HM
from hostile_memory import GUARD, Arena, assert_finite, first_nan, hostile


def _run(fn, x, g, shift=0):
    """`fn` and its backward in hostile memory on the CPU -> (y, g_x); raises what the harness raises."""
    arena = Arena()
    xg, gg = arena.guarded(x, shift).requires_grad_(True), arena.guarded(g, shift)
    with hostile(arena, shift, device_types=('cpu',)):
        y = fn(xg); y.backward(gg)
    arena.check()
    assert_finite(y, 'y', ('row', 'column')); assert_finite(xg.grad, 'g_x', ('row', 'column'))
    return y.detach(), xg.grad


class _Double(torch.autograd.Function):
    """Correct: y = 2x through a workspace it fills itself."""
    @staticmethod
    def forward(ctx, x):
        y, ws = torch.empty_like(x), torch.empty(x.shape[0], dtype=x.dtype, device=x.device)
        ws[:] = 2.0
        y.copy_(x*ws[:, None])
        return y

    @staticmethod
    def backward(ctx, g):
        gx = torch.empty(g.shape, dtype=g.dtype, device=g.device)
        gx.copy_(2*g)
        return gx


class _SkipsLastRow(_Double):
    """The last row band of the output is never written."""
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        y[:-1] = 2*x[:-1]
        return y


class _WritesPastGradient(_Double):
    """The backward writes one element past its gradient (still inside the arena's buffer: the first guard bytes)."""
    @staticmethod
    def backward(ctx, g):
        gx = torch.empty_like(g)
        gx.copy_(2*g)
        torch.as_strided(gx, (gx.numel() + 1,), (1,))[-1] = 0.0
        return gx


class _ReadsBeforeInput(_Double):
    """The forward reads the element before its input and masks it off by multiplying with zero."""
    @staticmethod
    def forward(ctx, x):
        before = torch.as_strided(x, (1,), (1,), x.storage_offset() - 1)
        y = torch.empty_like(x)
        y.copy_(2*x)
        y[0, 0] += before[0]*0.0
        return y


class _StaleWorkspace(_Double):
    """A partial sum is read from the workspace before anything wrote it."""
    @staticmethod
    def forward(ctx, x):
        ws = torch.empty(4, dtype=x.dtype, device=x.device)
        y = torch.empty_like(x)
        y.copy_(2*x)
        y[1, 2] += ws[3]
        ws[3] = 0.0
        return y


X0, G0 = torch.arange(12.).reshape(3, 4), torch.ones(3, 4)


@pytest.mark.parametrize('shift', [0, 1])
def test_a_correct_operator_passes_with_guards_intact(shift):
    y, gx = _run(_Double.apply, X0, G0, shift)
    assert torch.equal(y, 2*X0) and torch.equal(gx, 2*G0)
    assert torch.empty is HM._EMPTY and torch.empty_like is HM._EMPTY_LIKE


@pytest.mark.parametrize('op,match', [
    (_SkipsLastRow, r'y: 4 of 12 elements are not finite, first at \(row, column\) = \(2, 0\): nan'),
    (_WritesPastGradient, r'guard band overwritten: block #\d+ \(shape \(3, 4\), torch.float32, allocation \d+ of \d+\), right side, first at byte offset 0 of the band = 0 bytes past its end'),
    (_ReadsBeforeInput, r'y: 1 of 12 elements are not finite, first at \(row, column\) = \(0, 0\): nan'),
    (_StaleWorkspace, r'y: 1 of 12 elements are not finite, first at \(row, column\) = \(1, 2\): nan')])
@pytest.mark.parametrize('shift', [0, 1])
def test_each_faulty_operator_is_caught_and_named(op, match, shift):
    with pytest.raises(AssertionError, match=match): _run(op.apply, X0, G0, shift)
    assert torch.empty is HM._EMPTY and torch.empty_like is HM._EMPTY_LIKE


def test_a_write_before_the_payload_names_the_left_side():
    arena = Arena()
    v = arena.alloc((5,), torch.float32, 'cpu')
    torch.as_strided(v, (1,), (1,), v.storage_offset() - 2)[0] = 1.0
    with pytest.raises(AssertionError, match=r'block #0 \(shape \(5,\), torch.float32, allocation 0 of 1\), left side, first at byte offset \d+ of the band = 8 bytes before the payload'):
        arena.check()
    assert arena.blocks == []      # dropped, also on failure
    arena.check()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32])
@pytest.mark.parametrize('shift', [0, 1, 3])
def test_views_are_poisoned_contiguous_and_placed_as_asked(dtype, shift):
    arena = Arena()
    v = arena.alloc((2, 3, 5), dtype, 'cpu', shift)
    item = v.element_size()
    assert v.shape == (2, 3, 5) and v.dtype == dtype and v.is_contiguous()
    assert v.data_ptr() % 16 == (shift*item) % 16 and GUARD % 16 == 0
    assert bool(v.isnan().all()) if dtype.is_floating_point else bool((v == (255 if dtype == torch.uint8 else -1)).all())     # 0xFF..: NaN, 255, a wild index
    buf, off, nbytes = arena.blocks[0][:3]
    assert off == GUARD + shift*item and nbytes == 30*item and buf.numel() >= off + nbytes + GUARD and bool((buf == 0xFF).all())
    g = arena.guarded(torch.arange(6, dtype=torch.float32).to(dtype).reshape(2, 3), shift)
    assert torch.equal(g, torch.arange(6, dtype=torch.float32).to(dtype).reshape(2, 3)) and not g.requires_grad
    assert arena.alloc((), torch.float32, 'cpu').shape == () and arena.alloc((2, 0, 3), torch.float32, 'cpu').numel() == 0
    arena.check()


def test_what_the_patch_does_not_model_passes_through():
    arena = Arena()
    with hostile(arena):                                   # the default: device allocations only - every CPU-side call goes to the original
        a, b = torch.empty(3, 4), torch.empty((3, 4), dtype=torch.float64, device='cpu')
        c = torch.empty_like(a)
        assert arena.blocks == [] and a.shape == b.shape == c.shape == (3, 4) and b.dtype == torch.float64
    with hostile(arena, device_types=('cpu',)):
        assert torch.empty(2, 3, device='cpu').isnan().all() and torch.empty((2, 3), device='cpu', dtype=torch.bfloat16).isnan().all()       # both size forms
        assert torch.empty(torch.Size((2,)), device='cpu').isnan().all() and torch.empty_like(a, dtype=torch.float64).dtype == torch.float64
        assert len(arena.blocks) == 4
        torch.empty(2, 3, device='cpu', pin_memory=False); torch.empty(2, 3, device='cpu', memory_format=torch.contiguous_format)           # keyword forms
        torch.empty(2, 3, device='cpu', requires_grad=True); torch.empty_like(a, memory_format=torch.preserve_format)
        torch.empty_like(a.t())                                                                                                             # non-contiguous source
        torch.empty(2, 3, device='meta')                                                                                                    # another device
        out = torch.zeros(3)
        torch.empty(3, out=out)
        assert len(arena.blocks) == 4
        assert bool((torch.zeros(4, device='cpu') == 0).all()) and bool((torch.ones_like(a) == 1).all())                                    # zero is their contract
    arena.check()


def test_the_patch_is_removed_after_an_exception():
    with pytest.raises(RuntimeError, match='inside'):
        with hostile(Arena(), device_types=('cpu',)):
            assert torch.empty is not HM._EMPTY
            raise RuntimeError('inside')
    assert torch.empty is HM._EMPTY and torch.empty_like is HM._EMPTY_LIKE


def test_first_nan_names_the_first_non_finite_element():
    t = torch.zeros(2, 3, 4)
    assert first_nan(t) is None and first_nan(torch.full((3,), 255, dtype=torch.uint8)) is None
    t[1, 0, 2], t[1, 2, 3] = float('inf'), float('nan')
    assert first_nan(t, ('sample', 'y', 'x')) == '2 of 24 elements are not finite, first at (sample, y, x) = (1, 0, 2): inf'
    assert first_nan(t.to(torch.bfloat16)).startswith('2 of 24 elements are not finite, first at (d0, d1, d2) = (1, 0, 2)')


def test_the_case_table_covers_every_public_operator():
    """Case names + NOT_COVERED == what `functional` re-exports; NOT_COVERED holds nothing that launches a kernel of its own (other than the debug self-test)."""
    import test_gpu_hostile_memory as G
    from slowtv_monodepth_amd import functional
    covered = {op for c in G.CASES for op in c.ops}
    public = set(functional.__all__)
    assert covered | set(G.NOT_COVERED) == public, (sorted(public - covered - set(G.NOT_COVERED)), sorted((covered | set(G.NOT_COVERED)) - public))
    assert not covered & set(G.NOT_COVERED) and all(isinstance(r, str) and r for r in G.NOT_COVERED.values())
    import inspect
    for name in G.NOT_COVERED:      # nothing listed there reaches the C ABI, except through the `smd_debug_*` helpers
        src = inspect.getsource(getattr(functional, name))
        if name == 'lane_shift_selftest': assert "call('smd_debug_" in src and src.count('call(') == 1
        else: assert 'call(' not in src and 'torch.empty' not in src and '_workspace(' not in src, name
    assert len({c.name for c in G.CASES}) == len(G.CASES)
