"""Memory arranged so that a tiled kernel's usual faults show (test_hostile_memory_host.py checks the harness on the CPU, test_gpu_hostile_memory.py
runs the operators in it).

The suite's other tests run on whatever the caching allocator hands out: a second call at one shape gets back the block the first call just freed, which
still holds the right answer, so an output tile that is never written passes; a read a few elements outside a tensor lands in the allocator's own segment
and a masked-off tail (`garbage * 0`) hides it; a write there corrupts nothing anybody looks at.  Here every buffer is the middle of a larger `uint8` buffer
whose every byte is 0xFF - NaN as fp32, bf16 and fp64, 255 as uint8, a huge index as an integer - with a guard band of `GUARD` bytes on each side:

    unwritten output, stale workspace, read outside a tensor   ->  a NaN (or a wild value) in what the operator returns: `assert_finite` / `first_nan`
    write outside a tensor                                     ->  a guard byte that is no longer 0xFF: `Arena.check`

`hostile(arena)` serves the `torch.empty` / `torch.empty_like` calls of the operator modules from the arena while it is active; `Arena.guarded` puts an
operand there.  `shift_elems=k` moves a payload k elements off its 16-byte alignment.  Device-agnostic: CPU tensors work too (the self-tests use them)."""
import contextlib

import torch

# The allocator's own functions, bound at import: the arena allocates with THESE (through the patched names it would call itself), and `hostile` puts them back.
_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like

GUARD = 64*1024      # bytes on each side of a payload; a multiple of 16, so that a payload stays 16-byte aligned unless a shift is asked for
POISON = 0xFF


class Arena:
    """Poisoned, guarded blocks.  `alloc` / `guarded` hand out payload views; `check()` verifies every guard band and drops the blocks."""

    def __init__(self):
        self.blocks = []       # (buffer, payload offset in bytes, payload bytes, shape, dtype): in allocation order

    def alloc(self, shape, dtype, device, shift_elems: int = 0) -> torch.Tensor:
        """A contiguous view of `shape` in the middle of a buffer of 0xFF bytes, `shift_elems` elements past the 16-byte aligned end of the left guard."""
        shape = tuple(int(v) for v in shape)
        item = _EMPTY((), dtype=dtype).element_size()
        numel = 1
        for v in shape: numel *= v
        nbytes, off = numel*item, GUARD + int(shift_elems)*item
        total = off + -(-nbytes//16)*16 + GUARD
        buf = _EMPTY(total, dtype=torch.uint8, device=device)
        buf.fill_(POISON)
        if buf.data_ptr() % 16: raise AssertionError('the allocator returned a buffer that is not 16-byte aligned')
        self.blocks.append((buf, off, nbytes, shape, dtype))
        return buf[off:off + nbytes].view(dtype).view(shape)

    def guarded(self, t: torch.Tensor, shift_elems: int = 0) -> torch.Tensor:
        """A copy of the operand `t` in a block of its own (detached: a fresh leaf for the caller to mark)."""
        v = self.alloc(t.shape, t.dtype, t.device, shift_elems)
        v.copy_(t.detach())
        return v

    def check(self) -> None:
        """Synchronise, assert that every guard byte of every block is still 0xFF, drop the blocks (also when the assertion fails)."""
        blocks, self.blocks = self.blocks, []
        if any(b[0].is_cuda for b in blocks): torch.cuda.synchronize()
        for order, (buf, off, nbytes, shape, dtype) in enumerate(blocks):
            for side, band, origin in (('left', buf[:off], -off), ('right', buf[off + nbytes:], 0)):
                bad = band != POISON
                if not bool(bad.any()): continue
                k = int(bad.to(torch.uint8).argmax())
                where = f'{-(origin + k)} bytes before the payload' if side == 'left' else f'{k} bytes past its end'
                raise AssertionError(f'guard band overwritten: block #{order} (shape {shape}, {dtype}, allocation {order} of {len(blocks)}), {side} side, '
                                     f'first at byte offset {k} of the band = {where}: 0x{int(band[k]):02x} instead of 0xff; {int(bad.sum())} guard bytes changed')


def _device_of(kwargs):
    """The device type a `torch.empty` call names (no `device=`: the default, the CPU)."""
    return torch.device(kwargs['device']).type if kwargs.get('device') is not None else 'cpu'


@contextlib.contextmanager
def hostile(arena: Arena, shift_elems: int = 0, device_types=('cuda',)):
    """While active, `torch.empty` and `torch.empty_like` serve allocations on `device_types` from `arena`.  Everything the patch does not model goes
    straight to the originals: other devices (the CPU, by default), non-contiguous `empty_like` sources, any keyword other than `dtype` / `device`
    (`memory_format`, `pin_memory`, `out`, ...).  `torch.zeros` and friends are not touched: zero is their contract."""
    def empty(*size, **kw):
        if set(kw) - {'dtype', 'device'} or _device_of(kw) not in device_types: return _EMPTY(*size, **kw)
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)): size = tuple(size[0])
        if not all(isinstance(v, int) for v in size): return _EMPTY(*size, **kw)
        return arena.alloc(size, kw.get('dtype') or torch.get_default_dtype(), kw['device'], shift_elems)

    def empty_like(t, **kw):
        if set(kw) - {'dtype'} or t.device.type not in device_types or not t.is_contiguous() or t.layout != torch.strided: return _EMPTY_LIKE(t, **kw)
        return arena.alloc(t.shape, kw.get('dtype') or t.dtype, t.device, shift_elems)

    torch.empty, torch.empty_like = empty, empty_like
    try: yield arena
    finally: torch.empty, torch.empty_like = _EMPTY, _EMPTY_LIKE


def first_nan(t: torch.Tensor, names=None):
    """None where every element of `t` is finite (integer tensors always are), else 'names = index: value' for the first one that is not and how many."""
    if not (t.is_floating_point() or t.is_complex()): return None
    bad = ~torch.isfinite(t)
    n = int(bad.sum())
    if n == 0: return None
    flat = int(bad.reshape(-1).to(torch.uint8).argmax())
    idx = []
    for d in reversed(t.shape): idx.append(flat % d); flat //= d
    idx = tuple(reversed(idx))
    names = tuple(names) if names is not None else tuple(f'd{k}' for k in range(t.ndim))
    return f'{n} of {t.numel()} elements are not finite, first at ({", ".join(names)}) = {idx}: {t[idx].item()!r}'


def assert_finite(t: torch.Tensor, what: str, names=None) -> None:
    msg = first_nan(t, names)
    assert msg is None, f'{what}: {msg} (poison read: an output or workspace element nobody wrote, or a read outside a tensor)'
