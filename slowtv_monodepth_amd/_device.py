"""Which device's stream a launch goes to, the operand checks every operator starts with, and how operands and workspaces reach the C call.
Private: the operator modules import it."""
from __future__ import annotations

import threading

import torch

from ._lib import call as _raw_call, ptr_array

# Device of the operands of the operator this THREAD is executing: launches go to ITS current stream.  Thread-local, and set at
# the top of every forward (by `_check`) AND every backward (by `_on`): autograd runs the backward of each device on its own
# thread and has already made that device current there, so a process-wide "last validated device" would send the backward of
# one GPU's graph to another GPU's stream as soon as two devices are used in one process.  Exactly ONE such object exists (every
# module imports it from here): with a second, one module's `_check` and another's `_stream()` would disagree about the device.
_tls = threading.local()


def _on(t: torch.Tensor) -> torch.device:
    """Declare `t`'s device the device of the operator being executed on this thread (call first in every backward)."""
    _tls.device = t.device
    return t.device


def call(name: str, *args):
    """Launch with the operands' device current (the library launches on the calling thread's current HIP device)."""
    dev = getattr(_tls, 'device', None)
    if dev is not None and dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev): return _raw_call(name, *args)
    return _raw_call(name, *args)


def _stream() -> int:
    """The HIP stream of the operands' device.  (Not simply `torch.cuda.current_stream()`: with tensors on a GPU that is not the
    process's current device that would be a stream of another device.)"""
    dev = getattr(_tls, 'device', None)
    return torch.cuda.current_stream(dev if dev is not None else torch.cuda.current_device()).cuda_stream


ALIGN = 16     # bytes: what the C ABI requires of every pointer it is handed (include/smd_hotpath.h)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """`t` contiguous at a base the C ABI accepts.  The kernels read and write through naturally aligned vector types (16-byte `f4` rows, `float2`
    pairs, dwords over bf16 rows).  The caching allocator's blocks are aligned far beyond that, but a contiguous VIEW with a storage offset (a slice of a flat
    parameter or gradient bucket) is only element-aligned: it is copied to a block of its own.  One modulo per operand."""
    t = t.contiguous()
    return t if t.data_ptr() % ALIGN == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(name: str, t: torch.Tensor, shape=None, align: bool = True) -> torch.Tensor:
    """`align=False`: for an entry point that takes 4-byte aligned pointers (the header says so where one does), a contiguous storage-offset view goes as it is."""
    if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    if not t.is_cuda: raise RuntimeError(f'{name} must live on the GPU: the view-synthesis hot path has no CPU implementation')
    _tls.device = t.device
    if t.dtype != torch.float32: raise TypeError(f'{name} must be float32 (the loss path is fp32 only), got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape): raise ValueError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    return _aligned(t) if align else t.contiguous()


def _check_fb(name: str, t: torch.Tensor, shape=None) -> torch.Tensor:
    """Like `_check`, for the operators that also take bfloat16 tensors at an autocast boundary."""
    if not isinstance(t, torch.Tensor): raise TypeError(f'{name} must be a Tensor, got {type(t)}')
    if not t.is_cuda: raise RuntimeError(f'{name} must live on the GPU')
    if t.dtype not in (torch.float32, torch.bfloat16): raise TypeError(f'{name} must be float32 or bfloat16, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape): raise ValueError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    return _aligned(t)


def _ptr(t):
    """The device pointer of an optional operand: None (NULL in the C call) for None."""
    return t.data_ptr() if t is not None else None


def _ptrs(ts):
    """The pointer array of a sequence of tensors (the per-scale operands)."""
    return ptr_array([t.data_ptr() for t in ts])


def _workspace(device, query, *args, floor: int = 0):
    """-> (uint8 workspace, nbytes): `nbytes = query(*args)`, one of the library's `*_workspace_bytes` (or a size already asked for), is what the C call
    takes as `workspace_bytes`; at least `floor` bytes are allocated, so that a launch that needs no workspace still gets a pointer."""
    nbytes = query(*args) if callable(query) else query
    return torch.empty(max(nbytes, floor), device=device, dtype=torch.uint8), nbytes
