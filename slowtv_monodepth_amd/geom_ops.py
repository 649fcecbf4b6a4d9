"""The pose / intrinsics prologue of the training step as `torch.autograd.Function`s (`smd_pose_*`, `smd_intrinsics_*`).  `functional` re-exports the wrappers."""
import torch

from ._device import _aligned, _check, _on, _ptr, _stream, call


class _PoseMatrices(torch.autograd.Function):
    """`T_from_AAt` (+ rigid inverse where flagged) in one launch (src/tools/geometry.py:181-209, src/core/trainer.py:253)."""

    @staticmethod
    def forward(ctx, aa, t, invert):
        aa = _check('aa', aa); t = _check('t', t, aa.shape)
        if aa.ndim != 2 or aa.shape[1] != 3: raise ValueError(f'aa and t must be (N,3), got {tuple(aa.shape)}')
        N = aa.shape[0]
        if invert is not None:
            if invert.dtype != torch.uint8 or tuple(invert.shape) != (N,) or not invert.is_cuda: raise ValueError('invert must be a CUDA uint8 (N,) tensor')
            invert = _aligned(invert)
        T = torch.empty((N, 4, 4), device=aa.device, dtype=torch.float32)
        call('smd_pose_fwd', aa.data_ptr(), t.data_ptr(), _ptr(invert), N, T.data_ptr(), _stream())
        ctx.save_for_backward(aa, t, invert)
        return T

    @staticmethod
    def backward(ctx, g_T):
        aa, t, invert = ctx.saved_tensors
        _on(aa)
        g_T = _aligned(g_T)
        g_aa, g_t = torch.empty_like(aa), torch.empty_like(t)
        call('smd_pose_bwd', aa.data_ptr(), t.data_ptr(), _ptr(invert), aa.shape[0], g_T.data_ptr(), g_aa.data_ptr(), g_t.data_ptr(), _stream())
        return g_aa, g_t, None


def pose_matrices(aa, t, invert=None):
    """Axis-angle + translation (N,3) -> (N,4,4) transforms; rows with `invert[i] != 0` hold the inverse transform."""
    return _PoseMatrices.apply(aa, t, invert)


class _Intrinsics(torch.autograd.Function):
    """`resize_K(build_K(fs, cs), (h, w))` and its inverse in one launch (src/networks/pose.py:60-73, geometry.py:249-263, 383)."""

    @staticmethod
    def forward(ctx, fs, cs, h, w):
        fs = _check('fs', fs); cs = _check('cs', cs, fs.shape)
        if fs.ndim != 2 or fs.shape[1] != 2: raise ValueError(f'fs and cs must be (b,2), got {tuple(fs.shape)}')
        b = fs.shape[0]
        K = torch.empty((b, 4, 4), device=fs.device, dtype=torch.float32); K_inv = torch.empty_like(K)
        call('smd_intrinsics_fwd', fs.data_ptr(), cs.data_ptr(), None, b, h, w, K.data_ptr(), K_inv.data_ptr(), _stream())
        ctx.save_for_backward(fs, cs); ctx.size = (h, w)
        return K, K_inv

    @staticmethod
    def backward(ctx, g_K, g_Kinv):
        fs, cs = ctx.saved_tensors
        _on(fs)
        h, w = ctx.size
        g_fs, g_cs = torch.empty_like(fs), torch.empty_like(cs)
        call('smd_intrinsics_bwd', fs.data_ptr(), cs.data_ptr(), fs.shape[0], h, w, _aligned(g_K).data_ptr(), _aligned(g_Kinv).data_ptr(), g_fs.data_ptr(),
             g_cs.data_ptr(), _stream())
        return g_fs, g_cs, None, None


def intrinsics(fs, cs, size):
    """Normalised focal lengths / principal point (b,2) -> (K, K_inv) (b,4,4) at image size `size=(h, w)`."""
    return _Intrinsics.apply(fs, cs, int(size[0]), int(size[1]))


def inv_intrinsics(K):
    """Inverse of caller-supplied intrinsics (b,4,4) (3x3 block; not differentiable — dataset intrinsics are constants)."""
    K = _check('K', K.detach())
    if K.ndim != 3 or tuple(K.shape[1:]) != (4, 4): raise ValueError(f'K must be (b,4,4), got {tuple(K.shape)}')
    K_inv = torch.empty_like(K)
    call('smd_intrinsics_fwd', None, None, K.data_ptr(), K.shape[0], 1, 1, None, K_inv.data_ptr(), _stream())
    return K_inv
