"""Image-logging operators: `rgb_from_disp` and `rgb_from_feat` with the reference's signatures (src/tools/viz.py:20-74), and `make_grid`, torchvision's
grid as the reference's HeavyLogger calls it (src/core/heavy_logger.py:35-42), over `smd_viz_*` / `smd_make_grid` (csrc/smd_viz.hip).

float32 GPU tensors take the kernels (`make_grid` also bool / uint8 masks); CPU tensors, numpy arrays and other dtypes take the plain path: the reference's
host sequence restated with numpy, with matplotlib and sklearn imported lazily (an ImportError names the missing one).  The kernels import neither.
Differences, stated: the fused `rgb_from_disp` returns float32 (the reference returns what numpy produced, float64: the table's entries are the same, rounded
once); the kernels (`fused_rgb_from_feat`) always take the exact covariance route (sklearn's `covariance_eigh`: means, the centred C x C matrix, `eigh`, `svd_flip`'s
sign) — sklearn's 'auto' picks LAPACK's SVD or, above 500 samples or channels with few samples per channel, a randomized SVD drawn from an unseeded
generator, which is not restated.  One exception to "float32 GPU tensors take the kernels": `rgb_from_feat` hands many channels over few samples to
the plain path where sklearn imports (`feat_routed_plain`), so for that shape class the result is sklearn's — its randomized solver included, two calls
then differ in the last digits — and depends on sklearn being installed; `fused_rgb_from_feat` is the kernels at every shape.  Not differentiable; not re-exported by `functional`.

`cmaps.json` holds the 256-entry tables of 'turbo', 'magma' and 'viridis': written by scripts/dev/make_cmaps.py from matplotlib 3.10.8 (data taken from
matplotlib; tests/test_viz_host.py compares them with the installed one)."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from ._device import _check, _on, _stream, _workspace, call
from ._lib import lib

__all__ = ['rgb_from_disp', 'rgb_from_feat', 'make_grid', 'plain_rgb_from_disp', 'plain_rgb_from_feat', 'plain_make_grid', 'percentile95', 'CMAPS', 'fused_rgb_from_feat', 'feat_routed_plain']

CMAPS = ('turbo', 'magma', 'viridis')
_tables: dict = {}
_luts: dict = {}
_eps = float(np.finfo(np.float32).eps)


def cmap_table(name: str) -> np.ndarray:
    """(256,3) float64 table of one of `CMAPS`; KeyError (naming the three) for any other name."""
    if name not in CMAPS: raise KeyError(f'cmap {name!r}: the fused path holds {", ".join(CMAPS)} (any other matplotlib name needs matplotlib)')
    if not _tables:
        doc = json.loads((Path(__file__).resolve().parent/'cmaps.json').read_text())
        _tables.update({k: np.asarray(doc[k], dtype=np.float64) for k in CMAPS})
    return _tables[name]


def _lut(device, name: str) -> torch.Tensor:
    key = (device.type, device.index, name)
    if key not in _luts: _luts[key] = torch.from_numpy(cmap_table(name).astype(np.float32)).to(device)
    return _luts[key]


def _need(module: str):
    import importlib
    try: return importlib.import_module(module)
    except ImportError as e: raise ImportError(f'the plain path of slowtv_monodepth_amd.viz needs {module.split(".")[0]} ({e}); float32 GPU tensors do not') from e


# ---------------------------------------------------------------------------------------------------------------- the reference's numpy conventions

def _from_np(x):
    """`allow_np(permute=True)` (src/tools/ops.py:179-207): a numpy input is (..., h, w, c) above two dimensions."""
    t = torch.as_tensor(x)
    return t.permute(*range(t.ndim - 3), -1, -3, -2) if t.ndim > 2 else t


def _to_np(t):
    t = t.permute(*range(t.ndim - 3), -2, -1, -3) if t.ndim > 2 else t
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- rgb_from_disp

def percentile95(x: np.ndarray) -> np.float32:
    """np.percentile(x, 95) of a non-empty float32 vector from its two order statistics, statement by statement as numpy 2 evaluates it for a float32
    array: q = 95/float32(100), the virtual index (n - 1) q in float32, and `_lerp` with its `t >= 0.5` form.  What `smd_viz_disp` computes per item."""
    f = np.float32
    x = np.sort(np.asarray(x, dtype=f).ravel())
    n = x.size
    vi = f(n - 1)*f(0.95)
    k0 = min(int(np.floor(vi)), n - 1); k1 = min(k0 + 1, n - 1)
    t = f(vi - f(np.floor(vi)))
    with np.errstate(invalid='ignore'):
        d = f(x[k1] - x[k0])
        r = f(x[k0] + f(d*t))
        if t >= 0.5: r = f(x[k1] - f(d*f(f(1) - t)))
    return r


def _disp4(disp):
    n = disp.ndim
    if n == 2: disp = disp[None, None]
    elif n == 3: disp = disp[None]
    if disp.ndim != 4 or disp.shape[1] != 1: raise ValueError(f'disp must be (h,w), (1,h,w) or (b,1,h,w), got {tuple(disp.shape)}')
    return disp, n


def _vmax_list(vmax, b):
    if isinstance(vmax, torch.Tensor): vmax = vmax.tolist()
    if vmax is None: return None
    if isinstance(vmax, (int, float)): return [vmax]*b
    if len(vmax) != b: raise ValueError(f'Non-matching vmax and disp. ({len(vmax)} vs. {b})')
    return list(vmax)


def plain_rgb_from_disp(disp: torch.Tensor, invert: bool = False, cmap: str = 'turbo', vmin=0, vmax=None) -> torch.Tensor:
    """viz.py:34-50 with `apply_cmap` (src/utils/misc.py:54-60) on the host -> (*b,3,h,w) in numpy's dtype (float64)."""
    plt = _need('matplotlib.pyplot')
    if isinstance(vmin, torch.Tensor): vmin = vmin.tolist()
    disp, n = _disp4(disp)
    if invert: disp = (disp > 0)/disp.clamp(min=torch.finfo(disp.dtype).eps if disp.is_floating_point() else _eps)
    d = disp.detach().cpu().numpy()[:, 0]
    vm = _vmax_list(vmax, d.shape[0])
    if vm is None:
        vm = []
        for x in d:
            try: vm.append(np.percentile(x[x > 0], 95))
            except IndexError: vm.append(0.0)
    cm = plt.get_cmap(cmap)
    out = []
    for x, v in zip(d, vm):
        x = x.clip(vmin, v)
        x = (x - vmin)/(v - vmin + 1e-5)
        out.append(torch.as_tensor(cm(x)[..., :-1]).permute(2, 0, 1))
    rgb = torch.stack(out)
    return rgb.squeeze(0) if n in (2, 3) else rgb


@torch.no_grad()
def _fused_disp(disp, invert, cmap, vmin, vmax):
    """disp (b,1,h,w) float32 on the GPU -> (rgb (b,3,h,w), vmax (b,)) through `smd_viz_disp`."""
    if isinstance(vmin, torch.Tensor): vmin = vmin.tolist()
    disp = _check('disp', disp.detach(), align=False)
    b, _, h, w = disp.shape
    dev = disp.device
    lut = _lut(dev, cmap)
    vm = _vmax_list(vmax, b)
    rgb = torch.empty((b, 3, h, w), device=dev, dtype=torch.float32)
    if vm is None:
        vmx = torch.empty((b,), device=dev, dtype=torch.float32); den = torch.empty((b,), device=dev, dtype=torch.float32)
    else:      # a Python-float vmax: the array is clipped at its float32 rounding, the denominator is formed in Python floats and rounded once
        vmx = torch.tensor(np.asarray(vm, dtype=np.float32), device=dev)
        den = torch.tensor(np.asarray([float(v) - vmin + 1e-5 for v in vm], dtype=np.float32), device=dev)
    ws, nbytes = _workspace(dev, lib.smd_viz_disp_workspace_bytes, b, h, w, floor=256)
    call('smd_viz_disp', disp.data_ptr(), b, h, w, int(bool(invert)), int(vm is None), float(vmin), float(np.float32(0.0 - vmin + 1e-5)), lut.data_ptr(),
         lut.shape[0], rgb.data_ptr(), vmx.data_ptr(), den.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return rgb, vmx


def _fused_ok(x) -> bool: return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32


def rgb_from_disp(disp, invert: bool = False, cmap: str = 'turbo', vmin=0, vmax=None):
    """Disparity / depth map (h,w), (1,h,w) or (b,1,h,w) -> its colour map (*b,3,h,w) (viz.py:20-50).  `invert`: `to_inv` first; `vmax` None: the 95th
    percentile of each item's positive values, else a number or one per item.  A numpy input follows the reference's (..., h, w, 1) convention."""
    if isinstance(disp, np.ndarray): return _to_np(plain_rgb_from_disp(_from_np(disp), invert, cmap, vmin, vmax))
    fused = _fused_ok(disp)
    if fused and cmap not in CMAPS:
        try: import matplotlib  # noqa: F401
        except ImportError: cmap_table(cmap)           # raises the KeyError that names the three
        fused = False
    if not fused: return plain_rgb_from_disp(disp, invert, cmap, vmin, vmax)
    d4, n = _disp4(disp)
    rgb, _ = _fused_disp(d4, invert, cmap, vmin, vmax)
    return rgb.squeeze(0) if n in (2, 3) else rgb


# ---------------------------------------------------------------------------------------------------------------- rgb_from_feat

def _feat4(feat):
    n = feat.ndim
    if n == 3: feat = feat[None]
    if feat.ndim != 4: raise ValueError(f'feat must be (c,h,w) or (b,c,h,w), got {tuple(feat.shape)}')
    return feat, n


def plain_rgb_from_feat(feat: torch.Tensor) -> torch.Tensor:
    """viz.py:62-74 on the host: sklearn's PCA over all b*h*w samples, `proj -= min; proj /= max` per channel."""
    PCA = _need('sklearn.decomposition').PCA
    feat, n = _feat4(feat)
    b, _, h, w = feat.shape
    x = feat.detach().permute(0, 2, 3, 1).flatten(0, 2).cpu().numpy()
    proj = PCA(n_components=3).fit_transform(x)
    proj -= proj.min(0)
    proj /= proj.max(0)
    out = torch.as_tensor(proj.reshape(b, h, w, 3)).permute(0, 3, 1, 2)
    return out.squeeze(0) if n == 3 else out


def leading_components(cov: torch.Tensor) -> torch.Tensor:
    """Symmetric (C,C) float64 on the host -> (C,3): the eigenvectors of the three largest eigenvalues, each signed so that its entry of largest magnitude is
    positive (`PCA._fit_full`'s covariance_eigh branch and `svd_flip(u_based_decision=False)`, sklearn 1.7.2)."""
    _, vecs = torch.linalg.eigh(cov)
    V = vecs[:, [-1, -2, -3]].clone()
    idx = V.abs().argmax(dim=0)
    return V*torch.sign(V[idx, torch.arange(3)])


def feat_routed_plain(C: int, n: int) -> bool:
    """The static rule for the one shape class at which the fused operator loses (profiles/viz_times.txt: (12,512,6,20) 14.8 ms against 3.7 ms): many
    channels and few samples, where the host's `eigh` of the C x C matrix (~C^3) outweighs everything the kernels save (the plain path works on n x C).
    Only where sklearn imports: without it the fused operator serves every shape.  The thresholds rest on that ONE measured shape (and on (12,64,..) shapes
    that win); they are a guess between them, not a fitted boundary.  A routed call returns what sklearn's 'auto' solver gives (viz.py module docstring)."""
    import importlib.util
    return C >= 256 and n <= 16*C and importlib.util.find_spec('sklearn') is not None


@torch.no_grad()
def fused_rgb_from_feat(feat):
    """feat (b,C,h,w) float32 on the GPU -> (b,3,h,w) through `smd_viz_feat_*`, whatever `feat_routed_plain` says."""
    feat = _check('feat', feat.detach(), align=False)
    b, C, h, w = feat.shape
    if min(b*h*w, C) < 3: raise ValueError(f'n_components=3 must be between 0 and min(n_samples, n_features)={min(b*h*w, C)}')
    dev = feat.device
    ws, nbytes = _workspace(dev, lib.smd_viz_feat_workspace_bytes, b, C, h, w, floor=256)
    mean = torch.empty((C,), device=dev, dtype=torch.float64); cov = torch.empty((C, C), device=dev, dtype=torch.float64)
    call('smd_viz_feat_moments', feat.data_ptr(), b, C, h, w, mean.data_ptr(), cov.data_ptr(), ws.data_ptr(), nbytes, _stream())
    V = leading_components(cov.cpu()).to(torch.float32).contiguous().to(dev)       # the only copy to the host: C x C
    rgb = torch.empty((b, 3, h, w), device=dev, dtype=torch.float32)
    call('smd_viz_feat_project', feat.data_ptr(), mean.data_ptr(), V.data_ptr(), b, C, h, w, rgb.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return rgb


def rgb_from_feat(feat):
    """Dense features (c,h,w) or (b,c,h,w) -> their three leading principal components over the whole batch, each scaled to [0, 1] (viz.py:54-74)."""
    if isinstance(feat, np.ndarray): return _to_np(plain_rgb_from_feat(_from_np(feat)))
    if not _fused_ok(feat): return plain_rgb_from_feat(feat)
    f4, n = _feat4(feat)
    if feat_routed_plain(f4.shape[1], f4.shape[0]*f4.shape[2]*f4.shape[3]): return plain_rgb_from_feat(feat).to(feat.device)
    rgb = fused_rgb_from_feat(f4)
    return rgb.squeeze(0) if n == 3 else rgb


# ---------------------------------------------------------------------------------------------------------------- make_grid

def _grid_check(x):
    if not isinstance(x, torch.Tensor): raise TypeError(f'x must be a Tensor, got {type(x)}')
    if x.ndim != 4 or x.shape[1] not in (1, 3): raise ValueError(f'x must be (b,1,h,w) or (b,3,h,w), got {tuple(x.shape)}')


def plain_make_grid(x: torch.Tensor, n_imgs: int = 6, nrow: int = 2, padding: int = 2, pad_value: float = 0.0, normalize: bool = False) -> torch.Tensor:
    """torchvision's `make_grid(x[:n_imgs], nrow, padding, pad_value=pad_value, normalize=normalize)` from its documented behaviour, with torch slicing."""
    _grid_check(x)
    if n_imgs < 1: raise ValueError(f'n_imgs must be positive, got {n_imgs}')
    x = x[:n_imgs]
    if not x.is_floating_point(): x = x.float()
    if x.shape[1] == 1: x = x.expand(-1, 3, -1, -1)
    if normalize:
        lo, hi = float(x.min()), float(x.max())
        x = x.clamp(min=lo, max=hi).sub(lo).div(max(hi - lo, 1e-5))
    n, _, h, w = x.shape
    if n == 1: return x[0].clone()
    xmaps = min(nrow, n); ymaps = -(-n//xmaps)
    grid = x.new_full((3, (h + padding)*ymaps + padding, (w + padding)*xmaps + padding), pad_value)
    for k in range(n):
        y0, x0 = (k//xmaps)*(h + padding) + padding, (k % xmaps)*(w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = x[k]
    return grid


@torch.no_grad()
def make_grid(x: torch.Tensor, n_imgs: int = 6, nrow: int = 2, padding: int = 2, pad_value: float = 0.0, normalize: bool = False) -> torch.Tensor:
    """(b,1|3,h,w) -> (3,Hg,Wg): the first `n_imgs` images, `nrow` per row, `padding` pixels of `pad_value` around each; one image alone comes back as it is.
    float32, bool and uint8 GPU tensors take one gather (`smd_make_grid`; masks are read as they are); everything else `plain_make_grid`."""
    _grid_check(x)
    if not (x.is_cuda and x.dtype in (torch.float32, torch.bool, torch.uint8)): return plain_make_grid(x, n_imgs, nrow, padding, pad_value, normalize)
    if n_imgs < 1: raise ValueError(f'n_imgs must be positive, got {n_imgs}')
    u8 = x.dtype != torch.float32
    x = x.detach().contiguous()
    if x.dtype == torch.bool: x = x.view(torch.uint8)
    if not u8: x = _check('x', x, align=False)
    b, c, h, w = x.shape
    n = min(b, n_imgs); pad = 0 if n == 1 else padding
    xmaps = min(nrow, n); ymaps = -(-n//xmaps)
    grid = torch.empty((3, (h + pad)*ymaps + pad, (w + pad)*xmaps + pad), device=x.device, dtype=torch.float32)
    _on(x)                                             # (a mask does not pass `_check`: declare its device the operator's, for `call` and `_stream`)
    ws, nbytes = _workspace(x.device, lib.smd_make_grid_workspace_bytes, floor=256)
    call('smd_make_grid', x.data_ptr(), int(u8), b, c, h, w, int(n_imgs), int(nrow), int(padding), float(pad_value), int(bool(normalize)), grid.data_ptr(),
         ws.data_ptr(), nbytes, _stream())
    return grid
