"""Synthetic three-frame batches with the layout and value ranges of the reference's dataloader output
(`(x, y, m)` of src/datasets/base_mde.py:158-184; KITTI intrinsics of src/datasets/kitti_raw.py:76-81).

There is no dataset on the GPU box, so training throughput is measured on device-resident synthetic triplets:
a smooth random texture (sum of sinusoids + 5 % noise, so SSIM is non-degenerate) and copies of it shifted by a
few pixels as support frames (so the warps matter and roughly half the pixels survive automasking).
"""
from __future__ import annotations

import math

import torch

from . import ops

__all__ = ['texture', 'kitti_K', 'lidar_depth', 'depth_hints_field', 'make_batch', 'STEREO_BASELINE', 'STEREO_SHIFT']


def texture(gen: torch.Generator, b: int, h: int, w: int, shift=(0.0, 0.0), device='cpu', waves: int = 6, coeffs=None):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device),
                            torch.arange(w, dtype=torch.float32, device=device), indexing='ij')
    xs, ys = xs + shift[0], ys + shift[1]
    if coeffs is None:
        coeffs = dict(f=torch.rand(waves, 2, generator=gen, device=device)*0.35 + 0.02,
                      ph=torch.rand(waves, b, 3, 1, 1, generator=gen, device=device)*2*math.pi,
                      amp=torch.rand(waves, b, 3, 1, 1, generator=gen, device=device),
                      noise=torch.rand(b, 3, h, w, generator=gen, device=device))
    img = torch.zeros(b, 3, h, w, device=device)
    for k in range(waves):
        img = img + coeffs['amp'][k]*torch.sin(coeffs['f'][k, 0]*xs + coeffs['f'][k, 1]*ys + coeffs['ph'][k])
    lo, hi = img.amin(dim=(2, 3), keepdim=True), img.amax(dim=(2, 3), keepdim=True)
    img = 0.95*(img - lo)/(hi - lo).clamp(min=1e-6) + 0.05*coeffs['noise']
    return img.clamp(0, 1), coeffs


def kitti_K(b: int, h: int, w: int, device='cpu') -> torch.Tensor:
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=device)
    return K[None].repeat(b, 1, 1)


def lidar_depth(gen: torch.Generator, b: int, H: int, W: int, device='cpu', density: float = 0.05) -> torch.Tensor:
    """(b,1,H,W) LiDAR-like ground truth: a smooth positive depth field (2 .. 60 m, nearer towards the bottom rows, modulated by a few sinusoids)
    kept at about `density` of the pixels and 0 (= no return) elsewhere."""
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H, device=device), torch.linspace(0, 1, W, device=device), indexing='ij')
    ph = torch.rand(b, 3, 1, 1, generator=gen, device=device)*2*math.pi
    field = 2 + 58*(1 - ys)**2*(0.75 + 0.25*torch.sin(6*xs + ph[:, 0])*torch.cos(4*ys + ph[:, 1])) + 0.5*torch.sin(9*xs + ph[:, 2])**2
    keep = torch.rand(b, H, W, generator=gen, device=device) < density
    return torch.where(keep, field, torch.zeros_like(field))[:, None]


STEREO_BASELINE = 0.1   # KITTI's 0.54 m baseline in the reference's 5.4-scaled units (src/datasets/kitti_raw.py:134)
STEREO_SHIFT = 3.0      # pixels the stereo partner's texture is shifted by, horizontally only


def depth_hints_field(gen: torch.Generator, b: int, h: int, w: int, device='cpu') -> torch.Tensor:
    """(b,1,h,w) proxy depth as a stereo matcher leaves it (`y['depth_hints']`): a dense, smooth, positive field (`lidar_depth`'s, 2 .. 60), 0 = "no hint" on
    three rectangular holes per sample and on about 10 % of scattered pixels; the LAST sample has hints in its lower half only."""
    field = lidar_depth(gen, b, h, w, device=device, density=2.0)          # density > 1: every pixel kept
    keep = torch.rand(b, 1, h, w, generator=gen, device=device) >= 0.1
    box = torch.rand(b, 3, 4, generator=gen, device=device)                # per hole: centre (y, x) and half extents, as fractions of the map
    ys, xs = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing='ij')
    for k in range(3):
        cy, cx = box[:, k, 0, None, None]*h, box[:, k, 1, None, None]*w
        ry, rx = 1 + box[:, k, 2, None, None]*h/6, 1 + box[:, k, 3, None, None]*w/6
        keep &= ~(((ys - cy).abs() <= ry) & ((xs - cx).abs() <= rx))[:, None]
    keep[-1, :, :h//2] = False
    return torch.where(keep, field, torch.zeros_like(field))


def make_batch(b: int, h: int, w: int, supp_idxs=(-1, 1), seed: int = 42, device='cpu', depth_shape=None, depth_hints: bool = False):
    """-> (x, y, m): x = network inputs (ImageNet-standardised), y = loss inputs (raw [0,1] images, K), m = metadata.
    `depth_shape=(H, W)` adds `y['depth']` (`lidar_depth`), drawn after everything else: the other entries are the same with and without it.
    A 0 among `supp_idxs` is the stereo partner: that support is the texture shifted HORIZONTALLY only, and `y['T_stereo']` (b,4,4) is its known pose —
    identity rotation, t = (-+STEREO_BASELINE, 0, 0): even samples are the left camera (t_x < 0, as the reference's KITTI loader signs it), odd ones the right,
    and the shift has the matching sign.  `depth_hints=True` adds `y['depth_hints']` (`depth_hints_field`), drawn last of all."""
    gen = torch.Generator(device=device).manual_seed(seed)
    imgs, coeffs = texture(gen, b, h, w, device=device)
    sign = torch.where(torch.arange(b, device=device) % 2 == 0, -1.0, 1.0)      # the sign of T_stereo's t_x per sample
    supp = []
    for k, i in enumerate(supp_idxs):
        if int(i) == 0:    # a point at target column u projects to u + f t_x/z in the partner: supp(x) = tex(x - f t_x/z), a shift against the sign of t_x
            shift = (-STEREO_SHIFT*sign.view(b, 1, 1, 1), 0.0)
        else:
            dx = (2.0 + k)*(1 if i > 0 else -1)
            shift = (dx, 0.5*dx)
        supp.append(texture(gen, b, h, w, shift=shift, device=device, coeffs=coeffs)[0])
    supp = torch.stack(supp)
    x = {'imgs': ops.standardize(imgs), 'supp_imgs': ops.standardize(supp), 'supp_idxs': torch.tensor(list(supp_idxs))}
    y = {'imgs': imgs, 'supp_imgs': supp, 'K': kitti_K(b, h, w, device)}
    m = {'supp': [str(i) for i in supp_idxs]}
    if any(int(i) == 0 for i in supp_idxs):
        T = torch.eye(4, device=device)[None].repeat(b, 1, 1)
        T[:, 0, 3] = STEREO_BASELINE*sign
        y['T_stereo'] = T
    if depth_shape is not None: y['depth'] = lidar_depth(gen, b, int(depth_shape[0]), int(depth_shape[1]), device=device)
    if depth_hints: y['depth_hints'] = depth_hints_field(gen, b, h, w, device=device)
    return x, y, m
