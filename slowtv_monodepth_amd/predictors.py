"""Predictors: a pretrained network run over batches of images -> disparities (reference: `src/core/predictors.py:22-208`).

`MonoDepthPredictor` is the reference's base class (pre-process, forward, post-process, the optional flip-and-blend of a second, mirrored pass) and
`BenchmarkPredictor`, registry key `ours`, loads this package's own checkpoints and the reference's.  Two things differ from the reference on purpose: with
`use_stereo_blend` the mirrored pass's prediction is NOT flipped back and blended by ATen, it goes to `functional.flip_blend` as it is (one launch, with the
predictor's disparity scaling folded in where the post-process is the stock one); and `__call__` / `apply` take any iterable of batches whose first element is
a dict with `imgs`, not only a DataLoader over the reference's `BaseDataset` (datasets are out of scope here).  The external predictors (`newcrfs`, `midas`)
are not restated."""
from __future__ import annotations

import logging
from abc import ABC, abstractmethod

import torch
import torch.nn as nn

from . import io
from .blend import flip_blend, plain_flip_blend
from .geometry import to_scaled
from .registry import register

__all__ = ['MonoDepthPredictor', 'BenchmarkPredictor']


def _device(device) -> torch.device:
    """`ops.get_device` of the reference: the given device, else the GPU when there is one."""
    if device is not None: return torch.device(device)
    return torch.device('cuda' if torch.cuda.is_available() else 'cpu')


class MonoDepthPredictor(ABC):
    """Base class for computing depth predictions over batches of images: pre-process, forward, post-process (src/core/predictors.py:22-147).
    Subclasses override `load_model`, and `get_img_shape` / `preprocess` / `forward` / `postprocess` where the defaults (no-ops, `net(imgs)`) do not fit."""
    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        cls.logger = logging.getLogger(f'slowtv_monodepth_amd.{cls.__qualname__}')

    @abstractmethod
    def load_model(self, *args, **kwargs) -> nn.Module:
        """Load a pretrained model.  Must be overridden."""

    @staticmethod
    def get_img_shape(data_type: str):
        """(h, w) the images of a dataset type are resized to; None: the dataset's own size."""
        return None

    def preprocess(self, imgs: torch.Tensor) -> torch.Tensor:
        """(b,3,h,w) dataset images (resized, standardised) -> what the network takes.  Default: as they are."""
        return imgs

    def forward(self, net: nn.Module, imgs: torch.Tensor) -> torch.Tensor:
        """-> (b,*1,h,w) raw prediction."""
        return net(imgs)

    def postprocess(self, pred: torch.Tensor, imgs: torch.Tensor) -> torch.Tensor:
        """(b,*1,h,w) raw prediction, (b,3,h,w) images before `preprocess` -> (b,1,h,w) DISPARITY.  Default: as it is."""
        return pred

    def blend(self, pred: torch.Tensor, pred_mirrored: torch.Tensor, imgs: torch.Tensor) -> torch.Tensor:
        """The prediction blended with the one for the mirrored image (NOT flipped back), then post-processed: the reference's
        `postprocess(blend_stereo(pred, pred_flip.flip(-1)))` (src/core/predictors.py:80-85)."""
        blended = flip_blend(pred, pred_mirrored) if pred.ndim == 4 else plain_flip_blend(pred, pred_mirrored)
        return self.postprocess(blended, imgs)

    def forward_batch(self, x: dict, net: nn.Module, device, use_stereo_blend: bool = False) -> torch.Tensor:
        with torch.no_grad():
            imgs = self.preprocess(x['imgs']).to(device)
            pred = self.forward(net, imgs)
            if not use_stereo_blend: return self.postprocess(pred, x['imgs'])
            # the mirrored images: flipped on the device, after the copy; a `preprocess` of the subclass's own sees the flipped images first, as in the reference
            own = type(self).preprocess is not MonoDepthPredictor.preprocess
            mirrored = self.preprocess(x['imgs'].flip(dims=[-1])).to(device) if own else imgs.flip(dims=[-1])
            return self.blend(pred, self.forward(net, mirrored), x['imgs'])

    def _batches(self, dl):
        for batch in dl: yield batch, (batch[0] if isinstance(batch, (tuple, list)) else batch)

    def apply(self, net: nn.Module, dl, func, use_stereo_blend: bool = False, device=None, *args, **kwargs) -> None:
        """Predict every batch of `dl` and call `func(batch, pred, *args, **kwargs)` with the prediction on the host."""
        device = _device(device)
        net = net.to(device)
        for batch, x in self._batches(dl):
            pred = self.forward_batch(x, net, device, use_stereo_blend)
            assert pred.ndim == 4, f'Prediction must be 4-D, got {pred.shape}!'
            func(batch, pred.detach().cpu(), *args, **kwargs)

    def __call__(self, net: nn.Module, dl, use_stereo_blend: bool = False, device=None):
        """-> (n, h, w) ndarray (squeezed): the predictions for every image of `dl`, an iterable of batches `(x, ...)` or `x` with `x['imgs']` (b,3,h,w)."""
        device = _device(device)
        net = net.to(device)
        preds = []
        for _, x in self._batches(dl):
            pred = self.forward_batch(x, net, device, use_stereo_blend)
            assert pred.ndim == 4, f'Prediction must be 4-D, got {pred.shape}!'
            preds.append(pred.detach().cpu())
        preds = torch.cat(preds) if preds else torch.zeros(0, 1, 0, 0)
        sanity = preds.flatten(1, -1).sum(1)
        if len(idxs := (sanity == 0).nonzero()): raise ValueError(f"Found empty predictions at indices '{idxs}'!")
        return preds.squeeze().numpy()


@register('ours')
class BenchmarkPredictor(MonoDepthPredictor):
    """Predictions of the models this package (or the reference) trained (src/core/predictors.py:152-207)."""
    min_depth = max_depth = None

    @staticmethod
    def get_img_shape(data_type: str):
        """Width 640 (mapfree: portrait), height by dataset."""
        return {'ddad': (416, 640), 'diode': (480, 640), 'kitti': (192, 640), 'kitti_lmdb': (192, 640), 'mannequin': (384, 640), 'mannequin_lmdb': (384, 640),
                'mapfree': (512, 384), 'nyud': (480, 640), 'sintel': (288, 640), 'syns_patches': (192, 640), 'tum': (480, 640)}[data_type]

    def load_model(self, ckpt_file, cfg_files=None) -> nn.Module:
        """The depth network of a checkpoint in the reference's Lightning layout (this package's `last.ckpt` is one): the module is built from the cfg the
        checkpoint carries, or from `cfg_files` (then loaded non-strictly, for legacy checkpoints), put in `eval()` and frozen."""
        import pickle
        from .networks.checkpoint import load_reference_checkpoint
        from .trainer import MonoDepthModule
        self.logger.info(f"Loading pretrained weights from '{ckpt_file}'...")
        try: ckpt = torch.load(ckpt_file, map_location='cpu', weights_only=True)
        except pickle.UnpicklingError: ckpt = torch.load(ckpt_file, map_location='cpu', weights_only=False)      # (a Lightning checkpoint's hyper-parameter objects)
        cfg = io.load_merge_yaml(*cfg_files) if cfg_files else (ckpt.get('hyper_parameters') or {}).get('cfg')
        if not cfg: raise ValueError(f"'{ckpt_file}' carries no cfg (hyper_parameters.cfg): pass cfg_files")
        mod = MonoDepthModule(cfg)
        load_reference_checkpoint(mod, ckpt, strict=not cfg_files)
        self.min_depth, self.max_depth = getattr(mod, 'min_depth', None), getattr(mod, 'max_depth', None)
        mod.eval().requires_grad_(False)
        return next(v for k, v in mod.nets.items() if 'depth' in k)

    def forward(self, net: nn.Module, imgs: torch.Tensor) -> torch.Tensor:
        """-> (b,1,h,w) the highest-resolution sigmoid disparity."""
        return net(imgs)['disp'][0]

    def postprocess(self, pred: torch.Tensor, imgs: torch.Tensor) -> torch.Tensor:
        """Sigmoid disparity -> scaled disparity where the loaded module had a depth range; the constants are the reference's literals (src/core/predictors.py:206)."""
        if self.min_depth or self.max_depth: pred = to_scaled(pred, min=0.1, max=100)[0]
        return pred

    def blend(self, pred, pred_mirrored, imgs):
        """With the stock `postprocess` the scaling rides in the blend's launch; a subclass's own `postprocess` runs behind the blend, as in the reference."""
        if type(self).postprocess is not BenchmarkPredictor.postprocess or pred.ndim != 4: return super().blend(pred, pred_mirrored, imgs)
        rng = dict(min_depth=0.1, max_depth=100) if (self.min_depth or self.max_depth) else {}
        return flip_blend(pred, pred_mirrored, **rng)
