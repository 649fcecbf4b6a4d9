"""The reference's image logger (src/core/heavy_logger.py) without Lightning: the batch, the network outputs and the losses' artefacts as image grids, under
the reference's keys, written to a writer object with `add_images(key, tensor, step)` and `add_text(key, str, step)`.

`HeavyLogger.log_step(module, batch, mode, step)` runs `module.step` under `no_grad` (the module must have been built with `trainer.log_images`, which
makes the loss path keep `supp_imgs_warp`, `automask`, ...) and calls `log_batch`, `log_fwd` and `log_loss`.  Every grid of a call is built on the tensors'
device by `viz.rgb_from_disp`, `viz.rgb_from_feat` and `viz.make_grid` — kernels for float32 GPU tensors, the plain host sequence otherwise (or with
`plain=True`, which is what the tests compare with) — and the writer sees finished grids only.  Writers: `NpyWriter` (one .npy per key and step, one
text.jsonl; no dependencies), `TensorBoardWriter` (needs `torch.utils.tensorboard`), `RecordingWriter` (keeps everything in lists).  Not served: wandb."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from . import viz

__all__ = ['HeavyLogger', 'NpyWriter', 'TensorBoardWriter', 'RecordingWriter']

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # ImageNet statistics (src/tools/ops.py: `unstandardize`)


def unstandardize(x: torch.Tensor) -> torch.Tensor:
    shape = [1]*(x.ndim - 3) + [3, 1, 1]
    return x*x.new_tensor(_STD).view(shape) + x.new_tensor(_MEAN).view(shape)


class RecordingWriter:
    """Keeps what it is given: `images` [(key, tensor, step)], `texts` [(key, str, step)]."""
    def __init__(self): self.images, self.texts = [], []
    def add_images(self, key, tensor, step): self.images.append((key, tensor, step))
    def add_text(self, key, text, step): self.texts.append((key, text, step))


class NpyWriter:
    """`dir/<key with '/' as '-'>_<step:06>.npy` per image grid (1,3,H,W) float32, and one line of `dir/text.jsonl` per text."""
    def __init__(self, dir):
        self.dir = Path(dir)
        self.dir.mkdir(parents=True, exist_ok=True)

    def add_images(self, key, tensor, step):
        np.save(self.dir/f'{key.replace("/", "-")}_{int(step):06}.npy', tensor.detach().to(torch.float32).cpu().numpy())

    def add_text(self, key, text, step):
        with open(self.dir/'text.jsonl', 'a') as f: f.write(json.dumps({'key': key, 'step': int(step), 'text': text}) + '\n')


class TensorBoardWriter:
    """A `SummaryWriter` behind the two methods; ImportError at construction where `torch.utils.tensorboard` does not import."""
    def __init__(self, dir):
        try: from torch.utils.tensorboard import SummaryWriter
        except ImportError as e: raise ImportError(f'TensorBoardWriter needs torch.utils.tensorboard, which needs the tensorboard package ({e}); NpyWriter has no dependencies') from e
        self.writer = SummaryWriter(str(dir))

    def add_images(self, key, tensor, step): self.writer.add_images(key, tensor.detach().clamp(0, 1).cpu(), global_step=step)
    def add_text(self, key, text, step): self.writer.add_text(key, text, global_step=step)


class HeavyLogger:
    """`HeavyLogger(n_imgs=6, n_cols=2)`: at most `n_imgs` images per grid, `n_cols` per row (heavy_logger.py:25-27)."""
    def __init__(self, n_imgs: int = 6, n_cols: int = 2, writer=None, plain: bool = False):
        self.n, self.n_cols, self.writer, self.plain = n_imgs, n_cols, writer, plain
        self.mode, self.step = None, None

    # ---- the three operators, fused or plain
    def make_grid(self, x, **kw):
        """(b,1|3,h,w) -> (1,3,Hg,Wg) (heavy_logger.py:35-42)."""
        if self.plain: return viz.plain_make_grid(x.cpu(), self.n, self.n_cols, **kw)[None]      # on the host: a true division (ATen's GPU `div` by a number multiplies by its reciprocal)
        return viz.make_grid(x, self.n, self.n_cols, **kw)[None]

    def _disp(self, x, **kw): return viz.plain_rgb_from_disp(x, **kw).to(torch.float32) if self.plain else viz.rgb_from_disp(x, **kw)
    def _feat(self, x): return viz.plain_rgb_from_feat(x) if self.plain else viz.rgb_from_feat(x)

    def _key(self, k): return f'{self.mode}_{k}'
    def write_images(self, d):
        for k, v in d.items(): self.writer.add_images(self._key(k), v, self.step)
    def write_text(self, d):
        for k, v in d.items(): self.writer.add_text(self._key(k), v, self.step)

    @torch.no_grad()
    def log_step(self, module, batch, mode: str, step: int, writer=None) -> None:
        """One forward pass + losses of `batch` and the three logs (heavy_logger.py:75-88)."""
        if not getattr(module, 'want_aux', False): raise ValueError('the module was built without `trainer.log_images`: the losses keep no artefacts to log')
        self.mode, self.step = mode, step
        if writer is not None: self.writer = writer
        if self.writer is None: raise ValueError('no writer')
        _, loss_dict, fwd = module.step(tuple(dict(d) for d in batch), mode=mode)
        self.log_batch(batch); self.log_fwd(fwd); self.log_loss(loss_dict, batch[0]['supp_idxs'])

    def log_batch(self, batch) -> None:
        """The inputs (heavy_logger.py:90-131): augmented (train only) and plain images, LiDAR depth and depth hints where present, the items' names."""
        x, y, m = batch
        idxs = [int(i) for i in x['supp_idxs']]
        if self.mode == 'train':
            self.write_images({'imgs_aug/target': self.make_grid(unstandardize(x['imgs'])),
                               **{f'imgs_aug/supp_{i}': self.make_grid(unstandardize(v)) for i, v in zip(idxs, x['supp_imgs'])}})
        self.write_images({'imgs/target': self.make_grid(y['imgs']), **{f'imgs/supp_{i}': self.make_grid(v) for i, v in zip(idxs, y['supp_imgs'])}})
        if y.get('depth') is not None: self.write_images({'depth/lidar': self.make_grid(self._disp(y['depth'], invert=True))})
        if y.get('depth_hints') is not None: self.write_images({'depth/hints': self.make_grid(self._disp(y['depth_hints'], invert=True))})
        text = {'items': ' - '.join(m.get('items', []))}
        for key, src in (('items_original', 'items_original'), ('supp', 'supp'), ('errors', 'errors'), ('aug', 'augs')):
            if any(m.get(src, [])): text[key] = ' - '.join(m[src])
        self.write_text(text)

    def log_fwd(self, fwd) -> None:
        """The networks' outputs (heavy_logger.py:133-159); only the first support's mask is shown."""
        self.write_images({
            **{f'feats/target_{s}': self.make_grid(self._feat(f)) for s, f in enumerate(fwd.get('depth_feats', []))},
            **{f'disp/target_{s}': self.make_grid(self._disp(d)) for s, d in fwd['disp'].items()},
            **{f'disp/stereo_{s}': self.make_grid(self._disp(d)) for s, d in fwd.get('disp_stereo', {}).items()},
            **{f'masks/mask_0_{s}': self.make_grid(mk[:, 0][:, None]) for s, mk in fwd.get('mask', {}).items()},
            **{f'imgs/autoenc_{s}': self.make_grid(v) for s, v in fwd.get('autoenc_imgs', {}).items()},
            **{f'feats/autoenc_{s}': self.make_grid(self._feat(f)) for s, f in enumerate(fwd.get('autoenc_feats', []))}})

    def log_loss(self, loss_dict, supp_idxs) -> None:
        """The losses' artefacts (heavy_logger.py:161-210).  The stereo keys appear only when a handler was given stereo inputs."""
        idxs = [int(i) for i in supp_idxs]
        ld = loss_dict
        self.write_images({
            **{f'imgs_warp/supp_{i}': self.make_grid(v) for i, v in zip(idxs, ld.get('supp_imgs_warp', []))},
            **{f'imgs_warp/stereo_supp_{i}': self.make_grid(v) for i, v in zip(idxs, ld.get('stereo_supp_imgs_warp', []))},
            **{f'feats_warp/supp_{i}': self.make_grid(self._feat(v)) for i, v in zip(idxs, ld.get('supp_feats_warp', []))}})
        if ld.get('disps_warp') is not None:
            self.write_images({'disp/warp': self.make_grid(self._disp(ld['disps_warp'])), 'disp/stereo_warp': self.make_grid(self._disp(ld['stereo_disps_warp']))})
        for key, src in (('masks/automask', 'automask'), ('masks/stereo_automask', 'stereo_automask'), ('masks/hints', 'mask_regr')):
            if ld.get(src) is not None: self.write_images({key: self.make_grid(ld[src] if ld[src].dtype in (torch.bool, torch.uint8) else ld[src].float())})
        if 'image_grad' in ld:
            self.write_images({'grad/image': self.make_grid(ld['image_grad'], normalize=True), 'grad/disp': self.make_grid(ld['disp_grad'], normalize=True)})
        if 'stereo_image_grad' in ld:
            self.write_images({'grad/stereo_image': self.make_grid(ld['stereo_image_grad'], normalize=True),
                               'grad/stereo_disp': self.make_grid(ld['stereo_disp_grad'], normalize=True)})
