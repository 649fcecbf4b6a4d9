"""Seeded inputs of the CADepth fixtures (`make_golden_cadepth.py` records with them, the tests regenerate them): `exact_inputs.decoder_state` with the
BatchNorm entries moved to where a BatchNorm lives (gain around 1, positive running variance, an integer batch counter), and the operator inputs."""
from __future__ import annotations

import torch

from exact_inputs import decoder_state

CADEPTH_KW = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32], out_sc=[0, 1, 2, 3], out_ch=1, out_act='sigmoid')
CADEPTH_BATCH = 2     # two samples: the training-mode BatchNorm statistics cross the batch
GFEAT_STEP = {0: 2}   # feature gradients recorded on every `step`-th channel only (key `gfeat_{j}`), the others through per-(sample, channel) sums (`gfeat_{j}_stats`)

SP_SHAPES = [(2, 24, 3, 5), (1, 40, 2, 3), (1, 7, 1, 1)]


def cadepth_state(shapes: dict, seed: int = 91) -> dict:
    """{key: tensor} for {key: shape} of a module with BatchNorm layers (keys ending in `conv.1.*`: the detail-emphasis normalisation)."""
    out = decoder_state(shapes, seed)
    for k, v in out.items():
        if k.endswith('num_batches_tracked'): out[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith('running_var'): out[k] = 0.5 + 5.0*v.abs()
        elif k.endswith('conv.1.weight'): out[k] = 1.0 + v
    return out


def gfeat_sample(j: int, grad: torch.Tensor) -> torch.Tensor:
    """The channels of the gradient w.r.t. encoder feature j that the decoder fixture holds in full."""
    return grad[:, ::GFEAT_STEP.get(j, 1)]


def gfeat_stats(grad: torch.Tensor) -> torch.Tensor:
    """(b, C, 2) in fp64: per sample and channel, the sum and the sum of magnitudes of a feature gradient."""
    g = grad.double()
    return torch.stack((g.sum((2, 3)), g.abs().sum((2, 3))), -1)


def sp_inputs(seed: int = 92) -> list:
    """The three structure-perception inputs: a spread softmax (Gaussian entries scaled by 1/sqrt(n)), a peaked one (post-ReLU entries of order 1), one pixel."""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for k, shape in enumerate(SP_SHAPES):
        x = torch.randn(shape, generator=g)
        xs.append(torch.relu(x) + 0.25*torch.rand(shape, generator=g) if k == 1 else x/float(shape[2]*shape[3])**0.5)
    return xs


def sp_out_grads(seed: int = 93) -> list:
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for shape in SP_SHAPES]
