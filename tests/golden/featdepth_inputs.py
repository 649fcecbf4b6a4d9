"""Seeded inputs of the FeatDepth fixture (`op_featreg.npz`), shared by tests/golden/make_golden_featdepth.py and the tests."""
from __future__ import annotations

import torch

__all__ = ['FEAT_CASES', 'FEAT_WEIGHTS', 'feat_case', 'feat_expected', 'handler_case', 'AUTOENC_DECODER_KW', 'autoenc_decoder_state']

# (name, (b, c, h, w)): the smallest shapes at which the kernel can still go wrong.  3x3: every pixel touches a border; h = 1 / w = 1: one of the two directions does
# not exist; 2x2: the second-order differences see only padded zeros; 4x6: no whole four-column group fits its halo; 7x67: whole aligned groups are impossible
# (w % 4 = 3), a tail of 3 and two tiles along x; 64 channels at 6x10: two channel chunks.  `quant`: features in multiples of 1/4, so that many first- and
# second-order differences are exactly 0 (sign(0) = 0, the zero last row and column); `const`: both losses and the gradient are exactly 0.  `vec` (w % 4 == 0):
# the 16-byte path with its halos, over more than one tile in both directions.
FEAT_CASES = [('b2c3_3x3', (2, 3, 3, 3)), ('h1', (1, 1, 1, 5)), ('w1', (1, 2, 5, 1)), ('2x2', (2, 1, 2, 2)), ('4x6', (1, 3, 4, 6)), ('7x67', (2, 5, 7, 67)),
              ('c64', (1, 64, 6, 10)), ('quant', (2, 3, 5, 9)), ('const', (1, 2, 4, 6)), ('vec', (1, 2, 11, 136))]
FEAT_WEIGHTS = (0.75, 1.5)      # the weights of (peaky, smooth) in the recorded weighted sum


def feat_case(k: int):
    """-> dict(feat (b,c,h,w), img (b,3,h,w) in [0, 1])"""
    name, shape = FEAT_CASES[k]
    gen = torch.Generator().manual_seed(31000 + k)
    feat = torch.randn(*shape, generator=gen)
    img = torch.rand(shape[0], 3, *shape[2:], generator=gen)
    if name == 'quant': feat = (feat*2).round()/4
    if name == 'const': feat = torch.full(shape, 0.625)
    return dict(feat=feat, img=img)


def feat_expected(g: dict, k: int, edges: bool):
    """-> dict(l_peaky, l_smooth, g_peaky, g_smooth, g_both) of case k from the loaded fixture (the gradients are stored flat over the cases in order)."""
    numel = lambda j: FEAT_CASES[j][1][0]*FEAT_CASES[j][1][1]*FEAT_CASES[j][1][2]*FEAT_CASES[j][1][3]
    first, e = sum(numel(j) for j in range(k)), int(edges)
    out = {n: g[f'{n}_e{e}'][k] for n in ('l_peaky', 'l_smooth')}
    out.update({n: g[f'{n}_e{e}'][first:first + numel(k)].reshape(FEAT_CASES[k][1]) for n in ('g_peaky', 'g_smooth', 'g_both')})
    return out


def handler_case():
    """The `handlers.feat_smooth` case: two scales, n = 2 supports, b = 2.  -> dict(feats [..], imgs, supp_feats [..], supp_imgs)"""
    gen = torch.Generator().manual_seed(31500)
    shapes = [(4, 6, 10), (6, 3, 5)]
    return dict(feats=[torch.randn(2, *s, generator=gen) for s in shapes], imgs=torch.rand(2, 3, 12, 20, generator=gen),
                supp_feats=[torch.randn(2, 2, *s, generator=gen) for s in shapes], supp_imgs=torch.rand(2, 2, 3, 12, 20, generator=gen))


# the autoencoder's decoder: the Monodepth decoder WITHOUT skips and with three sigmoid channels (src/networks/autoencoder.py:45-49), on exact_inputs.decoder_feats()
AUTOENC_DECODER_KW = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32], upsample_mode='nearest', use_skip=False, out_sc=[0, 1, 2, 3], out_ch=3,
                          out_act='sigmoid')


def autoenc_decoder_state(shapes: dict) -> dict:
    from exact_inputs import decoder_state
    return decoder_state(shapes, seed=177)
