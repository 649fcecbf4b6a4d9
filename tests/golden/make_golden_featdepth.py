#!/usr/bin/env python3
"""Golden vectors for FeatDepth training, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are reused
here).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_featdepth.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/regularizers/smooth.py:100-176   FeatPeakReg, FeatSmoothReg
  * src/core/handlers.py:284-311         feat_smooth
  * src/networks/decoders/monodepth.py   MonodepthDecoder(use_skip=False, out_ch=3): the autoencoder's decoder (src/networks/autoencoder.py:45-49 builds it; the
                                         network itself needs timm, which is not in this image)

tests/golden/op_featreg.npz (read it with featdepth_inputs.feat_expected): `chk` the bit checksums of the seeded inputs of every case of
featdepth_inputs.FEAT_CASES; per `use_edges` e in {0, 1}: `l_peaky_e`, `l_smooth_e` (one value per case) and `g_peaky_e`, `g_smooth_e`, `g_both_e`, autograd's
feat.grad under each loss alone and under FEAT_WEIGHTS[0]*peaky + FEAT_WEIGHTS[1]*smooth, flattened and concatenated over the cases; `hd_*`: the handler case
(two scales, n = 2) for both criteria with use_edges, the loss and the gradients of every feature tensor; `dec_*`: the decoder's four reconstructions and its
feature gradients.  The fixture holds data only (checksums + expected outputs); no reference source text is stored."""
import numpy as np
import torch

from make_golden import import_reference, save


def main():
    torch.set_num_threads(1)
    import_reference()
    from src.core import handlers
    from src.networks.decoders.monodepth import MonodepthDecoder as RefDec
    from src.regularizers.smooth import FeatPeakReg, FeatSmoothReg
    from exact_inputs import bit_checksum, decoder_feats
    from featdepth_inputs import AUTOENC_DECODER_KW, FEAT_CASES, FEAT_WEIGHTS, autoenc_decoder_state, feat_case, handler_case
    rec = {'chk': []}
    flat = {f'{n}_e{e}': [] for e in (0, 1) for n in ('l_peaky', 'l_smooth', 'g_peaky', 'g_smooth', 'g_both')}
    for k, (name, shape) in enumerate(FEAT_CASES):
        ins = feat_case(k)
        rec['chk'].append(sum(bit_checksum(t) for t in ins.values()))
        for e in (0, 1):
            peaky, smooth = FeatPeakReg(use_edges=bool(e)), FeatSmoothReg(use_edges=bool(e))
            for tag, wp, ws in (('peaky', 1.0, 0.0), ('smooth', 0.0, 1.0), ('both', *FEAT_WEIGHTS)):
                x = ins['feat'].clone().requires_grad_(True)
                lp, ls = peaky(x, ins['img'])[0], smooth(x, ins['img'])[0]
                (lp if tag == 'peaky' else ls if tag == 'smooth' else wp*lp + ws*ls).backward()
                flat[f'g_{tag}_e{e}'].append(x.grad.reshape(-1))
            flat[f'l_peaky_e{e}'].append(lp.detach().reshape(1)); flat[f'l_smooth_e{e}'].append(ls.detach().reshape(1))
        print(f'feat_regs[{k}] {name} {shape}: peaky {lp.item():.6f} smooth {ls.item():.6f}')
    rec['chk'] = np.array(rec['chk'], dtype=np.int64)
    rec.update({n: torch.cat(v) for n, v in flat.items()})

    ins = handler_case()
    rec['hd_chk'] = np.int64(sum(bit_checksum(t) for v in ins.values() for t in (v if isinstance(v, list) else [v])))
    for tag, crit in (('peaky', FeatPeakReg(use_edges=True)), ('smooth', FeatSmoothReg(use_edges=True))):
        feats = [f.clone().requires_grad_(True) for f in ins['feats']]
        supp = [f.clone().requires_grad_(True) for f in ins['supp_feats']]
        l, ld = handlers.feat_smooth(crit, feats, ins['imgs'], supp, ins['supp_imgs'])
        assert ld == {}
        l.backward()
        rec[f'hd_{tag}_loss'] = l.detach()
        for s, (f, sf) in enumerate(zip(feats, supp)): rec[f'hd_{tag}_g_feat_{s}'], rec[f'hd_{tag}_g_supp_{s}'] = f.grad, sf.grad
        print(f'handlers.feat_smooth[{tag}]: {l.item():.6f}')

    dec = RefDec(**AUTOENC_DECODER_KW)
    holder = torch.nn.Module(); holder.decoder = dec
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    state = autoenc_decoder_state(shapes)
    holder.load_state_dict(state, strict=True)
    feats = [f.requires_grad_(True) for f in decoder_feats()]
    out = dec(feats)
    sum(o.sum() for o in out.values()).backward()
    rec['dec_keys'] = np.array(sorted(shapes))
    rec['dec_chk_state'] = np.int64(sum(bit_checksum(v) for v in state.values()))
    for i, o in out.items(): rec[f'dec_out_{i}'] = o[:, :, ::2, ::2] if i == 0 else o        # (scale 0 every second pixel: the fixture stays small)
    rec['dec_gfeat_4'] = feats[4].grad
    print('autoencoder decoder: out_0', tuple(out[0].shape), 'mean', out[0].mean().item(), 'keys', len(shapes))
    save('op_featreg', rec)


if __name__ == '__main__':
    main()
