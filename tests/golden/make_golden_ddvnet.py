#!/usr/bin/env python3
"""Golden vectors for the DDVNet decoder, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are
reused here).

    PYTHONPATH=/root/reference python tests/golden/make_golden_ddvnet.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/networks/decoders/utils.py            conv3x3 (reflection-padded)
  * src/networks/decoders/ddvnet.py:116-124   DDVNetDecoder.expected_disparity
  * src/networks/decoders/ddvnet.py:57-152    DDVNetDecoder

The fixture files hold data only (inputs + expected outputs + lists of names); no reference source text is stored.
"""
import copy

import numpy as np
import torch

from make_golden import import_reference, save


def rel(a, r):
    return ((a.double() - r.double()).abs().max()/r.double().abs().max().clamp(min=1e-300)).item()


def run_head():
    """The head as the reference's forward does it (ddvnet.py:147-150): conv3x3, chunk per output channel, expected disparity of each."""
    from ddvnet_inputs import DDV_CASES, DDV_OVERFLOW, DDVNET_KW, ddv_case
    from exact_inputs import bit_checksum
    from src.networks.decoders.ddvnet import DDVNetDecoder
    from src.networks.decoders.utils import conv3x3
    rec = {}
    for k, (B, C, h, w, G, scale) in enumerate(DDV_CASES):
        x, weight, bias, gout = ddv_case(k)
        res = {}
        for dt in (torch.float32, torch.float64):
            dec = DDVNetDecoder(**{**DDVNET_KW, 'out_ch': G}).to(dt)
            conv = conv3x3(C, dec.num_bins*G).to(dt)
            with torch.no_grad(): conv.weight.copy_(weight); conv.bias.copy_(bias)
            leaf = x.to(dt).clone().requires_grad_(True)
            logits = conv(leaf)
            out = torch.cat([dec.expected_disparity(l) for l in logits.chunk(G, dim=1)], dim=1)
            (out*gout.to(dt)).sum().backward()
            res[dt] = (out.detach(), leaf.grad, conv.weight.grad, conv.bias.grad, logits.detach())
        if k == DDV_OVERFLOW: assert (res[torch.float64][4].max() - res[torch.float64][4].min()).item() > 88
        rec[f'chk_{k}'] = np.int64(sum(bit_checksum(t) for t in (x, weight, bias, gout)))      # (the inputs are regenerated from their seeds: ddvnet_inputs.ddv_case)
        for name, a, r in zip(('out', 'grad_x', 'grad_w', 'grad_b'), res[torch.float32], res[torch.float64]):
            rec[f'{name}_{k}'] = a
            rec[f'meta_ref_fp32_vs_fp64_{name}_{k}'] = rel(a, r)
        rec[f'meta_logit_span_{k}'] = (res[torch.float64][4].max() - res[torch.float64][4].min()).item()
        print(f'op_ddv_head[{k}] {DDV_CASES[k]}: logit span {rec[f"meta_logit_span_{k}"]:.1f}  reference fp32 vs fp64 ' +
              ' '.join(f'{n} {rec[f"meta_ref_fp32_vs_fp64_{n}_{k}"]:.2e}' for n in ('out', 'grad_x', 'grad_w', 'grad_b')))
    save('op_ddv_head', rec)


def run_decoder():
    """The reference decoder on one sample with the ResNet-18 arguments of `net_decoder_64x96`: the four outputs, all feature gradients, parameter
    gradients in full up to 5000 elements and as (sum, sum of magnitudes) pairs for all."""
    from ddvnet_inputs import DDVNET_BATCH, DDVNET_KW, ddvnet_state
    from exact_inputs import bit_checksum, decoder_feats, decoder_out_grads
    from src.networks.decoders.ddvnet import DDVNetDecoder as RefDec
    dec = RefDec(**DDVNET_KW).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    state = ddvnet_state(shapes)
    holder.load_state_dict(state, strict=True)
    feats0, gouts = decoder_feats(seed=98, b=DDVNET_BATCH), decoder_out_grads(seed=99, b=DDVNET_BATCH)
    res = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(holder).to(dt)
        feats = [f.to(dt).clone().requires_grad_(True) for f in feats0]
        out = h.decoders['disp'](feats)
        sum((out[i]*gouts[i].to(dt)).sum() for i in out).backward()
        res[dt] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in feats], {k: p.grad for k, p in h.named_parameters() if p.requires_grad},
                   {i: tuple(l.shape) for i, l in h.decoders['disp'].logits.items()})
    out, gfeat, gp, lshapes = res[torch.float32]
    o64, gf64, gp64, _ = res[torch.float64]
    pkeys = sorted(gp)
    rec = {'meta_keys': np.array(sorted(shapes)), 'meta_param_keys': np.array(pkeys), 'meta_batch': DDVNET_BATCH,
           'chk_state': np.int64(sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32)),
           'chk_feats': np.int64(sum(bit_checksum(f) for f in feats0)), 'chk_gouts': np.int64(sum(bit_checksum(v) for v in gouts.values()))}
    for i, o in out.items(): rec[f'out_{i}'] = o
    for i, s in lshapes.items(): rec[f'shape_logits_{i}'] = np.array(s)
    for j, f in enumerate(gfeat): rec[f'gfeat_{j}'] = f
    stats = []
    for k in pkeys:
        gk = gp[k].double()
        stats.append([gk.sum().item(), gk.abs().sum().item()])
        if gk.numel() <= 5000: rec['gparam_' + k] = gp[k]
    rec['gparam_stats'] = np.array(stats)
    rec['meta_ref_fp32_vs_fp64_out'] = max((out[i].double() - o64[i]).abs().max().item() for i in out)
    rec['meta_ref_fp32_vs_fp64_grad'] = max([rel(a, b) for a, b in zip(gfeat, gf64)] + [rel(gp[k], gp64[k]) for k in pkeys])
    save('net_decoder_ddvnet_64x96', rec)
    print(f'net_decoder_ddvnet_64x96: out_0 mean {out[0].mean().item():.6f} std {out[0].std().item():.6f} params {len(pkeys)} '
          f'reference fp32 vs fp64 out {rec["meta_ref_fp32_vs_fp64_out"]:.2e} grad {rec["meta_ref_fp32_vs_fp64_grad"]:.2e}')


def main():
    torch.set_num_threads(8)
    import_reference()
    run_head()
    run_decoder()


if __name__ == '__main__':
    main()
