#!/usr/bin/env python3
"""Golden vectors for the SuperDepth decoder, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are
reused here).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_superdepth.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/networks/decoders/superdepth.py:13-26    SubPixelConv
  * src/networks/decoders/superdepth.py:29-118   SuperdepthDecoder

The fixture files hold data only (inputs' checksums + expected outputs + lists of names); no reference source text is stored.
"""
import copy

import numpy as np
import torch
import torch.nn as nn

from make_golden import import_reference, save


def rel(a, r):
    return ((a.double() - r.double()).abs().max()/r.double().abs().max().clamp(min=1e-300)).item()


def run_subpixel():
    """The reference's `SubPixelConv` with the operators that stand around it in the decoder applied here — the `conv_block`'s bias and ELU in front, the
    ReLU or the head's sigmoid behind, `torch.cat` with the skip and the next convolution's `ReflectionPad2d(1)`: what `subpixel_conv` computes."""
    from exact_inputs import bit_checksum
    from src.networks.decoders.superdepth import SubPixelConv
    from superdepth_inputs import SUBPIXEL_CASES, SUBPIXEL_SATURATED, subpixel_case
    rec = {}
    for k, (B, C, Cs, h, w, r, pre, act, pad) in enumerate(SUBPIXEL_CASES):
        ins = subpixel_case(k)
        rec[f'chk_{k}'] = np.int64(sum(bit_checksum(t) for t in ins.values() if t is not None))
        res = {}
        for dt in (torch.float32, torch.float64):
            m = SubPixelConv(C, r).to(dt)
            with torch.no_grad(): m.conv.weight.copy_(ins['weight']); m.conv.bias.copy_(ins['bias'])
            lx = ins['x'].to(dt).clone().requires_grad_(True)
            lb = ins['pre_bias'].to(dt).clone().requires_grad_(True) if ins['pre_bias'] is not None else None
            ls = ins['skip'].to(dt).clone().requires_grad_(True) if ins['skip'] is not None else None
            u = lx if lb is None else lx + lb[None, :, None, None]
            if pre == 'elu': u = nn.ELU()(u)
            v = m(u)
            z = nn.ReLU()(v) if act == 'relu' else (nn.Sigmoid()(v) if act == 'sigmoid' else v)
            if ls is not None: z = torch.cat([z, ls], 1)
            out = nn.ReflectionPad2d(1)(z) if pad else z
            (out*ins['gout'].to(dt)).sum().backward()
            res[dt] = dict(out=out.detach(), grad_x=lx.grad, grad_weight=m.conv.weight.grad, grad_bias=m.conv.bias.grad, v=v.detach(), pre=(lx if lb is None else lx + lb[None, :, None, None]).detach())
            if lb is not None: res[dt]['grad_pre_bias'] = lb.grad
            if ls is not None: res[dt]['grad_skip'] = ls.grad
        v64, p64 = res[torch.float64].pop('v'), res[torch.float64].pop('pre')
        res[torch.float32].pop('v'); res[torch.float32].pop('pre')
        for name, t in res[torch.float32].items():
            rec[f'{name}_{k}'] = t
            rec[f'meta_ref_fp32_vs_fp64_{name}_{k}'] = rel(t, res[torch.float64][name])
        rec[f'meta_v_min_{k}'], rec[f'meta_v_max_{k}'], rec[f'meta_pre_min_{k}'] = v64.min().item(), v64.max().item(), p64.min().item()
        print(f'op_subpixel[{k}] {SUBPIXEL_CASES[k]}: v in [{v64.min().item():.3g}, {v64.max().item():.3g}] pre-activation min {p64.min().item():.3g}  reference fp32 vs fp64 ' +
              ' '.join(f'{n} {rec[f"meta_ref_fp32_vs_fp64_{n}_{k}"]:.1e}' for n in res[torch.float32]))
        if k == SUBPIXEL_SATURATED: assert rec[f'meta_v_min_{k}'] < -40 and rec[f'meta_v_max_{k}'] > 40 and rec[f'meta_pre_min_{k}'] < -50
    save('op_subpixel', rec)


def run_decoder():
    """The reference decoder on one sample with the ResNet-18 arguments of `net_decoder_64x96`: the four outputs, all feature gradients, parameter
    gradients in full up to 5000 elements and as (sum, sum of magnitudes) pairs for all, the state-dict key list."""
    from exact_inputs import bit_checksum, decoder_feats
    from src.networks.decoders.superdepth import SuperdepthDecoder as RefDec
    from superdepth_inputs import SUPERDEPTH_BATCH, SUPERDEPTH_KW, superdepth_out_grads, superdepth_state
    dec = RefDec(**SUPERDEPTH_KW).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    state = superdepth_state(shapes)
    holder.load_state_dict(state, strict=True)
    feats0 = decoder_feats(seed=108, b=SUPERDEPTH_BATCH)
    gouts = superdepth_out_grads(seed=109, b=SUPERDEPTH_BATCH)
    res = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(holder).to(dt)
        feats = [f.to(dt).clone().requires_grad_(True) for f in feats0]
        out = h.decoders['disp'](feats)
        sum((out[i]*gouts[i].to(dt)).sum() for i in out).backward()
        res[dt] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in feats], {k: p.grad for k, p in h.named_parameters() if p.requires_grad})
    out, gfeat, gp = res[torch.float32]
    o64, gf64, gp64 = res[torch.float64]
    pkeys = sorted(gp)
    rec = {'meta_keys': np.array(sorted(shapes)), 'meta_param_keys': np.array(pkeys), 'meta_batch': SUPERDEPTH_BATCH,
           'chk_state': np.int64(sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32)),
           'chk_feats': np.int64(sum(bit_checksum(f) for f in feats0)), 'chk_gouts': np.int64(sum(bit_checksum(v) for v in gouts.values()))}
    for i, o in out.items(): rec[f'out_{i}'] = o
    for j, f in enumerate(gfeat): rec[f'gfeat_{j}'] = f
    stats = []
    for k in pkeys:
        gk = gp[k].double()
        stats.append([gk.sum().item(), gk.abs().sum().item()])
        if gk.numel() <= 5000: rec['gparam_' + k] = gp[k]
    rec['gparam_stats'] = np.array(stats)
    rec['meta_ref_fp32_vs_fp64_out'] = max((out[i].double() - o64[i]).abs().max().item() for i in out)
    rec['meta_ref_fp32_vs_fp64_grad'] = max([rel(a, b) for a, b in zip(gfeat, gf64)] + [rel(gp[k], gp64[k]) for k in pkeys])
    save('net_decoder_superdepth_64x96', rec)
    print(f'net_decoder_superdepth_64x96: out_0 mean {out[0].mean().item():.6f} std {out[0].std().item():.6f} out_3 {tuple(out[3].shape)} keys {len(shapes)} params {len(pkeys)} '
          f'reference fp32 vs fp64 out {rec["meta_ref_fp32_vs_fp64_out"]:.2e} grad {rec["meta_ref_fp32_vs_fp64_grad"]:.2e}')


def main():
    torch.set_num_threads(8)
    import_reference()
    run_subpixel()
    run_decoder()


if __name__ == '__main__':
    main()
