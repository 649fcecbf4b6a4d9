#!/usr/bin/env python3
"""Golden vectors for the DiffNet decoder, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are
reused here).

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_diffnet.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/networks/decoders/diffnet.py:21-47    ChannelAttention
  * src/networks/decoders/diffnet.py:50-74    AttentionBlock
  * src/networks/decoders/diffnet.py:77-146   DiffNetDecoder

The fixture files hold data only (inputs + expected outputs + lists of names); no reference source text is stored.
"""
import copy

import numpy as np
import torch
import torch.nn as nn

from make_golden import import_reference, save


def rel(a, r):
    return ((a.double() - r.double()).abs().max()/r.double().abs().max().clamp(min=1e-300)).item()


def run_fuse():
    """The reference's AttentionBlock with its convolution replaced by that convolution's reflection padding and its ReLU taken out: what
    `up_cat_gate_pad` computes.  Two modes per case: 'none' — x is the leaf; 'relu' — x = relu(a + bias), the previous block's tail (diffnet.py:67), with
    a and bias the leaves.  Also `pad(relu(a + bias))` by itself: what `relu_pad` computes."""
    from diffnet_inputs import FUSE_CASES, FUSE_SATURATED, fuse_case
    from exact_inputs import bit_checksum
    from src.networks.decoders.diffnet import AttentionBlock
    rec = {}
    for k, (B, Ca, Cs, h, w, scale) in enumerate(FUSE_CASES):
        a, bias, skip, w1, w2, gout = fuse_case(k)
        rec[f'chk_{k}'] = np.int64(sum(bit_checksum(t) for t in (a, bias, skip, w1, w2, gout)))      # (the inputs are regenerated from their seeds: diffnet_inputs.fuse_case)
        for mode in ('none', 'relu'):
            res = {}
            for dt in (torch.float32, torch.float64):
                blk = AttentionBlock(Ca, Cs, Ca)
                blk.layers[1], blk.layers[2] = nn.ReflectionPad2d(1), nn.Identity()
                blk = blk.to(dt)
                fc = blk.layers[0].fc
                with torch.no_grad(): fc[0].weight.copy_(w1); fc[2].weight.copy_(w2)
                la, lb, ls = (t.to(dt).clone().requires_grad_(True) for t in (a, bias, skip))
                x = nn.ReLU()(la + lb[None, :, None, None]) if mode == 'relu' else la
                out = blk(x, ls)
                (out*gout.to(dt)).sum().backward()
                gate = fc(blk.layers[0].avg_pool(torch.cat((torch.nn.functional.interpolate(x, scale_factor=2), ls), 1)).flatten(1)).sigmoid().detach()
                res[dt] = dict(out=out.detach(), grad_a=la.grad, grad_skip=ls.grad, grad_w1=fc[0].weight.grad, grad_w2=fc[2].weight.grad, gate=gate)
                if mode == 'relu': res[dt]['grad_bias'] = lb.grad
            for name, v in res[torch.float32].items():
                rec[f'{name}_{mode}_{k}'] = v
                rec[f'meta_ref_fp32_vs_fp64_{name}_{mode}_{k}'] = rel(v, res[torch.float64][name])
            g64 = res[torch.float64]['gate']
            rec[f'meta_gate_min_{mode}_{k}'], rec[f'meta_gate_max_{mode}_{k}'] = g64.min().item(), g64.max().item()
            print(f'op_diffnet_fuse[{k}] {FUSE_CASES[k]} {mode}: gate in [{g64.min().item():.3g}, {g64.max().item():.3g}]  reference fp32 vs fp64 ' +
                  ' '.join(f'{n} {rec[f"meta_ref_fp32_vs_fp64_{n}_{mode}_{k}"]:.1e}' for n in res[torch.float32]))
        if k == FUSE_SATURATED: assert rec[f'meta_gate_min_none_{k}'] < 1e-6 and rec[f'meta_gate_max_none_{k}'] > 1 - 1e-6
        res = {}
        for dt in (torch.float32, torch.float64):
            la, lb = (t.to(dt).clone().requires_grad_(True) for t in (a, bias))
            out = nn.ReflectionPad2d(1)(nn.ReLU()(la + lb[None, :, None, None]))
            (out*gout[:, :Ca, :h + 2, :w + 2].to(dt)).sum().backward()
            res[dt] = dict(pad_out=out.detach(), pad_grad_x=la.grad, pad_grad_bias=lb.grad)
        for name, v in res[torch.float32].items():
            rec[f'{name}_{k}'] = v
            rec[f'meta_ref_fp32_vs_fp64_{name}_{k}'] = rel(v, res[torch.float64][name])
    save('op_diffnet_fuse', rec)


def run_decoder():
    """The reference decoder on one sample with the ResNet-18 arguments of `net_decoder_64x96`: the four outputs, all feature gradients, parameter
    gradients in full up to 5000 elements and as (sum, sum of magnitudes) pairs for all, the state-dict key list."""
    from diffnet_inputs import DIFFNET_BATCH, DIFFNET_KW, diffnet_state
    from exact_inputs import bit_checksum, decoder_feats, decoder_out_grads
    from src.networks.decoders.diffnet import DiffNetDecoder as RefDec
    dec = RefDec(**DIFFNET_KW).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    state = diffnet_state(shapes)
    holder.load_state_dict(state, strict=True)
    feats0, gouts = decoder_feats(seed=98, b=DIFFNET_BATCH), decoder_out_grads(seed=99, b=DIFFNET_BATCH)
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
    rec = {'meta_keys': np.array(sorted(shapes)), 'meta_param_keys': np.array(pkeys), 'meta_batch': DIFFNET_BATCH,
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
    save('net_decoder_diffnet_64x96', rec)
    print(f'net_decoder_diffnet_64x96: out_0 mean {out[0].mean().item():.6f} std {out[0].std().item():.6f} keys {len(shapes)} params {len(pkeys)} '
          f'reference fp32 vs fp64 out {rec["meta_ref_fp32_vs_fp64_out"]:.2e} grad {rec["meta_ref_fp32_vs_fp64_grad"]:.2e}')


def main():
    torch.set_num_threads(8)
    import_reference()
    run_fuse()
    run_decoder()


if __name__ == '__main__':
    main()
