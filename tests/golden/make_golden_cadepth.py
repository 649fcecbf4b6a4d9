#!/usr/bin/env python3
"""Golden vectors for the CADepth decoder, made by IMPORTING the reference (build container only; see make_golden.py, whose import shim and writer are
reused here).

    PYTHONPATH=/root/reference python tests/golden/make_golden_cadepth.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/networks/decoders/cadepth.py:14-27    StructurePerception
  * src/networks/decoders/cadepth.py:30-46    DetailEmphasis(ch=12), train mode
  * src/networks/decoders/cadepth.py:49-126   CaDepthDecoder, train mode

The fixture files hold data only (inputs + expected outputs + lists of names); no reference source text is stored.
"""
import copy

import numpy as np
import torch

from make_golden import import_reference, save


def rel(a, r):
    return ((a.double() - r.double()).abs().max()/r.double().abs().max().clamp(min=1e-300)).item()


def run_structure_perception():
    from cadepth_inputs import sp_inputs, sp_out_grads
    from src.networks.decoders.cadepth import StructurePerception
    sp, rec = StructurePerception(), {}
    for k, (x, g) in enumerate(zip(sp_inputs(), sp_out_grads())):
        res = {}
        for dt in (torch.float32, torch.float64):
            leaf = x.to(dt).clone().requires_grad_(True)
            out = sp(leaf)
            (out*g.to(dt)).sum().backward()
            res[dt] = (out.detach(), leaf.grad)
        rec[f'in_x_{k}'] = x; rec[f'gout_{k}'] = g
        rec[f'out_{k}'], rec[f'grad_x_{k}'] = res[torch.float32]
        rec[f'meta_ref_fp32_vs_fp64_out_{k}'] = rel(res[torch.float32][0], res[torch.float64][0])
        rec[f'meta_ref_fp32_vs_fp64_grad_{k}'] = rel(res[torch.float32][1], res[torch.float64][1])
        print(f'op_structure_perception[{k}] {tuple(x.shape)}: reference fp32 vs fp64 out {rec[f"meta_ref_fp32_vs_fp64_out_{k}"]:.2e} grad {rec[f"meta_ref_fp32_vs_fp64_grad_{k}"]:.2e}')
    save('op_structure_perception', rec)


def run_detail_emphasis():
    from cadepth_inputs import cadepth_state
    from src.networks.decoders.cadepth import DetailEmphasis
    de = DetailEmphasis(ch=12).train()
    state = cadepth_state({k: tuple(v.shape) for k, v in de.state_dict().items()}, seed=94)
    de.load_state_dict(state, strict=True)
    g = torch.Generator().manual_seed(95)
    x, gout = torch.randn(3, 12, 5, 7, generator=g), torch.randn(3, 12, 5, 7, generator=g)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(de).to(dt)
        leaf = x.to(dt).clone().requires_grad_(True)
        out = m(leaf)
        (out*gout.to(dt)).sum().backward()
        res[dt] = (out.detach(), leaf.grad, {k: p.grad for k, p in m.named_parameters()}, {k: b.detach().clone() for k, b in m.named_buffers()})
    out, gx, gp, bufs = res[torch.float32]
    rec = {'in_x': x, 'gout': gout, 'out': out, 'grad_x': gx, 'meta_keys': np.array(sorted(state))}
    rec.update({f'in_state_{k}': v for k, v in state.items()})
    rec.update({f'gparam_{k}': v for k, v in gp.items()})
    rec.update({f'buf_{k}': v for k, v in bufs.items()})
    rec['meta_ref_fp32_vs_fp64_out'] = rel(out, res[torch.float64][0])
    rec['meta_ref_fp32_vs_fp64_grad'] = max([rel(gx, res[torch.float64][1])] + [rel(gp[k], res[torch.float64][2][k]) for k in gp if k != 'conv.0.bias'])
    save('op_detail_emphasis', rec)
    print(f'op_detail_emphasis: reference fp32 vs fp64 out {rec["meta_ref_fp32_vs_fp64_out"]:.2e} grad {rec["meta_ref_fp32_vs_fp64_grad"]:.2e}')


def run_decoder():
    """The reference decoder in train mode on two samples (`CADEPTH_BATCH`), recorded as `net_decoder_mask_64x96_*` is, except that the gradient w.r.t. the
    largest encoder feature (two thirds of all feature gradients) is stored in full on every second channel only and through per-(sample, channel) sums on
    all of them (`GFEAT_STEP`; `make_golden.save_compact` samples its large maps likewise): whole, it would make the file 1.3 MB, and a committed file stays under 1 MiB."""
    from cadepth_inputs import CADEPTH_BATCH, CADEPTH_KW, GFEAT_STEP, cadepth_state, gfeat_sample, gfeat_stats
    from exact_inputs import bit_checksum, decoder_feats, decoder_out_grads
    from src.networks.decoders.cadepth import CaDepthDecoder as RefDec
    dec = RefDec(**CADEPTH_KW).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    state = cadepth_state(shapes)
    holder.load_state_dict(state, strict=True)
    feats0, gouts = decoder_feats(seed=96, b=CADEPTH_BATCH), decoder_out_grads(seed=97, b=CADEPTH_BATCH)
    res = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(holder).to(dt)
        feats = [f.to(dt).clone().requires_grad_(True) for f in feats0]
        out = h.decoders['disp'](feats)
        sum((out[i]*gouts[i].to(dt)).sum() for i in out).backward()
        res[dt] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in feats], {k: p.grad for k, p in h.named_parameters()},
                   {k: b.detach().clone() for k, b in h.named_buffers()})
    out, gfeat, gp, bufs = res[torch.float32]
    o64, gf64, gp64, _ = res[torch.float64]
    pkeys = sorted(gp)
    rec = {'meta_keys': np.array(sorted(shapes)), 'meta_param_keys': np.array(pkeys), 'meta_batch': CADEPTH_BATCH,
           'chk_state': np.int64(sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32)),
           'chk_feats': np.int64(sum(bit_checksum(f) for f in feats0)), 'chk_gouts': np.int64(sum(bit_checksum(v) for v in gouts.values()))}
    for i, o in out.items(): rec[f'out_{i}'] = o
    for j, f in enumerate(gfeat):
        rec[f'gfeat_{j}'] = gfeat_sample(j, f).contiguous()
        if j in GFEAT_STEP: rec[f'gfeat_{j}_stats'] = gfeat_stats(f)
    stats = []
    for k in pkeys:
        gk = gp[k].double()
        stats.append([gk.sum().item(), gk.abs().sum().item()])
        if gk.numel() <= 5000: rec['gparam_' + k] = gp[k]
    rec['gparam_stats'] = np.array(stats)
    rec.update({f'buf_{k}': v for k, v in bufs.items()})
    rec['meta_ref_fp32_vs_fp64_out'] = max((out[i].double() - o64[i]).abs().max().item() for i in out)
    # (the bias of a convolution that feeds a training-mode BatchNorm has a zero gradient in exact arithmetic: rounding noise in both runs, no yardstick)
    rec['meta_ref_fp32_vs_fp64_grad'] = max([rel(a, b) for a, b in zip(gfeat, gf64)] + [rel(gp[k], gp64[k]) for k in pkeys if not k.endswith('.conv.0.bias')])
    save('net_decoder_cadepth_64x96', rec)
    print(f'net_decoder_cadepth_64x96: out_0 mean {out[0].mean().item():.6f} std {out[0].std().item():.6f} params {len(pkeys)} '
          f'reference fp32 vs fp64 out {rec["meta_ref_fp32_vs_fp64_out"]:.2e} grad {rec["meta_ref_fp32_vs_fp64_grad"]:.2e}')


def main():
    torch.set_num_threads(8)
    import_reference()
    run_structure_perception()
    run_detail_emphasis()
    run_decoder()


if __name__ == '__main__':
    main()
