#!/usr/bin/env python3
"""Golden vectors for predictive-mask training, made by IMPORTING the reference (build container only; see make_golden.py, whose
import shim, input generator and writer are reused here).

    PYTHONPATH=/root/reference python tests/golden/make_golden_masks.py

Reference entry points driven here (paths relative to the reference checkout):
  * src/core/trainer.py:280-348, 350-472  MonoDepthModule.forward_postprocess / forward_loss with `fwd['mask']` present
    (mask up-sampling, the masked `img_recon`, `disp_smooth`, `disp_occ`, `disp_mask`)
  * src/core/handlers.py:314-347          disp_occ / disp_mask around src/regularizers/occlusion.py, mask.py
  * src/networks/decoders/monodepth.py    MonodepthDecoder(out_ch=2, out_act='sigmoid' | 'relu'): the mask decoder of src/networks/depth.py:108-114

The fixture files hold data only (inputs + expected outputs + lists of names); no reference source text is stored.
"""
import types

import numpy as np
import torch

from make_golden import import_reference, make_inputs, save

W_OCC, W_MASK, W_SMOOTH = 0.01, 0.2, 0.001


def mask_inputs(seed, kind, b, n, h, w, scales, zeros_at=None):
    """sigmoid(randn) for explainability masks, relu(randn) for uncertainty masks (about half the entries exactly 0: the relu kink).
    `zeros_at`: a scale of an explainability mask that gets a handful of exact zeros (the logarithm's clamp in `disp_mask`)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for s in scales:
        z = torch.randn(b, n, max(h >> s, 1), max(w >> s, 1), generator=g)
        m = torch.sigmoid(z) if kind == 'explainability' else torch.relu(z)
        if zeros_at == s: m.view(-1)[torch.randperm(m.numel(), generator=g)[:5]] = 0.0
        out[s] = m
    return out


def run_mask_trainer_case(R, name, *, seed, kind, use_min, use_automask, with_disp_mask, dtype=torch.float32, noise=None, quiet=False):
    from src.regularizers import MaskReg, OccReg
    b, h, w, n, scales, supp_idxs = 2, 48, 64, 2, [0, 1, 2, 3], [-1, 1]
    inp = make_inputs(seed, b, h, w, n, scales)
    masks = mask_inputs(seed + 3, kind, b, n, h, w, scales, zeros_at=2 if with_disp_mask else None)
    cast = lambda t: t.to(dtype)
    leaves = {f'disp_{s}': cast(d).clone().requires_grad_(True) for s, d in inp['disp'].items()}
    leaves.update({f'mask_{s}': cast(m).clone().requires_grad_(True) for s, m in masks.items()})
    aa, t = cast(inp['aa']).clone().requires_grad_(True), cast(inp['t']).clone().requires_grad_(True)
    leaves.update(aa=aa, t=t)
    Ts = R.T_from_AAt(aa=aa.flatten(0, 1), t=t.flatten(0, 1)).unflatten(0, (n, b))
    fwd = {'disp': {s: leaves[f'disp_{s}'] for s in scales}, 'mask': {s: leaves[f'mask_{s}'] for s in scales}}
    for i, T in zip(supp_idxs, Ts): fwd[f'T_{i}'] = T.inverse() if i < 0 else T
    y = {'imgs': cast(inp['imgs']), 'supp_imgs': cast(inp['supp_imgs']), 'K': cast(inp['K'])}
    x = {'imgs': y['imgs'], 'supp_idxs': torch.tensor(supp_idxs)}
    losses = {'img_recon': R.ReconstructionLoss(loss_name='ssim', use_min=use_min, use_automask=use_automask, mask_name=kind),
              'disp_smooth': R.SmoothReg(use_edges=True), 'disp_occ': OccReg()}
    weights = {'img_recon': torch.tensor(1.0), 'disp_smooth': torch.tensor(W_SMOOTH), 'disp_occ': torch.tensor(W_OCC)}
    if with_disp_mask: losses['disp_mask'] = MaskReg(); weights['disp_mask'] = torch.tensor(W_MASK)
    ns = types.SimpleNamespace(losses=losses, weights=weights, synth=R.ViewSynth((h, w)).to(dtype), timer=R.MultiLevelTimer(name='golden'),
                               to_depth=lambda d: R.to_scaled(d, 0.1, 100)[1])
    noise_log, orig = [], torch.randn_like

    def rec(tensor, *a, **k):
        out = noise.to(tensor) if noise is not None else orig(tensor, *a, **k)
        noise_log.append(out.clone()); return out

    torch.manual_seed(seed + 7)
    torch.randn_like = rec
    try:
        fwd = R.MonoDepthModule.forward_postprocess(ns, fwd, x, y)
        loss, ld = R.MonoDepthModule.forward_loss(ns, fwd, x, y)
    finally:
        torch.randn_like = orig
    loss.backward()
    out = {'loss': loss.detach(), 'ld': {k: v.detach() for k, v in ld.items()}, 'grads': {k: v.grad for k, v in leaves.items()},
           'noise': noise_log[0] if noise_log else None, 'mask_up': {s: v.detach() for s, v in fwd['mask_up'].items()}}
    if dtype != torch.float32: return out
    rec_ = {'meta_b': b, 'meta_h': h, 'meta_w': w, 'meta_n': n, 'meta_scales': np.array(scales), 'meta_supp_idxs': np.array(supp_idxs),
            'meta_always_fwd_pose': 1, 'meta_min_depth': 0.1, 'meta_max_depth': 100.0, 'meta_learn_K': 0, 'meta_w_smooth': W_SMOOTH, 'meta_w_occ': W_OCC,
            'meta_w_mask': W_MASK if with_disp_mask else -1.0, 'meta_loss_name': 'ssim', 'meta_use_min': int(use_min), 'meta_use_automask': int(use_automask),
            'meta_use_edges': 1, 'meta_mask_name': kind}
    rec_.update({f'in_{k}': v for k, v in inp.items() if k != 'disp'})
    rec_.update({f'in_disp_{s}': d for s, d in inp['disp'].items()})
    rec_.update({f'in_mask_{s}': m for s, m in masks.items()})
    if noise_log: rec_['in_noise'] = noise_log[0]
    rec_.update({f'out_mask_up_{s}': v for s, v in out['mask_up'].items()})
    rec_['out_loss'] = out['loss']
    for k, v in out['ld'].items():
        if k.startswith('loss_') or k == 'automask': rec_[f'out_{k}'] = v
    for k, v in out['grads'].items(): rec_[f'grad_{k}'] = v
    # the reference against itself in fp64 on the same inputs and the same tie-break noise: what fp32 arithmetic alone moves
    r64 = run_mask_trainer_case(R, name, seed=seed, kind=kind, use_min=use_min, use_automask=use_automask, with_disp_mask=with_disp_mask,
                                dtype=torch.float64, noise=out['noise'])
    flips = int((r64['ld']['automask'] != out['ld']['automask']).sum()) if use_automask else 0
    gerr = {k: ((out['grads'][k].double() - r64['grads'][k]).abs().max()/r64['grads'][k].abs().max()).item() for k in out['grads']}
    rec_['meta_ref_fp32_vs_fp64_grad'] = max(gerr.values())
    rec_['meta_ref_fp32_vs_fp64_loss'] = abs(out['loss'].item() - r64['loss'].item())/abs(r64['loss'].item())
    rec_['meta_ref_fp32_vs_fp64_automask_flips'] = flips
    save(name, rec_)
    print(f'{name}: loss={loss.item():.8f} ' + ' '.join(f'{k}={v.item():.6f}' for k, v in out['ld'].items() if v.ndim == 0))
    print(f'  reference fp32 vs fp64: loss rel {rec_["meta_ref_fp32_vs_fp64_loss"]:.2e}, worst gradient (rel. to max) {max(gerr.values()):.2e} '
          f'({max(gerr, key=gerr.get)}), automask decisions that differ: {flips} of {out["ld"]["automask"].numel() if use_automask else 0}')
    return out


def run_reg_cases(R):
    from src.regularizers import MaskReg, OccReg
    g = torch.Generator().manual_seed(515)
    shapes = [(2, 2, 24, 40), (2, 2, 12, 20), (2, 2, 6, 10), (2, 2, 3, 5)]
    masks = {s: torch.sigmoid(2*torch.randn(sh, generator=g)).requires_grad_(True) for s, sh in enumerate(shapes)}
    with torch.no_grad(): masks[1].view(-1)[[3, 77, 500]] = 0.0; masks[0].view(-1)[11] = 1.0     # the logarithm's clamp / an exact one
    loss, _ = R.handlers.disp_mask(MaskReg(), masks)
    loss.backward()
    rec = {'out_loss': loss}
    for s, m in masks.items(): rec[f'in_x_{s}'] = m; rec[f'grad_x_{s}'] = m.grad
    save('op_disp_mask', rec)
    print('op_disp_mask: loss', loss.item())
    disps = {s: torch.rand((sh[0], 1) + sh[2:], generator=g) for s, sh in enumerate(shapes)}
    rec = {f'in_x_{s}': d for s, d in disps.items()}
    for inv in (False, True):
        leaves = {s: d.clone().requires_grad_(True) for s, d in disps.items()}
        loss, _ = R.handlers.disp_occ(OccReg(invert=inv), leaves)
        loss.backward()
        rec[f'out_loss_invert{int(inv)}'] = loss
        for s, d in leaves.items(): rec[f'grad_x_{s}_invert{int(inv)}'] = d.grad
    save('op_disp_occ', rec)
    print('op_disp_occ: loss', rec['out_loss_invert0'].item(), rec['out_loss_invert1'].item())


MASK_DECODER_KW = dict(num_ch_enc=[64, 64, 128, 256, 512], enc_sc=[2, 4, 8, 16, 32], out_sc=[0, 1, 2, 3], out_ch=2)


def run_mask_decoder_cases(R):
    """The reference decoder with two output channels and either activation, recorded as `net_decoder_64x96` is (one sample: the feature gradients are most of the file)."""
    from exact_inputs import bit_checksum, decoder_state
    from src.networks.decoders.monodepth import MonodepthDecoder as RefDec
    for act in ('sigmoid', 'relu'):
        dec = RefDec(**MASK_DECODER_KW, out_act=act)
        holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'mask': dec})
        shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
        state = decoder_state(shapes, seed=87)
        holder.load_state_dict(state, strict=True)
        g = torch.Generator().manual_seed(88)
        feats = [torch.randn(1, c, 64//s, 96//s, generator=g).requires_grad_(True) for c, s in zip(MASK_DECODER_KW['num_ch_enc'], MASK_DECODER_KW['enc_sc'])]
        gouts = {i: torch.randn(1, 2, 64 >> i, 96 >> i, generator=g) for i in MASK_DECODER_KW['out_sc']}
        out = dec(feats)
        sum((out[i]*gouts[i]).sum() for i in out).backward()
        rec = {'meta_keys': np.array(sorted(shapes)), 'meta_act': act, 'chk_state': np.int64(sum(bit_checksum(v) for v in state.values())),
               'chk_feats': np.int64(sum(bit_checksum(f.detach()) for f in feats))}
        for i, o in out.items(): rec[f'out_{i}'] = o; rec[f'gout_{i}'] = gouts[i]
        for j, f in enumerate(feats): rec[f'gfeat_{j}'] = f.grad
        named = dict(holder.named_parameters())
        stats = []
        for k in sorted(shapes):
            gk = named[k].grad.double()
            stats.append([gk.sum().item(), gk.abs().sum().item()])
            if gk.numel() <= 5000: rec['gparam_' + k] = named[k].grad
        rec['gparam_stats'] = np.array(stats)
        save(f'net_decoder_mask_64x96_{act}', rec)
        print(f'net_decoder_mask_64x96_{act}: out_0 mean', out[0].mean().item(), 'zeros', int((out[0] == 0).sum()), 'params', len(shapes))


def main():
    torch.set_num_threads(8)
    R = import_reference()
    # (seed: one at which the reference's own fp32 run and its fp64 run on the same inputs take the same min / automask decisions everywhere — with 61 or 66 a
    # near-tie of the two supports moves a mask gradient by 2e-3 / 4e-2 of its maximum between the two precisions, more than the parity bound itself)
    run_mask_trainer_case(R, 'train_mask_expl_48x64', seed=64, kind='explainability', use_min=True, use_automask=True, with_disp_mask=True)
    run_mask_trainer_case(R, 'train_mask_uncert_48x64', seed=62, kind='uncertainty', use_min=False, use_automask=False, with_disp_mask=False)
    run_reg_cases(R)
    run_mask_decoder_cases(R)


if __name__ == '__main__':
    main()
