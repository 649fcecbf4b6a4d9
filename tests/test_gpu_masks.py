"""GPU tests of predictive-mask training: the n-channel output heads (`smd_conv3x3_headn_*`), the multi-scale up-sampling (`smd_upsample_stack_*`), the
regularisers' reduction (`smd_scale_mean_*`) against fp64 torch on the same inputs; the trainer's post-process + loss phases against what the REFERENCE
produced with `fwd['mask']` present (`train_mask_*`, tests/golden/make_golden_masks.py); the mask decoder against the reference decoder; and the example
config end to end."""
import copy

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT, case_inputs, load_golden, parity_note, rel_to_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def _act64(z, act): return torch.sigmoid(z) if act == 'sigmoid' else (torch.relu(z) if act == 'relu' else z)


def _headn_inputs(B, C, n, h, w, act, gen):
    """relu: operands on a binary grid so that every pre-activation is an odd multiple of 1/512 (exact in fp32 and fp64, never within 1e-4 of the kink):
    the comparison then measures the kernel, not which side of zero two roundings fall; the other activations: Gaussian operands."""
    if act != 'relu':
        return (torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen), torch.randn(n, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5),
                torch.randn(n, device='cuda', generator=gen))
    xp = torch.round(torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen)*4)/4
    xp[:, 0] = 1/64                                                      # channel 0 contributes (1/64) x the sum of its nine weights ...
    wt = torch.round(torch.randn(n, C, 3, 3, device='cuda', generator=gen)*8)/8
    even = (torch.round(wt[:, 0].sum((1, 2))*8).long() % 2) == 0
    wt[even, 0, 1, 1] += 1/8                                             # ... an ODD multiple of 1/8: odd/512, every other term a multiple of 1/32
    bs = torch.round(torch.randn(n, device='cuda', generator=gen)*32)/32
    return xp, wt, bs


@pytest.mark.parametrize('B,C,h,w', [(2, 16, 50, 70), (1, 128, 24, 80), (3, 5, 2, 2), (2, 32, 17, 129), (1, 64, 96, 64), (12, 16, 192, 640)])
@pytest.mark.parametrize('act', ['sigmoid', 'relu', None])
@pytest.mark.parametrize('n', [2, 3, 4])
def test_conv3x3_headn_kernel(F, B, C, h, w, act, n):
    """`conv3x3_headn` against ATen's `conv2d` (+ activation) in fp64 on the same padded input: output and the three gradients within the one-channel head's
    bound (2e-6 of the tensor's max), with and without bias; the shapes of `test_conv3x3_head_kernel`."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w + n)
    xp, wt, bs = _headn_inputs(B, C, n, h, w, act, gen)
    gy = torch.randn(B, n, h, w, device='cuda', generator=gen)
    for bias in (bs, None):
        L = [t.clone().requires_grad_(True) for t in (xp, wt)] + ([bias.clone().requires_grad_(True)] if bias is not None else [])
        y = F.conv3x3_headn(L[0], L[1], L[2] if bias is not None else None, act)
        y.backward(gy)
        R = [t.double().clone().requires_grad_(True) for t in (xp, wt)] + ([bias.double().clone().requires_grad_(True)] if bias is not None else [])
        z = TF.conv2d(R[0], R[1], R[2] if bias is not None else None)
        if act == 'relu': assert (z.detach().abs() >= 1e-4).all(), 'a pre-activation of the fp64 reference lies within 1e-4 of the relu kink'
        yr = _act64(z, act)
        yr.backward(gy.double())
        assert y.shape == (B, n, h, w) and rel_to_max(y.double(), yr) <= 2e-6, rel_to_max(y.double(), yr)
        for nm, a, r in zip(('g_xp', 'g_weight', 'g_bias'), L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6, (nm, rel_to_max(a.grad.double(), r.grad))
    # only the weights ask for a gradient (a frozen encoder side), and only the input (every subset, bit for bit against the full backward: test_gpu_grad_subsets.py)
    L = [xp.clone(), wt.clone().requires_grad_(True)]
    F.conv3x3_headn(L[0], L[1], None, act).backward(gy); assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6
    L = [xp.clone().requires_grad_(True), wt.clone()]
    F.conv3x3_headn(L[0], L[1], None, act).backward(gy); assert rel_to_max(L[0].grad.double(), R[0].grad) <= 2e-6


def test_conv3x3_headn_refusals(F):
    xp, wt = torch.randn(1, 8, 10, 12, device='cuda'), torch.randn(5, 8, 3, 3, device='cuda')
    with pytest.raises(ValueError): F.conv3x3_headn(xp, wt, None, 'sigmoid')                  # n = 5
    with pytest.raises(ValueError): F.conv3x3_headn(xp, wt[:2, :4].contiguous(), None, 'relu')   # channel mismatch
    with pytest.raises(RuntimeError): F.conv3x3_headn(xp.cpu(), wt[:2].cpu(), None, 'relu')
    with pytest.raises(ValueError): F.conv3x3_head(xp, wt[:2].contiguous(), None, 'sigmoid')   # the one-channel entry keeps refusing wider weights


# (B, C, h, w), the smallest that reach each path: C < 8 -> the unsplit forward of 4 rows per thread, two tile columns, ragged last row group and column;
# the split forward of 2 rows, 22 row tiles -> 8 weight-gradient chunks with a short last one; the split forward of 1 row, even width (bf16: the dword reader);
# the same with an odd width (bf16: the element reader) and the data gradient's channel groups capped by C
@pytest.mark.parametrize('B,C,h,w', [(2, 4, 9, 70), (2, 8, 342, 130), (1, 16, 6, 8), (1, 8, 5, 7)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('act', ['sigmoid', None])
def test_conv3x3_head_and_headn_agree_bit_for_bit_on_one_channel(F, B, C, h, w, dtype, act):
    """`conv3x3_head` and `conv3x3_headn` with a (1, C, 3, 3) weight run the same kernels: output, `g_xp`, `g_weight` and `g_bias` are equal bit for bit,
    with and without bias, over an fp32 and a bf16 padded activation."""
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w)
    xp, wt, bs = _headn_inputs(B, C, 1, h, w, act, gen)
    xp = xp.to(dtype)
    gy = torch.randn(B, 1, h, w, device='cuda', generator=gen)
    for bias in (bs, None):
        runs = []
        for op in (F.conv3x3_head, F.conv3x3_headn):
            L = [t.clone().requires_grad_(True) for t in ((xp, wt) if bias is None else (xp, wt, bias))]
            y = op(L[0], L[1], None if bias is None else L[2], act)
            y.backward(gy)
            runs.append([y.detach()] + [t.grad for t in L])
        assert runs[0][1].dtype == dtype
        for nm, a, b in zip(('y', 'g_xp', 'g_weight', 'g_bias'), *runs): assert torch.equal(a, b), (nm, bias is not None, rel_to_max(a.double(), b.double()))


@pytest.mark.parametrize('B,C,h,w', [(2, 16, 50, 70), (12, 16, 192, 640), (1, 64, 24, 80)])
@pytest.mark.parametrize('act', ['sigmoid', 'relu'])
def test_conv3x3_headn_bf16_activation(F, B, C, h, w, act):
    """A bf16 padded activation (`SMD_HEADN_X_BF16`; the decoder under bf16 autocast): fp32 output and weight gradient against fp64 on the same rounded input
    (2e-6), `g_xp` back in bf16 (half an ulp: 4e-3 of the max) — the bounds of `test_conv3x3_head_bf16_activation`."""
    import torch.nn.functional as TF
    BF = torch.bfloat16
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w)
    xp, wt, bs = _headn_inputs(B, C, 2, h, w, act, gen)
    xp = xp.to(BF)      # (the binary grid of the relu inputs is exact in bf16 too)
    gy = torch.randn(B, 2, h, w, device='cuda', generator=gen)
    L = [xp.clone().requires_grad_(True), wt.clone().requires_grad_(True), bs.clone().requires_grad_(True)]
    y = F.conv3x3_headn(L[0], L[1], L[2], act); y.backward(gy)
    assert y.dtype == torch.float32 and L[0].grad.dtype == BF
    R = [t.double().clone().requires_grad_(True) for t in (xp, wt, bs)]
    z = TF.conv2d(R[0], R[1], R[2])
    if act == 'relu': assert (z.detach().abs() >= 1e-4).all()
    yr = _act64(z, act); yr.backward(gy.double())
    assert rel_to_max(y.double(), yr) <= 2e-6
    assert rel_to_max(L[0].grad.double(), R[0].grad) <= 4e-3
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6 and rel_to_max(L[2].grad.double(), R[2].grad) <= 2e-6


@pytest.mark.parametrize('b,n,size,sizes', [(2, 2, (48, 64), [(48, 64), (24, 32), (12, 16), (6, 8)]), (1, 3, (33, 47), [(33, 47), (17, 23), (5, 9), (1, 1)]),
                                            (3, 1, (25, 38), [(12, 19), (7, 5)]), (12, 2, (192, 640), [(192, 640), (96, 320), (48, 160), (24, 80)])])
def test_upsample_stack_matches_interpolate_and_its_adjoint(F, b, n, size, sizes):
    """`upsample_stack` against `F.interpolate(mode='bilinear', align_corners=False)` per scale in fp64: forward 1e-6 absolute on [0, 1] data, backward 2e-6 of
    the maximum, and the adjoint identity <U x, g> == <x, U^T g> accumulated in fp64; odd sizes, a scale already at the output size, one to three channels."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(b*100 + n)
    xs = [torch.rand(b, n, hs, ws, device='cuda', generator=gen) for hs, ws in sizes]
    g = torch.randn(len(sizes), b, n, *size, device='cuda', generator=gen)
    L = [x.clone().requires_grad_(True) for x in xs]
    up = F.upsample_stack(L, size)
    up.backward(g)
    R = [x.double().clone().requires_grad_(True) for x in xs]
    ref = torch.stack([TF.interpolate(r, size=size, mode='bilinear', align_corners=False) for r in R])
    ref.backward(g.double())
    assert up.shape == ref.shape and (up.double() - ref).abs().max().item() <= 1e-6
    for s, (a, r) in enumerate(zip(L, R)): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6, (s, rel_to_max(a.grad.double(), r.grad))
    lhs = (up.detach().double()*g.double()).sum().item()
    rhs = sum((x.double()*a.grad.double()).sum().item() for x, a in zip(xs, L))
    assert abs(lhs - rhs) <= 1e-6*(up.detach().double()*g.double()).abs().sum().item(), (lhs, rhs)   # (fp32 roundings of U x and U^T g: 6e-8 each, per term)
    with pytest.raises(ValueError): F.upsample_stack([xs[0], xs[0][:, :1].repeat(1, n + 1, 1, 1)], size)


@pytest.mark.parametrize('mode', ['bce_ones', 'identity', 'negate'])
def test_scale_mean_matches_fp64(F, mode):
    """Both forms of `scale_mean` against fp64 torch (loss 1e-6 relative, gradients 2e-6 of the maximum); the cross-entropy form with exact zeros (the
    logarithm's clamp: loss term 100, gradient -1e12 by ATen's backward) and an exact one; sizes off the 4096-element blocks; called twice (the workspace's
    arrival counter must be back at zero)."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(5)
    xs = [torch.sigmoid(3*torch.randn(sh, device='cuda', generator=gen)) for sh in [(12, 2, 96, 320), (2, 2, 33, 47), (1, 1, 1, 1), (3, 2, 64, 64)]]
    if mode == 'bce_ones': xs[1].view(-1)[[0, 5, 1000]] = 0.0; xs[3].view(-1)[7] = 1.0
    for _ in range(2):
        L = [x.clone().requires_grad_(True) for x in xs]
        loss = F.scale_mean(L, mode)
        (2.5*loss).backward()
        R = [x.double().clone().requires_grad_(True) for x in xs]
        if mode == 'bce_ones': ref = torch.stack([TF.binary_cross_entropy(r, torch.ones_like(r)) for r in R]).mean()
        else: ref = torch.stack([(r.mean() if mode == 'identity' else -r.mean()) for r in R]).mean()
        (2.5*ref).backward()
        assert abs(loss.item() - ref.item()) <= 1e-6*abs(ref.item()), (loss.item(), ref.item())
        for a, r in zip(L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6
    with pytest.raises(RuntimeError): F._ScaleMean.apply(0, xs[0].cpu())


def _noisy_backend(noise):
    """The product backend with the fixture's tie-break noise handed to `handlers.image_recon` (the reference drew it with `randn_like`)."""
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.trainer import HipLossBackend

    class Backend(HipLossBackend):
        def image_recon(self, crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks, want_warp=True, K_inv=None, prepared=None):
            return handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts.float(), Ks.float(), K_inv=K_inv, want_warp=want_warp, noise=noise)
    return Backend()


@pytest.mark.parametrize('name', ['train_mask_expl_48x64', 'train_mask_uncert_48x64'])
def test_trainer_phases_match_the_reference_with_predictive_masks(F, name):
    """`MonoDepthModule.forward_postprocess` + `forward_loss` on the HIP backend against the reference's own run of the same two phases with `fwd['mask']`
    present: `mask_up`, every `loss_*`, the total and the gradients w.r.t. every disparity, mask, rotation and translation.  Bounds: those of the small `train_*`
    parity tests on the un-fused path (losses 2e-5 relative, gradients 1e-3 of the maximum).  The fixtures record the reference's own fp32-vs-fp64 discrepancy on
    these inputs (printed below): 3e-5 / 6e-5 of the maximum, no min / automask decision differs — the bound is not set by near-ties."""
    import slowtv_monodepth_amd as amd
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    g = load_golden(name)
    leaves, static = case_inputs(g, device='cuda')
    scales, idxs, kind = static['scales'], static['supp_idxs'], str(g['meta_mask_name'])
    n, b = leaves['aa'].shape[:2]
    h, w = static['imgs'].shape[-2:]
    for s in scales: leaves[f'mask_{s}'] = g[f'in_mask_{s}'].cuda().clone().requires_grad_(True)
    loss_cfg = {'img_recon': {'weight': 1, 'loss_name': 'ssim', 'use_min': bool(g['meta_use_min']), 'use_automask': bool(g['meta_use_automask']), 'mask_name': kind},
                'disp_smooth': {'weight': float(g['meta_w_smooth']), 'use_edges': True}, 'disp_occ': {'weight': float(g['meta_w_occ'])}}
    if g['meta_w_mask'] > 0: loss_cfg['disp_mask'] = {'weight': float(g['meta_w_mask'])}
    cfg = {'net': {'depth': {'enc_name': 'resnet18', 'pretrained': False, 'mask_name': kind, 'num_ch_mask': n}}, 'loss': loss_cfg,
           'trainer': {'min_depth': 0.1, 'max_depth': 100}}
    m = MonoDepthModule(cfg, loss_backend=_noisy_backend(static['noise']))
    m.weights.cuda()
    m.synth = amd.geometry.ViewSynth((h, w))
    inv = torch.tensor([bool(g['meta_always_fwd_pose']) and i < 0 for i in idxs for _ in range(b)], dtype=torch.uint8).cuda()
    Ts = F.pose_matrices(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1), inv).unflatten(0, (n, b))
    fwd = {'disp': {s: leaves[f'disp_{s}'] for s in scales}, 'mask': {s: leaves[f'mask_{s}'] for s in scales}}
    for i, T in zip(idxs, Ts): fwd[f'T_{i}'] = T
    x = {'imgs': static['imgs'], 'supp_idxs': torch.tensor(idxs)}
    y = {'imgs': static['imgs'], 'supp_imgs': static['supp_imgs'], 'K': static['K']}
    fwd = m.forward_postprocess(fwd, x, y)
    assert fwd['mask_up'].stacked.shape == (len(scales), b, n, h, w)
    for s in scales: assert (fwd['mask_up'][s].detach().cpu() - g[f'out_mask_up_{s}']).abs().max().item() <= 1e-6, s
    loss, ld = m.forward_loss(fwd, x, y)
    loss.backward()
    report = [f'{name}: loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f}; reference fp32 vs fp64 on this fixture: loss {g["meta_ref_fp32_vs_fp64_loss"]:.1e}, '
              f'gradients {g["meta_ref_fp32_vs_fp64_grad"]:.1e}, automask flips {int(g["meta_ref_fp32_vs_fp64_automask_flips"])}']
    errs = {}
    for k in ['aa', 't'] + [f'disp_{s}' for s in scales] + [f'mask_{s}' for s in scales]: errs[k] = rel_to_max(leaves[k].grad.cpu(), g[f'grad_{k}'])
    report.append('  gradients (rel. to max): ' + ', '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    parity_note('\n'.join(report))
    for k in loss_cfg: torch.testing.assert_close(ld[f'loss_{k}'].detach().cpu(), g[f'out_loss_{k}'], rtol=2e-5, atol=1e-7, msg=lambda s, k=k: f'loss_{k}: {s}')
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    if g['meta_use_automask']:
        flips = (ld['automask'].cpu().reshape(-1) != g['out_automask'].bool().reshape(-1)).float().mean().item()
        assert flips <= 3e-3, f'automask differs on {flips:.2%} of pixels'
    for k, v in errs.items(): assert v < 1e-3, f'{name}: d loss / d {k} off by {v:.3e} (rel. to max) vs the reference autograd'


@pytest.mark.parametrize('act', ['sigmoid', 'relu'])
def test_mask_decoder_kernels_match_the_reference_decoder(F, act):
    """The reference's `MonodepthDecoder(out_ch=2, out_act=...)` — the mask decoder — through `_forward_glued` in fp32 (heads on `smd_conv3x3_headn_*`): outputs
    2e-5, gradients 2e-4, the bounds of tests/test_decoder_golden.py."""
    from exact_inputs import bit_checksum, decoder_state
    from slowtv_monodepth_amd.networks import checkpoint as ck
    from slowtv_monodepth_amd.networks.decoders import MonodepthDecoder
    g = load_golden(f'net_decoder_mask_64x96_{act}')
    with np.load(GOLDEN/f'net_decoder_mask_64x96_{act}.npz') as z: keys = [str(k) for k in z['meta_keys']]
    chs, scs = [64, 64, 128, 256, 512], [2, 4, 8, 16, 32]
    dec = MonodepthDecoder(num_ch_enc=chs, enc_sc=scs, out_sc=[0, 1, 2, 3], out_ch=2, out_act=act)
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'mask': dec})
    shapes = {k: tuple(v.shape) for k, v in ck.to_reference_state_dict(holder).items()}
    assert sorted(shapes) == keys
    state = decoder_state(shapes, seed=87)
    assert sum(bit_checksum(v) for v in state.values()) == int(g['chk_state'])
    ck.load_reference_state_dict(holder, state, strict=True)
    holder.cuda()
    gen = torch.Generator().manual_seed(88)
    feats = [torch.randn(1, c, 64//s, 96//s, generator=gen) for c, s in zip(chs, scs)]
    assert sum(bit_checksum(f) for f in feats) == int(g['chk_feats']), 'the seeded inputs are not the ones the fixture was made from'
    feats = [f.cuda().requires_grad_(True) for f in feats]
    out = dec._forward_glued(feats)
    sum((out[i]*g[f'gout_{i}'].cuda()).sum() for i in out).backward()
    for i in range(4):
        d = (out[i].detach().cpu() - g[f'out_{i}']).abs().max().item()
        assert out[i].shape[1] == 2 and d <= 2e-5, f'mask at scale {i}: {d:.2e}'
    for j, f in enumerate(feats):
        r = rel_to_max(f.grad.cpu(), g[f'gfeat_{j}'])
        assert r <= 2e-4, f'gradient w.r.t. encoder feature {j}: {r:.2e}'
    grads = {k: v for k, v in zip(ck.to_reference_state_dict(holder).keys(), (p.grad for p in holder.state_dict(keep_vars=True).values()))}
    stats = g['gparam_stats']
    for i, k in enumerate(keys):
        gk = grads[k].detach().double().cpu()
        if f'gparam_{k}' in g:
            r = rel_to_max(gk, g[f'gparam_{k}'].double())
            assert r <= 2e-4, f'gradient of {k}: {r:.2e}'
        assert abs(gk.abs().sum().item() - stats[i, 1].item()) <= 10*2e-4*stats[i, 1].item(), f'sum of |gradient| of {k}'


def _run_example(F, cfg, steps=2):
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    out = []
    for k in range(steps):
        batch = make_batch(2, 64, 96, (-1, 1), seed=42 + k, device='cuda')
        m.zero_grad(set_to_none=True)
        loss, ld, fwd = m.step(batch)
        loss.backward()
        out.append((loss.detach().clone(), {k_: v.detach().clone() for k_, v in ld.items() if k_.startswith('loss_')},
                    {k_: p.grad.detach().clone() for k_, p in m.named_parameters() if p.grad is not None}))
    return m, out, fwd


@pytest.mark.parametrize('kind', ['explainability', 'uncertainty'])
def test_example_config_trains_end_to_end(F, kind):
    """`cfg/kitti_sfm_learner.yaml` (and its uncertainty-mask form, without `disp_mask`) on a synthetic batch: two steps with backward — finite loss, the mask
    regulariser in `loss_dict`, a non-zero gradient in every parameter of the mask decoder, and bit-identical results from the same seed (wide convolutions
    pinned on the MFMA kernels — the 'auto' route may time its candidates — and MIOpen, which serves the encoders' strided convolutions, in its deterministic mode)."""
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_sfm_learner.yaml').read_text())
    if kind == 'uncertainty':
        cfg['net']['depth']['mask_name'] = cfg['loss']['img_recon']['mask_name'] = 'uncertainty'
        del cfg['loss']['disp_mask']
    F.set_conv_route('mfma')
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True    # the layers MIOpen serves (the encoders' strided convolutions): no atomically accumulated weight gradients
    try:
        m, run1, fwd = _run_example(F, cfg)
        _, run2, _ = _run_example(F, cfg)
    finally:
        F.set_conv_route('auto')
        torch.backends.cudnn.deterministic = det
    assert fwd['mask_up'].stacked.shape == (4, 2, 2, 64, 96) and set(fwd['mask']) == {0, 1, 2, 3}
    for (l1, ld1, g1), (l2, ld2, g2) in zip(run1, run2):
        assert torch.isfinite(l1) and ('loss_disp_mask' in ld1) == (kind == 'explainability')
        names = [k for k in g1 if k.startswith('nets.depth.decoders.mask.')]
        assert len(names) == 28
        for k in names: assert g1[k].abs().max() > 0, f'{k} got a zero gradient'
        assert torch.equal(l1, l2) and all(torch.equal(ld1[k], ld2[k]) for k in ld1)
        differ = [k for k in g1 if not torch.equal(g1[k], g2[k])]
        assert not differ, f'two runs from the same seed differ in {len(differ)} of {len(g1)} parameter gradients: {differ[:8]}'
