"""The fused Depth-Hints regression (csrc/smd_hints.hip) and what stands on it, on the GPU: `hints_regr` / `handlers.depth_regr_fused` against the REFERENCE's
fixtures (tests/golden/op_hints_regr.npz, train_hints_ms_24x32.npz; made by tests/golden/make_golden_hints.py), against `regression_loss` and the plain handler,
run-to-run bit equality, the shapes at which the kernel takes another path, the trainer on the stereo support, and this operator's own gradient-subset,
hostile-memory and value-edge cases.

Bounds.  The mask is a comparison of two photometric error maps: outside the band |err_pred - err_hint| < tau of the REFERENCE's maps (tau = twice the 2e-4 to
which test_gpu_parity.py holds the fused forward's error map; the fixture records it and asserts that at most 0.5 % of the pixels lie inside) it equals the
reference's.  With the reference's maps fed in, the mask is the reference's bit for bit and loss / gradient are held to `regression_loss`'s bounds on the
`op_regr_*` fixtures (test_gpu_parity.py::test_regression_loss_matches_reference: loss rtol 2e-6 atol 1e-7, gradient rtol 2e-5 atol 1e-8)."""
import copy
import functools

import pytest
import torch

from conftest import ROOT, case_inputs, load_golden, parity_note, rel_to_max
from hostile_memory import Arena, assert_finite, hostile

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = dict(rtol=2e-6, atol=1e-7), dict(rtol=2e-5, atol=1e-8)
MAX_NEAR = 5e-3


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available(): pytest.skip('no GPU')
    from slowtv_monodepth_amd import hints
    return hints


@functools.lru_cache(maxsize=None)
def fixture(): return load_golden('op_hints_regr')


def _tags(g):
    import numpy as np
    with np.load(ROOT/'tests'/'golden'/'op_hints_regr.npz') as z: return [str(t) for t in z['meta_cases']]


def _crit(tag):
    from slowtv_monodepth_amd.losses import RegressionLoss
    name = tag.replace('_auto', '').replace('_inv', '')
    return RegressionLoss(loss_name=name, invert='_inv' in tag, use_automask='_auto' in tag)


def _photo(loss_name='ssim', use_min=True):
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    return ReconstructionLoss(loss_name=loss_name, use_min=use_min, use_automask=True).compute_photo


@pytest.mark.parametrize('k', [0, 1])
def test_operator_matches_the_reference_fixture(H, k):
    """Every criterion, with and without invert and automask, at 24 x 32 (S = 4, b = 3, n = 3) and 33 x 47 (S = 2, b = 2, n = 1)."""
    g = fixture()
    S, b, h, w, n = (int(v) for v in g['meta_shapes'][k])
    tau = float(g['meta_tau'])
    p = lambda name: g[f's{k}_{name}']
    depth0, hints = p('in_depth').cuda(), p('in_hints').cuda()
    imgs, supp, Ts, K = p('in_imgs').cuda(), p('in_supp_imgs').cuda(), p('in_Ts').cuda(), p('in_K').cuda()
    e_pred, e_hint = p('mid_err_pred'), p('mid_err_hint')                                  # (S,b,1,h,w), (b,1,h,w)
    valid = (p('in_hints') > 0)[None].expand(S, b, 1, h, w)
    band = ((e_pred - e_hint[None]).abs() < tau) & valid
    assert band.float().mean().item() <= MAX_NEAR, 'the fixture keeps at most 0.5 % of its pixels within tau of a tie'
    err_ref = torch.cat((e_hint[None], e_pred)).cuda()
    own = H.hints_photo_errors(_photo().__self__, depth0.squeeze(2), hints.squeeze(1), imgs, supp, Ts, K)
    d_err = (own.cpu() - err_ref.cpu()).abs()
    assert d_err.max().item() <= 2e-4, 'the error stack [hints, depth_0 ..] against the reference\'s maps, slice by slice: the bound tau is derived from'
    parity_note(f'op_hints_regr shape {k}: |err - reference err| max {d_err.max():.2e}, > 2e-4 on {(d_err > 2e-4).float().mean():.2e} of the pixels; '
                f'{band.float().mean():.3%} of the pixels within tau of a tie')
    for tag in _tags(g):
        crit = _crit(tag)
        want_loss, want_grad, want_all = p(f'{tag}_out_loss'), p(f'{tag}_grad_depth'), p(f'{tag}_out_mask_all')
        # (1) the handler end to end: the mask against the reference's outside the tie band
        leaf = depth0.clone().requires_grad_(True)
        from slowtv_monodepth_amd import handlers
        l, ld = handlers.depth_regr_fused(crit, None, _photo(), {s: leaf[s] for s in range(S)}, hints, imgs, supp, Ts, K)
        assert ld['mask_regr'].dtype == torch.bool and tuple(ld['mask_regr'].shape) == (b, 1, h, w)
        l.backward(retain_graph=True)      # (the saved mask bits are read below)
        differs = ld['mask_regr'].cpu() != p(f'{tag}_out_mask_regr')
        assert not (differs & ~band[0]).any(), f'{tag}: the mask of scale 0 differs from the reference outside the tie band on {int((differs & ~band[0]).sum())} pixels'
        own_all = _mask_all(l, S, b, h, w)
        assert torch.equal(own_all[0], ld['mask_regr'].cpu())
        differs = own_all != want_all
        if not crit.use_automask: assert not differs.any()
        assert not (differs & ~band).any(), f'{tag}: the mask differs from the reference outside the tie band on {int((differs & ~band).sum())} pixels (all scales)'
        if not differs.any():      # the reference's mask at every scale: the handler's own loss and gradient at the regression bounds
            torch.testing.assert_close(l.detach().cpu(), want_loss, **LOSS_TOL, msg=lambda s: f'{tag} handler loss: {s}')
            torch.testing.assert_close(leaf.grad.cpu(), want_grad, **GRAD_TOL, msg=lambda s: f'{tag} handler g_depth: {s}')
        else: parity_note(f'op_hints_regr shape {k} {tag}: {int(differs.sum())} mask pixels inside the tie band differ from the reference')
        # (2) the reference's error maps in: the reference's mask bit for bit, loss and gradient to regression_loss's bounds
        leaf = depth0.clone().requires_grad_(True)
        name = tag.replace('_auto', '').replace('_inv', '')
        l, m0 = H.hints_regr(leaf, hints, err_ref if crit.use_automask else None, loss_name=name, invert=crit.invert)
        l.backward()
        assert torch.equal(m0.cpu(), p(f'{tag}_out_mask_regr')), tag
        torch.testing.assert_close(l.detach().cpu(), want_loss, **LOSS_TOL, msg=lambda s: f'{tag} loss: {s}')
        torch.testing.assert_close(leaf.grad.cpu(), want_grad, **GRAD_TOL, msg=lambda s: f'{tag} g_depth: {s}')
        if name != 'berhu': assert (leaf.grad.cpu()[~want_all] == 0).all(), 'no gradient outside the mask'      # (berHu: the element attaining the maximum may be outside)


def _mask_all(loss, S, b, h, w):
    """The kernel's mask of every scale, (S,b,1,h,w) bool, unpacked from the bit words the forward saved for its backward (bit 4 s + k of word g: scale s,
    pixel 4 g + k of the b*h*w pixels)."""
    bits = loss.grad_fn.saved_tensors[2].cpu().to(torch.int64) & 0xffffffff
    P = b*h*w
    pix = torch.arange(P)
    return torch.stack([((bits[pix//4] >> (4*s + pix % 4)) & 1).bool() for s in range(S)]).view(S, b, 1, h, w)


def _spy(monkeypatch, H):
    """Count the calls of the kernel's forward (`hints.hints_regr`): the trainer tests assert that the fused path ran, not merely the backend's method."""
    calls, real = [], H.hints_regr
    monkeypatch.setattr(H, 'hints_regr', lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _plain(crit, depth, hints):
    """`regression_loss(depth, hints expanded, hints > 0)`: what the fused operator computes with the automask off."""
    from slowtv_monodepth_amd import functional as F
    S = depth.shape[0]
    leaf = depth.clone().requires_grad_(True)
    tg = hints[None].expand(S, *hints.shape).contiguous()
    l, _ = F.regression_loss(leaf.flatten(0, 1), tg.flatten(0, 1), tg.flatten(0, 1) > 0, loss_name=crit.loss_name, invert=crit.invert)
    l.backward()
    return l.detach(), leaf.grad


@pytest.mark.parametrize('tag', ['l1', 'log_l1_inv', 'berhu', 'berhu_inv'])
def test_without_automask_it_is_regression_loss(H, tag):
    g = fixture()
    crit = _crit(tag)
    depth, hints = g['s0_in_depth'].cuda(), g['s0_in_hints'].cuda()
    runs = []
    for _ in range(2):
        leaf = depth.clone().requires_grad_(True)
        l, m0 = H.hints_regr(leaf, hints, None, loss_name=crit.loss_name, invert=crit.invert)
        l.backward()
        runs.append((l.detach().clone(), m0.clone(), leaf.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two consecutive runs are bit-equal'
    assert torch.equal(runs[0][1], hints > 0), 'the mask is hints > 0, bit for bit'
    l_ref, g_ref = _plain(crit, depth, hints)
    torch.testing.assert_close(runs[0][0], l_ref, **LOSS_TOL)
    torch.testing.assert_close(runs[0][2], g_ref, **GRAD_TOL)


def _random_case(S, b, h, w, n, seed, zero=None):
    from slowtv_monodepth_amd.synthetic import make_batch
    gen = torch.Generator().manual_seed(seed)
    _, y, _ = make_batch(b, h, w, tuple([-1, 1, 2][:n]), seed=seed)
    depth = 0.5 + 3*torch.rand(S, b, 1, h, w, generator=gen)
    hints = depth[0]*(1 + 0.2*(torch.randint(0, 2, (b, 1, h, w), generator=gen)*2 - 1))
    hints[torch.rand(b, 1, h, w, generator=gen) < 0.15] = 0
    if zero == 'sample': hints[0] = 0
    if zero == 'batch': hints[:] = 0
    aa, t = 0.005*torch.randn(n*b, 3, generator=gen), 0.03*torch.randn(n*b, 3, generator=gen)
    from slowtv_monodepth_amd import functional as F
    Ts = F.pose_matrices(aa.cuda(), t.cuda()).unflatten(0, (n, b))
    return depth.cuda(), hints.cuda(), y['imgs'].cuda(), y['supp_imgs'].cuda(), Ts, y['K'].cuda()


SHAPES = [(1, 1, 5, 7, 1), (4, 3, 24, 32, 3), (2, 2, 33, 47, 1), (3, 2, 17, 128, 3), (8, 1, 9, 16, 2)]
# (S,b,h,w,n): below one block | vector path | b*h*w % 4 != 0: element path with a ragged last group | more than one block | S = 8: the error stack takes two
# reconstruction calls (9 slices) and the mask word is full (bit 31)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('zero', [None, 'sample', 'batch'])
def test_shapes_against_the_plain_handler(H, shape, zero):
    """The fused handler against `handlers.depth_regr` on the same tensors: the mask may differ only where the plain handler's own two error maps are within tau
    of each other; with the plain handler's mask imposed (its error maps fed in) loss and gradient agree to the regression bounds.  One sample without hints;
    a whole batch without hints: NaN loss and a NaN gradient wherever the plain handler gives one."""
    from slowtv_monodepth_amd import handlers
    S, b, h, w, n = shape
    if zero == 'sample' and b == 1: zero = 'batch'      # (the only sample is the batch)
    depth, hints, imgs, supp, Ts, K = _random_case(*shape, seed=S*100 + w, zero=zero)
    for name, invert in (('log_l1', False), ('berhu', True)):
        from slowtv_monodepth_amd.losses import RegressionLoss
        crit, photo = RegressionLoss(name, invert=invert, use_automask=True), _photo()
        leaf_p = depth.clone().requires_grad_(True)
        l_p, ld_p = handlers.depth_regr(crit, None, photo, {s: leaf_p[s] for s in range(S)}, hints, imgs, supp, Ts, K)
        l_p.backward()
        leaf_f = depth.clone().requires_grad_(True)
        l_f, ld_f = handlers.depth_regr_fused(crit, None, photo, {s: leaf_f[s] for s in range(S)}, hints, imgs, supp, Ts, K)
        l_f.backward(retain_graph=True)      # (the saved mask bits are read below)
        # the plain handler's own error maps (the same two calls it makes), to find its near-ties and to impose its mask
        with torch.no_grad():
            from slowtv_monodepth_amd import functional as F
            K_inv = F.inv_intrinsics(K)
            _, _, _, dep, im, src, T, Kx, Ki = handlers._expand_views({s: depth[s] for s in range(S)}, imgs, supp, Ts, K, K_inv)
            ex = lambda z: z[None].expand(n, *z.shape).flatten(0, 1)
            tg = hints[None].expand(S, *hints.shape).flatten(0, 1).contiguous()
            e_h = photo(F.view_synth(src.flatten(0, 1), ex(tg), T, Kx, Ki)[0].unflatten(0, (n, S*b)), im).unflatten(0, (S, b))
            e_p = photo(F.view_synth(src.flatten(0, 1), ex(dep), T, Kx, Ki)[0].unflatten(0, (n, S*b)), im).unflatten(0, (S, b))
        band0 = ((e_p[0] - e_h[0]).abs() < 4e-4) & (hints > 0)
        differs = ld_f['mask_regr'] != ld_p['mask_regr']
        assert not (differs & ~band0).any(), (shape, name, int((differs & ~band0).sum()))
        leaf_i = depth.clone().requires_grad_(True)
        l_i, m_i = H.hints_regr(leaf_i, hints, torch.cat((e_h[:1], e_p)), loss_name=name, invert=invert)
        l_i.backward(retain_graph=True)
        assert torch.equal(m_i, ld_p['mask_regr'])
        plain_all = ((hints > 0)[None] & (e_p > e_h)).cpu()
        assert torch.equal(_mask_all(l_i, S, b, h, w), plain_all), 'with the plain handler\'s error maps: its mask at every scale'
        band_all = (((e_p - e_h).abs() < 4e-4) & (hints > 0)[None]).cpu()
        differs_all = _mask_all(l_f, S, b, h, w) != plain_all
        assert not (differs_all & ~band_all).any(), (shape, name, int((differs_all & ~band_all).sum()))
        if zero == 'batch':
            assert torch.isnan(l_f) and torch.isnan(l_p) and torch.isnan(l_i)
            assert torch.equal(torch.isnan(leaf_i.grad), torch.isnan(leaf_p.grad)) and torch.equal(torch.isnan(leaf_f.grad), torch.isnan(leaf_p.grad))
            assert torch.isnan(leaf_p.grad).any()
            continue
        assert torch.isfinite(l_f) and torch.isfinite(leaf_f.grad).all()
        if zero == 'sample': assert not ld_f['mask_regr'][0].any() and (leaf_f.grad[:, 0] == 0).all()
        torch.testing.assert_close(l_i.detach(), l_p.detach(), **LOSS_TOL)
        torch.testing.assert_close(leaf_i.grad, leaf_p.grad, **GRAD_TOL)
        if not differs_all.any():      # the handler end to end (its own error stack) against the plain handler, in value
            torch.testing.assert_close(l_f.detach(), l_p.detach(), **LOSS_TOL)
            torch.testing.assert_close(leaf_f.grad, leaf_p.grad, **GRAD_TOL)


def test_berhu_maximum_on_a_masked_out_pixel(H):
    """berHu's threshold is 0.2 * max|diff| over ALL elements: the largest difference sits on a pixel without a hint and still sets it."""
    depth, hints, *_ = _random_case(2, 2, 9, 13, 1, seed=5)
    hints[1, 0, 4, 6] = 0.0; depth[1, 1, 0, 4, 6] = 500.0            # |500 - 0|: far above every other difference, on a masked-out pixel
    from slowtv_monodepth_amd.losses import RegressionLoss
    leaf = depth.clone().requires_grad_(True)
    l, m0 = H.hints_regr(leaf, hints, None, loss_name='berhu')
    l.backward()
    l_ref, g_ref = _plain(RegressionLoss('berhu'), depth, hints)
    torch.testing.assert_close(l.detach(), l_ref, **LOSS_TOL)
    torch.testing.assert_close(leaf.grad, g_ref, **GRAD_TOL)
    moved = depth.clone(); moved[1, 1, 0, 4, 6] = 5.0
    assert H.hints_regr(moved, hints, None, loss_name='berhu')[0] != l.detach()


def test_served_and_plain_paths(H):
    """What the fused handler declines runs the plain one: an `l2` photometric criterion, a predictive-mask criterion, poses that require a gradient."""
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.losses import ReconstructionLoss, RegressionLoss
    depth, hints, imgs, supp, Ts, K = _random_case(2, 2, 9, 13, 2, seed=9)
    depths = {s: depth[s] for s in range(2)}
    crit = RegressionLoss('log_l1', use_automask=True)
    assert H.served(crit, _photo(), depths, hints, imgs, supp, Ts, K)
    assert H.served(crit, _photo('l1', False), depths, hints, imgs, supp, Ts, K)
    assert not H.served(crit, ReconstructionLoss('l2').compute_photo, depths, hints, imgs, supp, Ts, K)
    assert not H.served(crit, ReconstructionLoss(mask_name='explainability').compute_photo, depths, hints, imgs, supp, Ts, K)
    assert not H.served(crit, (lambda p, t: None), depths, hints, imgs, supp, Ts, K)
    assert not H.served(crit, _photo(), depths, hints, imgs, supp, Ts.clone().requires_grad_(True), K)
    assert not H.served(crit, _photo(), depths, hints, imgs, supp, Ts, K.clone().requires_grad_(True))
    assert not H.served(crit, _photo(), depths, hints.double(), imgs, supp, Ts, K)
    assert not H.served(crit, _photo(), depths, hints, imgs[:, :2], supp, Ts, K)
    assert H.served(RegressionLoss('l1'), None, depths, hints, None, None, None, None), 'without the automask nothing but depths and hints is read'
    a = handlers.depth_regr_fused(crit, None, _photo(), depths, hints, imgs, supp, Ts.clone().requires_grad_(True), K)
    b = handlers.depth_regr(crit, None, _photo(), depths, hints, imgs, supp, Ts, K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1]['mask_regr'], b[1]['mask_regr'])
    # l1 photometric criterion, mean over the supports: the error stack follows the criterion
    l, ld = handlers.depth_regr_fused(crit, None, _photo('l1', False), depths, hints, imgs, supp, Ts, K)
    lp, ldp = handlers.depth_regr(crit, None, _photo('l1', False), depths, hints, imgs, supp, Ts, K)
    assert (ld['mask_regr'] != ldp['mask_regr']).float().mean().item() <= 5e-2 and abs(l.item() - lp.item()) <= 5e-2*abs(lp.item())      # (a sanity bound: other flags would move half the mask)


# ------------------------------------------------------------------------------------------------- trainer
def test_trainer_phases_match_the_reference_with_a_stereo_support(H, monkeypatch):
    """train_hints_ms_24x32: `MonoDepthModule.forward_postprocess` + `forward_loss` (the two phases of `step` behind the networks, which a 24 x 32 frame is too
    small for) on `HipLossBackend` against the reference's run of the same two phases: supports [-1, 1, 0], `T_stereo` of both signs stacked at the position of
    the 0, `depth_regr` through the fused handler.  Bounds of the small `train_*` GPU tests: losses 2e-5 relative, gradients 1e-3 of their maximum; the
    regression mask equals the reference's on this fixture (asserted), so the same bounds hold for `depth_regr`.  The kernel's forward is spied on: the poses
    require a gradient here as they do in training, and the fused path must run all the same."""
    import slowtv_monodepth_amd as amd
    from slowtv_monodepth_amd import functional as F, handlers
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule
    g = load_golden('train_hints_ms_24x32')
    leaves, static = case_inputs(g, device='cuda')
    scales, idxs = static['scales'], static['supp_idxs']
    b, (h, w) = static['imgs'].shape[0], static['imgs'].shape[-2:]
    calls = []

    class Backend(HipLossBackend):
        def image_recon(self, crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks, want_warp=True, K_inv=None, prepared=None):
            return handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts.float(), Ks.float(), K_inv=K_inv, want_warp=want_warp, noise=static['noise'])

        def depth_regr(self, *a):
            calls.append(1); return super().depth_regr(*a)
    cfg = {'net': {'depth': {'enc_name': 'resnet18', 'pretrained': False}},
           'loss': {'img_recon': {'weight': 1, 'loss_name': 'ssim', 'use_min': True, 'use_automask': True}, 'disp_smooth': {'weight': float(g['meta_w_smooth']), 'use_edges': True},
                    'depth_regr': {'weight': float(g['meta_w_regr']), 'loss_name': 'log_l1', 'use_automask': True}}, 'trainer': {'min_depth': 0.1, 'max_depth': 100}}
    kernel_calls = _spy(monkeypatch, H)
    m = MonoDepthModule(cfg, loss_backend=Backend())
    m.weights.cuda()
    m.synth = amd.geometry.ViewSynth((h, w))
    inv = torch.tensor([i < 0 for i in idxs[:2] for _ in range(b)], dtype=torch.uint8).cuda()
    Ts = F.pose_matrices(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1), inv).unflatten(0, (2, b))
    fwd = {'disp': {s: leaves[f'disp_{s}'] for s in scales}}
    for i, T in zip(idxs[:2], Ts): fwd[f'T_{i}'] = T
    x = {'imgs': static['imgs'], 'supp_idxs': torch.tensor(idxs)}
    y = {'imgs': static['imgs'], 'supp_imgs': static['supp_imgs'], 'K': static['K'], 'T_stereo': g['in_T_stereo'].cuda(), 'depth_hints': g['in_hints'].cuda()}
    fwd = m.forward_postprocess(fwd, x, y)
    torch.testing.assert_close(fwd['Ts'].detach().cpu(), g['out_Ts'], rtol=1e-5, atol=1e-6)
    assert torch.equal(fwd['Ts'][2], y['T_stereo'])
    loss, ld = m.forward_loss(fwd, x, y)
    loss.backward()
    assert calls == [1] and kernel_calls == [1], 'the poses come from leaves that require a gradient, as in training: the kernel path ran all the same'
    assert fwd['Ts'].requires_grad
    tie = ((g['mid_err_pred'] - g['mid_err_hint']).abs() < float(g['meta_tau'])).unflatten(0, (len(scales), b))[0] & (g['in_hints'] > 0)
    differs = ld['mask_regr'].cpu() != g['out_mask_regr'].bool()
    flips = differs.float().mean().item()
    assert not (differs & ~tie).any() and float(g['meta_near']) <= MAX_NEAR      # (the fixture's share of near-ties, over the pixels of all four scales)
    errs = {k: rel_to_max(leaves[k].grad.cpu(), g[f'grad_{k}']) for k in ['aa', 't'] + [f'disp_{s}' for s in scales]}
    parity_note(f'train_hints_ms_24x32: loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f}; regression mask flips {flips:.2e} (all inside the tie band); gradients '
                + ', '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    for k in ('img_recon', 'disp_smooth'): torch.testing.assert_close(ld[f'loss_{k}'].detach().cpu(), g[f'out_loss_{k}'], rtol=2e-5, atol=1e-7)
    assert flips == 0, 'on this fixture no mask pixel differs from the reference\'s: the tight bounds hold without a condition'
    torch.testing.assert_close(ld['loss_depth_regr'].detach().cpu(), g['out_loss_depth_regr'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    for k, v in errs.items(): assert v < 1e-3, (k, v)


def test_one_synthetic_step_of_the_example_config(H, monkeypatch):
    from slowtv_monodepth_amd import io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_depth_hints.yaml')
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    batch = make_batch(2, 64, 96, [-1, 1, 0], seed=42, device='cuda', depth_hints=True)
    kernel_calls = _spy(monkeypatch, H)
    loss, ld, fwd = m.step(batch)
    loss.backward()
    assert kernel_calls == [1] and fwd['Ts'].requires_grad, 'the step ran smd_hints_regr_*, with poses that come out of the pose network'
    assert {k for k in ld if k.startswith('loss_')} == {f'loss_{k}' for k in cfg['loss']}
    assert torch.isfinite(loss) and all(torch.isfinite(ld[f'loss_{k}']) for k in cfg['loss'])
    assert ld['mask_regr'].dtype == torch.bool and ld['mask_regr'].any() and not ld['mask_regr'][-1, :, :32].any()
    assert torch.equal(fwd['Ts'][2], batch[1]['T_stereo']) and fwd['_pose_leaves'][3] == [-1, 1]
    for name in ('depth', 'pose'):
        grads = [p.grad for p in m.nets[name].parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads), name


# ------------------------------------------------------------------------------------------------- own-file cases
def _err_stack(S, b, h, w, seed):
    return torch.rand(S + 1, b, h, w, generator=torch.Generator().manual_seed(seed)).cuda()


def test_gradient_subsets(H):
    """`depth` frozen: no backward node, the same forward bits.  `g_loss` arriving as a strided view / scaled by a power of two: exactly that multiple."""
    depth, hints, *_ = _random_case(3, 2, 9, 14, 1, seed=21)
    err = _err_stack(3, 2, 9, 14, 3)
    for name in ('log_l1', 'berhu'):
        leaf = depth.clone().requires_grad_(True)
        l, m0 = H.hints_regr(leaf, hints, err, loss_name=name)
        l.backward()
        frozen, m1 = H.hints_regr(depth, hints, err, loss_name=name)
        assert not frozen.requires_grad and torch.equal(frozen, l.detach()) and torch.equal(m0, m1) and not m0.requires_grad
        buf = torch.tensor([[7.0, 0.5], [7.0, 7.0]], device='cuda')
        leaf2 = depth.clone().requires_grad_(True)
        H.hints_regr(leaf2, hints, err, loss_name=name)[0].backward(buf[0, 1])
        assert torch.equal(leaf2.grad, 0.5*leaf.grad)
        leaf3 = depth.clone().requires_grad_(True)
        (H.hints_regr(leaf3, hints, err, loss_name=name)[0]*buf.t()[1, 0]).backward()          # the scalar read through a transposed view
        assert torch.equal(leaf3.grad, 0.5*leaf.grad)
        # the 5-D forms the handler passes are views of the same operands
        l5, _ = H.hints_regr(depth, hints, err[:, :, None], loss_name=name)
        assert torch.equal(l5, frozen)


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('shape', [(4, 3, 24, 32), (2, 2, 33, 47)], ids=['vec', 'ragged'])
def test_hostile_memory(H, shift, shape):
    """Every operand in a guarded, poisoned block `shift` elements off its alignment, every buffer the operator allocates (block sums, loss, mask bytes, mask
    bits, gradient) served from the arena: the bits of the plain-memory run (shift 1 takes the element path, whose arithmetic and summation order are the
    vector path's), guards intact, every output fully overwritten."""
    S, b, h, w = shape
    depth, hints, *_ = _random_case(S, b, h, w, 1, seed=33)
    depth, hints, err = depth.squeeze(2), hints.squeeze(1), _err_stack(S, b, h, w, 4)
    for name, invert in (('log_l1', False), ('berhu', True)):
        for e in (err, None):
            leaf = depth.clone().requires_grad_(True)
            l0, m0 = H.hints_regr(leaf, hints, e, loss_name=name, invert=invert)
            l0.backward()
            arena = Arena()
            gd, gh, ge = arena.guarded(depth, shift), arena.guarded(hints, shift), (arena.guarded(e, shift) if e is not None else None)
            with hostile(arena, shift):
                x = gd.requires_grad_(True)
                l, m = H.hints_regr(x, gh, ge, loss_name=name, invert=invert)
                l.backward()
            assert_finite(l.detach(), f'{name} loss'); assert_finite(x.grad, f'{name} g_depth')
            assert torch.equal(l.detach(), l0.detach()) and torch.equal(m, m0) and torch.equal(x.grad, leaf.grad), (name, e is not None, shift)
            assert m.view(torch.uint8).max().item() <= 1, 'every mask byte written (the poison is 255)'
            arena.check()


def test_value_edges(H):
    """A hint equal to the prediction: sign(0) = 0, no gradient, no NaN (also under invert).  Hints of 1e-3 and 1e4.  Errors exactly tied: mask 0 (the comparison
    is `>`), also at +0 vs -0 and at equal infinities; an error that is NaN on either side: mask 0."""
    S, b, h, w = 2, 1, 3, 8
    depth = torch.full((S, b, h, w), 2.0, device='cuda')
    hints = torch.full((b, h, w), 2.0, device='cuda')
    hints[0, 0, :4] = torch.tensor([1e-3, 1e4, 2.0, 0.0], device='cuda')
    for name in ('l1', 'log_l1', 'berhu'):
        for invert in (False, True):
            leaf = depth.clone().requires_grad_(True)
            l, m0 = H.hints_regr(leaf, hints, None, loss_name=name, invert=invert)
            l.backward()
            assert torch.isfinite(l) and torch.isfinite(leaf.grad).all(), (name, invert)
            assert (leaf.grad[:, 0, 1:] == 0).all() and (leaf.grad[:, 0, 0, 2:] == 0).all(), 'equal operands and missing hints: exactly no gradient'
            assert (leaf.grad[:, 0, 0, :2] != 0).all(), 'hints of 1e-3 and 1e4 pull on the prediction'
            from slowtv_monodepth_amd.losses import RegressionLoss
            l_ref, g_ref = _plain(RegressionLoss(name, invert=invert), leaf.detach()[:, :, None], hints[:, None])
            torch.testing.assert_close(l.detach(), l_ref, **LOSS_TOL)
            torch.testing.assert_close(leaf.grad[:, :, None], g_ref, **GRAD_TOL)
    inf, nan = float('inf'), float('nan')
    e_hint = torch.tensor([0.25, 0.0, inf, 0.5, nan, 0.5, 0.25, 0.25], device='cuda')
    e_pred = torch.tensor([0.25, -0.0, inf, nan, 0.5, 0.5000001, 0.3, 0.2], device='cuda')
    want = torch.tensor([0, 0, 0, 0, 0, 1, 1, 0], dtype=torch.bool, device='cuda')
    err = torch.zeros(S + 1, b, h, w, device='cuda')
    err[0, 0, 1], err[1, 0, 1], err[2, 0, 1] = e_hint, e_pred, e_pred
    hints = torch.full((b, h, w), 3.0, device='cuda')
    l, m0 = H.hints_regr(depth, hints, err, loss_name='log_l1')
    assert torch.equal(m0[0, 0, 1], want) and not m0[0, 0, 0].any() and not m0[0, 0, 2].any(), 'ties (rows of equal zeros included) give mask 0'
    torch.testing.assert_close(l, torch.log(torch.tensor(2.0, device='cuda')), **LOSS_TOL)
