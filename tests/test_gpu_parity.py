"""GPU parity: the HIP hot path (through the C ABI) against the CPU oracle and the reference's golden vectors.

Tolerances (fp32 path, stated per BASELINE.json: loss within 1e-4 relative of the reference):
  * scalar losses: 2e-5 relative (observed ~1e-6)
  * per-pixel error maps: 2e-4 absolute (SSIM amplifies 1e-6 warp rounding in flat windows), selection maps <= 0.3 % flips
  * gradients: 1e-3 of the tensor's max magnitude (fp32 sums over up to 10^6 pixels in a different order)
"""
import pytest
import torch

from conftest import TRAIN_CASES, TRAIN_CASES_BASELINE, case_inputs, parity_note, ref_map, rel_to_max
from oracle import view_synth_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def test_lane_shift_primitive(F):
    left, right = F.lane_shift_selftest()
    lanes = torch.arange(64, dtype=torch.float32)
    exp_left = (lanes - 1).clamp(min=0); exp_left[0] = 0
    exp_right = lanes + 1; exp_right[63] = 0
    assert torch.equal(left.cpu(), exp_left), f'lane_left wrong: {left.cpu().tolist()}'
    assert torch.equal(right.cpu(), exp_right), f'lane_right wrong: {right.cpu().tolist()}'


def oracle_run(g, leaves, Ts, K, static):
    """Oracle on CPU with Ts / K as leaves (so their gradients can be compared directly)."""
    disps = {s: leaves[f'disp_{s}'] for s in static['scales']}
    loss, out = O.loss_path(
        disps, static['imgs'], static['supp_imgs'], Ts, K,
        min_depth=g['meta_min_depth'] or None, max_depth=g['meta_max_depth'] or None,
        loss_name=g['meta_loss_name'], use_min=bool(g['meta_use_min']), use_automask=bool(g['meta_use_automask']),
        use_edges=bool(g['meta_use_edges']), w_smooth=g['meta_w_smooth'] if g['meta_w_smooth'] >= 0 else None,
        noise=static['noise'])
    return loss, out


def impose_reference_routing(g, sel, knobs):
    """Compact (BASELINE-resolution) fixtures, between forward and backward: overwrite the kernel's decision map (`sel`, the tensor its
    backward reads) with the REFERENCE's (`out_sel_all`), so that the gradients that follow are compared under identical routing.
    Among 0.5-1 M pixels a few dozen have two candidate errors within the error map's fp32 noise (observed gap <= 5e-5; the synthetic
    frames are integer shifts of one 8-bit scene, which makes near-ties common) and rounding decides them; each re-routes the gradient of
    its 3x3 window by percents.  -> the kernel's own map (for the flip count / tie proof).  (`.data`: the forward saved `sel` for its
    backward; this is a test aid, nothing in the product writes to it.  The forward's liveness table describes the map it wrote itself, so the
    backward is told to ignore it: knob `bwd_live` = 0.)"""
    knobs('bwd_live', 0)
    own = sel.clone()
    sel.data.copy_(g['out_sel_all'].reshape(sel.shape).to(sel.device))
    return own


_FP64_CACHE: dict = {}


def fp64_gradients_under_reference_routing(g, name):
    """The oracle's whole chain (aa, t, (fs, cs), disparities -> loss) in fp64 with the reference's decisions imposed: the yardstick for
    "how far from the exactly-rounded gradient is an fp32 implementation allowed to be" at BASELINE resolution.  Cached per fixture."""
    if name not in _FP64_CACHE:
        leaves, static = case_inputs(g, dtype=torch.float64)
        n, b = leaves['aa'].shape[:2]
        h, w = static['imgs'].shape[-2:]
        Ts = O.T_from_AAt(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1)).unflatten(0, (n, b))
        if g['meta_always_fwd_pose']: Ts = torch.stack([torch.linalg.inv(T) if i < 0 else T for i, T in zip(static['supp_idxs'], Ts)])
        K = O.resize_K(O.build_K(leaves['fs'], leaves['cs']), (h, w)) if g['meta_learn_K'] else static['K']
        loss, _ = O.loss_path({s: leaves[f'disp_{s}'] for s in static['scales']}, static['imgs'], static['supp_imgs'], Ts, K, noise=static['noise'],
                              aten=True, force_sel=g['out_sel_all'], w_smooth=g['meta_w_smooth'])
        loss.backward()
        _FP64_CACHE[name] = {k: v.grad.float() for k, v in leaves.items()}
    return _FP64_CACHE[name]


def judge_against_reference_at_baseline_size(g, name, grads, sel_own):
    """Compact fixtures: the kernel's decisions (`sel_own`, before `impose_reference_routing`) and its gradients under the reference's routing
    against the REFERENCE's own (`out_sel_all`, `grad_*`).
    Decisions: <= 5e-4 of the pixels may differ (each proven a tie by the caller).
    Dense gradients: besides the arg-min the loss has other knife edges — sign(pred - target) of the L1 term above all: the sampling
    coordinates are fp32 numbers around 600 (ulp 6e-5 px), so two correct implementations' warped values differ by ~1e-6 and wherever
    |pred - target| is smaller than that the L1 term's gradient has either sign.  With a camera motion that explains the frames (these
    fixtures) that is a few dozen of the 10^7 (pixel, channel, support, scale) terms, each worth up to 1e-1 of the tensor's largest
    element, spread over a 3x3 window and the bilinear footprint.  The yardstick is the oracle in fp64 under the same routing: the
    REFERENCE's own fp32 gradient has such elements against it (37 in one tensor at 384x640, 62 over the four scales), so the kernel is held
    to: bulk (99 % quantile of |hip - ref|) <= 2e-4 of the tensor's max, nothing beyond 0.5 (the reference vs fp64: 0.28), and over the
    pyramid no more elements beyond 1e-3 — against the reference or against fp64 — than twice what the reference shows against fp64, + 16.
    Pose / intrinsics gradients (sums over all pixels of ONE sample): 2e-3 against the reference."""
    ref_sel = g['out_sel_all']
    g64 = fp64_gradients_under_reference_routing(g, name)
    flips = int((sel_own.cpu().reshape(ref_sel.shape) != ref_sel).sum())
    report, ok = [f'decisions differ from the reference on {flips} of {ref_sel.numel()} pixels'], flips <= 5e-4*ref_sel.numel()
    tot = [0, 0, 0]
    for k, v in grads.items():
        ref, v = g[f'grad_{k}'], v.cpu()
        mx = ref.abs().max().clamp(min=1e-20)
        d = (v - ref).abs()/mx
        if k.startswith('disp_'):
            n_out, n_hip64, n_ref64 = int((d > 1e-3).sum()), int(((v - g64[k]).abs()/mx > 1e-3).sum()), int(((ref - g64[k]).abs()/mx > 1e-3).sum())
            q = torch.quantile(d.flatten()[:: max(1, d.numel()//2_000_000)], 0.99).item()
            report.append(f'{k}: q99={q:.1e}, beyond 1e-3: {n_out} vs ref (largest {d.max():.1e}), {n_hip64} vs fp64; the reference vs fp64: {n_ref64}')
            ok &= q <= 2e-4 and d.max().item() < 0.5
            tot = [tot[0] + n_out, tot[1] + n_hip64, tot[2] + n_ref64]
        else:
            report.append(f'{k}={d.max():.1e} (ref vs fp64 {((ref - g64[k]).abs()/mx).max():.1e})')
            ok &= d.max().item() < 2e-3
    report.append(f'elements beyond 1e-3 over the pyramid: {tot[0]} vs ref, {tot[1]} vs fp64; the reference vs fp64: {tot[2]}')
    ok &= max(tot[0], tot[1]) <= 2*tot[2] + 16
    return report, ok


@pytest.mark.parametrize('name', TRAIN_CASES)
def test_fused_path_matches_oracle_and_reference(F, golden, knobs, name):
    g = golden(name)
    dev = 'cuda'
    compact = bool(g.get('meta_compact'))
    # --- oracle (CPU) with Ts, K as differentiable leaves
    leaves_c, static_c = case_inputs(g)
    Ts_c = g['out_Ts'].clone().requires_grad_(True)
    K_c = (g['out_K'] if g['meta_learn_K'] else g['in_K']).clone().requires_grad_(True)
    if not compact:
        loss_c, out_c = oracle_run(g, leaves_c, Ts_c, K_c, static_c)
        loss_c.backward()

    # --- HIP path
    leaves, static = case_inputs(g, device=dev)
    Ts = g['out_Ts'].to(dev).requires_grad_(True)
    K = (g['out_K'] if g['meta_learn_K'] else g['in_K']).to(dev).requires_grad_(True)
    scales = static['scales']
    h, w = static['imgs'].shape[-2:]
    depth_up, disp_up = F.disp_to_depth([leaves[f'disp_{s}'] for s in scales], (h, w), g['meta_min_depth'] or None,
                                        g['meta_max_depth'] or None, want_disp_up=True)
    flags = F.recon_flags(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask']))
    l_rec, err, sel, warp0 = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, flags=flags,
                                                  noise=static['noise'], want_warp=True)
    loss = l_rec
    if g['meta_w_smooth'] >= 0:
        l_sm, dgrad, igrad = F.disp_smooth_fused({s: leaves[f'disp_{s}'] for s in scales}, static['imgs'],
                                                 use_edges=bool(g['meta_use_edges']))
        loss = loss + g['meta_w_smooth']*l_sm
    if compact: sel_own = impose_reference_routing(g, sel, knobs)
    loss.backward()
    torch.cuda.synchronize()

    # --- K0
    for k, s in enumerate(scales):
        torch.testing.assert_close(*ref_map(g, f'out_depth_up_{s}', depth_up[k].cpu()), rtol=2e-5, atol=1e-5)
        torch.testing.assert_close(*ref_map(g, f'out_disp_up_{s}', disp_up[k].cpu()), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(*ref_map(g, 'out_supp_imgs_warp', warp0.cpu()), rtol=0, atol=1e-4)
    if compact:
        # BASELINE resolution: everything against what the REFERENCE produced — losses, the reduced error map (sampled), the decision of
        # every pixel at every scale, every gradient; then the oracle under the kernel's routing for the gradients w.r.t. T and K
        # (the reference differentiates through aa / t / fs / cs, tested in test_whole_chain_*).
        e_hip, e_ref = ref_map(g, 'mid_err', err.cpu().reshape(g['out_sel_all'].shape))
        bad = ((e_hip - e_ref).abs() > 2e-4).float().mean().item()
        torch.testing.assert_close(l_rec.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(l_sm.detach().cpu(), g['out_loss_disp_smooth'], rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(*ref_map(g, 'out_disp_grad', dgrad.cpu()), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(*ref_map(g, 'out_image_grad', igrad.cpu()), rtol=1e-4, atol=1e-5)
        report, ok = judge_against_reference_at_baseline_size(g, name, {f'disp_{s}': leaves[f'disp_{s}'].grad for s in scales}, sel_own)
        with torch.no_grad():      # every decision of the kernel that differs from the reference's must be a tie within the error map's noise
            _, out_t = O.loss_path({s: leaves_c[f'disp_{s}'] for s in scales}, static_c['imgs'], static_c['supp_imgs'], Ts_c, K_c, noise=static_c['noise'],
                                   aten=True, force_sel=sel_own.cpu().reshape(g['out_sel_all'].shape))
        tie = out_t['full']['tie_gap'].abs().max().item()
        loss_c, out_c = O.loss_path({s: leaves_c[f'disp_{s}'] for s in scales}, static_c['imgs'], static_c['supp_imgs'], Ts_c, K_c, noise=static_c['noise'],
                                    aten=True, force_sel=g['out_sel_all'])
        loss_c.backward()
        eT, eK = rel_to_max(Ts.grad.cpu()[..., :3, :], Ts_c.grad[..., :3, :]), rel_to_max(K.grad.cpu(), K_c.grad)
        parity_note(f'{name}: loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f} (rel {abs(loss.item() - g["out_loss"].item())/g["out_loss"].item():.1e}); '
                    f'|err - ref| > 2e-4 on {bad:.1e} of the sampled pixels (max {(e_hip - e_ref).abs().max():.1e}); ' + '; '.join(report)
                    + f'; largest gap of a differing decision {tie:.1e}; dT={eT:.1e} dK={eK:.1e} (oracle, reference routing)')
        assert bad <= 1e-3 and ok and tie <= 1e-4 and eT < 2e-3 and eK < 2e-3, report
        return
    # --- forward values
    report = [f'{name}: loss hip={loss.item():.8f} oracle={loss_c.item():.8f} ref={g["out_loss"].item():.8f}']
    err_o = out_c['full']['err'].detach()
    bad = ((err.cpu() - err_o).abs() > 2e-4).float().mean().item()
    assert bad <= 3e-3, f'per-pixel error map differs on {bad:.2%} of pixels (max {(err.cpu() - err_o).abs().max():.3e})'
    flip_map = sel.cpu() != out_c['full']['sel']
    flips = flip_map.float().mean().item()
    report.append(f'  sel flips per scale: {flip_map.flatten(1).sum(1).tolist()}  max |err diff| {(err.cpu() - err_o).abs().max():.3e}')
    assert flips <= 3e-3, f'selection differs on {flips:.2%} of pixels'
    torch.testing.assert_close(l_rec.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    if g['meta_w_smooth'] >= 0:
        torch.testing.assert_close(l_sm.detach().cpu(), g['out_loss_disp_smooth'], rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(dgrad.cpu(), g['out_disp_grad'], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(igrad.cpu(), g['out_image_grad'], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    # --- gradients
    errs = {}
    for s in scales:
        errs[f'disp_{s}'] = rel_to_max(leaves[f'disp_{s}'].grad.cpu(), leaves_c[f'disp_{s}'].grad)
        # and against the reference's own autograd
        errs[f'disp_{s}(ref)'] = rel_to_max(leaves[f'disp_{s}'].grad.cpu(), g[f'grad_disp_{s}'])
    errs['Ts'] = rel_to_max(Ts.grad.cpu()[..., :3, :], Ts_c.grad[..., :3, :])
    errs['K'] = rel_to_max(K.grad.cpu(), K_c.grad)
    report.append('  grad rel-to-max errors: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()))
    parity_note('\n'.join(report))
    # The pure-L1 error has a sign() gradient: the l1 fixture contains one pixel whose warped green channel equals the target
    # to 6e-8 (9.6e-9 in fp64), so its sign is decided by rounding and flips one +-2*w*slope term (scripts/dev/dbg_l1.py).
    tol = 1e-2 if g['meta_loss_name'] == 'l1' else 1e-3
    for k, v in errs.items(): assert v < tol, f'{name}: gradient {k} off by {v:.3e} (rel. to max)\n' + '\n'.join(report)


@pytest.mark.parametrize('name', TRAIN_CASES)
@pytest.mark.parametrize('depth_form', ['dict_of_tensors', 'lazy_from_disparities'])
def test_handlers_match_reference_fixtures(F, golden, name, depth_form):
    """The drop-in level itself: `handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks)` and
    `handlers.disp_smooth(crit, disps, imgs)` (src/core/handlers.py:14-67, 262-281) with the reference's criterion classes'
    keyword arguments, fed (a) the dict of up-sampled depths the reference trainer holds and (b) the `LazyDepths` the K0-fused
    trainer holds — loss, `supp_imgs_warp` and `automask` against the values the reference itself produced."""
    import slowtv_monodepth_amd as amd
    from slowtv_monodepth_amd.handlers import LazyDepths
    g = golden(name)
    dev = 'cuda'
    leaves, static = case_inputs(g, device=dev, requires_grad=False)
    scales = static['scales']
    h, w = static['imgs'].shape[-2:]
    Ts = g['out_Ts'].to(dev)
    K = (g['out_K'] if g['meta_learn_K'] else g['in_K']).to(dev)
    mind, maxd = g['meta_min_depth'] or None, g['meta_max_depth'] or None
    crit = amd.losses.ReconstructionLoss(loss_name=g['meta_loss_name'], use_min=bool(g['meta_use_min']), use_automask=bool(g['meta_use_automask']))
    if depth_form == 'dict_of_tensors':
        if g.get('meta_compact'): pytest.skip('the compact fixtures store the up-sampled depth sampled, not whole')
        depths = {s: g[f'out_depth_up_{s}'].to(dev) for s in scales}
    else: depths = LazyDepths(scales, [leaves[f'disp_{s}'] for s in scales], (h, w), mind, maxd)
    synth = amd.geometry.ViewSynth((h, w))
    loss, ld = amd.handlers.image_recon(crit, synth, depths, None, static['imgs'], static['supp_imgs'], Ts, K, noise=static['noise'])
    torch.testing.assert_close(loss.cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(*ref_map(g, 'out_supp_imgs_warp', ld['supp_imgs_warp'].cpu()), rtol=0, atol=1e-4)
    if g['meta_use_automask']:
        flips = (ld['automask'].cpu().reshape(-1) != g['out_automask'].bool().reshape(-1)).float().mean().item()
        assert flips <= (5e-4 if g.get('meta_compact') else 3e-3), f'automask differs on {flips:.2%} of pixels'
    if depth_form == 'lazy_from_disparities':      # the depth the fused kernel wrote is what a later consumer of fwd['depth_up'] reads
        assert not depths.pending
        for s in scales: torch.testing.assert_close(*ref_map(g, f'out_depth_up_{s}', depths[s].cpu()), rtol=2e-5, atol=1e-5)
    if g['meta_w_smooth'] >= 0:
        reg = amd.regularizers.SmoothReg(use_edges=bool(g['meta_use_edges']))
        l_sm, ld_sm = amd.handlers.disp_smooth(reg, {s: leaves[f'disp_{s}'] for s in scales}, static['imgs'])
        torch.testing.assert_close(l_sm.cpu(), g['out_loss_disp_smooth'], rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(*ref_map(g, 'out_disp_grad', ld_sm['disp_grad'].cpu()), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(*ref_map(g, 'out_image_grad', ld_sm['image_grad'].cpu()), rtol=1e-4, atol=1e-5)


def test_in_kernel_noise_is_a_tiebreak_only(F, golden):
    """noise=None uses the counter-based in-kernel Gaussian: loss must agree to ~eps, masks may differ only on ties."""
    g = golden('train_kbr_96x128')
    leaves, static = case_inputs(g, device='cuda', requires_grad=False)
    h, w = static['imgs'].shape[-2:]
    depth_up, _ = F.disp_to_depth([leaves[f'disp_{s}'] for s in static['scales']], (h, w), 0.1, 100)
    Ts, K = g['out_Ts'].cuda(), g['in_K'].cuda()
    flags = F.recon_flags('ssim', True, True)
    l0, e0, s0, _ = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, flags=flags, noise=static['noise'])
    l1, e1, s1, _ = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, flags=flags, noise=None, seed=123)
    l2, e2, s2, _ = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, flags=flags, noise=None, seed=123)
    assert torch.equal(s1, s2) and torch.equal(e1, e2), 'in-kernel noise must be deterministic for a fixed seed'
    assert abs(l0.item() - l1.item()) < 1e-6
    differ = (s0 != s1)
    assert ((e0 - e1).abs()[differ] < 1e-5).all(), 'selection may only change where the two errors tie'


def test_rejects_cpu_tensors_and_bad_shapes(F):
    with pytest.raises(RuntimeError): F.disp_to_depth([torch.rand(1, 1, 4, 4)], (4, 4), 0.1, 100)
    with pytest.raises(ValueError): F.disp_to_depth([torch.rand(1, 1, 4, 4, device='cuda')], (4, 4), 0.0, 100)
    d = torch.rand(1, 1, 1, 8, 8, device='cuda') + 0.5
    img = torch.rand(1, 3, 8, 8, device='cuda'); sup = torch.rand(2, 1, 3, 8, 8, device='cuda')
    T = torch.eye(4, device='cuda').repeat(2, 1, 1, 1); K = torch.eye(4, device='cuda')[None]
    with pytest.raises(ValueError): F.image_recon_fused(d, img[:, :2], sup, T, K, flags=0)
    with pytest.raises(NotImplementedError): F.recon_flags('l2')


# ---------------------------------------------------------------------------------------------------
# BASELINE sizes, value for value against the oracle (ATen primitives on the CPU: ~5 s per sample pair at 640x192)
# ---------------------------------------------------------------------------------------------------
def _baseline_inputs(b, h, w, supp, S, seed):
    from slowtv_monodepth_amd.synthetic import make_batch
    import torch.nn.functional as Fn
    n = len(supp)
    _, y, _ = make_batch(b, h, w, supp, seed=seed, device='cpu')
    g = torch.Generator().manual_seed(seed + 1)
    disps = {}
    for s in range(S):   # smooth field + pixel noise, like a partly trained network's output
        hs, ws = h >> s, w >> s
        low = 0.02 + 0.25*torch.rand(b, 1, 4, 10, generator=g)      # depth 0.4 .. 5: no pixel so close that it alone moves a pose gradient
        disps[s] = (Fn.interpolate(low, size=(hs, ws), mode='bilinear', align_corners=False) + 0.01*torch.rand(b, 1, hs, ws, generator=g))
    aa, t = 0.01*torch.randn(n, b, 3, generator=g), 0.08*torch.randn(n, b, 3, generator=g)
    noise = torch.randn(S*b, 1, h, w, generator=g)
    return y, disps, aa, t, noise


BASELINE_CASES = {
    # name: (b, h, w, supports, S, learned K)
    'cfg2_b12_192x640_n2': (12, 192, 640, (-1, 1), 4, False),       # the configuration the metric is quoted on, full batch
    'cfg4_b2_384x640_n2_learnK': (2, 384, 640, (-1, 1), 4, True),   # learned intrinsics: K gradient (SMD_NEED_K_GRAD)
    'cfg5_b2_384x640_n4': (2, 384, 640, (-2, -1, 1, 2), 4, False),  # four supports in one launch
}


def _judge_gradients(g_hip, g_ref, g_64, n_flips):
    """Gradient acceptance at BASELINE size (shared by the two baseline-size tests).  Dense gradients: 99.9 % quantile of the
    difference + an outlier budget tied to the number of decision flips; pose / intrinsics gradients: 5e-3 against the fp32
    oracle, or no further from the oracle's fp64 run than three times the fp32 oracle is."""
    report, ok = [], True
    for k in g_ref:
        diff, mx = (g_hip[k] - g_ref[k]).abs(), g_ref[k].abs().max()
        if k.startswith('disp_'):
            allow = 30*(n_flips + 3)                     # a flip touches its 3x3 window, at most 5x5 low-resolution pixels
            level = 1.0 - max(1e-3, 2.0*allow/diff.numel())
            q = torch.quantile(diff.flatten()[:: max(1, diff.numel()//2_000_000)], level).item()/mx.item()
            outl = int((diff > 1e-3*mx).sum())
            report.append(f'{k}: q{100*level:.1f}={q:.1e} outliers={outl}')
            ok &= q < 2e-4 and outl <= allow
        else:
            e = (diff.max()/mx).item()
            mx64 = g_64[k].abs().max()
            e_hip64, e_ref64 = ((g_hip[k] - g_64[k]).abs().max()/mx64).item(), ((g_ref[k] - g_64[k]).abs().max()/mx64).item()
            report.append(f'{k}={e:.1e} (vs fp64: hip {e_hip64:.1e}, fp32 oracle {e_ref64:.1e})')
            ok &= e < 5e-3 or e_hip64 <= 3.0*e_ref64
    return report, ok


@pytest.mark.parametrize('name', list(BASELINE_CASES))
def test_baseline_size_matches_oracle(F, name):
    """HIP vs oracle at the BASELINE shapes: loss 1e-4 relative (BASELINE.json; asserted at 2e-5), error map, selection flips,
    gradients w.r.t. every disparity scale, the pose vectors and (cfg 4) the intrinsics' network outputs."""
    b, h, w, supp, S, learn_k = BASELINE_CASES[name]
    n = len(supp)
    y, disps, aa, t, noise = _baseline_inputs(b, h, w, supp, S, seed=7)
    g = torch.Generator().manual_seed(99)
    fs, cs = 0.3*torch.randn(b, 2, generator=g), 0.2*torch.randn(b, 2, generator=g)

    def run(dev, hip, force_sel=None, dt=torch.float32):
        leaf = lambda v: v.detach().clone().to(dev, dt).requires_grad_(True)
        d = {s: leaf(v) for s, v in disps.items()}
        a_, t_, fs_, cs_ = leaf(aa), leaf(t), leaf(fs), leaf(cs)
        imgs, sup = y['imgs'].to(dev), y['supp_imgs'].to(dev)
        gap = None
        if hip:
            Ts = F.pose_matrices(a_.flatten(0, 1), t_.flatten(0, 1)).unflatten(0, (n, b))
            K, K_inv = F.intrinsics(fs_, cs_, (h, w)) if learn_k else (y['K'].to(dev), None)
            depth_up, _ = F.disp_to_depth(list(d.values()), (h, w), 0.1, 100)
            l_rec, err, sel, _ = F.image_recon_fused(depth_up, imgs, sup, Ts, K, K_inv, flags=F.recon_flags('ssim', True, True), noise=noise.to(dev))
            l_sm, *_ = F.disp_smooth_fused(d, imgs, use_edges=True, want_aux=False)
            loss = l_rec + 0.001*l_sm
        else:
            Ts = O.T_from_AAt(a_.flatten(0, 1), t_.flatten(0, 1)).unflatten(0, (n, b))
            K = O.resize_K(O.build_K(fs_, cs_), (h, w)) if learn_k else y['K'].to(dt)
            loss, out = O.loss_path(d, imgs.to(dt), sup.to(dt), Ts, K, noise=noise.to(dt), aten=True, force_sel=force_sel)
            err, sel, gap = out['full']['err'], out['full']['sel'], out['full'].get('tie_gap')
        loss.backward()
        grads = {f'disp_{s}': v.grad.cpu().float() for s, v in d.items()}
        grads['aa'], grads['t'] = a_.grad.cpu().float(), t_.grad.cpu().float()
        if learn_k: grads['fs'], grads['cs'] = fs_.grad.cpu().float(), cs_.grad.cpu().float()
        return loss.item(), err.detach().cpu().reshape(S, b, h, w), sel.cpu().reshape(S, b, h, w), grads, gap

    l_hip, e_hip, s_hip, g_hip, _ = run('cuda', True)
    torch.cuda.synchronize()
    # The oracle routes the gradient through ITS arg-min.  At this size a handful of pixels (a few per million) have two
    # candidate errors equal to within the fp32 noise of the error map (~1e-5) and rounding decides them differently; a flipped pixel close to the camera moves a
    # pose gradient by percents.  So: (1) free-running oracle -> loss, error map, selection flips; (2) oracle again with the
    # kernel's decisions imposed (and the proof that every imposed decision was a tie) -> gradients under identical routing.
    l_ref, e_ref, s_ref, g_free, _ = run('cpu', False)
    flips = (s_hip != s_ref)
    bad = ((e_hip - e_ref).abs() > 2e-4).float().mean().item()
    _, _, _, g_ref, gap = run('cpu', False, force_sel=s_hip.reshape(S*b, 1, h, w)) if flips.any() else (None, None, None, g_free, None)
    tie = gap.abs().max().item() if gap is not None else 0.0
    # fp64 run of the oracle under the same routing: the yardstick for the gradients that are sums over every pixel
    _, _, _, g_64, _ = run('cpu', False, force_sel=s_hip.reshape(S*b, 1, h, w), dt=torch.float64)
    # The loss has more discontinuities than the arg-min (clamp(0,1) of the SSIM term, sign() of the L1 term, border clamps): a
    # pixel sitting on one of them gets a different one-sided derivative from rounding alone.  Dense gradients are therefore
    # judged by their bulk (99.9 % quantile of the difference) plus a count of outliers tied to the number of decision flips.
    # The pose / intrinsics gradients are sums over all pixels in which one such pixel weighs ~1e-3 when there are only two
    # samples: they are judged by their relative error against the fp32 oracle (5e-3), or — where the fp32 oracle itself is
    # that far from its own fp64 run — by being no further from the fp64 result than three times the fp32 oracle is.
    n_flips = int(flips.sum())
    report, ok = _judge_gradients(g_hip, g_ref, g_64, n_flips)
    free = {k: rel_to_max(g_hip[k], g_free[k]) for k in g_free}
    parity_note(f'{name}: loss hip={l_hip:.8f} oracle={l_ref:.8f} (rel {abs(l_hip - l_ref)/abs(l_ref):.2e}); sel flips {n_flips} of {flips.numel()} '
          f'({flips.float().mean().item():.2e}, largest gap between the tied errors {tie:.1e}); |err diff| > 2e-4 on {bad:.2e} of pixels '
          f'(max {(e_hip - e_ref).abs().max():.2e})\n  gradients, same routing: ' + ' '.join(report)
          + '\n  max-norm rel-to-max against the free-running oracle: ' + ' '.join(f'{k}={v:.1e}' for k, v in free.items()))
    assert abs(l_hip - l_ref) <= 2e-5*abs(l_ref)
    assert bad <= 3e-3 and flips.float().mean().item() <= 1e-4
    assert tie <= 1e-4, 'a selection that differs from the oracle must be a tie within the error-map tolerance (2e-4)'
    assert ok, f'{name}: gradients differ: ' + ' '.join(report)



@pytest.mark.parametrize('name', list(BASELINE_CASES))
def test_baseline_size_timed_path_matches_oracle(F, name, monkeypatch):
    """The EXACT path `bench.py` times, at the BASELINE shapes, value for value against the oracle: the trainer's call
    `handlers.image_recon(crit, synth, LazyDepths(...), None, imgs, supp_imgs, Ts, K)` with `want_warp=False` (src/core/trainer.py:316-321,
    388-392 in the reference) -> `image_recon_fused_disp(noise=None, want_warp=False, want_err=False)` -> the hot instantiation
    `k_recon_main<n, true, true, false, true>` (K0 fused, in-kernel tie-break noise, no error map) and, through autograd,
    `smd_image_recon_disp_bwd` (k0_scale != 0, no incoming depth gradient) + the K0 adjoint; `handlers.disp_smooth(want_aux=False)`.
    Compared with `O.loss_path(noise=zeros)`: loss 2e-5 relative, `sel` equal off the ties (every difference proven a tie by the
    forced oracle run), the adopted `depth_up`, gradients w.r.t. every disparity scale, `aa`, `t` (`fs`, `cs` at cfg 4) under
    identical routing.  A second launch of the same build with `want_err=True` checks its error map."""
    import slowtv_monodepth_amd as amd
    from slowtv_monodepth_amd import functional as Fm
    from slowtv_monodepth_amd.handlers import LazyDepths
    b, h, w, supp, S, learn_k = BASELINE_CASES[name]
    n = len(supp)
    y, disps, aa, t, _ = _baseline_inputs(b, h, w, supp, S, seed=7)
    g = torch.Generator().manual_seed(99)
    fs, cs = 0.3*torch.randn(b, 2, generator=g), 0.2*torch.randn(b, 2, generator=g)
    zeros = torch.zeros(S*b, 1, h, w)

    seen = {}
    real = Fm.image_recon_fused_disp

    def spy(disps_, imgs_, supp_, Ts_, Ks_, K_inv_=None, **kw):
        out = real(disps_, imgs_, supp_, Ts_, Ks_, K_inv_, **kw)
        seen.update(kw=kw, err=out[1], sel=out[2], warp0=out[3], depth_up=out[4])
        return out
    monkeypatch.setattr(Fm, 'image_recon_fused_disp', spy)

    dev = 'cuda'
    leaf = lambda v, d=dev, dt=torch.float32: v.detach().clone().to(d, dt).requires_grad_(True)
    d = {s: leaf(v) for s, v in disps.items()}
    a_, t_, fs_, cs_ = leaf(aa), leaf(t), leaf(fs), leaf(cs)
    imgs, sup = y['imgs'].to(dev), y['supp_imgs'].to(dev)
    Ts = F.pose_matrices(a_.flatten(0, 1), t_.flatten(0, 1)).unflatten(0, (n, b))
    K, K_inv = F.intrinsics(fs_, cs_, (h, w)) if learn_k else (y['K'].to(dev), None)
    crit = amd.losses.ReconstructionLoss(loss_name='ssim', use_min=True, use_automask=True)
    reg = amd.regularizers.SmoothReg(use_edges=True)
    depths = LazyDepths(list(d.keys()), list(d.values()), (h, w), 0.1, 100)
    l_rec, ld = amd.handlers.image_recon(crit, amd.geometry.ViewSynth((h, w)), depths, None, imgs, sup, Ts, K, K_inv=K_inv, want_warp=False)
    l_sm, _ = amd.handlers.disp_smooth(reg, d, imgs, want_aux=False)
    (l_rec + 0.001*l_sm).backward()
    torch.cuda.synchronize()
    # this IS the timed instantiation: no caller noise, no warp output, no error map -> SINGLE && !AUX && DISP (smd_recon_fwd.hip: launch_recon_main)
    assert seen['kw']['noise'] is None and seen['kw']['want_warp'] is False and seen['kw']['want_err'] is False
    assert seen['err'] is None and seen['warp0'] is None and not depths.pending
    l_hip = (l_rec + 0.001*l_sm).item()
    s_hip = seen['sel'].cpu().reshape(S, b, h, w)
    g_hip = {f'disp_{s}': v.grad.cpu() for s, v in d.items()}
    g_hip['aa'], g_hip['t'] = a_.grad.cpu(), t_.grad.cpu()
    if learn_k: g_hip['fs'], g_hip['cs'] = fs_.grad.cpu(), cs_.grad.cpu()
    assert torch.equal(ld['automask'].cpu().reshape(b, h, w), s_hip[0] != 255)

    def oracle(force_sel=None, dt=torch.float32):
        dd = {s: leaf(v, 'cpu', dt) for s, v in disps.items()}
        ao, to, fo, co = leaf(aa, 'cpu', dt), leaf(t, 'cpu', dt), leaf(fs, 'cpu', dt), leaf(cs, 'cpu', dt)
        To = O.T_from_AAt(ao.flatten(0, 1), to.flatten(0, 1)).unflatten(0, (n, b))
        Ko = O.resize_K(O.build_K(fo, co), (h, w)) if learn_k else y['K'].to(dt)
        loss, out = O.loss_path(dd, y['imgs'].to(dt), y['supp_imgs'].to(dt), To, Ko, noise=zeros.to(dt), aten=True, force_sel=force_sel)
        loss.backward()
        grads = {f'disp_{s}': v.grad.float() for s, v in dd.items()}
        grads['aa'], grads['t'] = ao.grad.float(), to.grad.float()
        if learn_k: grads['fs'], grads['cs'] = fo.grad.float(), co.grad.float()
        full = out['full']
        return (loss.item(), full['err'].detach().reshape(S, b, h, w), full['sel'].reshape(S, b, h, w), grads, full.get('tie_gap'),
                torch.stack([out['depth_up'][s].detach() for s in dd]).reshape(S, b, h, w))

    l_ref, e_ref, s_ref, g_free, _, dep_ref = oracle()
    flips = s_hip != s_ref
    forced = s_hip.reshape(S*b, 1, h, w)
    _, _, _, g_ref, gap, _ = oracle(force_sel=forced) if flips.any() else (None, None, None, g_free, None, None)
    tie = gap.abs().max().item() if gap is not None else 0.0
    _, _, _, g_64, _, _ = oracle(force_sel=forced, dt=torch.float64)
    n_flips = int(flips.sum())
    report, ok = _judge_gradients(g_hip, g_ref, g_64, n_flips)

    # the error map of the same build (has_err is a run-time switch of the hot instantiation; same seed -> same decisions)
    with torch.no_grad():
        _, err2, sel2, _, _ = real([v.detach() for v in d.values()], imgs, sup, Ts.detach(), K.detach(), K_inv.detach() if K_inv is not None else None,
                                   flags=F.recon_flags('ssim', True, True), min_depth=0.1, max_depth=100, noise=None, seed=seen['kw']['seed'],
                                   want_warp=False, want_err=True)
    e_hip = err2.cpu().reshape(S, b, h, w)
    bad = ((e_hip - e_ref).abs() > 2e-4).float().mean().item()
    dep_diff = (seen['depth_up'].detach().cpu().reshape(S, b, h, w) - dep_ref).abs()
    dep_rel = (dep_diff/dep_ref.abs().clamp(min=1e-6)).max().item()
    parity_note(f'timed path {name}: loss hip={l_hip:.8f} oracle={l_ref:.8f} (rel {abs(l_hip - l_ref)/abs(l_ref):.2e}); sel differs on {n_flips} of '
                f'{flips.numel()} ({flips.float().mean().item():.2e}, largest gap between the tied errors {tie:.1e}); |err diff| > 2e-4 on {bad:.2e} of '
                f'pixels (max {(e_hip - e_ref).abs().max():.2e}); depth_up max rel diff {dep_rel:.1e}\n  gradients, same routing: ' + ' '.join(report))
    assert torch.equal(sel2.cpu().reshape(S, b, h, w), s_hip), 'want_err must not change the decisions of the same build and seed'
    assert abs(l_hip - l_ref) <= 2e-5*abs(l_ref)
    assert bad <= 3e-3 and flips.float().mean().item() <= 1e-4
    assert tie <= 1e-4, 'a selection that differs from the oracle must be a tie within the error-map tolerance (2e-4)'
    torch.testing.assert_close(seen['depth_up'].detach().cpu().reshape(S, b, h, w), dep_ref, rtol=2e-5, atol=1e-5)
    assert ok, f'{name}: gradients differ: ' + ' '.join(report)


def test_baseline_size_in_kernel_noise_matches_oracle_off_the_ties(F):
    """The product path (noise=None: counter-based Gaussian drawn in the kernel) at cfg-2 size against the oracle run WITHOUT
    noise: errors agree everywhere, selection may differ only where the warped and the static error tie (|diff| < 1e-5)."""
    b, h, w, supp, S = 2, 192, 640, (-1, 1), 4
    y, disps, aa, t, _ = _baseline_inputs(b, h, w, supp, S, seed=11)
    Ts_c = O.T_from_AAt(aa.flatten(0, 1), t.flatten(0, 1)).unflatten(0, (2, b))
    with torch.no_grad():
        l_ref, out = O.loss_path(disps, y['imgs'], y['supp_imgs'], Ts_c, y['K'], noise=torch.zeros(S*b, 1, h, w), aten=True)
    e_ref, s_ref = out['full']['err'].reshape(S, b, h, w), out['full']['sel'].reshape(S, b, h, w)
    dev = 'cuda'
    Ts = F.pose_matrices(aa.to(dev).flatten(0, 1), t.to(dev).flatten(0, 1)).unflatten(0, (2, b))
    depth_up, _ = F.disp_to_depth([d.to(dev) for d in disps.values()], (h, w), 0.1, 100)
    l_hip, err, sel, _ = F.image_recon_fused(depth_up, y['imgs'].to(dev), y['supp_imgs'].to(dev), Ts, y['K'].to(dev),
                                              flags=F.recon_flags('ssim', True, True), noise=None, seed=2024)
    e_hip, s_hip = err.cpu().reshape(S, b, h, w), sel.cpu().reshape(S, b, h, w)
    with torch.no_grad(): l_rec_ref = e_ref.mean().item()
    assert abs(l_hip.item() - l_rec_ref) <= 2e-5*abs(l_rec_ref)
    differ = s_hip != s_ref
    close = (e_hip - e_ref).abs() <= 2e-4
    parity_note(f'in-kernel noise: {int(differ.sum())} selection differences of {differ.numel()}, {int((~close).sum())} pixels with |err diff| > 2e-4')
    assert (~close).float().mean().item() <= 3e-3
    assert differ.float().mean().item() <= 3e-3


@pytest.mark.parametrize('shape', [(12, 192, 640, 2, 4), (3, 384, 640, 4, 4), (1, 50, 70, 3, 2), (12, 384, 640, 2, 4, 'learn_K')])
def test_full_size_properties(F, shape):
    """Size-independent properties at BASELINE sizes (on top of the value-for-value comparisons above):
    (1) identity pose + constant depth + fixed K: warped support == bilinear resample with the known w/(w-1) stretch,
        so err is finite, within [0, 1], and `loss == err.mean()`;
    (2) swapping the support order leaves the min-reprojection error unchanged and permutes `sel`;
    (3) batch linearity: evaluating two half-batches separately gives the same per-pixel maps;
    (4) gradients are finite and g_T's last row is zero.
    The last case is BASELINE cfg 4 at its full batch (b = 12, 384x640, two supports) with LEARNED intrinsics: K, K_inv come out of `functional.intrinsics`
    and the gradients must reach its (fs, cs) leaves, finite."""
    b, h, w, n, S = shape[:5]
    learn_K = len(shape) > 5
    gen = torch.Generator(device='cuda').manual_seed(5)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen)
    supp = torch.rand(n, b, 3, h, w, device='cuda', generator=gen)
    depth = (1 + 20*torch.rand(S, b, 1, h, w, device='cuda', generator=gen)).requires_grad_(True)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    K_inv, fs, cs = None, None, None
    if learn_K:   # normalised focal lengths / principal points around the fixed K's, one pair per sample (what PoseNet.build_K emits: src/networks/pose.py:60-73)
        fs = (torch.tensor([0.58, 1.92], device='cuda') + 0.02*torch.randn(b, 2, device='cuda', generator=gen)).requires_grad_(True)
        cs = (0.5 + 0.01*torch.randn(b, 2, device='cuda', generator=gen)).requires_grad_(True)
        K, K_inv = F.intrinsics(fs, cs, (h, w))
    T = torch.eye(4, device='cuda').repeat(n, b, 1, 1)
    T[..., :3, 3] = 0.05*torch.randn(n, b, 3, device='cuda', generator=gen)
    T.requires_grad_(True)
    flags = F.recon_flags('ssim', True, True)
    noise = torch.randn(S, b, 1, h, w, device='cuda', generator=gen)
    loss, err, sel, _ = F.image_recon_fused(depth, imgs, supp, T, K, K_inv, flags=flags, noise=noise)
    assert torch.isfinite(err).all() and (err >= -1e-6).all() and (err <= 1 + 1e-6).all()
    torch.testing.assert_close(loss, err.double().mean().float(), rtol=1e-5, atol=1e-7)
    loss.backward()
    assert torch.isfinite(depth.grad).all() and torch.isfinite(T.grad).all()
    assert (T.grad[..., 3, :] == 0).all()
    if learn_K:
        assert torch.isfinite(fs.grad).all() and torch.isfinite(cs.grad).all() and fs.grad.abs().max() > 0 and cs.grad.abs().max() > 0
        K, K_inv = K.detach(), K_inv.detach()
    # (2) permutation of supports
    perm = list(reversed(range(n)))
    loss_p, err_p, sel_p, _ = F.image_recon_fused(depth.detach(), imgs, supp[perm], T.detach()[perm], K, K_inv, flags=flags, noise=noise)
    torch.testing.assert_close(err_p, err, rtol=0, atol=1e-6)
    kept = (sel != 255) & (sel_p != 255)
    same = (torch.tensor(perm, device='cuda', dtype=torch.uint8)[sel_p[kept].long()] == sel[kept]).float().mean().item()
    assert same > 0.999
    # (3) batch split
    if b >= 2:
        hb = b//2
        _, err_a, sel_a, _ = F.image_recon_fused(depth.detach()[:, :hb], imgs[:hb], supp[:, :hb], T.detach()[:, :hb], K[:hb], K_inv[:hb] if K_inv is not None else None,
                                                 flags=flags, noise=noise[:, :hb])
        assert torch.equal(err_a, err[:, :hb]) and torch.equal(sel_a, sel[:, :hb])


# ---------------------------------------------------------------------------------------------------
# Un-fused, class-level operators against the reference's own vectors
# ---------------------------------------------------------------------------------------------------
def test_view_synth_operator_matches_reference(F, golden):
    from slowtv_monodepth_amd.geometry import T_from_AAt, ViewSynth
    g = golden('op_view_synth')
    dev = 'cuda'
    feat = g['in_input'].to(dev).requires_grad_(True); depth = g['in_depth'].to(dev).requires_grad_(True)
    aa = g['in_aa'].to(dev).requires_grad_(True); t = g['in_t'].to(dev).requires_grad_(True); K = g['in_K'].to(dev).requires_grad_(True)
    T = T_from_AAt(aa, t)
    warp, dwarp, valid = ViewSynth(feat.shape[-2:])(feat, depth, T, K)
    torch.testing.assert_close(warp.cpu(), g['out_warp'], rtol=0, atol=1e-4)
    torch.testing.assert_close(dwarp.cpu(), g['out_depth_warp'], rtol=1e-5, atol=1e-5)
    assert valid.dtype == torch.bool and (valid.cpu() != g['out_mask_valid']).float().mean() < 3e-3
    ((warp*g['in_gw'].to(dev)).sum() + (dwarp*g['in_gd'].to(dev)).sum()).backward()
    for name, leaf in dict(input=feat, depth=depth, aa=aa, t=t, K=K).items():
        assert rel_to_max(leaf.grad.cpu(), g[f'grad_{name}']) < 1e-3, name
    with pytest.raises(ValueError): ViewSynth((3, 3))(feat, depth, T, K)


@pytest.mark.parametrize('loss_name', ['ssim', 'l1'])
def test_photo_error_operator_matches_reference(F, golden, loss_name):
    g = golden('op_photo_error')
    pred = g['in_pred'].cuda().requires_grad_(True); tgt = g['in_target'].cuda()
    err = F.photo_error(pred, tgt, loss_name)
    pc = g['in_pred'].clone().requires_grad_(True)
    ref = O.photo_error(pc, g['in_target'], loss_name)
    if loss_name == 'ssim': torch.testing.assert_close(err.cpu(), g['out_err'], rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(err.detach().cpu(), ref.detach(), rtol=1e-5, atol=2e-6)
    ge = g['in_ge']
    (err*ge.cuda()).sum().backward(); (ref*ge).sum().backward()
    torch.testing.assert_close(pred.grad.cpu(), pc.grad, rtol=2e-4, atol=2e-5)
    if loss_name == 'ssim': torch.testing.assert_close(pred.grad.cpu(), g['grad_pred'], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize('name', ['train_kbr_24x32', 'train_mean_n1_s1_33x47', 'train_min_noauto_25x38'])
def test_class_level_path_matches_fused_path(F, golden, name):
    """ViewSynth -> ReconstructionLoss (un-fused HIP operators, reference call structure of handlers.py:45-62) must agree with
    the fused handler and with the reference's loss value."""
    from slowtv_monodepth_amd.geometry import ViewSynth
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    g = golden(name)
    leaves, static = case_inputs(g, device='cuda', requires_grad=False)
    scales = static['scales']; h, w = static['imgs'].shape[-2:]
    S, b, n = len(scales), g['meta_b'], g['meta_n']
    depth_up, _ = F.disp_to_depth([leaves[f'disp_{s}'] for s in scales], (h, w), g['meta_min_depth'] or None, g['meta_max_depth'] or None)
    depth_up = depth_up.detach().requires_grad_(True)
    Ts = g['out_Ts'].cuda().requires_grad_(True); K = g['in_K'].cuda()
    crit = ReconstructionLoss(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask']))
    # reference-style expansion to (n, S*b, ...)
    dep = depth_up.flatten(0, 1)[None].expand(n, -1, -1, -1, -1).flatten(0, 1)
    src = static['supp_imgs'][:, None].expand(n, S, b, 3, h, w).flatten(1, 2)
    T = Ts[:, None].expand(n, S, b, 4, 4).flatten(0, 2); Kx = K[None, None].expand(n, S, b, 4, 4).flatten(0, 2)
    warp = ViewSynth((h, w))(src.flatten(0, 1).contiguous(), dep.contiguous(), T.contiguous(), Kx.contiguous())[0].unflatten(0, (n, S*b))
    tgt = static['imgs'][None].expand(S, b, 3, h, w).flatten(0, 1)
    l, ld = crit(warp, tgt, source=src, noise=static['noise'])
    torch.testing.assert_close(l.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    l.backward()
    g_d_unfused, g_T_unfused = depth_up.grad.clone(), Ts.grad.clone()
    depth_up.grad = None; Ts.grad = None
    lf, _, _, _ = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, flags=F.recon_flags(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask'])), noise=static['noise'])
    lf.backward()
    torch.testing.assert_close(lf, l, rtol=1e-5, atol=1e-7)
    assert rel_to_max(g_d_unfused, depth_up.grad) < 1e-3 and rel_to_max(g_T_unfused[..., :3, :], Ts.grad[..., :3, :]) < 1e-3
    if g['meta_use_automask']:
        assert (ld['automask'].unflatten(0, (S, b))[0].cpu() != g['out_automask']).float().mean() < 3e-3


# ---------------------------------------------------------------------------------------------------
# Pose / intrinsics prologue (smd_pose_*, smd_intrinsics_*)
def test_pose_matrices_match_reference(F, golden):
    g = golden('op_T_from_AAt')
    aa = g['in_aa'].cuda().requires_grad_(True); t = g['in_t'].cuda().requires_grad_(True)
    T = F.pose_matrices(aa, t)
    torch.testing.assert_close(T.cpu(), g['out_T'], rtol=1e-6, atol=1e-6)
    T.backward(g['in_gT'].cuda())
    torch.testing.assert_close(aa.grad.cpu(), g['grad_aa'], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(t.grad.cpu(), g['grad_t'], rtol=1e-5, atol=1e-6)


def test_inverted_pose_matches_general_inverse(F):
    """Rows flagged `invert` hold T^-1 (src/core/trainer.py:253); gradients equal those of the general 4x4 inverse."""
    from oracle import view_synth_oracle as O
    gen = torch.Generator().manual_seed(5)
    N = 9
    aa = torch.randn(N, 3, generator=gen)*0.3; t = torch.randn(N, 3, generator=gen)
    aa[0] = 0.0                       # |aa| = 0: clip branch, zero sub-gradient of the norm
    aa[1] = aa[1]*1e-4/aa[1].norm()   # |aa| < eps branch
    inv = torch.tensor([0, 1, 1, 0, 1, 0, 1, 1, 0], dtype=torch.uint8)
    gT = torch.randn(N, 4, 4, generator=gen)
    aa_c, t_c = aa.clone().requires_grad_(True), t.clone().requires_grad_(True)
    T_c = O.T_from_AAt(aa_c, t_c)
    T_c = torch.stack([torch.linalg.inv(Ti) if f else Ti for Ti, f in zip(T_c, inv)])
    T_c.backward(gT)
    aa_g, t_g = aa.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    T_g = F.pose_matrices(aa_g, t_g, inv.cuda())
    T_g.backward(gT.cuda())
    torch.testing.assert_close(T_g.detach().cpu(), T_c.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(aa_g.grad.cpu(), aa_c.grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(t_g.grad.cpu(), t_c.grad, rtol=1e-5, atol=1e-6)


def test_intrinsics_match_oracle(F):
    from oracle import view_synth_oracle as O
    gen = torch.Generator().manual_seed(6)
    b, size = 5, (96, 320)
    fs = torch.rand(b, 2, generator=gen) + 0.5; cs = torch.rand(b, 2, generator=gen)*0.2 + 0.4
    gK, gKi = torch.randn(b, 4, 4, generator=gen), torch.randn(b, 4, 4, generator=gen)
    fs_c, cs_c = fs.clone().requires_grad_(True), cs.clone().requires_grad_(True)
    K_c = O.resize_K(O.build_K(fs_c, cs_c), size); Ki_c = torch.linalg.inv(K_c)
    ((K_c*gK).sum() + (Ki_c*gKi).sum()).backward()
    fs_g, cs_g = fs.cuda().requires_grad_(True), cs.cuda().requires_grad_(True)
    K_g, Ki_g = F.intrinsics(fs_g, cs_g, size)
    ((K_g*gK.cuda()).sum() + (Ki_g*gKi.cuda()).sum()).backward()
    torch.testing.assert_close(K_g.detach().cpu(), K_c.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(Ki_g.detach().cpu(), Ki_c.detach(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(fs_g.grad.cpu(), fs_c.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(cs_g.grad.cpu(), cs_c.grad, rtol=1e-4, atol=1e-5)
    # caller-supplied K (with skew): adjugate inverse of the 3x3 block
    K = K_c.detach().clone(); K[:, 0, 1] = 0.7
    torch.testing.assert_close(F.inv_intrinsics(K.cuda()).cpu(), torch.linalg.inv(K), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('name', ['train_learnK_n4_40x56', 'train_kbr_24x32'])
def test_whole_chain_from_network_outputs_matches_reference_gradients(F, golden, name):
    """aa, t, (fs, cs), disp -> pose/intrinsics kernels -> K0 -> fused loss; gradients w.r.t. every network output against the
    reference's own autograd (the fixtures were recorded through src/core/trainer.py's forward_postprocess + forward_loss)."""
    g = golden(name)
    leaves, static = case_inputs(g, device='cuda')
    scales, idxs = static['scales'], static['supp_idxs']
    n, b = leaves['aa'].shape[:2]
    h, w = static['imgs'].shape[-2:]
    inv = torch.tensor([bool(g['meta_always_fwd_pose']) and i < 0 for i in idxs for _ in range(b)], dtype=torch.uint8).cuda()
    Ts = F.pose_matrices(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1), inv).unflatten(0, (n, b))
    torch.testing.assert_close(Ts.detach().cpu(), g['out_Ts'], rtol=1e-5, atol=1e-6)
    if g['meta_learn_K']:
        K, K_inv = F.intrinsics(leaves['fs'], leaves['cs'], (h, w))
        torch.testing.assert_close(K.detach().cpu(), g['out_K'], rtol=1e-6, atol=1e-5)
    else:
        K, K_inv = static['K'], None
    depth_up, _ = F.disp_to_depth([leaves[f'disp_{s}'] for s in scales], (h, w), g['meta_min_depth'] or None, g['meta_max_depth'] or None)
    flags = F.recon_flags(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask']))
    loss, *_ = F.image_recon_fused(depth_up, static['imgs'], static['supp_imgs'], Ts, K, K_inv, flags=flags, noise=static['noise'])
    if g['meta_w_smooth'] >= 0:
        l_sm, _, _ = F.disp_smooth_fused({s: leaves[f'disp_{s}'] for s in scales}, static['imgs'], use_edges=bool(g['meta_use_edges']), want_aux=False)
        loss = loss + g['meta_w_smooth']*l_sm
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    for k in ['aa', 't'] + (['fs', 'cs'] if g['meta_learn_K'] else []) + [f'disp_{s}' for s in scales]:
        e = rel_to_max(leaves[k].grad.cpu(), g[f'grad_{k}'])
        assert e < 1e-3, f'{name}: d loss / d {k} off by {e:.3e} (rel. to max) vs the reference autograd'


@pytest.mark.parametrize('name', TRAIN_CASES_BASELINE)
def test_whole_chain_at_baseline_resolution_matches_reference(F, golden, knobs, name):
    """The trainer's operators at the resolutions BASELINE.json quotes, from the networks' outputs (aa, t, (fs, cs), the disparity pyramid)
    through `pose_matrices` / `intrinsics`, the K0-FUSED reconstruction (the kernel pair `bench.py` times, here with the recorded
    tie-break tensor instead of the in-kernel draw) and the smoothness sweep, to the loss and the gradient of every network output —
    against what the REFERENCE produced on the same inputs (src/core/trainer.py:280-472 driven by tests/golden/make_golden.py)."""
    g = golden(name)
    leaves, static = case_inputs(g, device='cuda')
    scales, idxs = static['scales'], static['supp_idxs']
    n, b = leaves['aa'].shape[:2]
    h, w = static['imgs'].shape[-2:]
    inv = torch.tensor([bool(g['meta_always_fwd_pose']) and i < 0 for i in idxs for _ in range(b)], dtype=torch.uint8).cuda()
    Ts = F.pose_matrices(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1), inv).unflatten(0, (n, b))
    torch.testing.assert_close(Ts.detach().cpu(), g['out_Ts'], rtol=1e-5, atol=1e-6)
    if g['meta_learn_K']:
        K, K_inv = F.intrinsics(leaves['fs'], leaves['cs'], (h, w))
        torch.testing.assert_close(K.detach().cpu(), g['out_K'], rtol=1e-6, atol=1e-5)
    else: K, K_inv = static['K'], None
    flags = F.recon_flags(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask']))
    l_rec, err, sel, _, depth_up = F.image_recon_fused_disp([leaves[f'disp_{s}'] for s in scales], static['imgs'], static['supp_imgs'], Ts, K, K_inv, flags=flags,
                                                            min_depth=g['meta_min_depth'] or None, max_depth=g['meta_max_depth'] or None, noise=static['noise'])
    l_sm, _, _ = F.disp_smooth_fused({s: leaves[f'disp_{s}'] for s in scales}, static['imgs'], use_edges=bool(g['meta_use_edges']), want_aux=False)
    loss = l_rec + g['meta_w_smooth']*l_sm
    sel_own = impose_reference_routing(g, sel, knobs)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(l_rec.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    for k, s in enumerate(scales): torch.testing.assert_close(*ref_map(g, f'out_depth_up_{s}', depth_up[k].cpu()), rtol=2e-5, atol=1e-5)
    e_hip, e_ref = ref_map(g, 'mid_err', err.cpu().reshape(g['out_sel_all'].shape))
    assert ((e_hip - e_ref).abs() > 2e-4).float().mean().item() <= 1e-3
    report, ok = judge_against_reference_at_baseline_size(g, name, {k: v.grad for k, v in leaves.items()}, sel_own)
    parity_note(f'{name} (whole chain, K0 fused): loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f}; ' + '; '.join(report))
    assert ok, report


@pytest.mark.parametrize('name', TRAIN_CASES_BASELINE)
def test_single_node_loss_path_at_baseline_resolution_matches_reference(F, golden, knobs, name):
    """The entry point `bench.py` times and the trainer calls — `smd_loss_path_fwd/_bwd` (`functional.loss_path_fused`: reconstruction + smoothness + weighted
    sum as ONE autograd node, the pose / intrinsics chain rule inside its backward) — put on the REFERENCE's fixtures at the resolutions BASELINE.json quotes
    DIRECTLY (until now it was held to them through bit-equality with the separate operators): total loss, both terms, `depth_up`, the
    decision map, and the gradient of every network output (aa, t, (fs, cs), the disparity pyramid) under the reference's routing.  The tie-break noise is
    the in-kernel draw (this entry point takes a seed, not a tensor): it moves the loss by ~1e-7/sqrt(N) and decides exact ties only."""
    g = golden(name)
    leaves, static = case_inputs(g, device='cuda')
    scales, idxs = static['scales'], static['supp_idxs']
    n, b = leaves['aa'].shape[:2]
    h, w = static['imgs'].shape[-2:]
    if g['meta_loss_name'] != 'ssim' or not g['meta_use_edges']: pytest.skip('not the configuration the single-node operator serves')
    inv = torch.tensor([bool(g['meta_always_fwd_pose']) and i < 0 for i in idxs for _ in range(b)], dtype=torch.uint8).cuda()
    aa, t = leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1)              # views of the leaves: the backward hands their gradients over directly
    Ts = F.pose_matrices(aa, t, inv).unflatten(0, (n, b))
    if g['meta_learn_K']: K, K_inv = F.intrinsics(leaves['fs'], leaves['cs'], (h, w)); intr = (leaves['fs'], leaves['cs'])
    else: K, K_inv, intr = static['K'], None, None
    flags = F.recon_flags('ssim', bool(g['meta_use_min']), bool(g['meta_use_automask']))
    loss, l_rec, l_sm, sel, depth_up = F.loss_path_fused({s: leaves[f'disp_{s}'] for s in scales}, static['imgs'], static['supp_imgs'], Ts, K, K_inv,
                                                         pose=(aa, t, inv), intrinsics=intr, flags=flags, min_depth=g['meta_min_depth'] or None,
                                                         max_depth=g['meta_max_depth'] or None, seed=1234, w_recon=1.0, w_smooth=float(g['meta_w_smooth']))
    sel_own = impose_reference_routing(g, sel, knobs)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(l_rec.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(l_sm.detach().cpu(), g['out_loss_disp_smooth'], rtol=2e-5, atol=1e-7)
    for k, s in enumerate(scales): torch.testing.assert_close(*ref_map(g, f'out_depth_up_{s}', depth_up[k].cpu()), rtol=2e-5, atol=1e-5)
    report, ok = judge_against_reference_at_baseline_size(g, name, {k: v.grad for k, v in leaves.items()}, sel_own)
    parity_note(f'{name} (single node: smd_loss_path_fwd/_bwd): loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f}; ' + '; '.join(report))
    assert ok, report


# ---------------------------------------------------------------------------------------------------
# §8f rank 3: generic-channel errors, RegressionLoss and the other ViewSynth users, against the reference's vectors
@pytest.mark.parametrize('name,loss_name', [('op_photo_l2_c7', 'l2'), ('op_photo_l1_c4', 'l1'), ('op_photo_ssim_c5', 'ssim')])
def test_generic_channel_photo_errors(F, golden, name, loss_name):
    g = golden(name)
    pred = g['in_pred'].cuda().requires_grad_(True)
    err = F.photo_error(pred, g['in_target'].cuda(), loss_name)
    torch.testing.assert_close(err.cpu(), g['out_err'], rtol=1e-5, atol=2e-6)
    (err*g['in_ge'].cuda()).sum().backward()
    assert rel_to_max(pred.grad.cpu(), g['grad_pred']) < 2e-4


@pytest.mark.parametrize('name', ['op_photo_w0', 'op_photo_w03', 'op_photo_w1'])
def test_photo_error_weight_ssim(F, golden, name):
    """`PhotoError(weight_ssim)` away from 0.85 (src/losses/photometric.py:65-88): values and gradient against the reference's."""
    import slowtv_monodepth_amd as amd
    g = golden(name)
    pred = g['in_pred'].cuda().requires_grad_(True)
    err = amd.losses.PhotoError(weight_ssim=float(g['meta_weight_ssim']))(pred, g['in_target'].cuda())
    (err*g['in_ge'].cuda()).sum().backward()
    torch.testing.assert_close(err.detach().cpu(), g['out_err'], rtol=1e-5, atol=2e-5)
    assert rel_to_max(pred.grad.cpu(), g['grad_pred']) < 1e-3
    with pytest.raises(ValueError): amd.losses.PhotoError(weight_ssim=1.5)


@pytest.mark.parametrize('name', ['op_recon_mask_expla_min1_auto1_c3', 'op_recon_mask_uncer_min1_auto1_c3', 'op_recon_mask_uncer_min0_auto0_c3',
                                  'op_recon_mask_expla_min0_auto1_c1'])
def test_masked_reconstruction_loss(F, golden, name):
    """`ReconstructionLoss(mask_name='explainability'|'uncertainty')` with a predictive mask (src/losses/reconstruction.py:46-57,
    70-71): loss, automask and the gradients w.r.t. the warped images AND the mask against the reference's autograd."""
    import slowtv_monodepth_amd as amd
    g = golden(name)
    crit = amd.losses.ReconstructionLoss(loss_name='ssim', use_min=bool(g['meta_use_min']), use_automask=bool(g['meta_use_automask']), mask_name=g['meta_mask_name'])
    pred, mask = g['in_pred'].cuda().requires_grad_(True), g['in_mask'].cuda().requires_grad_(True)
    noise = g['in_noise'].cuda() if 'in_noise' in g else None
    loss, ld = crit(pred, g['in_target'].cuda(), source=g['in_source'].cuda(), mask=mask, noise=noise)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    # The routing decisions (winning support / automask) against the oracle's on the same inputs: a pixel whose two candidates tie
    # to ~1e-6 may be decided differently and then moves a whole G = 1/N of gradient from one mask channel to another, so the
    # gradients are compared where the decisions agree (the 3x3 neighbourhood of a flip is excluded for the image gradient) and
    # the flips are counted.
    n, b = g['in_pred'].shape[:2]
    with torch.no_grad():
        tg = g['in_target'].cuda()[None].expand(n, *g['in_target'].shape).flatten(0, 1)
        ew = F.photo_error(pred.detach().flatten(0, 1), tg).view(n, b, *pred.shape[-2:])
        es = F.photo_error(g['in_source'].cuda().flatten(0, 1), tg).view(n, b, *pred.shape[-2:]) if g['meta_use_automask'] else None
        _, _, sel = F.recon_reduce(ew, es, use_min=bool(g['meta_use_min']), noise=noise, mask=mask.detach(), mask_name=g['meta_mask_name'])
        _, out = O.recon_loss(g['in_pred'], g['in_target'], source=g['in_source'], use_min=bool(g['meta_use_min']), use_automask=bool(g['meta_use_automask']),
                              noise=g.get('in_noise'), mask=g['in_mask'], mask_name=g['meta_mask_name'])
    agree = sel.cpu() == out['sel'].reshape(sel.shape)                                       # (b,h,w)
    if g['meta_use_automask'] and g['meta_use_min']:   # where the identity error won, the mask's gradient goes to the static winner: a decision too
        mk = lambda e, m: O.apply_mask(e.permute(1, 0, 2, 3), m, g['meta_mask_name'])          # (n,b,h,w) errors -> masked (b,n,h,w)
        es_ref = O.compute_photo(g['in_source'], g['in_target'], 'ssim', True)[1]             # (b,n,h,w) un-masked per-support identity errors
        j_hip = mk(es.cpu(), mask.detach().cpu().expand(b, n, -1, -1)).argmin(1)
        j_ref = O.apply_mask(es_ref, g['in_mask'].expand(b, n, -1, -1), g['meta_mask_name']).argmin(1)
        agree &= (sel.cpu() != 255) | (j_hip == j_ref)
    flips = int((~agree).sum())
    assert flips <= 2, f'{flips} routing decisions differ from the oracle'
    near = torch.nn.functional.max_pool2d((~agree).float()[:, None], 3, 1, 1)[:, 0] > 0    # pixels whose SSIM window contains a flip
    keep_m = agree[:, None].expand_as(g['grad_mask']); keep_p = (~near)[None, :, None].expand_as(g['grad_pred'])
    parity_note(f'{name}: loss hip={loss.item():.8f} ref={g["out_loss"].item():.8f}; routing flips {flips} of {agree.numel()}')
    assert ((pred.grad.cpu() - g['grad_pred']).abs()*keep_p).max() < 1e-3*g['grad_pred'].abs().max()
    assert ((mask.grad.cpu() - g['grad_mask']).abs()*keep_m).max() < 1e-3*g['grad_mask'].abs().max()
    with pytest.raises(ValueError): crit(pred, g['in_target'].cuda(), source=g['in_source'].cuda())   # "Must provide a 'mask' when masking..."


def test_image_recon_handler_with_predictive_masks_matches_oracle(F):
    """`handlers.image_recon(crit, synth, depths, masks, ...)` with masks {s: (b,n,h,w)} (src/core/handlers.py:47, 62) on the un-fused
    operators against the oracle's restatement of the same call."""
    import slowtv_monodepth_amd as amd
    from slowtv_monodepth_amd.synthetic import make_batch
    b, h, w, n, S = 2, 24, 40, 2, 2
    _, y, _ = make_batch(b, h, w, (-1, 1), seed=5)
    g = torch.Generator().manual_seed(3)
    depths = {s: 0.5 + 5*torch.rand(b, 1, h, w, generator=g) for s in range(S)}
    masks = {s: 0.2*torch.randn(b, n, h, w, generator=g) for s in range(S)}
    Ts = torch.eye(4).repeat(n, b, 1, 1); Ts[..., :3, 3] = 0.05*torch.randn(n, b, 3, generator=g)
    noise = torch.randn(S*b, 1, h, w, generator=g)
    leaf = lambda t, dev: t.clone().to(dev).requires_grad_(True)

    def run(dev):
        d = {s: leaf(v, dev) for s, v in depths.items()}; m = {s: leaf(v, dev) for s, v in masks.items()}
        imgs, sup, K, T = y['imgs'].to(dev), y['supp_imgs'].to(dev), y['K'].to(dev), Ts.to(dev)
        if dev == 'cuda':
            crit = amd.losses.ReconstructionLoss('ssim', use_min=True, use_automask=True, mask_name='uncertainty')
            loss, _ = amd.handlers.image_recon(crit, amd.geometry.ViewSynth((h, w)), d, m, imgs, sup, T, K, noise=noise.to(dev))
        else:
            dep = torch.stack(list(d.values())).flatten(0, 1)
            src = sup[:, None].expand(n, S, *sup.shape[1:]).flatten(1, 2)
            tgt = imgs[None].expand(S, *imgs.shape).flatten(0, 1)
            warp = O.view_synth(src.flatten(0, 1), dep[None].expand(n, *dep.shape).flatten(0, 1), T[:, None].expand(n, S, b, 4, 4).flatten(0, 2),
                                K[None, None].expand(n, S, b, 4, 4).flatten(0, 2))[0].unflatten(0, (n, S*b))
            loss, _ = O.recon_loss(warp, tgt, source=src, use_min=True, use_automask=True, noise=noise,
                                   mask=torch.stack(list(m.values())).flatten(0, 1), mask_name='uncertainty')
        loss.backward()
        return loss.item(), [v.grad.cpu() for v in d.values()] + [v.grad.cpu() for v in m.values()]
    l_hip, g_hip = run('cuda'); l_ref, g_ref = run('cpu')
    assert abs(l_hip - l_ref) <= 2e-5*abs(l_ref)
    for a, r in zip(g_hip, g_ref): assert rel_to_max(a, r) < 1e-3


@pytest.mark.parametrize('use_edges', [True, False])
def test_laplacian_smoothness(F, golden, use_edges):
    """`SmoothReg(use_laplacian=True)` (src/regularizers/smooth.py:33-48): loss, aux maps, gradient against the reference's; and the
    multi-scale handler at non-integer ratios against the oracle."""
    import slowtv_monodepth_amd as amd
    g = golden(f'op_smooth_lap_edges{int(use_edges)}')
    disp = g['in_disp'].cuda().requires_grad_(True)
    reg = amd.regularizers.SmoothReg(use_edges=use_edges, use_laplacian=True)
    loss, ld = reg(disp, g['in_img'].cuda())
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ld['disp_grad'].cpu(), g['out_disp_grad'], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ld['image_grad'].cpu(), g['out_image_grad'], rtol=1e-4, atol=1e-5)
    assert rel_to_max(disp.grad.cpu(), g['grad_disp']) < 1e-3
    gen = torch.Generator().manual_seed(8)
    img = torch.rand(2, 3, 33, 47, generator=gen)
    lows = [(33, 47), (16, 23), (5, 7), (2, 3)]
    d_c = {s: (0.05 + 0.9*torch.rand(2, 1, *hw, generator=gen)).requires_grad_(True) for s, hw in enumerate(lows)}
    d_g = {s: v.detach().clone().cuda().requires_grad_(True) for s, v in d_c.items()}
    l_ref = torch.stack([O.smooth_reg(d, O.resize_bilinear(img, d.shape[-2:]), use_edges, use_laplacian=True)[0]/2**s for s, d in d_c.items()]).mean()
    l_ref.backward()
    l_hip, _ = amd.handlers.disp_smooth(reg, d_g, img.cuda(), want_aux=False)
    l_hip.backward()
    assert abs(l_hip.item() - l_ref.item()) <= 2e-5*abs(l_ref.item())
    for s in d_c: assert rel_to_max(d_g[s].grad.cpu(), d_c[s].grad) < 1e-3
    with pytest.raises(NotImplementedError): amd.regularizers.SmoothReg(use_blur=True, use_laplacian=True)


@pytest.mark.parametrize('use_edges', [True, False])
def test_blurred_smoothness(F, use_edges):
    """`SmoothReg(use_blur=True)` (src/regularizers/smooth.py:21: kornia's 3x3 Gaussian before every `compute_grad`), first-order form.  kornia is
    absent: the oracle restates `gaussian_blur2d` from its published source (F.pad reflect + depth-wise conv2d), PARITY UNPINNED.  The blur
    launch and its adjoint, the regulariser (loss, aux maps, gradient) and the multi-scale handler at non-integer ratios against the oracle."""
    import slowtv_monodepth_amd as amd
    gen = torch.Generator().manual_seed(21)
    for shape in [(2, 3, 2, 2), (1, 1, 2, 9), (2, 3, 7, 5), (3, 2, 33, 70), (1, 4, 64, 130)]:
        x = torch.rand(*shape, generator=gen); g = torch.randn(*shape, generator=gen)
        xc = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
        yc = O.gaussian_blur3x3(xc); yc.backward(g)
        yg = F.gaussian_blur3x3(xg); yg.backward(g.cuda())
        torch.testing.assert_close(yg.detach().cpu(), yc.detach(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(xg.grad.cpu(), xc.grad, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError): F.gaussian_blur3x3(torch.rand(1, 1, 1, 5, device='cuda'))   # reflect padding by one needs two pixels (F.pad raises too)
    reg = amd.regularizers.SmoothReg(use_edges=use_edges, use_blur=True)
    img = torch.rand(2, 3, 33, 47, generator=gen)
    d0 = 0.05 + 0.9*torch.rand(2, 1, 33, 47, generator=gen)
    dc = d0.clone().requires_grad_(True); dg = d0.cuda().requires_grad_(True)
    l_ref, ld_ref = O.smooth_reg(dc, img, use_edges, use_blur=True); l_ref.backward()
    l_hip, ld = reg(dg, img.cuda()); l_hip.backward()
    torch.testing.assert_close(l_hip.detach().cpu(), l_ref.detach(), rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ld['disp_grad'].cpu(), ld_ref['disp_grad'].detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ld['image_grad'].cpu(), ld_ref['image_grad'], rtol=1e-4, atol=1e-5)
    assert rel_to_max(dg.grad.cpu(), dc.grad) < 1e-3
    lows = [(33, 47), (16, 23), (5, 7), (2, 3)]
    d_c = {s: (0.05 + 0.9*torch.rand(2, 1, *hw, generator=gen)).requires_grad_(True) for s, hw in enumerate(lows)}
    d_g = {s: v.detach().clone().cuda().requires_grad_(True) for s, v in d_c.items()}
    l_ref = torch.stack([O.smooth_reg(d, O.resize_bilinear(img, d.shape[-2:]), use_edges, use_blur=True)[0]/2**s for s, d in d_c.items()]).mean()
    l_ref.backward()
    l_hip, _ = amd.handlers.disp_smooth(reg, d_g, img.cuda(), want_aux=False)
    l_hip.backward()
    assert abs(l_hip.item() - l_ref.item()) <= 2e-5*abs(l_ref.item())
    for s in d_c: assert rel_to_max(d_g[s].grad.cpu(), d_c[s].grad) < 1e-3, s


@pytest.mark.parametrize('name', [f'op_regr_{l}{i}{m}' for l in ('l1', 'log_l1', 'berhu') for i in ('', '_inv') for m in ('', '_mask')])
def test_regression_loss_matches_reference(F, golden, name):
    import slowtv_monodepth_amd as amd
    g = golden(name)
    loss_name = name[len('op_regr_'):].replace('_mask', '').replace('_inv', '')
    pred = g['in_pred'].cuda().requires_grad_(True)
    crit = amd.losses.RegressionLoss(loss_name=loss_name, invert='_inv' in name)
    l, ld = crit(pred, g['in_target'].cuda(), g['in_mask'].cuda() if g['meta_has_mask'] else None)
    torch.testing.assert_close(l.cpu(), g['out_loss'], rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(ld['err_regr'].cpu(), g['out_err'], rtol=2e-6, atol=1e-7)
    l.backward()
    torch.testing.assert_close(pred.grad.cpu(), g['grad_pred'], rtol=2e-5, atol=1e-8)


def _gpu_poses(F, g):
    aa, t = g['in_aa'].cuda().requires_grad_(True), g['in_t'].cuda().requires_grad_(True)
    n, b = aa.shape[:2]
    return aa, t, F.pose_matrices(aa.flatten(0, 1), t.flatten(0, 1)).unflatten(0, (n, b))


def test_feat_recon_handler_matches_reference(F, golden):
    import slowtv_monodepth_amd as amd
    g = golden('hd_feat_recon')
    depth = g['in_depth'].cuda().requires_grad_(True)
    aa, t, Ts = _gpu_poses(F, g)
    crit = amd.losses.ReconstructionLoss(loss_name='l2', use_min=True, use_automask=True)
    l, ld = amd.handlers.feat_recon(crit, None, {0: depth}, None, g['in_feats'].cuda(), g['in_supp_feats'].cuda(), Ts, g['in_K'].cuda(),
                                    noise=g['in_noise'].cuda())
    torch.testing.assert_close(l.cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ld['supp_feats_warp'].cpu(), g['out_supp_feats_warp'], rtol=1e-4, atol=1e-4)
    l.backward()
    for k, v in (('depth', depth), ('aa', aa), ('t', t)): assert rel_to_max(v.grad.cpu(), g[f'grad_{k}']) < 1e-3, k


def test_autoenc_recon_handler_matches_reference(F, golden):
    import slowtv_monodepth_amd as amd
    g = golden('hd_autoenc_recon')
    preds = {s: g[f'in_pred_{s}'].cuda().requires_grad_(True) for s in (0, 1)}
    spreds = {s: g[f'in_supp_pred_{s}'].cuda().requires_grad_(True) for s in (0, 1)}
    l, _ = amd.handlers.autoenc_recon(amd.losses.ReconstructionLoss(loss_name='ssim', use_min=False), preds, g['in_targets'].cuda(), spreds,
                                      g['in_supp_targets'].cuda())
    torch.testing.assert_close(l.cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    l.backward()
    for s in (0, 1):
        assert rel_to_max(preds[s].grad.cpu(), g[f'grad_pred_{s}']) < 2e-4
        assert rel_to_max(spreds[s].grad.cpu(), g[f'grad_supp_pred_{s}']) < 2e-4


def test_stereo_const_handler_matches_reference(F, golden):
    import slowtv_monodepth_amd as amd
    g = golden('hd_stereo_const')
    mk = lambda key: {s: g[f'in_{key}_{s}'].cuda().requires_grad_(True) for s in (0, 1)}
    disps, disps_st = mk('disp'), mk('disp_stereo')
    to_depth = lambda d: F.disp_to_depth([d], tuple(d.shape[-2:]), 0.1, 100)[0][0]
    depths = {s: to_depth(d) for s, d in disps.items()}; depths_st = {s: to_depth(d) for s, d in disps_st.items()}
    l, ld = amd.handlers.stereo_const(amd.losses.RegressionLoss(loss_name='l1'), None, disps, depths, disps_st, depths_st,
                                      g['in_T_stereo'].cuda(), g['in_K'].cuda())
    torch.testing.assert_close(l.cpu(), g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ld['disps_warp'].cpu(), g['out_disps_warp'], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ld['stereo_disps_warp'].cpu(), g['out_stereo_disps_warp'], rtol=1e-4, atol=1e-5)
    l.backward()
    for s in (0, 1):
        assert rel_to_max(disps[s].grad.cpu(), g[f'grad_disp_{s}']) < 1e-3
        assert rel_to_max(disps_st[s].grad.cpu(), g[f'grad_disp_stereo_{s}']) < 1e-3


@pytest.mark.parametrize('tag', ['berhu', 'log_l1_inv', 'l1_noauto'])
def test_depth_regr_handler_matches_reference(F, golden, tag):
    import slowtv_monodepth_amd as amd
    g = golden(f'hd_depth_regr_{tag}')
    disps = {s: g[f'in_disp_{s}'].cuda().requires_grad_(True) for s in (0, 1)}
    to_depth = lambda d: F.disp_to_depth([d], tuple(d.shape[-2:]), 0.1, 100)[0][0]
    depths = {s: to_depth(d) for s, d in disps.items()}
    photo = amd.losses.ReconstructionLoss(loss_name='ssim', use_min=True, use_automask=True).compute_photo
    crit = amd.losses.RegressionLoss(loss_name=g['meta_loss_name'], invert=bool(g['meta_invert']), use_automask=bool(g['meta_use_automask']))
    l, ld = amd.handlers.depth_regr(crit, None, photo, depths, g['in_hints'].cuda(), g['in_imgs'].cuda(), g['in_supp_imgs'].cuda(),
                                    g['in_Ts'].cuda(), g['in_K'].cuda())
    flips = (ld['mask_regr'].cpu() != g['out_mask_regr']).float().mean().item()
    assert flips <= 2e-3, f'regression mask differs on {flips:.2%} of pixels'
    torch.testing.assert_close(l.cpu(), g['out_loss'], rtol=2e-3 if flips else 2e-5, atol=1e-7)
    l.backward()
    for s in (0, 1): assert rel_to_max(disps[s].grad.cpu(), g[f'grad_disp_{s}']) < (2e-2 if flips else 2e-4), s


def test_depth_hint_fusion_like_the_offline_tool(F):
    """api/data/preprocess/compute_kitti_hints.py:88-97: warp the stereo frame with H depth hypotheses, take the per-pixel
    argmin of the photometric error.  Class-level operators against the oracle."""
    from oracle import view_synth_oracle as O
    import slowtv_monodepth_amd as amd
    gen = torch.Generator().manual_seed(9)
    H, h, w = 12, 40, 96
    img = torch.rand(1, 3, h, w, generator=gen); supp = torch.rand(1, 3, h, w, generator=gen)
    depths = 1 + 40*torch.rand(H, 1, h, w, generator=gen)
    T = torch.eye(4)[None].repeat(H, 1, 1); T[:, 0, 3] = -0.54
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(H, 1, 1)
    warp_o = O.view_synth(supp.expand(H, -1, -1, -1), depths, T, K)[0]
    err_o = O.photo_error(warp_o, img.expand(H, -1, -1, -1))
    warp, _, _ = amd.geometry.ViewSynth((h, w))(supp.expand(H, -1, -1, -1).cuda(), depths.cuda(), T.cuda(), K.cuda())
    err = amd.losses.PhotoError()(warp, img.expand(H, -1, -1, -1).cuda())
    torch.testing.assert_close(err.cpu(), err_o, rtol=1e-4, atol=2e-5)
    srt = err_o.sort(dim=0)[0]
    decided = (srt[1] - srt[0]) > 1e-4      # ignore pixels whose two best hypotheses are tied to rounding
    assert (err.argmin(dim=0).cpu() == err_o.argmin(dim=0))[decided].all()


# ---------------------------------------------------------------------------------------------------
# §8f rank 4: decoder glue kernels.  Floating-point element-wise/gather kernels: the reference here is the ATen composition
# the reference decoder itself calls (F.pad reflect / F.elu / F.interpolate nearest / cat).
@pytest.mark.parametrize('shape', [(2, 5, 2, 2), (2, 3, 7, 9), (1, 16, 24, 40)])
@pytest.mark.parametrize('apply_elu', [True, False])
def test_elu_pad_kernel(F, shape, apply_elu):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=gen)
    xr = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
    ref = TF.pad(TF.elu(xr) if apply_elu else xr, (1, 1, 1, 1), mode='reflect')
    out = F.elu_pad(xg, None, apply_elu)
    g = torch.randn(ref.shape, generator=gen)
    ref.backward(g); out.backward(g.cuda())
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(xg.grad.cpu(), xr.grad, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('B,Ca,Cs,h,w', [(2, 3, 0, 1, 1), (2, 4, 3, 1, 2), (2, 5, 2, 6, 9), (1, 16, 8, 12, 20)])
def test_elu_up_cat_pad_kernel(F, B, Ca, Cs, h, w):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(4)
    a = torch.randn(B, Ca, h, w, generator=gen); skip = torch.randn(B, Cs, 2*h, 2*w, generator=gen) if Cs else None
    ar = a.clone().requires_grad_(True); ag = a.cuda().requires_grad_(True)
    sr = skip.clone().requires_grad_(True) if Cs else None; sg = skip.cuda().requires_grad_(True) if Cs else None
    up = TF.interpolate(TF.elu(ar), scale_factor=2, mode='nearest')
    ref = TF.pad(torch.cat((up, sr), 1) if Cs else up, (1, 1, 1, 1), mode='reflect')
    out = F.elu_up_cat_pad(ag, sg)
    g = torch.randn(ref.shape, generator=gen)
    ref.backward(g); out.backward(g.cuda())
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ag.grad.cpu(), ar.grad, rtol=1e-5, atol=1e-5)
    if Cs: torch.testing.assert_close(sg.grad.cpu(), sr.grad, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('B,C,h,w', [(2, 16, 50, 70), (1, 128, 24, 80), (3, 5, 2, 2), (2, 32, 17, 129), (1, 64, 96, 64), (12, 16, 192, 640)])
@pytest.mark.parametrize('act', ['sigmoid', None])
def test_conv3x3_head_kernel(F, B, C, h, w, act):
    """The decoder's one-channel output heads (src/networks/decoders/monodepth.py:52, 86-87) as a stencil (`smd_conv3x3_head_*`, round 5) against
    ATen's `conv2d` (+ `sigmoid`) in fp64 on the same padded input: output, and the gradients w.r.t. input, weight and bias; sizes off the 64 x 16 tiles,
    the smallest legal image, the widest head (128 channels) and cfg 2's full-resolution head."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w)
    xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen)
    wt = torch.randn(1, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    bs = torch.randn(1, device='cuda', generator=gen)
    gy = torch.randn(B, 1, h, w, device='cuda', generator=gen)
    refs = {}
    for bias in (bs, None):
        L = [t.clone().requires_grad_(True) for t in (xp, wt)] + ([bias.clone().requires_grad_(True)] if bias is not None else [])
        y = F.conv3x3_head(L[0], L[1], L[2] if bias is not None else None, act)
        y.backward(gy)
        R = [t.double().clone().requires_grad_(True) for t in (xp, wt)] + ([bias.double().clone().requires_grad_(True)] if bias is not None else [])
        yr = TF.conv2d(R[0], R[1], R[2] if bias is not None else None)
        if act == 'sigmoid': yr = torch.sigmoid(yr)
        yr.backward(gy.double())
        assert rel_to_max(y.double(), yr) <= 2e-6, rel_to_max(y.double(), yr)
        for nm, a, r in zip(('g_xp', 'g_weight', 'g_bias'), L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6, (nm, rel_to_max(a.grad.double(), r.grad))
        refs[bias is not None] = R
    # only the weights ask for a gradient (a frozen encoder side), and only the input: the values of the full backward (every subset, bit for bit:
    # test_gpu_grad_subsets.py)
    L = [xp.clone(), wt.clone().requires_grad_(True)]
    F.conv3x3_head(L[0], L[1], None, act).backward(gy); assert rel_to_max(L[1].grad.double(), refs[False][1].grad) <= 2e-6
    L = [xp.clone().requires_grad_(True), wt.clone()]
    F.conv3x3_head(L[0], L[1], bs, act).backward(gy); assert L[1].grad is None and rel_to_max(L[0].grad.double(), refs[True][0].grad) <= 2e-6
    with pytest.raises(ValueError): F.conv3x3_head(xp, wt.repeat(2, 1, 1, 1), None, act)
    with pytest.raises(RuntimeError): F.conv3x3_head(xp.cpu(), wt.cpu(), None, act)


@pytest.mark.parametrize('B,C,h,w', [(2, 16, 50, 70), (1, 16, 2, 2), (3, 16, 17, 129), (2, 32, 33, 65), (1, 32, 96, 320), (3, 16, 13, 128), (2, 16, 8, 64), (12, 16, 192, 640)])
def test_conv3x3_thin_kernel(F, B, C, h, w):
    """The decoder's thin up-convolution (sixteen output channels; src/networks/decoders/monodepth.py:45-50, 80-84) as a direct convolution
    (`smd_conv3x3_thin_*`, round 5: fp32 MFMA) against ATen's `conv2d` in fp64 on the same padded input: output and both gradients; sizes off the 64 x 4 tiles,
    the smallest legal image, both input widths the library serves and cfg 2's full-resolution layer."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w)
    xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen)
    wt = torch.randn(16, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, 16, h, w, device='cuda', generator=gen)
    L = [t.clone().requires_grad_(True) for t in (xp, wt)]
    y = F.conv3x3_thin(L[0], L[1]); y.backward(gy)
    R = [t.double().clone().requires_grad_(True) for t in (xp, wt)]
    yr = TF.conv2d(R[0], R[1]); yr.backward(gy.double())
    assert rel_to_max(y.double(), yr) <= 2e-6, rel_to_max(y.double(), yr)
    for nm, a, r in zip(('g_xp', 'g_weight'), L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6, (nm, rel_to_max(a.grad.double(), r.grad))
    L = [xp.clone(), wt.clone().requires_grad_(True)]
    F.conv3x3_thin(L[0], L[1]).backward(gy); assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6
    L = [xp.clone().requires_grad_(True), wt.clone()]
    F.conv3x3_thin(L[0], L[1]).backward(gy); assert rel_to_max(L[0].grad.double(), R[0].grad) <= 2e-6
    with pytest.raises(ValueError): F.conv3x3_thin(xp, wt[:8])
    from slowtv_monodepth_amd._lib import Unsupported
    with pytest.raises(Unsupported): F.conv3x3_thin(xp[:, :5].contiguous(), wt[:, :5].contiguous())


@pytest.mark.parametrize('B,C,CO,h,w', [(2, 16, 32, 5, 7), (2, 48, 64, 9, 70), (1, 32, 32, 33, 65), (2, 96, 32, 13, 100), (2, 32, 96, 7, 33), (2, 64, 128, 4, 20),
                                         (1, 16, 32, 1, 1), (3, 160, 64, 6, 20), (2, 512, 256, 6, 20), (12, 96, 32, 96, 320), (12, 128, 64, 24, 80), (12, 16, 64, 96, 160), (12, 32, 64, 64, 192),
                                         (2, 16, 16, 7, 70), (1, 16, 16, 2, 2), (2, 32, 16, 9, 33), (3, 16, 16, 13, 129), (12, 16, 16, 192, 640), (12, 32, 16, 96, 320)])
def test_conv3x3_mfma_kernel(F, B, C, CO, h, w):
    """The decoder's wide up-convolutions (src/networks/decoders/monodepth.py:40-50, 71-84) on the bf16 matrix cores with every fp32 operand split exactly
    into three bf16 pieces (`smd_conv3x3_mfma_*`, round 6) against ATen's `conv2d` in fp64 on the same padded input: output and both gradients, held to the
    bound the f32-MFMA kernels are held to (2e-6 of the tensor's max; MIOpen's fp32 kernels sit at 2-8e-7 on these shapes, these at 1e-7 - 1e-6:
    profiles/r06_decoder_convs.txt).  Sizes off both tile shapes (64 x 4 and 32 x 8 pixels), the smallest image, channel counts off the weight gradient's
    128-channel blocks (ConvNeXt's 160), a K-split shape (6 x 20 at 512 -> 256), two of cfg 2's own wide layers, and the thin last stage (sixteen output
    channels: the 16 x 16 x 32 form of the instruction, two taps per K step) incl. both of cfg 2's thin layers."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + CO + h + w)
    xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen)
    wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, CO, h, w, device='cuda', generator=gen)
    L = [t.clone().requires_grad_(True) for t in (xp, wt)]
    y = F.conv3x3_mfma(L[0], L[1]); y.backward(gy)
    R = [t.double().clone().requires_grad_(True) for t in (xp, wt)]
    yr = TF.conv2d(R[0], R[1]); yr.backward(gy.double())
    assert rel_to_max(y.double(), yr) <= 2e-6, rel_to_max(y.double(), yr)
    for nm, a, r in zip(('g_xp', 'g_weight'), L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6, (nm, rel_to_max(a.grad.double(), r.grad))
    y2 = F.conv3x3_mfma(xp, wt)                                   # deterministic: the same bits on a second call
    assert torch.equal(y2, y.detach())
    from slowtv_monodepth_amd import _lib                          # ... and with two channel tiles over one staged patch (launch-shape knob, default off)
    try:
        _lib.set_knob('conv_two_tiles', 1)
        assert torch.equal(F.conv3x3_mfma(xp, wt), y.detach())
    finally: _lib.reset_knobs()
    L = [xp.clone(), wt.clone().requires_grad_(True)]
    F.conv3x3_mfma(L[0], L[1]).backward(gy)                          # only the weights ask for a gradient, and only the input
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6
    L = [xp.clone().requires_grad_(True), wt.clone()]
    F.conv3x3_mfma(L[0], L[1]).backward(gy); assert rel_to_max(L[0].grad.double(), R[0].grad) <= 2e-6


def test_conv3x3_mfma_refuses_what_it_does_not_tile(F):
    from slowtv_monodepth_amd._lib import Unsupported
    xp = torch.randn(1, 16, 6, 6, device='cuda')
    with pytest.raises(Unsupported): F.conv3x3_mfma(torch.randn(1, 48, 6, 6, device='cuda'), torch.randn(16, 48, 3, 3, device='cuda'))   # 16 output channels: 16 or 32 inputs only
    with pytest.raises(Unsupported): F.conv3x3_mfma(xp[:, :5].contiguous(), torch.randn(32, 5, 3, 3, device='cuda'))
    with pytest.raises(ValueError): F.conv3x3_mfma(xp, torch.randn(32, 8, 3, 3, device='cuda'))
    with pytest.raises(RuntimeError): F.conv3x3_mfma(xp.cpu(), torch.randn(32, 16, 3, 3))


@pytest.mark.parametrize('B,C,CO,h,w', [(2, 16, 16, 7, 70), (2, 32, 16, 9, 33), (2, 64, 64, 9, 70), (2, 96, 32, 13, 100), (2, 512, 256, 6, 20), (12, 16, 16, 384, 640), (3, 32, 16, 192, 320)])
def test_conv3x3_mfma_bf16_tensors(F, B, C, CO, h, w):
    """The decoder under bf16 autocast (BASELINE cfg 5 = the reference's `cfg/kbr/default.yaml`: bf16-mixed): bf16 activations in and out, ONE bf16 product per
    product, the fp32 weights as their bf16 rounding (what autocast hands a bf16 convolution), fp32 accumulation, fp32 weight gradient
    (`smd_conv3x3_mfma_*`, pieces = 1).  Against fp64 `conv2d` on the SAME rounded operands: bf16 outputs to half an ulp of bf16 (2^-9 of the value, i.e.
    <= 4e-3 of the tensor's max), the fp32 weight gradient to 1e-5 (its products are exact, only the order of the fp32 sums differs).  Incl. cfg 5's two thin
    layers at full size."""
    import torch.nn.functional as TF
    BF = torch.bfloat16
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + CO + h + w)
    xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen).to(BF)
    wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, CO, h, w, device='cuda', generator=gen).to(BF)
    L = [xp.clone().requires_grad_(True), wt.clone().requires_grad_(True)]
    y = F.conv3x3_mfma(L[0], L[1]); y.backward(gy)
    assert y.dtype == BF and L[0].grad.dtype == BF and L[1].grad.dtype == torch.float32
    R = [xp.double().requires_grad_(True), wt.to(BF).double().requires_grad_(True)]
    yr = TF.conv2d(R[0], R[1]); yr.backward(gy.double())
    assert rel_to_max(y.double(), yr) <= 4e-3, rel_to_max(y.double(), yr)
    assert rel_to_max(L[0].grad.double(), R[0].grad) <= 4e-3, rel_to_max(L[0].grad.double(), R[0].grad)
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 1e-5, rel_to_max(L[1].grad.double(), R[1].grad)
    assert torch.equal(F.conv3x3_mfma(xp, wt), y.detach())        # deterministic


@pytest.mark.parametrize('B,C,h,w', [(2, 16, 50, 70), (1, 128, 24, 80), (2, 32, 17, 129), (12, 16, 384, 640)])
def test_conv3x3_head_bf16_activation(F, B, C, h, w):
    """The output heads on a bf16 padded activation (`SMD_HEAD_X_BF16`; the decoder under bf16 autocast): fp32 output and weight gradient against fp64 on the
    same rounded input (2e-6), `g_xp` back in bf16 (half an ulp: 4e-3 of the max)."""
    import torch.nn.functional as TF
    BF = torch.bfloat16
    gen = torch.Generator(device='cuda').manual_seed(B*1000 + C*10 + h + w)
    xp = torch.randn(B, C, h + 2, w + 2, device='cuda', generator=gen).to(BF)
    wt = torch.randn(1, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5); bs = torch.randn(1, device='cuda', generator=gen)
    gy = torch.randn(B, 1, h, w, device='cuda', generator=gen)
    L = [xp.clone().requires_grad_(True), wt.clone().requires_grad_(True), bs.clone().requires_grad_(True)]
    y = F.conv3x3_head(L[0], L[1], L[2], 'sigmoid'); y.backward(gy)
    assert y.dtype == torch.float32 and L[0].grad.dtype == BF
    R = [t.double().clone().requires_grad_(True) for t in (xp, wt, bs)]
    yr = torch.sigmoid(TF.conv2d(R[0], R[1], R[2])); yr.backward(gy.double())
    assert rel_to_max(y.double(), yr) <= 2e-6
    assert rel_to_max(L[0].grad.double(), R[0].grad) <= 4e-3
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6 and rel_to_max(L[2].grad.double(), R[2].grad) <= 2e-6


def test_conv3x3_wide_routes_by_ab_and_agrees(F):
    """`conv3x3_wide` = the same convolution with each operator served by whichever of the MFMA kernels and MIOpen won this box's A/B for the shape: whatever
    the routes are, results agree with fp64 to the fp32 bound, the decisions are recorded, and pinning the route changes nothing but rounding."""
    import torch.nn.functional as TF
    gen = torch.Generator(device='cuda').manual_seed(11)
    xp = torch.randn(4, 64, 26, 82, device='cuda', generator=gen); wt = torch.randn(32, 64, 3, 3, device='cuda', generator=gen)/24; gy = torch.randn(4, 32, 24, 80, device='cuda', generator=gen)
    R = [t.double().clone().requires_grad_(True) for t in (xp, wt)]
    yr = TF.conv2d(R[0], R[1]); yr.backward(gy.double())
    try:
        for mode in ('auto', 'mfma', 'miopen'):
            F.set_conv_route(mode)
            L = [t.clone().requires_grad_(True) for t in (xp, wt)]
            y = F.conv3x3_wide(L[0], L[1]); y.backward(gy)
            assert rel_to_max(y.double(), yr) <= 2e-6
            for a, r in zip(L, R): assert rel_to_max(a.grad.double(), r.grad) <= 2e-6
            if mode == 'auto':
                routes = F.conv_routes()
                assert {k[0] for k in routes} == {'fwd', 'data', 'wgt'} and all(k[1:] == (4, 64, 32, 24, 80) for k in routes), routes
                print('routes:', {k[0]: (v[0], round(v[1], 1), round(v[2], 1)) for k, v in routes.items()})
    finally:
        F.set_conv_route('auto')


def test_glued_decoder_equals_plain_decoder(F):
    """The decoder with the glue kernels and the same decoder evaluated op by op (as the reference does) on the same weights."""
    import slowtv_monodepth_amd as amd
    torch.manual_seed(0)
    enc_ch, enc_sc = [64, 64, 128, 256, 512], [2, 4, 8, 16, 32]
    dec = amd.networks.decoders.MonodepthDecoder(enc_ch, enc_sc).cuda()
    feats = [torch.randn(2, c, 64//s, 96//s, device='cuda') for c, s in zip(enc_ch, enc_sc)]
    f1 = [f.clone().requires_grad_(True) for f in feats]; f2 = [f.clone().requires_grad_(True) for f in feats]
    out_g = dec(f1)
    out_p = _plain_decoder(dec, f2)
    gs = {i: torch.randn_like(o) for i, o in out_g.items()}
    sum((out_g[i]*gs[i]).sum() for i in out_g).backward()
    gp = [p.grad.clone() for p in dec.parameters()]
    dec.zero_grad()
    sum((out_p[i]*gs[i]).sum() for i in out_p).backward()
    for i in out_g: torch.testing.assert_close(out_g[i], out_p[i], rtol=1e-4, atol=1e-5)
    for a, b in zip(f1, f2): assert rel_to_max(a.grad, b.grad) < 1e-4
    for a, b in zip(gp, [p.grad for p in dec.parameters()]): assert rel_to_max(a, b) < 1e-4


def _plain_decoder(dec, feat):
    import torch.nn.functional as TF
    out, x = {}, feat[-1]
    for i in range(4, -1, -1):
        x = TF.interpolate(dec.up0[str(i)](x), scale_factor=2, mode='nearest')
        if dec.use_skip and 2**i in dec.enc_sc: x = torch.cat((x, feat[dec.enc_sc.index(2**i)]), 1)
        x = dec.up1[str(i)](x)
        if i in dec.out_sc: out[i] = dec.act(dec.out[str(i)](x))
    return out


# ---------------------------------------------------------------------------------------------------
# Producer side: BatchNorm (+ residual, + ReLU) kernels against ATen's batch_norm / add / relu
# (1, 2, 128, 128): N*HW = 16384, the last single-launch shape (a thread's register-kept values plus the re-read part); (1, 2, 101, 101): the same in 1-float steps;
# (1, 2, 4097, 4): 16388, the first chunked one; (3, 2, 4, 2049): HW = 8196, sample boundaries inside a chunk and inside a thread's stride
@pytest.mark.parametrize('shape', [(4, 8, 6, 20), (3, 5, 7, 9), (12, 64, 24, 80), (2, 130, 3, 5), (12, 6, 37, 41), (1, 2, 128, 128), (1, 2, 101, 101), (1, 2, 4097, 4),
                                   (3, 2, 4, 2049)])
@pytest.mark.parametrize('relu,res', [(False, False), (True, False), (True, True), (False, True)])
def test_batch_norm_act_kernel(F, shape, relu, res):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(8)
    N, C, H, W = shape
    x = (torch.randn(*shape, generator=gen)*2 + 3*torch.randn(1, C, 1, 1, generator=gen)).cuda()   # per-channel offsets: mean >> std for some
    r = torch.randn(*shape, generator=gen).cuda() if res else None
    w, b = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
    g = torch.randn(*shape, generator=gen).cuda()
    outs = []
    for fused in (True, False):   # the reference evaluation is ATen's batch_norm in fp64 on the CPU
        cast = (lambda t: t.clone()) if fused else (lambda t: t.detach().double().cpu())
        xx, ww, bb = cast(x).requires_grad_(True), cast(w).requires_grad_(True), cast(b).requires_grad_(True)
        rr = cast(r).requires_grad_(True) if res else None
        rm, rv = cast(torch.zeros(C, device='cuda')), cast(torch.ones(C, device='cuda'))
        if fused: y = F.batch_norm_act(xx, ww, bb, rm, rv, residual=rr, momentum=0.1, eps=1e-5, relu=relu)
        else:
            y = TF.batch_norm(xx, rm, rv, ww, bb, True, 0.1, 1e-5)
            if res: y = y + rr
            if relu: y = TF.relu(y)
        y.backward(cast(g))
        outs.append([t.detach().double().cpu() if t is not None else None for t in (y, xx.grad, ww.grad, bb.grad, rr.grad if res else None, rm, rv)])
    names = ('y', 'g_x', 'g_weight', 'g_bias', 'g_residual', 'running_mean', 'running_var')
    for nm, a, e in zip(names, outs[0], outs[1]):
        if e is None: continue
        assert rel_to_max(a, e) < 2e-5, f'{nm}: {rel_to_max(a, e):.3e}'


def test_resnet_encoder_with_fused_batch_norm_equals_aten(F):
    from slowtv_monodepth_amd.networks import encoders as E
    torch.manual_seed(1)
    net = E.create_encoder('resnet18', in_chans=3).cuda().train()
    x = torch.randn(4, 3, 64, 96, device='cuda')
    res = []
    for fused in (True, False):
        E.BatchNormAct2d.fused_enabled = fused
        try:
            net.zero_grad()
            state = {k: v.clone() for k, v in net.state_dict().items()}
            feats = net(x)
            sum((f*f).mean() for f in feats).backward()
            res.append(([f.detach() for f in feats], [p.grad.clone() for p in net.parameters()], {k: v.clone() for k, v in net.state_dict().items()}))
            net.load_state_dict(state)   # same running statistics for the second evaluation
        finally:
            E.BatchNormAct2d.fused_enabled = True
    for a, b in zip(res[0][0], res[1][0]): assert rel_to_max(a, b) < 1e-4
    for a, b in zip(res[0][1], res[1][1]): assert rel_to_max(a, b) < 2e-3
    for k in res[0][2]: assert rel_to_max(res[0][2][k].float(), res[1][2][k].float()) < 1e-4, k


@pytest.mark.parametrize('shape', [(2, 3, 1, 1), (2, 3, 5, 8), (3, 4, 9, 7), (4, 16, 48, 160)])
def test_max_pool_kernel(F, shape):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(2)
    x = torch.relu(torch.randn(*shape, generator=gen)).cuda()     # post-ReLU input: many exact ties at 0, as in the stem
    xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ref = TF.max_pool2d(xr, 3, 2, 1); out = F.max_pool3x3s2(xg)
    g = torch.randn(ref.shape, generator=gen).cuda()
    ref.backward(g); out.backward(g)
    assert torch.equal(out, ref)
    torch.testing.assert_close(xg.grad, xr.grad, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('B,Ca,Cs,h,w', [(2, 4, 3, 3, 5), (3, 16, 8, 24, 40)])
def test_decoder_glue_with_bias(F, B, Ca, Cs, h, w):
    """The glue kernels add the (bias-free) convolution's bias and return its gradient."""
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(12)
    a = torch.randn(B, Ca, h, w, generator=gen); skip = torch.randn(B, Cs, 2*h, 2*w, generator=gen); bias = torch.randn(Ca, generator=gen)
    mk = lambda t, dev: t.clone().to(dev).requires_grad_(True)
    res = []
    for dev in ('cuda', 'cpu'):
        aa, ss, bb = mk(a.double() if dev == 'cpu' else a, dev), mk(skip.double() if dev == 'cpu' else skip, dev), mk(bias.double() if dev == 'cpu' else bias, dev)
        if dev == 'cuda':
            o1 = F.elu_up_cat_pad(aa, ss, bias=bb); o2 = F.elu_pad(aa, bb, True); o3 = F.elu_pad(aa, bb, False)
        else:
            pre = aa + bb[None, :, None, None]
            o1 = TF.pad(torch.cat((TF.interpolate(TF.elu(pre), scale_factor=2, mode='nearest'), ss), 1), (1, 1, 1, 1), mode='reflect')
            o2 = TF.pad(TF.elu(pre), (1, 1, 1, 1), mode='reflect'); o3 = TF.pad(pre, (1, 1, 1, 1), mode='reflect')
        g = torch.Generator().manual_seed(13)
        loss = sum((o*torch.randn(o.shape, generator=g).to(o)).sum() for o in (o1, o2, o3))
        loss.backward()
        res.append([t.detach().double().cpu() for t in (o1, o2, o3, aa.grad, ss.grad, bb.grad)])
    for nm, x, e in zip(('up_cat_pad', 'elu_pad', 'pad', 'g_a', 'g_skip', 'g_bias'), *res):
        assert rel_to_max(x, e) < 1e-5, f'{nm}: {rel_to_max(x, e):.3e}'


# ---------------------------------------------------------------------------------------------------
# Strip-boundary sweep: a wave covers 62 interior columns forward and 60 backward, strips split the rows; widths and
# heights around those boundaries (and degenerate 2-3 pixel images) against the oracle with random poses/depths.
SWEEP = [(1, 2, 2, 1, 1), (2, 3, 5, 2, 1), (1, 5, 59, 1, 2), (1, 7, 60, 2, 1), (1, 4, 61, 2, 2), (2, 6, 62, 3, 1), (1, 9, 63, 2, 1),
         (1, 5, 64, 1, 1), (1, 6, 65, 2, 2), (1, 3, 120, 2, 1), (1, 4, 121, 3, 1), (1, 5, 124, 2, 1), (1, 33, 125, 2, 2), (1, 70, 30, 4, 1),
         (1, 20, 70, 5, 1), (2, 9, 40, 6, 2), (1, 14, 66, 8, 1)]   # more than four supports: passes of four with a carried minimum


@pytest.mark.parametrize('b,h,w,n,S', SWEEP)
@pytest.mark.parametrize('mode', ['min_automask', 'mean'])
def test_strip_boundary_shapes_match_oracle(F, b, h, w, n, S, mode):
    from oracle import view_synth_oracle as O
    gen = torch.Generator().manual_seed(1000*h + w + n)
    imgs = torch.rand(b, 3, h, w, generator=gen); supp = (imgs[None] + 0.1*torch.randn(n, b, 3, h, w, generator=gen)).clamp(0, 1)
    depth = 1 + 10*torch.rand(S, b, 1, h, w, generator=gen)
    aa = 0.02*torch.randn(n*b, 3, generator=gen); t = 0.2*torch.randn(n*b, 3, generator=gen)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(b, 1, 1)
    noise = torch.randn(S*b, 1, h, w, generator=gen)
    use_min = use_auto = mode == 'min_automask'
    # oracle
    d_c = depth.clone().requires_grad_(True); T_c = O.T_from_AAt(aa, t).unflatten(0, (n, b)).clone().requires_grad_(True)
    loss_c, _, full = O.image_recon({s: d_c[s] for s in range(S)}, imgs, supp, T_c, K, 'ssim', use_min, use_auto, noise=noise)
    loss_c.backward()
    # HIP
    d_g = depth.cuda().requires_grad_(True); T_g = T_c.detach().cuda().requires_grad_(True)
    loss, err, sel, _ = F.image_recon_fused(d_g, imgs.cuda(), supp.cuda(), T_g, K.cuda(), flags=F.recon_flags('ssim', use_min, use_auto),
                                            noise=noise.cuda())
    loss.backward()
    flips = (sel.cpu() != full['sel']).flatten()
    assert flips.float().mean().item() <= 0.01, f'selection differs on {flips.float().mean().item():.2%} of pixels'
    torch.testing.assert_close(err.cpu().flatten()[~flips], full['err'].detach().flatten()[~flips], rtol=0, atol=3e-4)
    torch.testing.assert_close(loss.detach().cpu(), loss_c.detach(), rtol=1e-4, atol=1e-6)
    tol = 5e-2 if flips.any() else 2e-3
    assert rel_to_max(d_g.grad.cpu(), d_c.grad) < tol
    assert rel_to_max(T_g.grad.cpu()[..., :3, :], T_c.grad[..., :3, :]) < tol


@pytest.mark.parametrize('b,h,w,n,S,b2,rh,rh2', [(3, 37, 70, 2, 2, 1, 12, 5), (5, 50, 130, 3, 1, 2, 16, 4), (4, 24, 61, 1, 3, 3, 8, 6)])
def test_tapered_partition_gives_the_same_result(F, knobs, b, h, w, n, S, b2, rh, rh2):
    """The fused kernels cut the last samples of the dispatch order into shorter strips (load balance at the end of a launch).
    The partition must not change anything: same error map and selection bit for bit, same gradients up to the order of the
    per-strip partial sums."""
    gen = torch.Generator().manual_seed(h*w + b)
    imgs = torch.rand(b, 3, h, w, generator=gen).cuda(); supp = (imgs[None].cpu() + 0.1*torch.randn(n, b, 3, h, w, generator=gen)).clamp(0, 1).cuda()
    depth = (1 + 10*torch.rand(S, b, 1, h, w, generator=gen)).cuda()
    aa = 0.02*torch.randn(n*b, 3, generator=gen).cuda(); t = 0.2*torch.randn(n*b, 3, generator=gen).cuda()
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(b, 1, 1).cuda()
    noise = torch.randn(S*b, 1, h, w, generator=gen).cuda()

    def run(taper):
        for k in ('fwd_rh', 'bwd_rh'): knobs(k, rh)
        for k in ('fwd_taper_b', 'bwd_taper_b'): knobs(k, b2 if taper else 0)
        for k in ('fwd_taper_rh', 'bwd_taper_rh'): knobs(k, rh2)
        d = depth.clone().requires_grad_(True)
        T = F.pose_matrices(aa, t).unflatten(0, (n, b)).detach().requires_grad_(True)
        loss, err, sel, _ = F.image_recon_fused(d, imgs, supp, T, K, flags=F.recon_flags('ssim', True, True), noise=noise)
        loss.backward()
        return loss.detach(), err, sel, d.grad, T.grad

    l0, e0, s0, gd0, gT0 = run(False)
    l1, e1, s1, gd1, gT1 = run(True)
    assert torch.equal(e0, e1) and torch.equal(s0, s1)
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)
    assert torch.equal(gd0, gd1)
    torch.testing.assert_close(gT1, gT0, rtol=1e-4, atol=1e-7*gT0.abs().max().item())


@pytest.mark.parametrize('b,h,w,lows', [(2, 33, 47, [(33, 47), (16, 23), (8, 11)]), (1, 8, 12, [(8, 12), (4, 6), (2, 3), (1, 1)]),
                                        (1, 192, 640, [(96, 320), (24, 80)]), (2, 21, 30, [(7, 10), (5, 30)])])
@pytest.mark.parametrize('use_edges', [True, False])
def test_k0_and_smoothness_at_non_integer_ratios(F, b, h, w, lows, use_edges):
    """Disparity pyramids whose sizes are not exact halvings (odd images, anisotropic ratios): K0 forward/adjoint and the
    smoothness sweep against the oracle."""
    from oracle import view_synth_oracle as O
    gen = torch.Generator().manual_seed(h*w)
    imgs = torch.rand(b, 3, h, w, generator=gen)
    disps = {s: 0.05 + 0.9*torch.rand(b, 1, hs, ws, generator=gen) for s, (hs, ws) in enumerate(lows)}
    gup = torch.randn(len(lows), b, 1, h, w, generator=gen)
    dc = {s: d.clone().requires_grad_(True) for s, d in disps.items()}; dg = {s: d.cuda().requires_grad_(True) for s, d in disps.items()}
    _, dep_c = O.disp_to_depth_up(dc, (h, w), 0.1, 100)
    l_c, _ = O.disp_smooth(dc, imgs, use_edges)
    (sum((dep_c[s]*gup[s]).sum() for s in dc)*1e-3 + l_c).backward()
    dep_g, _ = F.disp_to_depth([dg[s] for s in dg], (h, w), 0.1, 100)
    l_g, _, _ = F.disp_smooth_fused(dg, imgs.cuda(), use_edges=use_edges, want_aux=False)
    ((dep_g*gup.cuda()).sum()*1e-3 + l_g).backward()
    for s in dc:
        torch.testing.assert_close(dep_g[s].cpu(), dep_c[s].detach(), rtol=2e-5, atol=1e-5)
        assert rel_to_max(dg[s].grad.cpu(), dc[s].grad) < 1e-3, s
    torch.testing.assert_close(l_g.detach().cpu(), l_c.detach(), rtol=2e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------------
# K0 fused into the reconstruction kernel: disparity pyramid in, loss + depth stack out
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TRAIN_CASES)
def test_k0_fused_path_matches_reference_fixtures(F, golden, knobs, name):
    """`image_recon_fused_disp` on the reference's recorded cases: the depth stack it writes against `out_depth_up_*`, the loss
    against `out_loss_img_recon`, and the gradients w.r.t. every disparity scale against the reference's own autograd."""
    g = golden(name)
    leaves, static = case_inputs(g, device='cuda')
    scales = static['scales']
    Ts = g['out_Ts'].cuda().requires_grad_(True)
    K = (g['out_K'] if g['meta_learn_K'] else g['in_K']).cuda()
    flags = F.recon_flags(g['meta_loss_name'], bool(g['meta_use_min']), bool(g['meta_use_automask']))
    l_rec, err, sel, warp0, depth_up = F.image_recon_fused_disp([leaves[f'disp_{s}'] for s in scales], static['imgs'], static['supp_imgs'], Ts, K, flags=flags,
                                                                min_depth=g['meta_min_depth'] or None, max_depth=g['meta_max_depth'] or None,
                                                                noise=static['noise'], want_warp=True)
    for k, s in enumerate(scales):
        torch.testing.assert_close(*ref_map(g, f'out_depth_up_{s}', depth_up[k].cpu()), rtol=2e-5, atol=1e-5)
    torch.testing.assert_close(l_rec.detach().cpu(), g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(*ref_map(g, 'out_supp_imgs_warp', warp0.cpu()), rtol=0, atol=1e-4)
    loss = l_rec
    if g['meta_w_smooth'] >= 0:
        l_sm, _, _ = F.disp_smooth_fused({s: leaves[f'disp_{s}'] for s in scales}, static['imgs'], use_edges=bool(g['meta_use_edges']), want_aux=False)
        loss = loss + g['meta_w_smooth']*l_sm
    if g.get('meta_compact'): sel_own = impose_reference_routing(g, sel, knobs)
    loss.backward()
    if g.get('meta_compact'):
        report, ok = judge_against_reference_at_baseline_size(g, name, {f'disp_{s}': leaves[f'disp_{s}'].grad for s in scales}, sel_own)
        parity_note(f'{name} (K0 fused): ' + '; '.join(report))
        assert ok, report
        return
    tol = 1e-2 if g['meta_loss_name'] == 'l1' else 1e-3
    for s in scales:
        e = rel_to_max(leaves[f'disp_{s}'].grad.cpu(), g[f'grad_disp_{s}'])
        assert e < tol, f'{name}: d loss / d disp_{s} off by {e:.3e} (rel. to max) vs the reference autograd'


@pytest.mark.parametrize('b,h,w,lows', [(2, 33, 47, [(33, 47), (16, 23), (8, 11)]), (1, 24, 36, [(24, 36), (12, 18), (6, 9), (3, 4)]),
                                        (1, 96, 128, [(48, 64), (12, 16)]), (2, 21, 30, [(7, 10), (5, 30)]),
                                        # even integer row ratios take the STREAMING vertical pass of the K0 adjoint (round 4): odd chunk counts, more than one
                                        # 256-column block, ratio 16, a column ratio unrelated to the row ratio
                                        (2, 50, 520, [(50, 520), (25, 260)]), (1, 64, 300, [(64, 300), (32, 150), (16, 75), (4, 19)]), (1, 48, 70, [(24, 70), (6, 9)])])
def test_k0_fused_path_at_non_integer_ratios_and_with_a_second_consumer_of_depth(F, b, h, w, lows):
    """Pyramids that are not exact halvings / have no full-resolution scale, and a second consumer of `depth_up` (as `depth_regr`
    is in the trainer): fused path == K0 kernel followed by the plain fused path, values and gradients."""
    gen = torch.Generator(device='cuda').manual_seed(h*w)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen); supp = torch.rand(2, b, 3, h, w, device='cuda', generator=gen)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    T0 = torch.eye(4, device='cuda').repeat(2, b, 1, 1); T0[..., :3, 3] = 0.05*torch.randn(2, b, 3, device='cuda', generator=gen)
    d0 = [0.05 + 0.9*torch.rand(b, 1, hs, ws, device='cuda', generator=gen) for hs, ws in lows]
    gup = torch.randn(len(lows), b, 1, h, w, device='cuda', generator=gen)
    noise = torch.randn(len(lows)*b, 1, h, w, device='cuda', generator=gen)
    flags = F.recon_flags('ssim', True, True)

    def run(fused):
        d = [v.clone().requires_grad_(True) for v in d0]
        T = T0.clone().requires_grad_(True)
        if fused: loss, err, sel, _, dep = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, noise=noise)
        else:
            dep, _ = F.disp_to_depth(d, (h, w), 0.1, 100)
            loss, err, sel, _ = F.image_recon_fused(dep, imgs, supp, T, K, flags=flags, noise=noise)
        (loss + 1e-3*(dep*gup).sum()).backward()
        return loss.detach(), err, sel, dep.detach(), [v.grad for v in d], T.grad
    la, ea, sa, da, ga, ta = run(True)
    lb, eb, sb, db, gb, tb = run(False)
    torch.testing.assert_close(da, db, rtol=1e-6, atol=1e-7)       # v_rcp in the fused kernel vs the K0 kernel's division
    flips = (sa != sb).float().mean().item()
    assert flips <= 1e-3 and ((ea - eb).abs() > 1e-4).float().mean().item() <= 1e-3
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-7)
    for x, y in zip(ga + [ta], gb + [tb]): assert rel_to_max(x, y) < (1e-3 if flips == 0 else 5e-2)


@pytest.mark.parametrize('b,h,w,n,lows,rh,b2', [(2, 33, 47, 2, [(33, 47), (16, 23), (8, 11), (4, 5)], 8, 0), (3, 50, 130, 1, [(50, 130), (25, 65), (12, 32), (6, 16)], 16, 1),
                                                 (5, 96, 200, 4, [(96, 200), (48, 100), (24, 50), (12, 25)], 16, 2), (2, 7, 66, 3, [(7, 66), (3, 33), (2, 16), (1, 8)], 4, 0),
                                                 (12, 192, 640, 2, [(192, 640), (96, 320), (48, 160), (24, 80)], 0, -1)])
def test_shared_target_ring_equals_per_wave_loads(F, knobs, b, h, w, n, lows, rh, b2):
    """Round 3: with four scales the hot forward instantiation runs the four scales of a strip in one block and brings the target-side
    rows in once per block through an LDS ring (LDS-DMA + one barrier per four rows).  Only the way those rows reach the wave
    changes: error map, selection and adopted depth must be bit-identical to the per-wave loads (knob `fwd_share` = 0), at image
    heights that are not multiples of four, strips shorter than an epoch, a tapered partition and the BASELINE size; the loss up to
    the order of the block partials."""
    gen = torch.Generator(device='cuda').manual_seed(h*w + n)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen); supp = torch.rand(n, b, 3, h, w, device='cuda', generator=gen)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    T = torch.eye(4, device='cuda').repeat(n, b, 1, 1); T[..., :3, 3] = 0.05*torch.randn(n, b, 3, device='cuda', generator=gen)
    d = [0.05 + 0.9*torch.rand(b, 1, hs, ws, device='cuda', generator=gen) for hs, ws in lows]
    flags = F.recon_flags('ssim', True, True)
    if rh:
        knobs('fwd_rh', rh); knobs('fwd_taper_b', b2); knobs('fwd_taper_rh', max(rh//2, 4))

    def run(share):
        knobs('fwd_share', share)
        loss, err, sel, _, dep = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, seed=7, want_err=True)
        return loss, err, sel, dep
    l1, e1, s1, d1 = run(1)
    l0, e0, s0, d0 = run(0)
    assert torch.equal(d1, d0) and torch.equal(e1, e0) and torch.equal(s1, s0)
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)
    assert torch.isfinite(l1) and (s1 != 255).any() and (s1 == 255).any()   # both the warped supports and the automask win somewhere


def test_row_skip_tuner_times_both_row_loops_and_gradients_do_not_depend_on_the_choice(F, monkeypatch):
    """The fused backward has two row loops (with / without dead-row skipping) that give the same gradients bit for bit;
    `functional.row_skip_tuner` alternates them over the first calls of a period, times them with HIP events and keeps the faster."""
    b, h, w, n = 4, 96, 320, 2
    gen = torch.Generator(device='cuda').manual_seed(3)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    T0 = torch.eye(4, device='cuda').repeat(n, b, 1, 1); T0[..., :3, 3] = 0.05*torch.randn(n, b, 3, device='cuda', generator=gen)
    d0 = [0.05 + 0.9*torch.rand(b, 1, h >> s, w >> s, device='cuda', generator=gen) for s in range(4)]
    flags = F.recon_flags('ssim', True, True)
    tuner = F.row_skip_tuner(torch.cuda.current_device())

    def step(supp):
        d = [v.clone().requires_grad_(True) for v in d0]; T = T0.clone().requires_grad_(True)
        loss, _, sel, _, _ = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, seed=2, want_err=False)
        loss.backward()
        return sel, [v.grad for v in d] + [T.grad]

    for name, supp in (('noise', torch.rand(n, b, 3, h, w, device='cuda', generator=gen)),                  # every support wins somewhere in every row
                       ('static', (imgs[None] + 0.2*torch.rand(n, b, 3, h, w, device='cuda', generator=gen)).clamp(0, 1))):   # the un-warped frames win: masked
        grads = {}
        for mode in ('2', '0'):                      # pinned by the environment: the tuner stays out of it
            monkeypatch.setenv('SMD_BWD_SKIP', mode)
            sel, grads[mode] = step(supp)
        assert all(torch.equal(x, y) for x, y in zip(grads['2'], grads['0'])), name
        monkeypatch.delenv('SMD_BWD_SKIP')
        tuner.calls, tuner.pending, tuner.samples, tuner.last, tuner.skip = 0, [], {True: [], False: []}, None, False
        for _ in range(tuner.settle + 2*tuner.trials): _, g = step(supp)
        assert all(torch.equal(x, y) for x, y in zip(g, grads['0'])), name
        torch.cuda.synchronize(); step(supp)         # the next call harvests the event pairs
        assert tuner.last is not None and not tuner.pending
        assert tuner.skip == (tuner.last['skipping_ms'] < tuner.margin*tuner.last['plain_ms'])
        shares = F.dead_tile_shares(sel, True, n).mean(1).tolist()
        print(f'row-skip tuner, {name} masks (skippable share per support {[round(v, 3) for v in shares]}): with skipping {tuner.last["skipping_ms"]*1e3:.1f} us, '
              f'plain {tuner.last["plain_ms"]*1e3:.1f} us -> {"dead-row skipping" if tuner.skip else "plain rows"}')
    tuner.calls, tuner.pending, tuner.samples, tuner.skip = 0, [], {True: [], False: []}, False


@pytest.mark.parametrize('shape', [(2, 3, 1, 1), (2, 5, 6, 20), (1, 4, 33, 65), (3, 8, 48, 160), (2, 6, 40, 70)])
def test_depthwise_conv7x7_kernel(F, shape):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(21)
    N, C, H, W = shape
    x = torch.randn(*shape, generator=gen); w = torch.randn(C, 1, 7, 7, generator=gen)*0.2; b = torch.randn(C, generator=gen)
    g = torch.randn(*shape, generator=gen)
    res = []
    for dev in ('cuda', 'cpu'):
        cast = (lambda t: t.clone().cuda()) if dev == 'cuda' else (lambda t: t.clone().double())
        xx, ww, bb = cast(x).requires_grad_(True), cast(w).requires_grad_(True), cast(b).requires_grad_(True)
        y = F.dwconv7x7(xx, ww, bb) if dev == 'cuda' else TF.conv2d(xx, ww, bb, padding=3, groups=C)
        y.backward(cast(g))
        res.append([t.detach().double().cpu() for t in (y, xx.grad, ww.grad, bb.grad)])
    for nm, a, e in zip(('y', 'g_x', 'g_weight', 'g_bias'), *res):
        assert rel_to_max(a, e) < 2e-5, f'{nm}: {rel_to_max(a, e):.3e}'


@pytest.mark.parametrize('shape', [(2, 3, 1, 1), (2, 96, 6, 20), (1, 7, 33, 65), (3, 128, 24, 40), (2, 1030, 5, 7), (1, 5, 91, 91)])   # (the last: 8281 pixels, two chunks of the gamma / beta reduction)
def test_channel_layer_norm_kernel(F, shape):
    import torch.nn.functional as TF
    gen = torch.Generator().manual_seed(31)
    N, C, H, W = shape
    x = torch.randn(*shape, generator=gen)*2 + 3*torch.randn(N, 1, H, W, generator=gen); w = torch.rand(C, generator=gen) + 0.5; b = torch.randn(C, generator=gen)
    g = torch.randn(*shape, generator=gen)
    res = []
    for dev in ('cuda', 'cpu'):
        cast = (lambda t: t.clone().cuda()) if dev == 'cuda' else (lambda t: t.clone().double())
        xx, ww, bb = cast(x).requires_grad_(True), cast(w).requires_grad_(True), cast(b).requires_grad_(True)
        y = F.layer_norm_cf(xx, ww, bb, 1e-6) if dev == 'cuda' else TF.layer_norm(xx.permute(0, 2, 3, 1), (C,), ww, bb, 1e-6).permute(0, 3, 1, 2)
        y.backward(cast(g))
        res.append([t.detach().double().cpu() for t in (y, xx.grad, ww.grad, bb.grad)])
    for nm, a, e in zip(('y', 'g_x', 'g_weight', 'g_bias'), *res):
        assert rel_to_max(a, e) < 3e-5, f'{nm}: {rel_to_max(a, e):.3e}'


def test_convnext_encoder_nchw_path_equals_reference_formulation(F):
    """ConvNeXt-T with the NCHW block (HIP depthwise + channel LayerNorm, 1x1-conv MLP) against the permute/Linear formulation."""
    from slowtv_monodepth_amd.networks import encoders as E
    torch.manual_seed(2)
    net = E.create_encoder('convnext_tiny', in_chans=3).cuda().train()
    for m in net.modules():
        if isinstance(m, E.ConvNeXtBlock): m.gamma.data.fill_(0.5)   # make the residual branch matter (layer scale starts at 1e-6)
    x = torch.randn(2, 3, 64, 96, device='cuda')
    res = []
    for fused in (True, False):
        E.BatchNormAct2d.fused_enabled = fused
        try:
            net.zero_grad()
            feats = net(x)
            sum((f*f).mean() for f in feats).backward()
            res.append(([f.detach() for f in feats], [p.grad.clone() for p in net.parameters()]))
        finally:
            E.BatchNormAct2d.fused_enabled = True
    for a, b in zip(res[0][0], res[1][0]): assert rel_to_max(a, b) < 2e-4
    for a, b in zip(res[0][1], res[1][1]): assert rel_to_max(a, b) < 5e-3


def test_training_cli_runs_and_the_loss_decreases(tmp_path, capsys):
    """`python -m slowtv_monodepth_amd.train` on the shipped cfg: two short epochs on a fixed synthetic batch."""
    from slowtv_monodepth_amd import train
    from conftest import ROOT
    train.main(['-c', str(ROOT/'cfg'/'kitti_resnet18.yaml'), '-o', str(tmp_path), '-n', 'cli', '--steps', '12', '--shape', '96', '160'])
    out = capsys.readouterr().out
    losses = [float(l.split('loss ')[1].split()[0]) for l in out.splitlines() if l.startswith('epoch')]
    assert len(losses) == 2 and all(l == l for l in losses) and losses[1] < losses[0]
    ckpt = torch.load(tmp_path/'cli'/'000'/'last.ckpt', map_location='cpu', weights_only=False)
    # the reference's Lightning layout and parameter names (networks/checkpoint.py)
    assert 'nets.depth.encoder.layer1.0.conv1.weight' in ckpt['state_dict'] and 'nets.depth.decoders.disp.decoder.0.conv.weight' in ckpt['state_dict']
    assert ckpt['epoch'] == 1 and 'optimizer_states' in ckpt


def test_channel_layer_norm_bf16_io(F):
    """bf16 output / bf16 incoming gradient (autocast consumer): same fp32 arithmetic, rounded once at the boundary."""
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(2, 48, 9, 11, generator=gen).cuda(); w = (torch.rand(48, generator=gen) + 0.5).cuda(); b = torch.randn(48, generator=gen).cuda()
    g = torch.randn(2, 48, 9, 11, generator=gen).cuda()
    res = []
    for dt in (torch.float32, torch.bfloat16):
        xx, ww, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = F.layer_norm_cf(xx, ww, bb, 1e-6, out_dtype=dt)
        assert y.dtype == dt
        y.backward(g.to(dt))
        res.append((y.float(), xx.grad, ww.grad, bb.grad))
    assert rel_to_max(res[1][0], res[0][0]) < 1e-2     # bf16 rounding of the output
    for a, e in zip(res[1][1:], res[0][1:]): assert rel_to_max(a, e) < 2e-2   # gradient was rounded to bf16 on the way in


def test_decoder_glue_bf16_io(F):
    """bf16 conv outputs in, bf16 padded tensors out (decoder under bf16 autocast), fp32 skip: same arithmetic, rounded at the boundary."""
    gen = torch.Generator().manual_seed(14)
    B, Ca, Cs, h, w = 2, 6, 3, 5, 7
    a = torch.randn(B, Ca, h, w, generator=gen).cuda(); skip = torch.randn(B, Cs, 2*h, 2*w, generator=gen).cuda(); bias = torch.randn(Ca, generator=gen).cuda()
    res = []
    for bf in (False, True):
        aa = (a.bfloat16() if bf else a.clone()).requires_grad_(True); ss = skip.clone().requires_grad_(True); bb = bias.clone().requires_grad_(True)
        od = torch.bfloat16 if bf else None
        o1 = F.elu_up_cat_pad(aa, ss, bias=bb, out_dtype=od); o2 = F.elu_pad(aa, bb, True, out_dtype=od)
        assert o1.dtype == (torch.bfloat16 if bf else torch.float32) and o2.dtype == o1.dtype
        g = torch.Generator(device='cuda').manual_seed(15)
        (sum((o.float()*torch.randn(o.shape, generator=g, device='cuda')).sum() for o in (o1, o2))).backward()
        assert aa.grad.dtype == aa.dtype and ss.grad.dtype == torch.float32 and bb.grad.dtype == torch.float32
        res.append([t.detach().float() for t in (o1, o2, aa.grad, ss.grad, bb.grad)])
    for nm, x, e in zip(('up_cat_pad', 'elu_pad', 'g_a', 'g_skip', 'g_bias'), res[1], res[0]):
        assert rel_to_max(x, e) < 3e-2, f'{nm}: {rel_to_max(x, e):.3e}'


# ---------------------------------------------------------------------------------------------------
# GPU-side aspect-ratio augmentation
# ---------------------------------------------------------------------------------------------------
def test_crop_resize_kernel_matches_reference_resize_and_oracle(F, golden):
    """`smd_crop_resize` (one launch for every image tensor of the batch + K): (1) the resize half against the REFERENCE's
    `resize_aug` output (pinned fixture), (2) crop + resize at odd / even window offsets against the oracle (crop = kornia's
    `center_crop(align_corners=False)` resample restated from its published call chain, parity unpinned; 3e-5: the oracle builds its
    sampling grid in fp32 like kornia, the kernel evaluates the closed form in fp64), (3) crop only, identity, windows that touch the border."""
    from oracle import aspect_ratio_oracle as A
    g = golden('ar_reference')
    x = {k[5:]: v for k, v in g.items() if k.startswith('in_x_')}; y = {k[5:]: v for k, v in g.items() if k.startswith('in_y_')}
    sh = tuple(x['imgs'].shape[-2:]); res = tuple(int(v) for v in g['meta_res_shape'])
    keys = [('x', 'imgs'), ('y', 'imgs'), ('x', 'supp_imgs'), ('y', 'supp_imgs'), ('y', 'depth')]
    tens = [{'x': x, 'y': y}[d][k].cuda() for d, k in keys]
    outs, K = F.crop_resize(tens, sh, res, y['K'].cuda())
    for (d, k), o in zip(keys, outs): torch.testing.assert_close(o.cpu(), g[f'out_{d}_{k}'], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(K.cpu(), g['out_y_K'], rtol=1e-6, atol=1e-6)
    gen = torch.Generator().manual_seed(3)
    big = [torch.rand(2, 3, 37, 61, generator=gen), torch.rand(3, 2, 3, 37, 61, generator=gen), torch.rand(2, 1, 37, 61, generator=gen)]
    Kc = torch.rand(2, 4, 4, generator=gen)
    for crop, out in (((20, 33), (32, 64)), ((21, 32), (32, 32)), ((37, 61), (64, 96)), ((19, 40), (19, 40)), ((37, 61), (37, 61)), ((2, 3), (32, 32)),
                      ((36, 61), (32, 64)), ((37, 60), (37, 60)), ((36, 60), (18, 30))):
        o_hip, K_hip = F.crop_resize([t.cuda() for t in big], crop, out, Kc.cuda())
        o_ref, K_ref = A.crop_resize(big, crop, out, Kc)
        for a, r in zip(o_hip, o_ref): torch.testing.assert_close(a.cpu(), r, rtol=1e-5, atol=(1e-6 if crop == (37, 61) else 3e-5))
        torch.testing.assert_close(K_hip.cpu(), K_ref, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError): F.crop_resize([big[0].cuda()], (40, 10), (32, 32))          # crop larger than the image


def test_aspect_ratio_aug_on_a_training_batch(F):
    """The whole entry point on the HIP operator against the same call on the oracle's operator (same seeds -> same sampled shapes),
    then one training step of the trainer with `aspect_ratio_aug_prob = 1` on the augmented shapes."""
    import random
    from oracle import aspect_ratio_oracle as A
    from slowtv_monodepth_amd import aspect_ratio as AR
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    xb, yb, mb = make_batch(2, 96, 320, (-1, 1), seed=3)
    clone = lambda d, dev: {k: (v.clone().to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    random.seed(5); torch.manual_seed(5)
    xh, yh, mh = AR.aspect_ratio_aug((clone(xb, 'cuda'), clone(yb, 'cuda'), {}), p=1.0, ref_shape=(96, 320))
    random.seed(5); torch.manual_seed(5)
    xo, yo, mo = AR.aspect_ratio_aug((clone(xb, 'cpu'), clone(yb, 'cpu'), {}), p=1.0, ref_shape=(96, 320), resample=A.crop_resize)
    assert mh['augs'] == mo['augs'] and xh['imgs'].shape == xo['imgs'].shape and xh['imgs'].shape[-1] % 32 == 0
    for k in ('imgs', 'supp_imgs'):
        torch.testing.assert_close(xh[k].cpu(), xo[k], rtol=1e-5, atol=2e-4); torch.testing.assert_close(yh[k].cpu(), yo[k], rtol=1e-5, atol=3e-5)   # (x: standardised, range ~ +-2.6/0.22)
    torch.testing.assert_close(yh['K'].cpu(), yo['K'], rtol=1e-6, atol=1e-6)
    cfg = {'net': {'depth': {'enc_name': 'resnet18', 'pretrained': False, 'dec_name': 'monodepth', 'out_scales': [0, 1, 2, 3]},
                   'pose': {'enc_name': 'resnet18', 'pretrained': False}},
           'loss': {'img_recon': {'weight': 1, 'loss_name': 'ssim', 'use_min': True, 'use_automask': True}, 'disp_smooth': {'weight': 0.001, 'use_edges': True}},
           'trainer': {'min_depth': 0.1, 'max_depth': 100, 'aspect_ratio_aug_prob': 1.0, 'aspect_ratio_ref_shape': [128, 192]}}
    torch.manual_seed(0)
    m = MonoDepthModule(cfg).cuda()
    random.seed(5); torch.manual_seed(5)                  # samples a 16/9 crop (81, 145) of a (128, 192) frame -> resized to (96, 192)
    xs, ys, _ = make_batch(2, 128, 192, (-1, 1), seed=3)
    batch = (clone(xs, 'cuda'), clone(ys, 'cuda'), {})
    loss, ld, fwd = m.step(batch, mode='train')
    loss.backward()
    assert torch.isfinite(loss).item() and len(batch[2]['augs']) == 2 and tuple(batch[0]['imgs'].shape[-2:]) == (96, 192)


# ---------------------------------------------------------------------------------------------------
# Round 5: the whole loss path as ONE autograd node (smd_loss_path_fwd / _bwd)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,h,w,n,lows,learn_k,use_min,automask,prep', [
    (3, 50, 130, 2, [(50, 130), (25, 65), (12, 32), (6, 16)], False, True, True, False),
    (12, 192, 640, 2, [(192, 640), (96, 320), (48, 160), (24, 80)], False, True, True, True),      # cfg 2, frames prepared ahead
    (2, 96, 200, 4, [(96, 200), (48, 100), (24, 50), (12, 25)], True, True, True, True),            # four supports, learned intrinsics
    (2, 33, 47, 3, [(33, 47), (16, 23), (8, 11)], True, False, False, False),                       # mean over the supports, three levels
    (1, 64, 300, 1, [(32, 150), (16, 75), (4, 19)], False, True, False, False),                     # no level of the image's size, one support
    (2, 384, 640, 2, [(384, 640), (192, 320), (96, 160), (48, 80)], False, True, True, True)])      # cfg 4 / 5 size
@pytest.mark.parametrize('guests', [1, 0])
def test_single_node_loss_path_equals_the_two_handlers(F, knobs, b, h, w, n, lows, learn_k, use_min, automask, prep, guests):
    """`functional.loss_path_fused` (one autograd node: the reconstruction launch carrying the smoothness sweep as guest blocks and forming the
    weighted sum in-launch; the backward's pose epilogue continued to the pose network's outputs, the smoothness adjoint as guest blocks of
    the K0 adjoint, which adds) against the separate operators it replaces — `pose_matrices` / `intrinsics`, `image_recon_fused_disp`,
    `disp_smooth_fused`, `w_rec*l_rec + w_sm*l_sm` in eager mode and autograd's gradient additions.  Same kernels on the same operands:
    l_rec, l_sm, the total, `sel`, `depth_up` and the disparity gradients must be BIT-equal; the pose / intrinsics leaves, whose adjoint is
    compiled into another kernel (fp contraction may differ), to 1e-6 of the tensor's max.  `guests` = 0 (knob `loss_path_guests`) runs
    the guest work as launches of its own: same bits again."""
    from slowtv_monodepth_amd._lib import FLAGS
    knobs('loss_path_guests', guests)
    gen = torch.Generator(device='cuda').manual_seed(h*w + n)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen)
    supp = (imgs[None] + 0.15*torch.randn(n, b, 3, h, w, device='cuda', generator=gen)).clamp(0, 1)
    d0 = [0.05 + 0.9*torch.rand(b, 1, hs, ws, device='cuda', generator=gen) for hs, ws in lows]
    keys = list(range(len(lows)))
    aa0 = 0.01*torch.randn(n*b, 3, device='cuda', generator=gen); t0 = 0.05*torch.randn(n*b, 3, device='cuda', generator=gen)
    inv = torch.tensor([i % 2 == 0 for i in range(n) for _ in range(b)], dtype=torch.uint8, device='cuda')
    fs0 = torch.tensor([0.58, 1.92], device='cuda')[None].repeat(b, 1)*(1 + 0.05*torch.randn(b, 2, device='cuda', generator=gen))
    cs0 = 0.5 + 0.03*torch.randn(b, 2, device='cuda', generator=gen)
    K0 = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    flags = F.recon_flags('ssim', use_min, automask)
    w_rec, w_sm = torch.tensor(1.0, device='cuda'), torch.tensor(0.001, device='cuda')
    g_out = torch.tensor(0.5, device='cuda')            # an accumulation micro-step's 1/k

    def leaves():
        L = dict(d=[v.clone().requires_grad_(True) for v in d0], aa=aa0.clone().requires_grad_(True), t=t0.clone().requires_grad_(True))
        if learn_k: L.update(fs=fs0.clone().requires_grad_(True), cs=cs0.clone().requires_grad_(True))
        return L

    def prepared():
        return F.image_recon_prep(imgs, supp, flags=flags, pyramid=lows, smooth_edges=True) if prep else None

    def two_nodes():
        L = leaves()
        Ts = F.pose_matrices(L['aa'], L['t'], inv).unflatten(0, (n, b))
        K, K_inv = F.intrinsics(L['fs'], L['cs'], (h, w)) if learn_k else (K0, None)
        pr = prepared()
        l_rec, _, sel, _, dep = F.image_recon_fused_disp(L['d'], imgs, supp, Ts, K, K_inv, flags=flags, min_depth=0.1, max_depth=100, seed=11, want_err=False, prepared=pr)
        l_sm, _, _ = F.disp_smooth_fused(dict(zip(keys, L['d'])), imgs, use_edges=True, want_aux=False, prepared=pr)
        loss = 0. + w_rec*l_rec
        loss = loss + w_sm*l_sm
        loss.backward(g_out)
        return loss.detach(), l_rec.detach(), l_sm.detach(), sel, dep.detach(), L

    def one_node():
        L = leaves()
        Ts = F.pose_matrices(L['aa'], L['t'], inv).unflatten(0, (n, b))
        K, K_inv = F.intrinsics(L['fs'], L['cs'], (h, w)) if learn_k else (K0, None)
        loss, l_rec, l_sm, sel, dep = F.loss_path_fused(dict(zip(keys, L['d'])), imgs, supp, Ts, K, K_inv, pose=(L['aa'], L['t'], inv),
                                                        intrinsics=(L['fs'], L['cs']) if learn_k else None, flags=flags, min_depth=0.1, max_depth=100, seed=11,
                                                        w_recon=1.0, w_smooth=float(w_sm), prepared=prepared())
        loss.backward(g_out)
        return loss.detach(), l_rec, l_sm, sel, dep.detach(), L

    monkey_skip = pytest.MonkeyPatch()
    monkey_skip.setenv('SMD_BWD_SKIP', '0')      # one row loop for both (the tuner would otherwise time its two loops on different calls)
    try:
        la, ra, sa, sel_a, dep_a, A = two_nodes()
        lb, rb, sb, sel_b, dep_b, B = one_node()
        torch.cuda.synchronize()
    finally: monkey_skip.undo()
    assert torch.equal(sel_a, sel_b) and torch.equal(dep_a, dep_b)
    assert torch.equal(ra, rb) and torch.equal(sa, sb), (ra.item(), rb.item(), sa.item(), sb.item())
    assert torch.equal(la, lb), (la.item(), lb.item())
    for k, (x, y) in enumerate(zip(A['d'], B['d'])): assert torch.equal(x.grad, y.grad), f'd loss / d disp[{k}]: max diff {(x.grad - y.grad).abs().max().item():.3e}'
    for k in ('aa', 't') + (('fs', 'cs') if learn_k else ()):
        assert rel_to_max(B[k].grad, A[k].grad) <= 1e-6, (k, rel_to_max(B[k].grad, A[k].grad))
    assert torch.isfinite(lb) and all(torch.isfinite(x.grad).all() for x in B['d'])


def test_single_node_loss_path_declines_what_it_does_not_serve(F):
    """SMD_E_UNSUPPORTED -> `_lib.Unsupported`, nothing launched: pure-L1 error, a single pyramid level."""
    from slowtv_monodepth_amd._lib import Unsupported
    b, h, w, n = 1, 16, 70, 2
    imgs = torch.rand(b, 3, h, w, device='cuda'); supp = torch.rand(n, b, 3, h, w, device='cuda')
    T = torch.eye(4, device='cuda').repeat(n, b, 1, 1); K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None]
    d = {0: torch.rand(b, 1, h, w, device='cuda') + 0.1, 1: torch.rand(b, 1, h//2, w//2, device='cuda') + 0.1}
    with pytest.raises(Unsupported): F.loss_path_fused(d, imgs, supp, T, K, flags=F.recon_flags('l1', True, True), min_depth=0.1, max_depth=100)
    with pytest.raises(Unsupported): F.loss_path_fused({0: d[0]}, imgs, supp, T, K, flags=F.recon_flags('ssim', True, True), min_depth=0.1, max_depth=100)
    loss, *_ = F.loss_path_fused(d, imgs, supp, T, K, flags=F.recon_flags('ssim', True, True), min_depth=0.1, max_depth=100)
    assert torch.isfinite(loss)


@pytest.mark.parametrize('b,h,w,n,lows,use_min,rows', [(3, 96, 320, 4, [(96, 320), (48, 160), (24, 80), (12, 40)], True, 'bands'), (2, 50, 130, 2, [(50, 130), (25, 65)], True, 'bands'),
                                                       (2, 64, 200, 3, [(64, 200), (32, 100), (16, 50)], False, 'bands'), (2, 40, 70, 4, [(40, 70), (20, 35)], True, 'dead')])
@pytest.mark.parametrize('skip', ['0', '2'])
def test_backward_liveness_table_skips_only_exact_zeros(F, knobs, monkeypatch, b, h, w, n, lows, use_min, rows, skip):
    """Round 5: the forward leaves, per forward strip and support, the columns in which some row's final selection is that support; a backward
    wave (one support of one strip) whose 3x3-dilated footprint overlaps none of them parks zeros instead of running its row loop.  Every gradient
    must be BIT-equal to the run that ignores the table (knob `bwd_live` = 0) — on frames built so that whole supports are dead in whole
    bands of the image (their frames are unrelated noise there), that one support is dead everywhere, and with the automask taking regions."""
    monkeypatch.setenv('SMD_BWD_SKIP', skip)
    gen = torch.Generator(device='cuda').manual_seed(h + w + n)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen)
    supp = torch.rand(n, b, 3, h, w, device='cuda', generator=gen)                    # unrelated: never the best candidate where another one is close
    if rows == 'bands':
        for i in range(n):      # support i resembles the target in the i-th horizontal band only (and in a vertical stripe for the last one)
            r0, r1 = i*h//n, (i + 1)*h//n
            supp[i, :, :, r0:r1] = (imgs[:, :, r0:r1] + 0.02*torch.randn(b, 3, r1 - r0, w, device='cuda', generator=gen)).clamp(0, 1)
        supp[n - 1, :, :, :, w//3: w//3 + 9] = imgs[:, :, :, w//3: w//3 + 9]
    else:
        supp[0] = (imgs + 0.02*torch.randn(b, 3, h, w, device='cuda', generator=gen)).clamp(0, 1)    # support 0 wins everywhere (or the automask does): 1 .. n-1 are dead
    imgs[:, :, : h//5, : w//4] = 1.0; supp[:, :, :, : h//5 + 2, : w//4 + 2] = 1.0      # a saturated corner: exact ties, auto-masked
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    T0 = torch.eye(4, device='cuda').repeat(n, b, 1, 1); T0[..., :3, 3] = 0.002*torch.randn(n, b, 3, device='cuda', generator=gen)
    d0 = [0.05 + 0.9*torch.rand(b, 1, hs, ws, device='cuda', generator=gen) for hs, ws in lows]
    automask = rows == 'dead'      # (bands: min-reprojection alone routes each band to its support; with the automask on, the un-warped frames win nearly everywhere)
    flags = F.recon_flags('ssim', use_min, automask)

    def run(live):
        knobs('bwd_live', live)
        d = [v.clone().requires_grad_(True) for v in d0]; T = T0.clone().requires_grad_(True)
        loss, _, sel, _, _ = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, seed=5, want_err=False)
        loss.backward(); torch.cuda.synchronize()
        return sel, [v.grad for v in d] + [T.grad]
    sel, g1 = run(1)
    _, g0 = run(0)
    for k, (x, y) in enumerate(zip(g1, g0)): assert torch.equal(x, y), f'gradient #{k} differs with the liveness table (max {(x - y).abs().max().item():.3e})'
    shares = [(sel == i).float().mean().item() for i in range(n)] + [(sel == 255).float().mean().item()]
    assert all(torch.isfinite(x).all() for x in g1), shares
    if use_min and rows == 'bands': assert all(0.1 < v < 0.9 for v in shares[:n]), shares        # every support is live in its band and dead elsewhere
    if rows == 'dead': assert shares[-1] > 0.01 and max(shares[1:n]) < 0.02, shares               # supports 1 .. n-1 are (nearly) dead everywhere; the automask takes a region


@pytest.mark.parametrize('b,h,w,n,lows', [(3, 96, 320, 4, [(96, 320), (48, 160), (24, 80), (12, 40)]), (2, 50, 130, 2, [(50, 130), (25, 65)]),
                                          (2, 64, 200, 3, [(64, 200), (32, 100), (16, 50)]), (12, 192, 640, 2, [(192, 640), (96, 320), (48, 160), (24, 80)]),
                                          (12, 384, 640, 4, [(384, 640), (192, 320), (96, 160), (48, 80)])])       # cfg 5's size: what the heuristic itself picks there is checked too
@pytest.mark.parametrize('skip', ['0', '2'])
def test_one_wave_per_strip_equals_one_wave_per_support(F, knobs, monkeypatch, b, h, w, n, lows, skip):
    """Round 5: in launches of three or more generations the backward runs ONE wave per strip that takes the supports in turn (and passes over the
    ones the liveness table calls dead) instead of one wave per (strip, support).  Same operations on the same operands, the supports' shares of
    dL/d depth added in the same order: every disparity gradient BIT-equal between knob `bwd_wps` = 1 and = min(n, 4), with dead supports in bands of
    the image (the pose gradient to 1e-6: its fp32 per-block partial sums group other strips)."""
    monkeypatch.setenv('SMD_BWD_SKIP', skip)
    gen = torch.Generator(device='cuda').manual_seed(h + w + n)
    imgs = torch.rand(b, 3, h, w, device='cuda', generator=gen)
    supp = torch.rand(n, b, 3, h, w, device='cuda', generator=gen)
    for i in range(n):
        r0, r1 = i*h//n, (i + 1)*h//n
        supp[i, :, :, r0:r1] = (imgs[:, :, r0:r1] + 0.02*torch.randn(b, 3, r1 - r0, w, device='cuda', generator=gen)).clamp(0, 1)
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device='cuda')[None].repeat(b, 1, 1)
    T0 = torch.eye(4, device='cuda').repeat(n, b, 1, 1); T0[..., :3, 3] = 0.002*torch.randn(n, b, 3, device='cuda', generator=gen)
    d0 = [0.05 + 0.9*torch.rand(b, 1, hs, ws, device='cuda', generator=gen) for hs, ws in lows]
    flags = F.recon_flags('ssim', True, False)

    def run(wps):
        knobs('bwd_wps', wps)
        d = [v.clone().requires_grad_(True) for v in d0]; T = T0.clone().requires_grad_(True)
        loss, _, sel, _, _ = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, seed=5, want_err=False)
        loss.backward(); torch.cuda.synchronize()
        from slowtv_monodepth_amd import _lib
        return [v.grad for v in d] + [T.grad], _lib.lib.smd_last_kernel_variant(1).decode()
    def run_default():
        d = [v.clone().requires_grad_(True) for v in d0]; T = T0.clone().requires_grad_(True)
        loss, *_ = F.image_recon_fused_disp(d, imgs, supp, T, K, flags=flags, min_depth=0.1, max_depth=100, seed=5, want_err=False)
        loss.backward(); torch.cuda.synchronize()
        from slowtv_monodepth_amd import _lib
        return [v.grad for v in d] + [T.grad], _lib.lib.smd_last_kernel_variant(1).decode()
    g1, k1 = run(1); gn, kn = run(min(n, 4))
    assert f', 1, true' in k1 and f', {min(n, 4)}, true' in kn, (k1, kn)
    # with four scales a one-wave-per-strip block is the four SCALES of a strip (where every block then has its strip) — against four strips of a scale
    knobs('bwd_scales_block', 0); gs, _ = run(1); knobs('bwd_scales_block', 1)
    for k, (x, y) in enumerate(zip(g1[:-1], gs[:-1])): assert torch.equal(x, y), f'd loss / d disp[{k}]: blocks of four scales differ from blocks of four strips (max {(x - y).abs().max().item():.3e})'
    assert rel_to_max(g1[-1], gs[-1]) <= 1e-6
    for k, (x, y) in enumerate(zip(g1[:-1], gn[:-1])): assert torch.equal(x, y), f'd loss / d disp[{k}]: one wave per strip differs from one wave per support (max {(x - y).abs().max().item():.3e})'
    # dL/dT: a block's pose sums are added in fp32 over its waves before the fp64 sum over the blocks, and a block is now four strips instead of one
    assert rel_to_max(g1[-1], gn[-1]) <= 1e-6
    if b*h*w >= 12*384*640:      # three or more generations of strip waves: the library's own choice is one wave per strip (smd_api.hip)
        from slowtv_monodepth_amd import _lib
        _lib.reset_knobs()
        gd, kd = run_default()
        assert ', 1, true' in kd, kd
        assert all(torch.equal(x, y) for x, y in zip(gd, g1))
