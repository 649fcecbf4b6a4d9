"""The fused masked image reconstruction (csrc/smd_maskrecon.hip, maskrecon.py, `handlers.image_recon_masked_fused`) on the GPU: its decisions (`sel`, the static
winner, `automask`) and `warp0` against the plain handler's operators bit for bit; loss and gradients against the fp64 oracle under the project's 4x rule (the
plain handler's own error on the same inputs is the yardstick); the reference's `train_mask_*` fixtures; gradient subsets, hostile memory and value edges
(harnesses: grad_subsets.py, hostile_memory.py); run-to-run bit equality; one step of cfg/kitti_sfm_learner.yaml with the fused and with the plain route.

The static winner of the plain route is not an output of any operator: it is restated here from `F.photo_error`'s identity errors and the mask.  For the
explainability mask that is one fp32 product, the kernel's; for the uncertainty mask torch's exp is not the kernel's, so a pixel whose two best masked
identity errors lie within STAT_MARGIN relative of each other is left out of that one comparison (counted and printed)."""
import copy
import itertools

import pytest
import torch

from conftest import ROOT, case_inputs, load_golden, parity_note, rel_to_max
from grad_subsets import check_subsets, subsets_of
from hostile_memory import Arena, assert_finite, hostile
from oracle import view_synth_oracle as O

pytestmark = pytest.mark.gpu
STAT_MARGIN = 1e-5
SIZES = [(24, 40), (17, 23), (2, 2), (9, 65)]      # tile remainders both ways, the smallest legal frame, one column more than a multiple of 64
KINDS = ('explainability', 'uncertainty')


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available(): pytest.skip('no GPU')
    from slowtv_monodepth_amd import maskrecon
    return maskrecon


def note(line): parity_note(f'maskrecon_parity {line}')


def make_inputs(h, w, n, S, b, kind, seed=0, hard=True):
    """Seeded operands on the CPU.  `hard`: support 0 steps sideways by 1.2 units (a part of the frame leaves the image) and the last support's camera stands 1.5
    units ahead, so that points nearer than that lie behind it (transformed depth below 0, at the 0.1 clamp, beyond it)."""
    from slowtv_monodepth_amd.synthetic import kitti_K
    g = torch.Generator().manual_seed(1000*seed + 97*h + 13*w + 5*n + 3*S + b)
    depth = 0.5 + 5*torch.rand(S, b, h, w, generator=g)
    imgs = torch.rand(b, 3, h, w, generator=g)
    supp = 0.6*imgs[None] + 0.4*torch.rand(n, b, 3, h, w, generator=g)
    mask = torch.rand(S, b, n, h, w, generator=g) if kind == 'explainability' else 0.3*torch.randn(S, b, n, h, w, generator=g)
    Ts = torch.eye(4).repeat(n, b, 1, 1); Ts[..., :3, 3] = 0.05*torch.randn(n, b, 3, generator=g)
    if hard: Ts[0, :, 0, 3] += 1.2; Ts[-1, :, 2, 3] -= 1.5
    noise = torch.randn(S, b, h, w, generator=g)
    return dict(depth=depth, mask=mask, imgs=imgs, supp=supp, Ts=Ts, K=kitti_K(b, h, w), noise=noise)


def fused(R, c, flags, kind, *, noise=True, seed=0, want_warp=True, need=('depth', 'mask', 'Ts'), gy=None):
    """One forward (+ backward when anything asks) of the operator on GPU operands `c` -> dict of GPU tensors."""
    loss_name, use_min, use_automask = flags
    lv = {k: c[k].clone().requires_grad_(k in need) for k in ('depth', 'mask', 'Ts')}
    loss, sel, stat, warp = R.mask_recon_loss(lv['depth'], lv['mask'], c['imgs'], c['supp'], lv['Ts'], c['K'], c.get('K_inv'), loss_name=loss_name, use_min=use_min,
                                              use_automask=use_automask, mask_name=kind, noise=c['noise'] if noise else None, seed=seed, want_warp=want_warp)
    if need: loss.backward(gy) if gy is not None else loss.backward()
    return {'loss': loss.detach(), 'sel': sel, 'stat': stat, 'warp': warp, **{f'g_{k}': v.grad for k, v in lv.items()}}


def plain_pieces(c, flags, kind, *, noise=True, seed=0):
    """The plain handler's own operators on the same operands (`handlers._image_recon_generic`'s calls, with `sel` kept): F.view_synth, F.photo_error,
    F.recon_reduce -> sel (S,b,h,w), the static winner restated (and the pixels where that restatement is within STAT_MARGIN of a tie), warp0."""
    from slowtv_monodepth_amd import functional as F, handlers
    loss_name, use_min, use_automask = flags
    S, b, h, w = c['depth'].shape
    depths = {s: c['depth'][s].unsqueeze(1) for s in range(S)}
    K_inv = F.inv_intrinsics(c['K'])
    n, S, b, dep, tgt, src, T, K, Ki = handlers._expand_views(depths, c['imgs'], c['supp'], c['Ts'], c['K'], K_inv)
    warp = F.view_synth(src.flatten(0, 1), dep[None].expand(n, *dep.shape).flatten(0, 1), T, K, Ki)[0].unflatten(0, (n, S*b))
    tg = tgt[None].expand_as(warp).flatten(0, 1)
    ew = F.photo_error(warp.flatten(0, 1), tg, loss_name=loss_name).view(n, S*b, h, w)
    es = F.photo_error(src.flatten(0, 1), tg, loss_name=loss_name).view(n, S*b, h, w) if use_automask else None
    m = c['mask'].flatten(0, 1)
    loss, _, sel = F.recon_reduce(ew, es, use_min=use_min, noise=c['noise'].reshape(S*b, 1, h, w) if noise else None, seed=seed, mask=m, mask_name=kind)
    out = {'loss': loss, 'sel': sel.reshape(S, b, h, w), 'warp': warp.unflatten(1, (S, b))[:, 0], 'stat': None, 'stat_near': None}
    if use_min and use_automask:
        e = es.permute(1, 0, 2, 3)
        me = e*m if kind == 'explainability' else e*(-m).exp() + m
        out['stat'] = me.argmin(1).reshape(S, b, h, w).to(torch.uint8)
        if n > 1 and kind == 'uncertainty':
            two = (e.double()*(-m.double()).exp() + m.double()).topk(2, dim=1, largest=False)[0]
            out['stat_near'] = ((two[:, 1] - two[:, 0]) <= STAT_MARGIN*two.abs().amax(1)).reshape(S, b, h, w)
    return out


def plain_handler(c, flags, kind, *, noise=True, seed=0, need=('depth', 'mask', 'Ts')):
    """`handlers.image_recon` (the un-fused route) with gradients -> dict."""
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    S, b, h, w = c['depth'].shape
    lv = {k: c[k].clone().requires_grad_(k in need) for k in ('depth', 'mask', 'Ts')}
    crit = ReconstructionLoss(flags[0], use_min=flags[1], use_automask=flags[2], mask_name=kind); crit.noise_seed = seed - 1
    loss, ld = handlers.image_recon(crit, None, {s: lv['depth'][s].unsqueeze(1) for s in range(S)}, {s: lv['mask'][s] for s in range(S)}, c['imgs'], c['supp'], lv['Ts'], c['K'],
                                    noise=c['noise'].reshape(S*b, 1, h, w) if noise else None)
    if need: loss.backward()
    return {'loss': loss.detach(), 'ld': ld, **{f'g_{k}': v.grad for k, v in lv.items()}}


def same_decisions(tag, f, p, n):
    assert torch.equal(f['sel'], p['sel']), f'{tag}: sel differs from the plain route on {int((f["sel"] != p["sel"]).sum())} pixels'
    assert int(((f['sel'] != 255) & (f['sel'] >= n)).sum()) == 0
    assert torch.equal(f['warp'], p['warp']), f'{tag}: warp0 is not F.view_synth\'s bit for bit'
    if p['stat'] is not None:
        diff = f['stat'] != p['stat']
        if p['stat_near'] is not None: diff &= ~p['stat_near']
        assert not diff.any(), f'{tag}: the static winner differs on {int(diff.sum())} pixels'
    else: assert f['stat'] is None
    return 0 if p['stat_near'] is None else int(p['stat_near'].sum())


# ------------------------------------------------------------------------------------------------- decisions and bits against the plain handler
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_decisions_and_warp_are_the_plain_routes(R, size):
    """Every combination of mask kind, use_min, use_automask and loss_name crossed with n in {1, 2, 3}, the (S, b) pairs in rotation; poses that send part of the
    frame outside the image and depths that put points behind the camera.  Explicit noise everywhere, and once per combination the in-kernel noise at equal seeds."""
    h, w = size
    left_out = cases = 0
    sb = itertools.cycle([(1, 1), (2, 2), (1, 2), (2, 1)])
    for kind, use_min, use_automask, loss_name in itertools.product(KINDS, (True, False), (True, False), ('ssim', 'l1')):
        for n in (1, 2, 3):
            S, b = next(sb)
            c = {k: v.cuda() for k, v in make_inputs(h, w, n, S, b, kind, seed=cases).items()}
            flags = (loss_name, use_min, use_automask)
            tag = f'{h}x{w} n={n} S={S} b={b} {kind} {flags}'
            f, p = fused(R, c, flags, kind, need=()), plain_pieces(c, flags, kind)
            left_out += same_decisions(tag, f, p, n); cases += 1
            if use_automask: assert torch.equal(f['sel'] != 255, p['sel'] != 255), f'{tag}: automask'
            torch.testing.assert_close(f['loss'], p['loss'], rtol=2e-6, atol=1e-7, msg=lambda s: f'{tag}: loss {s}')
            if n == 2 and use_automask:
                f, p = fused(R, c, flags, kind, need=(), noise=False, seed=77), plain_pieces(c, flags, kind, noise=False, seed=77)
                left_out += same_decisions(tag + ' seeded noise', f, p, n)
    note(f'{h}x{w}: {cases} cases, sel / warp0 / automask bit-equal to the plain route; static winner: {left_out} pixels within {STAT_MARGIN} of a tie left out')


def test_frame_leaves_the_image_and_points_lie_behind_the_camera():
    """What the `hard` poses of the cases above do, restated in fp64: a part of support 0's samples fall outside the frame, a part of the last support's points
    have a transformed depth below 0 and a part between 0 and the 0.1 clamp."""
    c = make_inputs(24, 40, 2, 1, 1, 'uncertainty')
    d, K, T = c['depth'][0].double(), c['K'].double()[:, :3, :3], c['Ts'].double()
    ys, xs = torch.meshgrid(torch.arange(24.), torch.arange(40.), indexing='ij')
    pix = torch.stack((xs, ys, torch.ones_like(xs))).reshape(3, -1).double()
    pts = torch.linalg.inv(K) @ pix*d.reshape(1, 1, -1)
    cam = T[:, :, :3, :3] @ pts[None] + T[:, :, :3, 3:]
    proj = K[None] @ (cam/cam[:, :, 2:3].clamp(min=0.1))
    outside = (proj[0, :, 0] < 0) | (proj[0, :, 0] > 39)
    assert 0.05 < outside.double().mean() < 0.9
    z = cam[1, :, 2]
    assert (z < 0).any() and ((z > 0) & (z < 0.1)).any() or (z < 0).double().mean() > 0.05


# ------------------------------------------------------------------------------------------------- values against fp64
def oracle64(ins, flags, kind):
    """The oracle's restatement of the handler (`O.view_synth` + `O.recon_loss` with `mask` / `mask_name`, as
    test_gpu_parity.py::test_image_recon_handler_with_predictive_masks_matches_oracle builds it) in float64 on the CPU."""
    c = {k: v.double() for k, v in ins.items()}
    S, b, h, w = c['depth'].shape
    n = c['supp'].shape[0]
    lv = {k: c[k].clone().requires_grad_(True) for k in ('depth', 'mask', 'Ts')}
    dep = lv['depth'].reshape(S*b, 1, h, w)
    src = c['supp'][:, None].expand(n, S, *c['supp'].shape[1:]).flatten(1, 2)
    tgt = c['imgs'][None].expand(S, *c['imgs'].shape).flatten(0, 1)
    warp = O.view_synth(src.flatten(0, 1), dep[None].expand(n, *dep.shape).flatten(0, 1), lv['Ts'][:, None].expand(n, S, b, 4, 4).flatten(0, 2),
                        c['K'][None, None].expand(n, S, b, 4, 4).flatten(0, 2))[0].unflatten(0, (n, S*b))
    m = lv['mask'].flatten(0, 1)
    loss, out = O.recon_loss(warp, tgt, source=src, loss_name=flags[0], use_min=flags[1], use_automask=flags[2], noise=c['noise'].reshape(S*b, 1, h, w), mask=m, mask_name=kind)
    loss.backward()
    stat = None
    if flags[1] and flags[2]:
        with torch.no_grad(): stat = O.apply_mask(O.compute_photo(src, tgt, flags[0], True)[1], m, kind).argmin(1).reshape(S, b, h, w)
    return {'loss': loss.detach(), 'sel': out['sel'].reshape(S, b, h, w), 'stat': stat, **{f'g_{k}': v.grad for k, v in lv.items()}}


@pytest.mark.parametrize('kind', KINDS)
def test_values_against_fp64_within_four_times_the_plain_handlers_error(R, kind):
    """Loss, g_depth, g_mask and g_T at (24, 40), n = 2, S = 2, b = 2, ssim + min + automask.  The bound is the plain handler's own error against the same fp64
    result on the same inputs, times four (a different but equally valid summation order: the margin `feat_recon_fused` was given).  The per-pixel gradients are
    compared where the fp32 and the fp64 decisions agree (g_depth: where no flip lies in the pixel's 5x5 neighbourhood, the reach of the SSIM adjoint); the
    flips are counted.  g_T sums over all pixels: it carries the flips on both routes alike."""
    flags = ('ssim', True, True)
    ins = make_inputs(24, 40, 2, 2, 2, kind, seed=41, hard=False)
    c = {k: v.cuda() for k, v in ins.items()}
    o, f, p = oracle64(ins, flags, kind), fused(R, c, flags, kind), plain_handler(c, flags, kind)
    agree = f['sel'].cpu() == o['sel']
    agree &= (f['sel'].cpu() != 255) | (f['stat'].cpu() == o['stat'])
    flips = int((~agree).sum())
    assert flips <= 4, f'{flips} decisions differ from the fp64 oracle'
    far = torch.nn.functional.max_pool2d((~agree).float(), 5, 1, 2) == 0
    keep = {'g_depth': far, 'g_mask': agree[:, :, None].expand_as(o['g_mask']), 'g_Ts': torch.ones_like(o['g_Ts'], dtype=torch.bool)}
    lines, fails = [f'{kind}: decision flips against fp64: {flips} of {agree.numel()}'], []
    e_f, e_p = abs(f['loss'].item() - o['loss'].item())/abs(o['loss'].item()), abs(p['loss'].item() - o['loss'].item())/abs(o['loss'].item())
    lines.append(f'{kind}: loss        fused {e_f:.3e}  plain {e_p:.3e}  (relative)')
    if e_f > 4*e_p: fails.append(f'loss {e_f:.3e} > 4 x {e_p:.3e}')
    for k in ('g_depth', 'g_mask', 'g_Ts'):
        scale = o[k].abs().max()
        e_f = (((f[k].cpu().double() - o[k]).abs()*keep[k]).max()/scale).item(); e_p = (((p[k].cpu().double() - o[k]).abs()*keep[k]).max()/scale).item()
        lines.append(f'{kind}: {k:<11} fused {e_f:.3e}  plain {e_p:.3e}  (relative to the maximum)')
        if e_f > 4*e_p: fails.append(f'{k} {e_f:.3e} > 4 x {e_p:.3e}')
    for line in lines: note(line)      # (profiles/maskrecon_parity.txt records these lines)
    assert not fails, '; '.join(fails)


# ------------------------------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize('name', ['train_mask_expl_48x64', 'train_mask_uncert_48x64'])
def test_reference_fixture(R, name):
    """`image_recon_masked_fused` on the fixture's operands: `loss_img_recon` to rtol 2e-5 of the reference's; the disparity, mask, rotation and translation
    gradients of that loss alone against the plain handler's at 1e-3 of the maximum (tests/test_gpu_masks.py's bounds)."""
    from slowtv_monodepth_amd import functional as F, handlers
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    g = load_golden(name)
    kind = str(g['meta_mask_name'])

    def run(fn):
        leaves, static = case_inputs(g, device='cuda')
        scales, idxs = static['scales'], static['supp_idxs']
        n, b = leaves['aa'].shape[:2]
        h, w = static['imgs'].shape[-2:]
        for s in scales: leaves[f'mask_{s}'] = g[f'in_mask_{s}'].cuda().clone().requires_grad_(True)
        inv = torch.tensor([bool(g['meta_always_fwd_pose']) and i < 0 for i in idxs for _ in range(b)], dtype=torch.uint8).cuda()
        Ts = F.pose_matrices(leaves['aa'].flatten(0, 1), leaves['t'].flatten(0, 1), inv).unflatten(0, (n, b))
        depth_up, _ = F.disp_to_depth([leaves[f'disp_{s}'] for s in scales], (h, w), 0.1, 100)
        mask_up = F.upsample_stack([leaves[f'mask_{s}'] for s in scales], (h, w))
        crit = ReconstructionLoss('ssim', use_min=bool(g['meta_use_min']), use_automask=bool(g['meta_use_automask']), mask_name=kind)
        loss, ld = fn(crit, None, handlers.ScaleDict.from_stack(scales, depth_up), handlers.ScaleDict.from_stack(scales, mask_up), static['imgs'], static['supp_imgs'], Ts,
                      static['K'], noise=static['noise'])
        loss.backward()
        return loss.detach().cpu(), ld, {k: v.grad.cpu() for k, v in leaves.items()}
    lf, ldf, gf = run(handlers.image_recon_masked_fused)
    lp, ldp, gp = run(handlers.image_recon)
    torch.testing.assert_close(lf, g['out_loss_img_recon'], rtol=2e-5, atol=1e-7)
    assert ldf.keys() == ldp.keys() and torch.equal(ldf['supp_imgs_warp'], ldp['supp_imgs_warp'])
    if 'automask' in ldp: assert torch.equal(ldf['automask'], ldp['automask'])
    errs = {k: rel_to_max(gf[k], gp[k]) for k in gp}
    note(f'{name}: loss fused {lf.item():.8f} plain {lp.item():.8f} reference {g["out_loss_img_recon"].item():.8f}; gradients vs. plain: ' + ', '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    for k, v in errs.items(): assert v < 1e-3, (k, v)


# ------------------------------------------------------------------------------------------------- gradient subsets, hostile memory, determinism
@pytest.mark.parametrize('flags,kind', [(('ssim', True, True), 'uncertainty'), (('l1', False, True), 'explainability'), (('ssim', False, False), 'explainability')],
                         ids=['ssim_min_auto_uncert', 'l1_mean_auto_expl', 'ssim_mean_expl'])
def test_gradient_subsets(R, flags, kind):
    """Only `depth`, only `mask`, only `Ts`, every pair, or none requires a gradient: each subset gives the bits of the full backward for what it asks for and None
    for the rest (a NULL g_depth, g_mask or g_T selects a launch that never forms its terms); strided and expanded incoming gradients scale it exactly."""
    c = {k: v.cuda() for k, v in make_inputs(17, 23, 3, 2, 2, kind, seed=5).items()}
    diff = ('depth', 'mask', 'Ts')

    def run(subset, gy=None):
        out = fused(R, c, flags, kind, need=tuple(k for k in diff if k in subset), want_warp=False, gy=gy)
        return {k: out[k] for k in ('loss', 'sel', 'stat', 'g_depth', 'g_mask', 'g_Ts')}
    full = run(frozenset(diff))
    check_subsets(run, full, subsets_of(diff), diff, name=f'mask_recon_loss {flags} {kind}')
    frozen = run(frozenset())
    assert torch.equal(frozen['loss'], full['loss']) and torch.equal(frozen['sel'], full['sel']) and all(frozen[f'g_{k}'] is None for k in diff)
    buf = torch.tensor([[7.0, 0.5], [7.0, 7.0]], device='cuda')
    for gy in (buf[0, 1], buf.t()[1, 0], torch.tensor(0.5, device='cuda').expand(3)[1]):
        half = run(frozenset(diff), gy)
        for k in diff: assert torch.equal(half[f'g_{k}'], 0.5*full[f'g_{k}']), k


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('size', [(17, 23), (9, 65)], ids=['17x23', '9x65'])
def test_hostile_memory(R, size, shift):
    """Every operand in a guarded, poisoned block `shift` elements off its alignment, every buffer the operator allocates (block sums, pose sums, loss, sel, stat,
    warp, gradients) served from the arena: the bits of the plain-memory run, guards intact, every element of g_mask, g_depth and sel written."""
    from slowtv_monodepth_amd import functional as F
    flags, kind, n = ('ssim', True, True), 'uncertainty', 2
    c = {k: v.cuda() for k, v in make_inputs(*size, n, 2, 2, kind, seed=9).items()}
    c['K_inv'] = F.inv_intrinsics(c['K'])
    ref = fused(R, c, flags, kind)
    arena = Arena()
    g = {k: arena.guarded(v, shift) for k, v in c.items()}
    with hostile(arena, shift): got = fused(R, g, flags, kind)
    for k in ('loss', 'warp', 'g_depth', 'g_mask', 'g_Ts'):
        assert_finite(got[k], f'{size} {k}')
        assert torch.equal(got[k], ref[k]), f'{size} shift {shift} {k}: the bits of the plain-memory run'
    assert torch.equal(got['sel'], ref['sel']) and torch.equal(got['stat'], ref['stat'])
    assert int(((got['sel'] != 255) & (got['sel'] >= n)).sum()) == 0 and int((got['stat'] >= n).sum()) == 0, 'every sel / stat byte written: a support index or 255'
    arena.check()


def test_two_runs_give_the_same_bits(R):
    c = {k: v.cuda() for k, v in make_inputs(24, 40, 2, 2, 2, 'uncertainty', seed=3).items()}
    a, b = (fused(R, c, ('ssim', True, True), 'uncertainty') for _ in range(2))
    for k, v in a.items(): assert torch.equal(v, b[k]), k


# ------------------------------------------------------------------------------------------------- value edges
def _edge(name, kind):
    """-> (operands on the CPU, flags, n)."""
    n = 2
    c = make_inputs(17, 23, n, 1, 2, kind, seed=21, hard=False)
    if name == 'depth_edges':      # transformed depth = D + tz with a pure z step: below 0, at 0, at eps, either side of 0.1
        c['Ts'] = torch.eye(4).repeat(n, 2, 1, 1); c['Ts'][:, :, 2, 3] = -1.0
        vals = torch.tensor([0.5, 1.0, 1.0 + 2.0**-23, 1.1 - 2.0**-20, 1.1, 1.1 + 2.0**-20, 3.0])
        c['depth'] = vals[torch.arange(17*23) % 7].reshape(1, 1, 17, 23).expand(1, 2, 17, 23).contiguous()
    if name == 'borders':          # identity rotation, a sideways step of whole pixels at constant depth: samples exactly on and beyond each border
        c['Ts'] = torch.eye(4).repeat(n, 2, 1, 1)
        fx, fy = c['K'][0, 0, 0].item(), c['K'][0, 1, 1].item()
        c['Ts'][0, :, 0, 3] = 3.0*2.0/fx; c['Ts'][1, :, 1, 3] = -2.0*2.0/fy
        c['depth'] = torch.full_like(c['depth'], 2.0)
    if name == 'equal':            # identity pose: the warped pixel equals the support; supports equal to the target: error 0
        c['Ts'] = torch.eye(4).repeat(n, 2, 1, 1); c['supp'] = c['imgs'][None].expand_as(c['supp']).contiguous()
    if name == 'flat':             # constant 3x3 windows (the flat-window SSIM case)
        c['imgs'] = torch.full_like(c['imgs'], 0.75); c['supp'] = torch.full_like(c['supp'], 0.75); c['supp'][1] = 0.25
    if name == 'mask0': c['mask'] = torch.zeros_like(c['mask'])
    if name == 'mask1': c['mask'] = torch.ones_like(c['mask'])
    if name == 'mask50': c['mask'] = torch.full_like(c['mask'], 50.0)
    if name == 'tied': c['supp'][1] = c['supp'][0]; c['Ts'][1] = c['Ts'][0]; c['mask'][:, :, 1] = c['mask'][:, :, 0]
    if name == 'one_ulp':          # the same supports, masks one ulp apart (explainability: the masked errors are one ulp apart, either way round)
        c['supp'][1] = c['supp'][0]; c['Ts'][1] = c['Ts'][0]
        m0 = c['mask'][:, :, 0].abs() + 0.25
        up = torch.nextafter(m0, torch.full_like(m0, 9.0)); dn = torch.nextafter(m0, torch.zeros_like(m0))
        chk = (torch.arange(17)[:, None] + torch.arange(23)[None]) % 2 == 0
        c['mask'][:, :, 0] = m0; c['mask'][:, :, 1] = torch.where(chk, up, dn)
    return c, ('ssim', True, True), n


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['depth_edges', 'borders', 'equal', 'flat', 'mask0', 'mask1', 'mask50', 'tied', 'one_ulp'])
def test_value_edges(R, name, kind):
    """The operands that sit on a comparison or a clamp of the statements.  On each: everything finite, zero decision flips against the plain route (`sel`, the
    static winner, warp0 bit-equal), the loss at the plain route's within rounding, the gradients at the plain handler's within 1e-3 of the maximum."""
    ins, flags, n = _edge(name, kind)
    c = {k: v.cuda() for k, v in ins.items()}
    f, p = fused(R, c, flags, kind), plain_pieces(c, flags, kind)
    for k in ('loss', 'warp', 'g_depth', 'g_mask', 'g_Ts'): assert_finite(f[k], f'{name} {kind} {k}')
    if name in ('mask0', 'mask50', 'tied', 'equal'): p['stat_near'] = None      # exact arithmetic on both routes (products with 0 or 1, sums that round to the mask): ties take the first index
    same_decisions(f'{name} {kind}', f, p, n)
    torch.testing.assert_close(f['loss'], p['loss'], rtol=2e-6, atol=1e-7)
    h = plain_handler(c, flags, kind)
    for k in ('g_depth', 'g_mask', 'g_Ts'):
        scale = h[k].abs().max().clamp(min=1e-20)
        assert ((f[k] - h[k]).abs().max()/scale).item() < 1e-3 or float(h[k].abs().max()) == float(f[k].abs().max()) == 0, (name, kind, k)
    if name == 'tied': assert int(((f['sel'] != 255) & (f['sel'] != 0)).sum()) == 0 and int((f['stat'] != 0).sum()) == 0, 'a tie: the first index'
    if name == 'mask0' and kind == 'explainability':
        assert torch.equal(f['sel'] == 255, c['noise'] < 0), '0 against 0 + eps * noise: the noise\'s sign'
        assert float(f['g_depth'].abs().max()) == 0 and float(f['g_Ts'].abs().max()) == 0, 'a mask of 0 on every support passes no gradient to the geometry'
    if name == 'one_ulp' and kind == 'explainability': assert (f['stat'] == 0).any() and (f['stat'] == 1).any(), 'one ulp decides, both ways'


# ------------------------------------------------------------------------------------------------- the trainer
def test_training_step_against_the_plain_route(R, monkeypatch):
    """One step of cfg/kitti_sfm_learner.yaml on make_batch(2, 64, 96, (-1, 1)) with the fused handler and with `HipLossBackend.image_recon` sent to the plain route:
    the automask equal, every loss within rtol 2e-5, every parameter gradient within 1e-3 of its maximum."""
    from slowtv_monodepth_amd import handlers, io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_sfm_learner.yaml')
    batch = make_batch(2, 64, 96, (-1, 1), seed=5, device=torch.device('cuda'))
    calls = []

    def step(plain):
        if plain:
            monkeypatch.setattr(HipLossBackend, 'image_recon', lambda self, crit, synth, depths, masks, imgs, supp_imgs, Ts, Ks, want_warp=True, K_inv=None, prepared=None:
                                handlers.image_recon(crit, synth, depths, masks, imgs, supp_imgs, Ts.float(), Ks.float(), K_inv=K_inv, want_warp=want_warp, prepared=prepared))
        else:
            real = R.mask_recon_loss
            monkeypatch.setattr(R, 'mask_recon_loss', lambda *a, **k: calls.append(1) or real(*a, **k))
        torch.manual_seed(3)
        m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
        loss, ld, _ = m.step(tuple(dict(d) for d in batch))
        loss.backward()
        monkeypatch.undo()
        return loss.detach(), ld, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    (lf, ldf, gf), (lp, ldp, gp) = step(False), step(True)
    assert calls, 'the trainer reached the fused operator'
    for k in ldp:
        if k.startswith('loss_'): torch.testing.assert_close(ldf[k].detach(), ldp[k].detach(), rtol=2e-5, atol=1e-7, msg=lambda s, k=k: f'{k}: {s}')
    torch.testing.assert_close(lf, lp, rtol=2e-5, atol=1e-7)
    if 'automask' in ldp: assert torch.equal(ldf['automask'], ldp['automask'])
    assert gf.keys() == gp.keys() and gf
    worst = max(rel_to_max(gf[k], gp[k]) for k in gp)
    note(f'kitti_sfm_learner step: loss fused {lf.item():.8f} plain {lp.item():.8f}; worst parameter gradient {worst:.1e} of its maximum')
    assert worst < 1e-3
