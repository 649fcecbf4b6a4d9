"""The fused feature-metric reconstruction loss (csrc/smd_featrecon.hip) on the GPU: `handlers.feat_recon_fused` against the REFERENCE's fixture
(tests/golden/hd_feat_recon.npz) at the bounds test_gpu_parity.py::test_feat_recon_handler_matches_reference holds the plain handler to, `sel` against the plain
path's; the seeded cases of test_featrecon_host.py against the fp64 oracle under the project's 4x rule, their decisions against the oracle's; run-to-run bit
equality; this operator's gradient-subset, hostile-memory and value-edge cases (harnesses: grad_subsets.py, hostile_memory.py, value_edges.py); two training
steps of cfg/kitti_featdepth.yaml with the fused and with the plain handler.

Bound of the oracle cases (`value_edges.excess` under ('yard_ulp',), the rule of profiles/featdepth_parity.txt): the kernel's largest error against the fp64 oracle
is at most 4x the plain handler's largest error against the same fp64 values on the same case, and never asked to be below 2 ulp of the largest fp64 magnitude.
It holds for loss, warp, g_depth, g_aa and g_t on every case, every element taking part.  Pixels may differ from the oracle's selection only where
test_featrecon_host.py's `near` allows it (at most 0.5 % of a case) and on its structural ties; where some do, the fp64 values are the oracle's statements evaluated
again under the selection that was taken (`run_oracle(force_sel=...)`: a pixel decided differently carries another candidate's error and gradient), for the kernel
and for the plain handler alike.  On every case `sel` equals the plain path's pixel for pixel.  Measured ratios: profiles/featrecon_parity.txt."""
import copy

import pytest
import torch

from conftest import ROOT, load_golden, parity_note, rel_to_max
from grad_subsets import check_subsets, subsets_of
from hostile_memory import Arena, assert_finite, hostile
from test_featrecon_host import CASES, MAX_LEFT_OUT, case_inputs, fixture_inputs, oracle_case
from value_edges import excess

pytestmark = pytest.mark.gpu
YARD = ('yard_ulp',)


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available(): pytest.skip('no GPU')
    from slowtv_monodepth_amd import featrecon
    return featrecon


def note(line): parity_note(f'featrecon_parity {line}')


def _crit(loss_name='l2', use_min=True, use_automask=True):
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    return ReconstructionLoss(loss_name=loss_name, use_min=use_min, use_automask=use_automask)


def _run(ins, flags=('l2', True, True), *, fused=True, want_warp=False, need=('depth', 'pose'), noise=True, seed=None):
    """One forward + backward of the fused or the plain handler on a case -> dict on the CPU: loss, sel (b,1,H,W), warp | None, g_depth, g_aa, g_t (None if frozen)."""
    from slowtv_monodepth_amd import functional as F, handlers
    c = {k: v.cuda() for k, v in ins.items()}
    depth = c['depth'].clone().requires_grad_('depth' in need)
    aa, t = c['aa'].clone().requires_grad_('pose' in need), c['t'].clone().requires_grad_('pose' in need)
    n, b = aa.shape[:2]
    Ts = F.pose_matrices(aa.flatten(0, 1), t.flatten(0, 1)).unflatten(0, (n, b))
    crit = _crit(*flags)
    if seed is not None: crit.noise_seed = seed - 1
    nz = c['noise'] if noise else None
    sels, real = [], F.recon_reduce
    if fused:
        from slowtv_monodepth_amd import featrecon
        real_loss = featrecon.feat_recon_loss
        def spy(*a, **k):
            out = real_loss(*a, **k); sels.append(out[1]); return out
        featrecon.feat_recon_loss = spy
        try: loss, ld = handlers.feat_recon_fused(crit, None, {0: depth}, None, c['feats'], c['supp_feats'], Ts, c['K'], noise=nz, want_warp=want_warp)
        finally: featrecon.feat_recon_loss = real_loss
    else:
        def spy(*a, **k):
            out = real(*a, **k); sels.append(out[2].unsqueeze(1)); return out
        F.recon_reduce = spy
        try: loss, ld = handlers.feat_recon(crit, None, {0: depth}, None, c['feats'], c['supp_feats'], Ts, c['K'], noise=nz)
        finally: F.recon_reduce = real
    assert len(sels) == 1, 'the kernel path (or the plain path) ran exactly once'
    if need: loss.backward()
    g = lambda v: None if v.grad is None else v.grad.cpu()
    return dict(loss=loss.detach().cpu(), sel=sels[0].cpu(), warp=ld['supp_feats_warp'].detach().cpu() if 'supp_feats_warp' in ld else None, g_depth=g(depth), g_aa=g(aa), g_t=g(t))


# ------------------------------------------------------------------------------------------------- the reference's fixture
def test_fused_handler_matches_the_reference_fixture(R):
    g, ins = load_golden('hd_feat_recon'), fixture_inputs()
    got, plain = _run(ins, want_warp=True), _run(ins, fused=False)
    note(f'fixture: loss fused {got["loss"].item():.8f} plain {plain["loss"].item():.8f} reference {g["out_loss"].item():.8f}; warp max |d| {(got["warp"] - g["out_supp_feats_warp"]).abs().max():.2e}; '
         + ', '.join(f'g_{k} {rel_to_max(got[f"g_{k}"], g[f"grad_{k}"]):.1e}' for k in ('depth', 'aa', 't')) + f'; sel differs from the plain path on {int((got["sel"] != plain["sel"]).sum())} pixels')
    torch.testing.assert_close(got['loss'], g['out_loss'], rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(got['warp'], g['out_supp_feats_warp'], rtol=1e-4, atol=1e-4)
    for k in ('depth', 'aa', 't'): assert rel_to_max(got[f'g_{k}'], g[f'grad_{k}']) < 1e-3, k
    assert torch.equal(got['sel'], plain['sel']), 'sel equals the plain path\'s everywhere'
    o = oracle_case('fixture')
    differs = got['sel'] != o['sel']
    assert not (differs & ~o['tied']).any(), 'the fixture has no near-tie: outside its structural ties the oracle\'s selection'


# ------------------------------------------------------------------------------------------------- the seeded cases against the fp64 oracle
def _decisions(name, got, o):
    """`sel` against the oracle's: differences only on `near` pixels (at most 0.5 % of the case) and on the structural ties, where it is one of the two tied candidates."""
    differs = got['sel'] != o['sel']
    assert not (differs & ~(o['near'] | o['tied'])).any(), f'{name}: {int((differs & ~(o["near"] | o["tied"])).sum())} pixels decided against a margin above 1e-5'
    left_out = (differs & o['near']).float().mean().item()
    assert left_out <= MAX_LEFT_OUT, (name, left_out)
    on_tie = differs & o['tied']
    assert ((got['sel'] == 255) | (o['sel'] == 255))[on_tie].all(), f'{name}: a structural tie is between the static candidate and the warped winner'
    return differs


def _under(ins, flags, sel, o):
    """The fp64 oracle's loss, warp and gradients under the selection `sel`: the oracle's own run where `sel` is its selection, else its statements again with the
    decisions taken from `sel` (a pixel decided differently carries another candidate's error and gradient; `_decisions` has said where that is allowed)."""
    from test_featrecon_host import run_oracle
    return o if torch.equal(sel, o['sel']) else run_oracle(ins, *flags, force_sel=sel)


def _against_fp64(name, ins, flags, got, plain, o):
    """Loss, warp and the three gradients of the kernel against fp64 under the kernel's own selection, the plain handler's against fp64 under the plain handler's
    own selection (the same one wherever `sel` is equal), under the 4x rule; every element and every output takes part.  -> the list of misses."""
    ref = _under(ins, flags, got['sel'], o)
    ref_plain = ref if torch.equal(plain['sel'], got['sel']) else _under(ins, flags, plain['sel'], o)
    fails = []
    for k in ('loss', 'warp', 'g_depth', 'g_aa', 'g_t'):
        assert_finite(got[k], f'{name} {k}')
        own_err = plain[k].double() - ref_plain[k]
        e = excess(got[k], ref[k], YARD, yard=ref[k] + own_err)                          # the yardstick's error, measured against its own reference
        own, mine = own_err.abs().max().item(), (got[k].double() - ref[k]).abs().max().item()
        note(f'{name} {k}: kernel {mine:.3e}  plain {own:.3e}  ratio to the bound {e:.2f}')
        if not e <= 1.0: fails.append(f'{k}: {mine:.3e} against plain {own:.3e} ({e:.2f} x the bound)')
    return fails


@pytest.mark.parametrize('name', list(CASES))
def test_cases_against_the_fp64_oracle(R, name):
    flags = CASES[name][7:10]
    ins, o = case_inputs(name), oracle_case(name)
    got, plain = _run(ins, flags, want_warp=True), _run(ins, flags, fused=False)
    again = _run(ins, flags)
    for k in ('loss', 'sel', 'g_depth', 'g_aa', 'g_t'): assert torch.equal(got[k], again[k]), f'{k}: two runs differ, or the loss depends on want_warp'
    _decisions(name, got, o); _decisions(name, plain, o)
    note(f'{name}: sel differs from the oracle on {int((got["sel"] != o["sel"]).sum())} pixels (near {int(o["near"].sum())}, tied {int(o["tied"].sum())}), from the plain path on {int((got["sel"] != plain["sel"]).sum())}')
    assert torch.equal(got['sel'], plain['sel']), f'{name}: sel equals the plain path\'s everywhere'
    fails = _against_fp64(name, ins, flags, got, plain, o)
    assert not fails, f'{name}: ' + '; '.join(fails)
    if name == 'border':
        frozen = got['g_depth'] == 0
        assert 0.2 <= frozen.float().mean().item(), 'border-clamped and auto-masked pixels carry no gradient'


def test_seeded_noise_is_recon_reduce_s(R):
    """Without a noise tensor both paths draw from the shared generator under the criterion's seed: the same selection, bit-equal to the run under the same seed
    again, different under another seed."""
    ins = case_inputs('n3')
    a, p, other = _run(ins, noise=False, seed=7), _run(ins, noise=False, seed=7, fused=False), _run(ins, noise=False, seed=8)
    o = oracle_case('n3')
    assert torch.equal(a['sel'], p['sel']) and torch.equal(a['sel'], _run(ins, noise=False, seed=7)['sel']), 'equal seeds draw equal noise on both paths'
    assert (a['sel'] != other['sel'])[o['tied']].any() or int(o['tied'].sum()) == 0, 'another seed decides the ties differently'
    torch.testing.assert_close(a['loss'], p['loss'], rtol=2e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------- gradient subsets, hostile memory, value edges
def _operands(ins):
    from slowtv_monodepth_amd import functional as F
    c = {k: v.cuda() for k, v in ins.items()}
    n, b = c['aa'].shape[:2]
    c['Ts'] = F.pose_matrices(c['aa'].flatten(0, 1), c['t'].flatten(0, 1)).unflatten(0, (n, b))
    c['K_inv'] = F.inv_intrinsics(c['K'])
    return c


@pytest.mark.parametrize('flags', [('l2', True, True), ('l1', False, False)], ids=['l2_min_auto', 'l1_mean'])
def test_gradient_subsets(R, flags):
    """depth only, poses only, both: the bits of the full backward and nothing for the operand left out (`g_T` absent selects the launch that never forms the pose
    sums, `g_depth` absent the one that never stores it); an incoming gradient that is a strided view, and an expanded one, scale it exactly."""
    c = _operands(case_inputs('n3'))
    diff = ('depth', 'Ts')

    def run(subset, gy=None):
        leaves = {k: c[k].clone().requires_grad_(k in subset) for k in diff}
        loss, sel, _ = R.feat_recon_loss(leaves['depth'], c['feats'], c['supp_feats'], leaves['Ts'], c['K'], c['K_inv'], loss_name=flags[0], use_min=flags[1], use_automask=flags[2],
                                         noise=c['noise'])
        if subset: loss.backward(gy) if gy is not None else loss.backward()
        return {'loss': loss.detach(), 'sel': sel, **{f'g_{k}': leaves[k].grad for k in diff}}
    full = run(frozenset(diff))
    check_subsets(run, full, subsets_of(diff), diff, name=f'feat_recon_loss {flags}')
    frozen = run(frozenset())
    assert torch.equal(frozen['loss'], full['loss']) and torch.equal(frozen['sel'], full['sel']), 'the forward does not depend on who asks'
    buf = torch.tensor([[7.0, 0.5], [7.0, 7.0]], device='cuda')
    for gy in (buf[0, 1], buf.t()[1, 0], torch.tensor(0.5, device='cuda').expand(3)[1]):
        half = run(frozenset(diff), gy)
        assert torch.equal(half['g_depth'], 0.5*full['g_depth']) and torch.equal(half['g_Ts'], 0.5*full['g_Ts'])


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('name', ['w67', 'ratio_5x7_18x26'])
def test_hostile_memory(R, name, shift):
    """Every operand in a guarded, poisoned block `shift` elements off its alignment, every buffer the operator allocates (block sums, pose sums, loss, sel, warp,
    gradients) served from the arena: the bits of the plain-memory run, guards intact, every output fully overwritten."""
    flags = CASES[name][7:10]
    c = _operands(case_inputs(name))
    kw = dict(loss_name=flags[0], use_min=flags[1], use_automask=flags[2], want_warp=True)
    d0, T0 = c['depth'].clone().requires_grad_(True), c['Ts'].clone().requires_grad_(True)
    l0, s0, w0 = R.feat_recon_loss(d0, c['feats'], c['supp_feats'], T0, c['K'], c['K_inv'], noise=c['noise'], **kw)
    l0.backward()
    arena = Arena()
    g = {k: arena.guarded(c[k], shift) for k in ('depth', 'feats', 'supp_feats', 'Ts', 'K', 'K_inv', 'noise')}
    with hostile(arena, shift):
        d, T = g['depth'].requires_grad_(True), g['Ts'].requires_grad_(True)
        l, s, w = R.feat_recon_loss(d, g['feats'], g['supp_feats'], T, g['K'], g['K_inv'], noise=g['noise'], **kw)
        l.backward()
    for what, a, ref in (('loss', l.detach(), l0.detach()), ('warp', w, w0), ('g_depth', d.grad, d0.grad), ('g_T', T.grad, T0.grad)):
        assert_finite(a, f'{name} {what}')
        assert torch.equal(a, ref), f'{name} shift {shift} {what}: the bits of the plain-memory run'
    assert torch.equal(s, s0) and int(((s != 255) & (s >= CASES[name][6])).sum()) == 0, 'every sel byte written: a support index or 255'
    arena.check()


def _edge_case(fill):
    ins = case_inputs('n1' if fill in ('equal', 'equal_const') else 'n3')
    if fill == 'equal': ins['supp_feats'] = ins['feats'][None].expand_as(ins['supp_feats']).contiguous()
    if fill == 'equal_const': ins['feats'] = torch.full_like(ins['feats'], 0.75); ins['supp_feats'] = torch.full_like(ins['supp_feats'], 0.75)
    if fill == 'zero': ins['feats'] = torch.zeros_like(ins['feats']); ins['supp_feats'] = torch.zeros_like(ins['supp_feats'])
    if fill in ('equal_const', 'zero'):      # eps * noise must not vanish against sqrt(eps) (half an ulp of it is eps * 1.2e-4)
        nz = ins['noise']
        ins['noise'] = torch.where(nz.abs() < 1e-2, torch.where(nz < 0, -1e-2, 1e-2).to(nz.dtype), nz)
    if fill == 'scale_1e4': ins['feats'] = 1e4*ins['feats']; ins['supp_feats'] = 1e4*ins['supp_feats']
    if fill == 'scale_1e-4': ins['feats'] = 1e-4*ins['feats']; ins['supp_feats'] = 1e-4*ins['supp_feats']
    if fill == 'min_depth': ins['depth'] = torch.full_like(ins['depth'], 0.1)
    if fill == 'max_depth': ins['depth'] = torch.full_like(ins['depth'], 100.0)
    if fill == 'const': ins['feats'] = torch.full_like(ins['feats'], 0.5); ins['supp_feats'] = torch.full_like(ins['supp_feats'], 0.75)
    return ins


@pytest.mark.parametrize('fill', ['equal', 'equal_const', 'zero', 'scale_1e4', 'scale_1e-4', 'min_depth', 'max_depth', 'const'])
def test_value_edges(R, fill):
    """Supports equal to the target: the static error is exactly 0 under the square root, clamp(min=eps) is active, every pixel is auto-masked and no gradient flows.
    Equal constant maps and all-zero features: the warped and the static error are both sqrt(eps), the noise alone decides (sel = 255 exactly where it is
    negative) and the gradient is exactly 0.  Features at 1e4 and 1e-4, depth at min_depth and max_depth: the fp64 oracle under the 4x rule.  A constant map per
    tensor (ratio 4, dyadic values): zero spatial derivative, g_depth exactly 0."""
    from test_featrecon_host import run_oracle
    ins = _edge_case(fill)
    flags = ('l2', True, fill != 'const')
    got = _run(ins, flags, want_warp=True)
    for k in ('loss', 'warp', 'g_depth', 'g_aa', 'g_t'): assert_finite(got[k], f'{fill} {k}')
    root_eps = torch.tensor(2.0**-23, dtype=torch.float64).sqrt()
    est = root_eps + 2.0**-23*ins['noise'].double()
    zero_grad = all(float(got[k].abs().max()) == 0 for k in ('g_depth', 'g_aa', 'g_t'))
    if fill == 'equal':
        masked = got['sel'] == 255
        assert (masked | (ins['noise'] > 0)).all() and masked.float().mean().item() >= 0.97, 'un-masked only in the clamped corners, where the warp is the support itself and the noise is positive'
        assert zero_grad, 'where a warped support is selected its error is under the clamp: no gradient anywhere'
        want = torch.where(masked, est, root_eps).mean().item()
        assert abs(got['loss'].item() - want) <= 2e-6*want
    elif fill in ('equal_const', 'zero'):
        assert ins['noise'].abs().min().item() > 1e-3, 'no noise value so small that eps * noise is lost against sqrt(eps)'
        assert torch.equal(got['sel'] == 255, ins['noise'] < 0), 'a tie of sqrt(eps) against sqrt(eps) + eps * noise: the noise\'s sign'
        assert zero_grad and float((got['warp'] - (0.75 if fill == 'equal_const' else 0.0)).abs().max()) == 0
    elif fill == 'const':
        assert zero_grad, 'a constant map has no spatial derivative'
        assert float((got['warp'] - 0.75).abs().max()) == 0 and (got['sel'] == 0).all() and abs(got['loss'].item() - 0.25*6**0.5) <= 2e-6
    else:
        o, plain = run_oracle(ins, *flags), _run(ins, flags, fused=False)
        _decisions(fill, got, o); _decisions(fill, plain, o)
        note(f'value edge {fill}: sel differs from the oracle on {int((got["sel"] != o["sel"]).sum())} pixels, from the plain path on {int((got["sel"] != plain["sel"]).sum())}')
        fails = _against_fp64(f'value edge {fill}', ins, flags, got, plain, o)
        assert not fails, f'{fill}: ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------- the training step
def test_two_training_steps_against_the_plain_handler(R, monkeypatch):
    """cfg/kitti_featdepth.yaml at b = 1, 64 x 96 on synthetic data, two optimizer steps from one seed with the fused and with the plain handler: the first step's
    `loss_feat_recon` to the fixture's loss bound (rtol 2e-5, atol 1e-7), every parameter gradient of the first step to 1e-3 of its maximum; the second step runs
    and stays finite.  (Both runs draw the automask's noise from the criterion's seed, the same generator on both paths.)"""
    from slowtv_monodepth_amd import featrecon, io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_featdepth.yaml')
    batch = make_batch(1, 64, 96, [-1, 1], seed=5, device=torch.device('cuda'))

    def two_steps(plain):
        calls, real = [], featrecon.feat_recon_loss
        monkeypatch.setattr(featrecon, 'served', (lambda *a: False) if plain else featrecon.served)
        monkeypatch.setattr(featrecon, 'feat_recon_loss', lambda *a, **k: calls.append(1) or real(*a, **k))
        torch.manual_seed(3)
        m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
        opt = m.configure_optimizers()['optimizer']
        out = []
        for _ in range(2):
            loss, ld, _ = m.step(tuple(dict(d) for d in batch))
            loss.backward()
            out.append(({k: v.detach().cpu() for k, v in ld.items() if k.startswith('loss_')}, {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}))
            opt.step(); opt.zero_grad()
        monkeypatch.undo()
        return out, len(calls)
    fused, n_fused = two_steps(False)
    plain, n_plain = two_steps(True)
    assert n_fused == 2 and n_plain == 0, 'the kernel ran once per step, and not at all in the plain run'
    assert 'supp_feats_warp' not in fused[0][0]
    torch.testing.assert_close(fused[0][0]['loss_feat_recon'], plain[0][0]['loss_feat_recon'], rtol=2e-5, atol=1e-7)
    assert set(fused[0][1]) == set(plain[0][1])
    worst = max((rel_to_max(fused[0][1][n], plain[0][1][n]), n) for n in plain[0][1] if plain[0][1][n].abs().max() > 0)
    note(f'train step 1: loss_feat_recon fused {fused[0][0]["loss_feat_recon"].item():.8f} plain {plain[0][0]["loss_feat_recon"].item():.8f}; worst parameter gradient {worst[0]:.2e} ({worst[1]})')
    assert worst[0] <= 1e-3, worst
    for k, v in fused[1][0].items(): assert torch.isfinite(v), k
