"""The fused feature regularisers (csrc/smd_featreg.hip) and what stands on them, on the GPU: `feat_regs` / `feat_regs_pyramid` against the REFERENCE's fixture
(tests/golden/op_featreg.npz) for every case and both `use_edges` settings, run-to-run bit equality, the fused handler against the plain one, the
gradient-subset cases (only peaky, only smooth, an offset incoming gradient), one hostile-memory case, and two training steps of cfg/kitti_featdepth.yaml
against the same module forced onto the plain regularisers.

The bound is test_featdepth_host.featreg_bound (profiles/featdepth_parity.txt): against the reference formula in fp64, at most 4x the error of the reference's
own fp32 ATen result against the same fp64 values, and at least 2 ulp of the tensor's largest magnitude.  Shapes: featdepth_inputs.FEAT_CASES."""
import copy

import pytest
import torch

from conftest import ROOT, parity_note
from featdepth_inputs import FEAT_CASES, FEAT_WEIGHTS, feat_case, handler_case
from hostile_memory import Arena, assert_finite, hostile
from test_featdepth_host import QUANTITIES, featreg_bound, fixture, ref64, ulp_of

pytestmark = pytest.mark.gpu
NAMES = [n for n, _ in FEAT_CASES]


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import featreg
    return featreg


def note(line): parity_note(f'featdepth_parity {line}')


def _run(R, feat, img, edges, **kw):
    """`feat_regs` forward + the three backwards -> dict of QUANTITIES on the CPU."""
    out = {}
    for tag, wp, ws in (('peaky', 1.0, 0.0), ('smooth', 0.0, 1.0), ('both', *FEAT_WEIGHTS)):
        x = feat.detach().clone().requires_grad_(True)
        lp, ls = R.feat_regs(x, img, edges, edges, **kw)
        (lp if tag == 'peaky' else ls if tag == 'smooth' else wp*lp + ws*ls).backward()
        out[f'g_{tag}'] = x.grad.cpu()
    out['l_peaky'], out['l_smooth'] = lp.detach().cpu(), ls.detach().cpu()
    return out


@pytest.mark.parametrize('edges', [False, True], ids=['plain', 'edges'])
@pytest.mark.parametrize('k', range(len(FEAT_CASES)), ids=NAMES)
def test_feat_regs_matches_the_reference_fixture(R, k, edges):
    """Both losses and feat.grad under each loss alone and under their weighted sum within `featreg_bound` of the fp64 reference; everything finite; two runs
    bit-equal; the one-level pyramid form gives the same bits."""
    ins = feat_case(k)
    feat, img = ins['feat'].cuda(), ins['img'].cuda()
    got, again = _run(R, feat, img, edges), _run(R, feat, img, edges)
    fails = []
    for n in QUANTITIES:
        bound, own = featreg_bound(k, edges, n)
        assert torch.isfinite(got[n]).all(), f'{n} is not finite'
        err = (got[n].double() - ref64(k, edges)[n]).abs().max().item()
        note(f'{NAMES[k]} edges={int(edges)} {n}: kernel {err:.3e}  ATen fp32 {own:.3e}  bound {bound:.3e}')
        if not err <= bound: fails.append(f'{n}: {err:.3e} > {bound:.3e}')
        assert torch.equal(got[n], again[n]), f'{n}: two runs on the same inputs differ'
    assert not fails, '; '.join(fails)
    lp, ls = R.feat_regs_pyramid([feat], [img], edges, edges)
    assert torch.equal(lp.cpu(), got['l_peaky']) and torch.equal(ls.cpu(), got['l_smooth']) and lp.shape == () and lp.dtype == torch.float32
    if NAMES[k] == 'const': assert all(float(got[n].abs().max()) == 0 for n in QUANTITIES), 'a constant map: both losses and the gradient are exactly 0'


def _pyramid64(feats, imgs, edges):
    from slowtv_monodepth_amd.featreg import plain_feat_regs
    xs = [f.double().clone().requires_grad_(True) for f in feats]
    lp, ls = plain_feat_regs(xs, [i.double() for i in imgs], edges, edges)
    (FEAT_WEIGHTS[0]*lp + FEAT_WEIGHTS[1]*ls).backward()
    return lp.detach(), ls.detach(), [x.grad for x in xs]


def test_pyramid_form_is_one_launch_and_matches_the_plain_loop(R):
    """Levels of different channel counts and sizes (one of them on the 16-byte path) in ONE autograd node, against the per-scale loop in fp64 and in fp32 by the
    4x rule; a level's gradient is its one-level gradient scaled by 1/(2^s S) up to rounding."""
    from slowtv_monodepth_amd.featreg import plain_feat_regs
    ks = [NAMES.index('vec'), NAMES.index('c64'), NAMES.index('4x6')]
    feats = [feat_case(k)['feat'][:1] for k in ks]; imgs = [feat_case(k)['img'][:1] for k in ks]
    for edges in (False, True):
        want_p, want_s, want_g = _pyramid64(feats, imgs, edges)
        x32 = [f.clone().requires_grad_(True) for f in feats]
        a_p, a_s = plain_feat_regs(x32, imgs, edges, edges)
        (FEAT_WEIGHTS[0]*a_p + FEAT_WEIGHTS[1]*a_s).backward()
        xs = [f.cuda().requires_grad_(True) for f in feats]
        lp, ls = R.feat_regs_pyramid(xs, [i.cuda() for i in imgs], edges, edges)
        assert lp.grad_fn is not None and lp.grad_fn is ls.grad_fn, 'both losses of every level are outputs of ONE autograd node: one launch'
        (FEAT_WEIGHTS[0]*lp + FEAT_WEIGHTS[1]*ls).backward()
        for n, mine, aten, want in [('l_peaky', lp, a_p, want_p), ('l_smooth', ls, a_s, want_s)] + [(f'g[{s}]', xs[s].grad, x32[s].grad, want_g[s]) for s in range(3)]:
            own = (aten.detach().double() - want).abs().max().item()
            bound = max(4*own, 2*ulp_of(want.abs().max().item()))
            err = (mine.detach().cpu().double() - want).abs().max().item()
            note(f'pyramid edges={int(edges)} {n}: kernel {err:.3e}  ATen fp32 {own:.3e}  bound {bound:.3e}')
            assert err <= bound, (n, err, bound)


@pytest.mark.parametrize('tag', ['peaky', 'smooth'])
def test_fused_handler_against_the_plain_handler_and_the_fixture(R, tag, monkeypatch):
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.regularizers import FeatPeakReg, FeatSmoothReg
    g, ins = fixture(), handler_case()
    crit = FeatPeakReg(True) if tag == 'peaky' else FeatSmoothReg(True)

    def run(dev, dtype=torch.float32):
        feats = [f.to(dev, dtype).requires_grad_(True) for f in ins['feats']]; supp = [f.to(dev, dtype).requires_grad_(True) for f in ins['supp_feats']]
        l, ld = handlers.feat_smooth(crit, feats, ins['imgs'].to(dev, dtype), supp, ins['supp_imgs'].to(dev, dtype))
        assert ld == {}
        l.backward()
        return [l.detach().cpu()] + [t.grad.cpu() for t in feats + supp]
    want = run('cpu', torch.float64)
    aten = [g[f'hd_{tag}_loss']] + [g[f'hd_{tag}_g_feat_{s}'] for s in range(2)] + [g[f'hd_{tag}_g_supp_{s}'] for s in range(2)]
    fused = run('cuda')
    monkeypatch.setattr(handlers, '_fused_feat_regs', lambda *a: False)
    plain = run('cuda')
    for j, (mine, pl, at, w) in enumerate(zip(fused, plain, aten, want)):
        own = max((at.double() - w).abs().max().item(), (pl.double() - w).abs().max().item())      # (the GPU's ATen resize differs from the CPU's in the last bit)
        bound = max(4*own, 2*ulp_of(w.abs().max().item()))
        err = (mine.double() - w).abs().max().item()
        note(f'handler {tag} [{j}]: fused {err:.3e}  ATen fp32 {own:.3e}  bound {bound:.3e}')
        assert err <= bound, (j, err, bound)
    monkeypatch.undo()
    pair = handlers.feat_smooth_pair(FeatPeakReg(True), FeatSmoothReg(True), [f.cuda() for f in ins['feats']], ins['imgs'].cuda(), [f.cuda() for f in ins['supp_feats']],
                                     ins['supp_imgs'].cuda())
    assert pair is not None and torch.equal(pair[0 if tag == 'peaky' else 1].cpu(), fused[0]), 'the pair computes the same bits as each loss alone'


@pytest.mark.parametrize('k', [NAMES.index('7x67'), NAMES.index('vec')], ids=['7x67', 'vec'])
def test_gradient_subsets(R, k):
    """Only one of the two losses has an incoming gradient, the other's is absent, or it arrives as an offset view: the written gradient is exactly that loss's,
    i.e. the bits of the run that computes that loss alone, whose value the fixture test holds to the reference."""
    ins = feat_case(k)
    feat, img = ins['feat'].cuda(), ins['img'].cuda()

    def grad(which, seed=None, **kw):
        x = feat.clone().requires_grad_(True)
        out = R.feat_regs(x, img, True, True, **kw)
        l = out[0 if which == 'peaky' else 1]
        l.backward(seed) if seed is not None else l.backward()
        return x.grad
    for which, alone in (('peaky', dict(want_smooth=False)), ('smooth', dict(want_peaky=False))):
        full, only = grad(which), grad(which, **alone)
        assert torch.equal(full, only), f'{which}: the gradient with the other loss unused differs from the run that never computed it'
        buf = torch.tensor([7.0, 0.5, 7.0], device='cuda')
        assert torch.equal(grad(which, seed=buf[1]), 0.5*full), 'an incoming gradient of 1/2 (a power of two: exact), read through an offset view'
    x = feat.clone().requires_grad_(True)
    lp, ls = R.feat_regs(x, img, True, True)
    assert torch.autograd.grad(lp + 0*ls.detach(), x, allow_unused=True)[0] is not None
    frozen = R.feat_regs(feat, img, True, True)
    assert not frozen[0].requires_grad and torch.equal(frozen[0], lp.detach()) and torch.equal(frozen[1], ls.detach()), 'the forward does not depend on who asks'


@pytest.mark.parametrize('shift', [0, 1])
def test_hostile_memory(R, shift):
    """Every operand in a guarded, poisoned block `shift` elements off its alignment, every buffer the operator allocates (the block sums, the two losses, the
    gradient) served from the arena: the bits of the aligned run (shift 1 takes the element path, whose arithmetic and summation order are the vector path's),
    guards intact, every output fully overwritten."""
    ks = [NAMES.index('vec'), NAMES.index('7x67')]
    for k in ks:
        ins = feat_case(k)
        feat, img = ins['feat'].cuda(), ins['img'].cuda()
        want = _run(R, feat, img, True)
        arena = Arena()
        gf, gi = arena.guarded(feat, shift), arena.guarded(img, shift)
        with hostile(arena, shift):
            x = gf.requires_grad_(True)
            lp, ls = R.feat_regs(x, gi, True, True)
            (FEAT_WEIGHTS[0]*lp + FEAT_WEIGHTS[1]*ls).backward()
        for n, t in (('l_peaky', lp), ('l_smooth', ls), ('g_both', x.grad)):
            assert_finite(t.detach(), f'{NAMES[k]} {n}')
            assert torch.equal(t.detach().cpu(), want[n]), f'{NAMES[k]} shift {shift} {n}: the bits of the aligned run'
        arena.check()


def test_two_training_steps_against_the_plain_regularisers(R, monkeypatch):
    """cfg/kitti_featdepth.yaml on the GPU, two optimizer steps: with the fused pair and with the module forced onto the plain regularisers.  Step 1 runs on
    identical weights: the two regularisers' losses agree to 1e-5 relative (fp32 means over up to 3e5 elements, five scales) and every other loss bit for bit
    is not required (the autoencoder's gradients differ in the last bits); step 2 runs on weights one AdamW step apart by those bits: 1e-2."""
    from slowtv_monodepth_amd import handlers, io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_featdepth.yaml')
    batch = make_batch(2, 64, 96, [-1, 1], seed=5, device=torch.device('cuda'))

    def two_steps(plain):
        calls = []
        real = handlers.feat_smooth_pair
        monkeypatch.setattr(handlers, '_fused_feat_regs', (lambda *a: False) if plain else handlers._fused_feat_regs)
        monkeypatch.setattr(handlers, 'feat_smooth_pair', lambda *a: calls.append(1) or real(*a))
        torch.manual_seed(3)
        m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
        opt = m.configure_optimizers()['optimizer']
        out = []
        for _ in range(2):
            loss, ld, _ = m.step(tuple(dict(d) for d in batch))
            loss.backward(); opt.step(); opt.zero_grad()
            assert m._feat_pair is None
            out.append({k: float(v.detach()) for k, v in ld.items() if k.startswith('loss_')} | {'loss': float(loss.detach())})
        monkeypatch.undo()
        return out, len(calls)
    fused, n_fused = two_steps(False)
    plain, n_plain = two_steps(True)
    assert n_fused == 2 and n_plain == 2, 'the pair is asked for once per step'
    assert set(fused[0]) == {f'loss_{k}' for k in cfg['loss']} | {'loss'}
    for step, tol in ((0, 1e-5), (1, 1e-2)):
        for k in fused[step]:
            a, b = fused[step][k], plain[step][k]
            note(f'train step {step} {k}: fused {a:.8f} plain {b:.8f}')
            assert a == a and abs(a) != float('inf')
            assert abs(a - b) <= tol*max(abs(b), 1e-6), (step, k, a, b)
