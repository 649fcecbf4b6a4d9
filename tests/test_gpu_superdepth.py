"""The SuperDepth decoder on the GPU: `subpixel_conv` (csrc/smd_subpixel.hip) against the REFERENCE's fixture (tests/golden/op_subpixel.npz), its gradient
subsets and incoming-gradient layouts through grad_subsets.py's checker on a local entry, one hostile-memory case, the glued decoder against the reference's
`SuperdepthDecoder` (tests/golden/net_decoder_superdepth_64x96.npz) and against its own plain path, a ConvNeXt feature list, the mask decoder, the loss path on a
pyramid of four full-resolution scales, the example config through the trainer.  Observed figures: profiles/superdepth_parity.txt."""
import copy

import pytest
import torch
import yaml

import grad_subsets as G
from conftest import ROOT, load_golden, parity_note, rel_to_max
from hostile_memory import Arena, assert_finite, hostile
from superdepth_inputs import SUBPIXEL_CASES, SUBPIXEL_NAMES, SUPERDEPTH_KW, subpixel_aten, subpixel_case
from test_ddvnet_host import FLOOR
from test_superdepth_host import build, run_and_compare

pytestmark = pytest.mark.gpu
CASE_IDS = ['-'.join(map(str, c)) for c in SUBPIXEL_CASES]


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def note(line):
    parity_note(f'superdepth_parity {line}')


def _run(F, k, need=None, ins=None):
    """`subpixel_conv` on case k, forward and backward -> [out, grad_x, grad_pre_bias, grad_weight, grad_bias, grad_skip] (None where the operand is absent
    or, with `need`, did not ask)."""
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]
    ins = ins or {n: (t.cuda() if t is not None else None) for n, t in subpixel_case(k).items()}
    L = {n: (t.detach().clone().requires_grad_(need is None or n in need) if t is not None else None) for n, t in ins.items() if n != 'gout'}
    out = F.subpixel_conv(L['x'], L['weight'], L['bias'], r, pre_bias=L['pre_bias'], pre_act=pre, act=act, skip=L['skip'], pad=pad)
    out.backward(ins['gout'])
    return [out.detach()] + [L[n].grad if L[n] is not None else None for n in ('x', 'pre_bias', 'weight', 'bias', 'skip')]


@pytest.mark.parametrize('k', range(len(SUBPIXEL_CASES)), ids=CASE_IDS)
def test_subpixel_conv_matches_the_reference_fixture(F, k):
    """Output and all five gradients against what the reference's SubPixelConv (with its surroundings) produced: relative to each tensor's maximum, at most
    the larger of FLOOR and 4 x the reference's own fp32-vs-fp64 error; everything finite; two runs bit-equal."""
    g = load_golden('op_subpixel')
    got, again = _run(F, k), _run(F, k)
    fails = []
    for what, mine in zip(SUBPIXEL_NAMES, got):
        assert (mine is not None) == (f'{what}_{k}' in g), what
        if mine is None: continue
        assert torch.isfinite(mine).all(), f'{what} is not finite'
        err, yard = rel_to_max(mine.cpu(), g[f'{what}_{k}']), float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])
        note(f'subpixel_conv fixture[{k}] {CASE_IDS[k]:>28} {what:13}: kernel vs reference {err:.2e}  reference fp32 vs fp64 {yard:.2e}  bound {max(FLOOR, 4*yard):.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'{what}: {err:.2e} (bound {max(FLOOR, 4*yard):.2e})')
    differ = [n for n, x, y in zip(SUBPIXEL_NAMES, got, again) if x is not None and not torch.equal(x, y)]
    assert not differ, f'two runs on the same inputs differ in {differ}'
    assert not fails, f'case {k}: ' + '; '.join(fails)


def test_relu_output_of_exactly_zero_passes_no_gradient(F):
    """weight = 0 and bias = 0: v is exactly 0 everywhere, relu(0) = 0, and torch's convention gives such a pixel gradient 0."""
    x = torch.randn(1, 2, 3, 4, device='cuda', requires_grad=True)
    w, b = torch.zeros(8, 1, 3, 3, device='cuda', requires_grad=True), torch.zeros(8, device='cuda', requires_grad=True)
    out = F.subpixel_conv(x, w, b, 2, act='relu')
    out.backward(torch.ones_like(out))
    assert (out == 0).all() and (x.grad == 0).all() and (w.grad == 0).all() and (b.grad == 0).all()


# ------------------------------------------------------------------------------------------------- gradient subsets, gradient layouts, hostile memory
def _entry(k):
    """A `grad_subsets.Entry` for case k, built locally (the table of grad_subsets.py lists the `*_ops.py` modules' Functions; this operator's module is not one)."""
    from slowtv_monodepth_amd.subpixel import _SubPixelConv
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]

    def operands(gen, absent=frozenset()):
        o = {n: t for n, t in subpixel_case(k).items() if t is not None}
        o['gy_out'] = o.pop('gout')
        return {n: t for n, t in o.items() if n not in absent}
    call = lambda F, o: dict(out=F.subpixel_conv(o['x'], o['weight'], o['bias'], r, pre_bias=o.get('pre_bias'), pre_act=pre, act=act, skip=o.get('skip'), pad=pad))
    ref = lambda o: dict(out=subpixel_aten(o['x'], o.get('pre_bias'), o['weight'], o['bias'], o.get('skip'), r, pre, act, pad))
    diff = [n for n in ('x', 'pre_bias', 'weight', 'bias', 'skip') if n != 'skip' or Cs]
    return G.Entry(f'subpixel_conv{SUBPIXEL_CASES[k]}', _SubPixelConv, 'subpixel_conv', operands, tuple(diff), ('pre_bias',), ('out',), call, ref, {}, {},
                   (frozenset(['weight', 'bias']), frozenset(['x', 'pre_bias'])), True, {})


@pytest.mark.parametrize('k', [0, 6], ids=[CASE_IDS[0], CASE_IDS[6]])
def test_gradient_subsets_and_incoming_gradient_layouts(F, k):
    """grad_subsets.py's rule on a local entry: each subset of the operands asking for a gradient, in hostile memory, returns the BITS of the full backward for
    those and nothing for the rest; the full run is held to the fp64 restatement at the yardstick rule; a stride-0 expanded and a channels-last-strided
    incoming gradient give the bits of the contiguous one."""
    e = _entry(k)
    o = e.operands(None)
    ref, ref32 = G.run_reference(e, o), G.run_reference(e, o, torch.float32)
    bounds = G.bounds_of(e, o, ref, ref32)
    diff = list(e.diff)
    cuda = {n: t.cuda() for n, t in o.items()}
    full = G.run_entry(e, F, cuda, frozenset(diff))
    G.check_full(f'{e.name} (every operand asks)', full, ref, bounds)

    def in_hostile_memory(subset):
        arena = Arena()
        ops = {n: arena.guarded(t) for n, t in cuda.items()}
        with hostile(arena): out = G.run_entry(e, F, ops, subset)
        arena.check()
        return out
    subsets = G.subsets_of(diff, e.groups)
    G.check_subsets(in_hostile_memory, full, subsets, diff, name=e.name)
    note(f'{e.name}: {len(subsets)} gradient subsets bit-equal to the full backward')
    ones = G.run_entry(e, F, cuda, frozenset(diff), gy=dict(out=torch.ones_like(full['out'])))
    expanded = G.run_entry(e, F, cuda, frozenset(diff), gy=dict(out=torch.ones((), device='cuda').expand_as(full['out'])))
    strided = G.run_entry(e, F, cuda, frozenset(diff), gy=dict(out=cuda['gy_out'].contiguous(memory_format=torch.channels_last)))
    for d in diff:
        assert torch.equal(expanded[f'g_{d}'], ones[f'g_{d}']), f'{d}: stride-0 expanded gradient'
        assert torch.equal(strided[f'g_{d}'], full[f'g_{d}']), f'{d}: channels-last-strided gradient'
    # the optional operand absent, every gradient asked for
    oa = e.operands(None, frozenset(['pre_bias']))
    ra = G.run_reference(e, oa)
    G.check_full(f'{e.name} without pre_bias', G.run_entry(e, F, {n: t.cuda() for n, t in oa.items()}, frozenset(diff)), ra, G.bounds_of(e, oa, ra, G.run_reference(e, oa, torch.float32)))


@pytest.mark.parametrize('shift', [0, 1])
def test_operator_in_hostile_memory(F, shift):
    """Case 5 (skip, pad, a row that crosses a wave) on operands in guarded, poisoned, `shift`-element-offset blocks with every buffer the operator allocates
    served from the arena, forward and backward: guards intact, results finite and bit-equal to the run in plain memory."""
    k = 5
    ins = {n: (t.cuda() if t is not None else None) for n, t in subpixel_case(k).items()}
    plain = _run(F, k, ins=ins)
    arena = Arena()
    with hostile(arena):
        got = _run(F, k, ins={n: (arena.guarded(t, shift) if t is not None else None) for n, t in ins.items()})
        served = sum(1 for b in arena.blocks if b[4] == torch.uint8)
    for what, t in zip(SUBPIXEL_NAMES, got): assert_finite(t, what)
    differ = [n for n, x, y in zip(SUBPIXEL_NAMES, got, plain) if not torch.equal(x, y)]
    assert not differ, f'differs from the run in plain memory in {differ}'
    assert served >= 1, 'the backward\'s workspace did not come from the arena'
    arena.check()


def test_operator_refuses_wrong_operands_on_the_gpu(F):
    ins = {n: (t.cuda() if t is not None else None) for n, t in subpixel_case(0).items()}
    x, w, b, pb, skip = ins['x'], ins['weight'], ins['bias'], ins['pre_bias'], ins['skip']
    with pytest.raises(TypeError): F.subpixel_conv(x.double(), w, b, 2)
    with pytest.raises(TypeError): F.subpixel_conv(x, w.double(), b, 2)
    with pytest.raises(TypeError): F.subpixel_conv(x, w, b, 2, skip=skip.double(), pad=True)
    with pytest.raises(RuntimeError, match='GPU'): F.subpixel_conv(x, w.cpu(), b, 2)
    with pytest.raises(RuntimeError, match='GPU'): F.subpixel_conv(x, w, b, 2, pre_bias=pb.cpu())
    with pytest.raises(ValueError): F.subpixel_conv(x, w, b, 2, skip=skip.transpose(2, 3), pad=True)
    out = F.subpixel_conv(x, w, b, 2, pre_bias=pb, pre_act='elu', act='relu', skip=skip, pad=True)      # and what is right still runs
    assert out.shape == (2, 5, 8, 12) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------- decoder
def test_glued_decoder_matches_the_reference_decoder(F):
    """Outputs, feature gradients and parameter gradients against the reference's, at the rule with the fixture's recorded yardsticks."""
    g = load_golden('net_decoder_superdepth_64x96')
    dec, out, _ = run_and_compare('cuda', max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_out'])), max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_grad'])))
    assert all(o.is_cuda and o.shape == (1, 1, 64, 96) for o in out.values())


def _paths(dec, feats, gouts):
    """-> {'glued' | 'plain' | 'fp64': (outputs, feature gradients, parameter gradients)} of one decoder on the same inputs."""
    res = {}
    for name in ('glued', 'plain', 'fp64'):
        d = copy.deepcopy(dec).double() if name == 'fp64' else dec
        d.zero_grad(set_to_none=True)
        dt = torch.float64 if name == 'fp64' else torch.float32
        leaves = [f.detach().to(dt).clone().requires_grad_(True) for f in feats]
        if name == 'plain':
            with d.plain_path(): out = d(leaves)
        else: out = d(leaves)
        sum((out[i]*gouts[i].to(dt)).sum() for i in out).backward()
        res[name] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in leaves], {k: p.grad.clone() for k, p in d.named_parameters() if p.grad is not None})
    return res


def _hold_paths(tag, res):
    """The glued path against the fp64 run of the plain path, with the fp32 plain path's error against it as the yardstick (outputs in absolute terms)."""
    (o1, f1, p1), (o0, f0, p0), (o64, f64, p64) = res['glued'], res['plain'], res['fp64']
    fails = []
    assert sorted(o1) == sorted(o64) and sorted(p1) == sorted(p0) == sorted(p64)
    for i in o64:
        err, yard = (o1[i].double() - o64[i]).abs().max().item(), (o0[i].double() - o64[i]).abs().max().item()
        note(f'{tag} output {i}: glued {err:.2e}  plain fp32 {yard:.2e}')
        assert o1[i].dtype == torch.float32 and torch.isfinite(o1[i]).all()
        if not err <= max(FLOOR, 4*yard): fails.append(f'output {i}: {err:.2e} vs {yard:.2e}')
    for what, mine, t32, ref in [(f'feature {j}', a, b, c) for j, (a, b, c) in enumerate(zip(f1, f0, f64))] + [(k, p1[k], p0[k], p64[k]) for k in sorted(p64)]:
        err, yard = rel_to_max(mine.double(), ref), rel_to_max(t32.double(), ref)
        note(f'{tag} gradient of {what}: glued {err:.2e}  plain fp32 {yard:.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'gradient of {what}: {err:.2e} vs {yard:.2e}')
    assert not fails, '; '.join(fails)


def _feats(kw, b, seed, h=64, w=96):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(b, c, h//s, w//s, generator=g).cuda() for c, s in zip(kw['num_ch_enc'], kw['enc_sc'])], g


def _gouts(g, b, ch, scales): return {i: torch.randn(b, ch, 64, 96, generator=g).cuda() for i in scales}


def test_glued_path_equals_the_plain_path(F):
    """Two samples at 64 x 96 on the fixture's seeded parameters."""
    dec, *_ = build('cuda')
    feats, g = _feats(SUPERDEPTH_KW, 2, 271)
    _hold_paths('resnet18', _paths(dec, feats, _gouts(g, 2, 1, SUPERDEPTH_KW['out_sc'])))


def test_eval_mode_and_a_single_output_scale(F):
    """`out_sc=(0,)` in eval mode: one output, no gradient bookkeeping, the same numbers as the plain path under the rule; in training the one head's
    gradients reach every stage."""
    dec, *_ = build('cuda', out_sc=[0])
    assert len(dec.decoder) == 11
    feats, g = _feats(SUPERDEPTH_KW, 1, 272)
    dec.eval()
    with torch.no_grad():
        out = dec(feats)
        with dec.plain_path(): ref = dec(feats)
        ref64 = copy.deepcopy(dec).double()([f.double() for f in feats])
    assert sorted(out) == [0] and out[0].shape == (1, 1, 64, 96) and not out[0].requires_grad
    err, yard = (out[0].double() - ref64[0]).abs().max().item(), (ref[0].double() - ref64[0]).abs().max().item()
    note(f'eval out_sc=(0,): glued {err:.2e}  plain fp32 {yard:.2e}')
    assert err <= max(FLOOR, 4*yard)
    dec.train()
    _hold_paths('out_sc=(0,)', _paths(dec, feats, _gouts(g, 1, 1, [0])))


CONVNEXT_KW = dict(num_ch_enc=[96, 192, 384, 768], enc_sc=[4, 8, 16, 32], out_sc=[0, 1, 2, 3], out_ch=1, out_act='sigmoid')


def test_convnext_feature_list(F):
    """ConvNeXt-T's channels and strides: skips at stages 4, 3 and 2, none at stages 1 and 0."""
    from slowtv_monodepth_amd.networks.decoders import SuperdepthDecoder
    torch.manual_seed(5)
    dec = SuperdepthDecoder(**CONVNEXT_KW).cuda().train()
    with torch.no_grad():
        for m in dec.modules():      # the four rows of a sub-pixel group differ, the biases are not zero
            if getattr(m, 'groups', 1) > 1: m.weight.copy_(torch.randn_like(m.weight)/3); m.bias.copy_(0.2*torch.randn_like(m.bias))
    assert [dec._has_skip(i) for i in range(5)] == [False, False, True, True, True]
    feats, g = _feats(CONVNEXT_KW, 2, 273)
    _hold_paths('convnext_tiny', _paths(dec, feats, _gouts(g, 2, 1, range(4))))


def test_mask_decoder_with_two_channels(F):
    """The predictive-mask decoder of `DepthNet(dec_name='superdepth', mask_name='uncertainty', num_ch_mask=2)`: two-channel ReLU heads."""
    dec, *_ = build('cuda', out_ch=2, out_act='relu')
    feats, g = _feats(SUPERDEPTH_KW, 2, 274)
    res = _paths(dec, feats, _gouts(g, 2, 2, SUPERDEPTH_KW['out_sc']))
    assert all(o.shape == (2, 2, 64, 96) and (o >= 0).all() for o in res['glued'][0].values())
    _hold_paths('mask x2', res)


def test_glued_decoder_under_bf16_autocast_computes_in_fp32(F):
    dec, *_ = build('cuda')
    feats, _ = _feats(SUPERDEPTH_KW, 1, 275)
    F.set_conv_route('mfma')      # (one route for both calls: an A/B on first use may hand the two calls different kernels)
    try:
        with torch.no_grad():
            with torch.autocast('cuda', dtype=torch.bfloat16): out = dec([f.bfloat16() for f in feats])
            ref = dec([f.bfloat16().float() for f in feats])
    finally: F.set_conv_route('auto')
    for i in ref: assert out[i].dtype == torch.float32 and torch.equal(out[i], ref[i]), f'scale {i}'


# ------------------------------------------------------------------------------------------------- loss path and trainer
def test_loss_path_on_four_full_resolution_scales(F):
    """What this decoder hands the loss: a pyramid whose four scales are ALL 64 x 96.  Nothing else in the tree exercises equal-sized scales.
    FINDING: `loss_path_fused` declines such a pyramid (`Unsupported`: more than one full-resolution level), so the trainer takes the handlers for it — a
    static rule in `HipLossBackend.loss_path`, no tie-break seed drawn.  The operators it then runs (`image_recon_fused_disp` and `disp_smooth_fused`) are held
    here to the un-fused ones (`disp_to_depth` -> `view_synth` -> `photo_error` -> `recon_reduce`, plus the smoothness) at the fuzz test's tolerances; were
    the single-node operator to serve the pyramid one day, it is held to them as well."""
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd._lib import Unsupported
    from slowtv_monodepth_amd.losses.reconstruction import ReconstructionLoss
    b, h, w, n, S = 2, 64, 96, 2, 4
    gen = torch.Generator().manual_seed(77)
    imgs = torch.rand(b, 3, h, w, generator=gen).cuda()
    supp = 0.5*imgs[None] + 0.5*torch.rand(n, b, 3, h, w, generator=gen).cuda()
    d0 = [(0.05 + 0.9*torch.rand(b, 1, h, w, generator=gen)).cuda() for _ in range(S)]
    aa, t = 0.02*torch.randn(n*b, 3, generator=gen).cuda(), 0.1*torch.randn(n*b, 3, generator=gen).cuda()
    K = torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(b, 1, 1).cuda()
    Ts = F.pose_matrices(aa, t).unflatten(0, (n, b))
    # the mean over the supports and no automask, as the hostile-memory loss-path case: no routing decision that rounding could flip, no tie-break noise
    crit = ReconstructionLoss('ssim', use_min=False, use_automask=False)
    flags = F.recon_flags('ssim', False, False)
    w_sm = 0.1

    def unfused():
        d = [v.clone().requires_grad_(True) for v in d0]
        depth_up, _ = F.disp_to_depth(d, (h, w), 0.1, 100)
        l_rec, _ = handlers._image_recon_generic(crit, dict(enumerate(depth_up)), imgs, supp, Ts, K, None, None, False)
        l_sm, _, _ = F.disp_smooth_fused(dict(enumerate(d)), imgs, use_edges=True, want_aux=False)
        (l_rec + w_sm*l_sm).backward()
        return l_rec.detach(), l_sm.detach(), [v.grad for v in d]

    def fused_pair():
        d = [v.clone().requires_grad_(True) for v in d0]
        l_rec, _, sel, _, _ = F.image_recon_fused_disp(d, imgs, supp, Ts, K, flags=flags, min_depth=0.1, max_depth=100, want_err=False)
        l_sm, _, _ = F.disp_smooth_fused(dict(enumerate(d)), imgs, use_edges=True, want_aux=False)
        (l_rec + w_sm*l_sm).backward()
        return l_rec.detach(), l_sm.detach(), [v.grad for v in d]

    def single_node():
        d = [v.clone().requires_grad_(True) for v in d0]
        loss, l_rec, l_sm, sel, dep = F.loss_path_fused(dict(enumerate(d)), imgs, supp, Ts, K, flags=flags, min_depth=0.1, max_depth=100, w_recon=1.0, w_smooth=w_sm)
        loss.backward()
        return l_rec.detach(), l_sm.detach(), [v.grad for v in d]

    ref = unfused()
    runs = {'image_recon_fused_disp + disp_smooth_fused': fused_pair()}
    try: runs['loss_path_fused'] = single_node()
    except Unsupported as e: note(f'loss_path_fused on four 64x96 scales: declined ({e})')
    fails = []
    for name, (l_rec, l_sm, grads) in runs.items():
        e_rec, e_sm = abs(l_rec.item() - ref[0].item())/abs(ref[0].item()), abs(l_sm.item() - ref[1].item())/max(abs(ref[1].item()), 1e-20)
        worst = max(rel_to_max(gm, gr) for gm, gr in zip(grads, ref[2]))
        note(f'{name} on four 64x96 scales against the un-fused operators: l_rec {e_rec:.2e} l_smooth {e_sm:.2e} worst disparity gradient {worst:.2e}')
        if not e_rec <= 2e-3: fails.append(f'{name}: reconstruction loss {e_rec:.2e}')
        if not e_sm <= 2e-5: fails.append(f'{name}: smoothness {e_sm:.2e}')
        for s, (gm, gr) in enumerate(zip(grads, ref[2])):      # the fuzz test's rule: a few knife-edge elements (selection ties), bounded in number and size
            e = (gm - gr).abs()/gr.abs().max().clamp(min=1e-20)
            n_out = int((e > 2e-3).sum())
            if not (n_out <= max(3, int(2e-4*e.numel())) and e.max().item() < 5e-2): fails.append(f'{name}: d loss / d disp_{s}: {n_out} elements off by more than 2e-3, worst {e.max().item():.2e}')
    assert not fails, '; '.join(fails)
    if 'loss_path_fused' not in runs:      # the trainer's static rule: such a pyramid goes to the handlers, and no tie-break seed is drawn on the way
        from slowtv_monodepth_amd.regularizers.smooth import SmoothReg
        from slowtv_monodepth_amd.trainer import HipLossBackend
        backend, seed0 = HipLossBackend(), crit.noise_seed
        depths = handlers.LazyDepths(range(S), d0, (h, w), 0.1, 100)
        assert backend.loss_path(crit, SmoothReg(use_edges=True), depths, dict(enumerate(d0)), imgs, supp, Ts, K, None, 1.0, w_sm) is None and crit.noise_seed == seed0


def test_example_config_takes_two_optimizer_steps(F):
    """`cfg/kitti_superdepth.yaml` at 2 x 64 x 96 on a synthetic batch, two steps: a finite loss and a finite gradient in every decoder parameter."""
    from slowtv_monodepth_amd import parsers
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_superdepth.yaml').read_text())
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    opt = parsers.get_opt(m.nets, dict(cfg['optimizer']))
    dec = m.nets['depth'].decoders['disp']
    batch = make_batch(2, 64, 96, (-1, 1), seed=42, device='cuda')
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        loss, ld, fwd = m.step(batch)
        loss.backward()
        assert all(v.shape[-2:] == (64, 96) for v in fwd['disp'].values())
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for k_, v in ld.items() if k_.startswith('loss_')), f'step {step}'
        for k_, p in m.named_parameters(): assert p.grad is None or torch.isfinite(p.grad).all(), f'step {step}: {k_} has a non-finite gradient'
        for k_, p in dec.named_parameters(): assert p.grad is not None, f'step {step}: {k_} got no gradient'
        opt.step()
