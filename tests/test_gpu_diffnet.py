"""The DiffNet decoder on the GPU: `up_cat_gate_pad` and `relu_pad` (csrc/smd_decoder.hip) against an fp64 restatement and the REFERENCE's fixture, the
glued decoder against the reference's `DiffNetDecoder` (tests/golden/net_decoder_diffnet_64x96.npz) and against its own plain path, a ConvNeXt feature list,
the mask decoder, the example config through the trainer, both operators in hostile memory, and their refusals."""
import copy

import pytest
import torch
import yaml

from conftest import ROOT, load_golden, parity_note, rel_to_max
from diffnet_inputs import DIFFNET_KW, FUSE_CASES, fuse_case
from hostile_memory import Arena, assert_finite, hostile
from test_ddvnet_host import FLOOR
from test_diffnet_host import build, fuse_aten, relu_pad_aten, run_and_compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def _run(fn, ins, gout, act, dtype=torch.float32, need=None):
    """-> (out, [gradient or None per operand]); `need`: which operands ask for a gradient (default: every tensor operand)."""
    leaves = [None if t is None else t.detach().to(dtype).clone().requires_grad_(need is None or k in need) for k, t in enumerate(ins)]
    out = fn(*leaves, act) if act != 'pad' else fn(*leaves)
    out.backward(gout.to(dtype))
    return out.detach(), [None if t is None else t.grad for t in leaves]


def _fuse_inputs(shape, bias, saturated, seed):
    """Operands in `fuse_aten`'s order (a, bias, skip, w1, w2) and the output's gradient; every channel has a mean of its own, so the gates differ;
    'saturated': the Linear weights x 40, which drives gates to 0 and 1."""
    B, Ca, Cs, h, w, R = shape
    C = Ca + Cs
    g = torch.Generator().manual_seed(seed)
    scale = 40.0 if saturated else 1.0
    a = torch.randn(B, Ca, h, w, generator=g) + torch.randn(1, Ca, 1, 1, generator=g)
    b = 0.5*torch.randn(Ca, generator=g)
    skip = torch.randn(B, Cs, 2*h, 2*w, generator=g) + torch.randn(1, Cs, 1, 1, generator=g)
    w1 = torch.randn(R, C, generator=g)*(scale/float(C)**0.5)
    w2 = torch.randn(C, R, generator=g)*(scale/float(R)**0.5)
    ins = [a.cuda(), b.cuda() if bias else None, skip.cuda(), w1.cuda(), w2.cuda()]
    return ins, torch.randn(B, C, 2*h + 2, 2*w + 2, generator=g).cuda()


def _kernel(F):
    return lambda a, b, skip, w1, w2, act: F.up_cat_gate_pad(a, skip, w1, w2, b, act)


NAMES = ('out', 'grad_a', 'grad_bias', 'grad_skip', 'grad_w1', 'grad_w2')
# (B, Ca, Cs, h, w, R): one source pixel (every padded cell a mirror), odd sizes, channels off any tile and a width off the block, several samples,
# ResNet-18's deepest channel count on a tiny plane, several chunks per plane
FUSE_SHAPES = [(1, 8, 8, 1, 1, 1), (2, 16, 8, 3, 5, 1), (1, 40, 24, 2, 33, 4), (3, 32, 32, 7, 9, 4), (1, 512, 256, 2, 3, 48), (2, 16, 16, 33, 70, 2)]


def _hold(tag, names, mine, t32, ref):
    """The project's rule: relative to the tensor's maximum, at most the larger of FLOOR and 4 x the error of torch's own fp32 sequence against fp64."""
    fails = []
    for what, m, t, r in zip(names, mine, t32, ref):
        if r is None: continue
        assert torch.isfinite(m).all(), f'{what} is not finite'
        err, yard = rel_to_max(m.double(), r), rel_to_max(t.double(), r)
        parity_note(f'diffnet_parity {tag} {what:9}: kernel {err:.2e}  torch fp32 {yard:.2e}  bound {max(FLOOR, 4*yard):.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'{what}: {err:.2e} vs torch fp32 {yard:.2e}')
    assert not fails, '; '.join(fails)


@pytest.mark.parametrize('saturated', [False, True], ids=['spread', 'saturated'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('act', [None, 'relu'], ids=['none', 'relu'])
@pytest.mark.parametrize('shape', FUSE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_up_cat_gate_pad_matches_fp64(F, shape, act, bias, saturated):
    """Output and every gradient against the fp64 restatement, everything finite, two runs bit-equal.  (Where a saturated case drives EVERY gate to exactly 0 or
    1 in fp32 the weight gradients are 0 in fp32 and denormal-small in fp64: the relative figure is then 1 for torch's sequence and for the kernel alike.)"""
    ins, gout = _fuse_inputs(shape, bias, saturated, seed=5000 + sum(shape))
    o64, g64 = _run(fuse_aten, ins, gout, act, torch.float64)
    o32, g32 = _run(fuse_aten, ins, gout, act)
    o, gr = _run(_kernel(F), ins, gout, act)
    o2, gr2 = _run(_kernel(F), ins, gout, act)
    _hold(f'up_cat_gate_pad {"x".join(map(str, shape)):>18} {act or "none":4} {"bias" if bias else "nobias":6} {"sat" if saturated else "spread":6}', NAMES, [o] + gr, [o32] + g32, [o64] + g64)
    differ = [n for n, x, y in zip(NAMES, [o] + gr, [o2] + gr2) if x is not None and not torch.equal(x, y)]
    assert not differ, f'two runs on the same inputs differ in {differ}'


@pytest.mark.parametrize('shape', [(2, 16, 8, 3, 5, 1), (2, 16, 16, 33, 70, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_each_gradient_subset_alone_equals_the_full_backward(F, shape):
    """`a` only, `skip` only, the weights only (and the bias only): bit-equal to what the full backward returns for them, nothing for the others."""
    ins, gout = _fuse_inputs(shape, True, False, seed=5100 + sum(shape))
    _, full = _run(_kernel(F), ins, gout, 'relu')
    for need in ({0}, {2}, {3, 4}, {1}, {3}):
        _, part = _run(_kernel(F), ins, gout, 'relu', need=need)
        for k, (p, f) in enumerate(zip(part, full)):
            if k in need: assert p is not None and torch.equal(p, f), f'operand {k} asked for alone (subset {sorted(need)})'
            else: assert p is None, f'operand {k} got a gradient nobody asked for (subset {sorted(need)})'


@pytest.mark.parametrize('shape', [(2, 3, 2, 4, 5, 1), (1, 2, 1, 33, 35, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_gated_and_monodepth_glue_share_one_index_map(F, shape):
    """With w2 = 0 the gate is exactly 0.5 and its dmean exactly 0; with a > 0 and no bias ELU is the identity with derivative 1.  Then `up_cat_gate_pad` is
    bit for bit half of `elu_up_cat_pad`: the output, g_skip everywhere, and g_a on the interior pixels 1..h-2, 1..w-2 (on a border pixel the Monodepth
    kernel runs one accumulator through the four children and the gated kernel pairs them: two legitimate sum orders).  A scaling by 0.5 is exact, so any
    difference is a different source index, pad-adjoint cell or sum order."""
    B, Ca, Cs, h, w, R = shape
    C = Ca + Cs
    g = torch.Generator().manual_seed(5150 + sum(shape))
    a = (0.25 + torch.rand(B, Ca, h, w, generator=g)).cuda()
    skip = torch.randn(B, Cs, 2*h, 2*w, generator=g).cuda()
    w1, w2 = torch.randn(R, C, generator=g).cuda(), torch.zeros(C, R).cuda()
    gout = torch.randn(B, C, 2*h + 2, 2*w + 2, generator=g).cuda()
    res = {}
    for name in ('gated', 'monodepth'):
        la, ls = a.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        out = F.up_cat_gate_pad(la, ls, w1, w2, None, None) if name == 'gated' else F.elu_up_cat_pad(la, ls)
        out.backward(gout)
        res[name] = (out.detach(), ls.grad, la.grad)
    (o, gs, ga), (om, gsm, gam) = res['gated'], res['monodepth']
    assert torch.equal(o, 0.5*om), 'output'
    assert torch.equal(gs, 0.5*gsm), 'g_skip'
    assert torch.equal(ga[:, :, 1:h - 1, 1:w - 1], 0.5*gam[:, :, 1:h - 1, 1:w - 1]), 'g_a on the interior'
    assert torch.isfinite(ga).all() and ga.shape == gam.shape


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 16, 5, 33), (1, 3, 7, 70)], ids=lambda s: 'x'.join(map(str, s)))
def test_relu_pad_matches_fp64(F, shape, bias):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(5200 + sum(shape))
    ins = [torch.randn(B, C, h, w, generator=g).cuda(), 0.5*torch.randn(C, generator=g).cuda() if bias else None]
    gout = torch.randn(B, C, h + 2, w + 2, generator=g).cuda()
    o64, g64 = _run(relu_pad_aten, ins, gout, 'pad', torch.float64)
    o32, g32 = _run(relu_pad_aten, ins, gout, 'pad')
    o, gr = _run(F.relu_pad, ins, gout, 'pad')
    o2, gr2 = _run(F.relu_pad, ins, gout, 'pad')
    names = ('out', 'grad_x', 'grad_bias')
    _hold(f'relu_pad {"x".join(map(str, shape)):>10} {"bias" if bias else "nobias":6}', names, [o] + gr, [o32] + g32, [o64] + g64)
    assert torch.equal(o, o32), 'relu and a copy: the output is exact'
    differ = [n for n, x, y in zip(names, [o] + gr, [o2] + gr2) if x is not None and not torch.equal(x, y)]
    assert not differ, f'two runs on the same inputs differ in {differ}'


@pytest.mark.parametrize('k', range(len(FUSE_CASES)))
def test_both_operators_match_the_reference_fixture(F, k):
    """What the reference's AttentionBlock (its convolution replaced by that convolution's padding) produced, in both modes, and the ReLU + pad of its
    tail: the rule with the RECORDED fp32-vs-fp64 yardsticks."""
    g = load_golden('op_diffnet_fuse')
    a, bias, skip, w1, w2, gout = (t.cuda() for t in fuse_case(k))
    fails = []
    for mode in ('none', 'relu'):
        ins = [a, bias if mode == 'relu' else None, skip, w1, w2]
        o, gr = _run(_kernel(F), ins, gout, 'relu' if mode == 'relu' else None)
        for what, mine in zip(NAMES, [o] + gr):
            if mine is None: continue
            err, yard = rel_to_max(mine.cpu(), g[f'{what}_{mode}_{k}']), float(g[f'meta_ref_fp32_vs_fp64_{what}_{mode}_{k}'])
            parity_note(f'diffnet_parity up_cat_gate_pad fixture[{k}] {mode:4} {what:9}: kernel vs reference {err:.2e}  reference fp32 vs fp64 {yard:.2e}')
            assert torch.isfinite(mine).all()
            if not err <= max(FLOOR, 4*yard): fails.append(f'{mode} {what}: {err:.2e}')
    Ca, h, w = a.shape[1:]
    o, gr = _run(F.relu_pad, [a, bias], gout[:, :Ca, :h + 2, :w + 2].contiguous(), 'pad')
    for what, mine in zip(('pad_out', 'pad_grad_x', 'pad_grad_bias'), [o] + gr):
        err, yard = rel_to_max(mine.cpu(), g[f'{what}_{k}']), float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])
        parity_note(f'diffnet_parity relu_pad fixture[{k}] {what:13}: kernel vs reference {err:.2e}  reference fp32 vs fp64 {yard:.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'{what}: {err:.2e}')
    assert not fails, f'case {k}: ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------- decoder
def test_glued_decoder_matches_the_reference_decoder(F):
    """Outputs, feature gradients and parameter gradients against the reference's, at the rule with the fixture's recorded yardsticks."""
    g = load_golden('net_decoder_diffnet_64x96')
    dec, out, _ = run_and_compare('cuda', max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_out'])), max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_grad'])))
    assert all(o.is_cuda for o in out.values())


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
        parity_note(f'diffnet_parity {tag} output {i}: glued {err:.2e}  plain fp32 {yard:.2e}')
        assert o1[i].dtype == torch.float32 and torch.isfinite(o1[i]).all()
        if not err <= max(FLOOR, 4*yard): fails.append(f'output {i}: {err:.2e} vs {yard:.2e}')
    for what, mine, t32, ref in [(f'feature {j}', a, b, c) for j, (a, b, c) in enumerate(zip(f1, f0, f64))] + [(k, p1[k], p0[k], p64[k]) for k in sorted(p64)]:
        err, yard = rel_to_max(mine.double(), ref), rel_to_max(t32.double(), ref)
        parity_note(f'diffnet_parity {tag} gradient of {what}: glued {err:.2e}  plain fp32 {yard:.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'gradient of {what}: {err:.2e} vs {yard:.2e}')
    assert not fails, '; '.join(fails)


def _feats(kw, b, seed, h=64, w=96):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(b, c, h//s, w//s, generator=g).cuda() for c, s in zip(kw['num_ch_enc'], kw['enc_sc'])], g


def test_glued_path_equals_the_plain_path(F):
    """Two samples at 64 x 96 on the fixture's seeded parameters."""
    dec, *_ = build('cuda')
    feats, g = _feats(DIFFNET_KW, 2, 171)
    gouts = {i: torch.randn(2, 1, 64 >> i, 96 >> i, generator=g).cuda() for i in DIFFNET_KW['out_sc']}
    _hold_paths('resnet18', _paths(dec, feats, gouts))


def test_eval_mode_and_a_single_output_scale(F):
    """`out_sc=(0,)` in eval mode: one output, no gradient bookkeeping, the same numbers as the plain path under the rule; the heads of the other scales exist
    (the reference builds all four) and get no gradient in training."""
    dec, *_ = build('cuda', out_sc=[0])
    feats, g = _feats(DIFFNET_KW, 1, 172)
    dec.eval()
    with torch.no_grad():
        out = dec(feats)
        with dec.plain_path(): ref = dec(feats)
        ref64 = copy.deepcopy(dec).double()([f.double() for f in feats])
    assert sorted(out) == [0] and out[0].shape == (1, 1, 64, 96) and not out[0].requires_grad
    err, yard = (out[0].double() - ref64[0]).abs().max().item(), (ref[0].double() - ref64[0]).abs().max().item()
    parity_note(f'diffnet_parity eval out_sc=(0,): glued {err:.2e}  plain fp32 {yard:.2e}')
    assert err <= max(FLOOR, 4*yard)
    dec.train()
    res = _paths(dec, feats, {0: torch.randn(1, 1, 64, 96, generator=g).cuda()})
    assert not any(k.startswith(('convs.outconv_1', 'convs.outconv_2', 'convs.outconv_3')) for k in res['glued'][2])
    _hold_paths('out_sc=(0,)', res)


CONVNEXT_KW = dict(num_ch_enc=[96, 192, 384, 768], enc_sc=[4, 8, 16, 32], out_sc=[0, 1, 2, 3], out_ch=1, out_act='sigmoid')


def test_convnext_feature_list(F):
    """ConvNeXt-T's channels and strides: three attention stages (1152, 448 and 224 channels) and two `upsample_block` stages behind them."""
    from slowtv_monodepth_amd.networks.decoders import AttentionBlock, DiffNetDecoder
    torch.manual_seed(5)
    dec = DiffNetDecoder(**CONVNEXT_KW).cuda().train()
    assert [isinstance(dec.convs[f'upconv_{i}'], AttentionBlock) for i in range(5)] == [False, False, True, True, True]
    feats, g = _feats(CONVNEXT_KW, 2, 173)
    gouts = {i: torch.randn(2, 1, 64 >> i, 96 >> i, generator=g).cuda() for i in range(4)}
    _hold_paths('convnext_tiny', _paths(dec, feats, gouts))


def test_mask_decoder_with_two_channels(F):
    """The predictive-mask decoder of `DepthNet(dec_name='diffnet', mask_name='uncertainty', num_ch_mask=2)`: two-channel ReLU heads."""
    dec, *_ = build('cuda', out_ch=2, out_act='relu')
    feats, g = _feats(DIFFNET_KW, 2, 174)
    gouts = {i: torch.randn(2, 2, 64 >> i, 96 >> i, generator=g).cuda() for i in DIFFNET_KW['out_sc']}
    res = _paths(dec, feats, gouts)
    assert res['glued'][0][0].shape == (2, 2, 64, 96) and (res['glued'][0][0] >= 0).all()
    _hold_paths('mask x2', res)


def test_glued_decoder_under_bf16_autocast_computes_in_fp32(F):
    dec, *_ = build('cuda')
    feats, _ = _feats(DIFFNET_KW, 1, 175)
    F.set_conv_route('mfma')      # (one route for both calls: an A/B on first use may hand the two calls different kernels)
    try:
        with torch.no_grad():
            with torch.autocast('cuda', dtype=torch.bfloat16): out = dec([f.bfloat16() for f in feats])
            ref = dec([f.bfloat16().float() for f in feats])
    finally: F.set_conv_route('auto')
    for i in ref: assert out[i].dtype == torch.float32 and torch.equal(out[i], ref[i]), f'scale {i}'


# ------------------------------------------------------------------------------------------------- trainer
def test_example_config_takes_two_optimizer_steps(F):
    """`cfg/kitti_diffnet.yaml` at 2 x 64 x 96 on a synthetic batch, two steps: a finite loss and a finite gradient in every decoder parameter."""
    from slowtv_monodepth_amd import parsers
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_diffnet.yaml').read_text())
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    opt = parsers.get_opt(m.nets, dict(cfg['optimizer']))
    dec = m.nets['depth'].decoders['disp']
    batch = make_batch(2, 64, 96, (-1, 1), seed=42, device='cuda')
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        loss, ld, fwd = m.step(batch)
        loss.backward()
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for k_, v in ld.items() if k_.startswith('loss_')), f'step {step}'
        for k_, p in m.named_parameters(): assert p.grad is None or torch.isfinite(p.grad).all(), f'step {step}: {k_} has a non-finite gradient'
        for k_, p in dec.named_parameters(): assert p.grad is not None, f'step {step}: {k_} got no gradient'
        opt.step()


# ------------------------------------------------------------------------------------------------- hostile memory
@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('shape', [(2, 16, 8, 3, 5, 1), (2, 16, 16, 33, 70, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_both_operators_in_hostile_memory(F, shape, shift):
    """Both operators on operands in guarded, poisoned, `shift`-element-offset blocks with every buffer they allocate served from the arena, forward and
    backward: guards intact, results finite and bit-equal to the run in plain memory."""
    ins, gout = _fuse_inputs(shape, True, False, seed=5300 + sum(shape))
    B, Ca, Cs, h, w, R = shape
    gpad = gout[:, :Ca, :h + 2, :w + 2].contiguous()
    o_p, g_p = _run(_kernel(F), ins, gout, 'relu')
    r_p, rg_p = _run(F.relu_pad, ins[:2], gpad, 'pad')
    arena = Arena()
    with hostile(arena):
        leaves = [arena.guarded(t, shift).requires_grad_(True) for t in ins]
        out = _kernel(F)(*leaves, 'relu')
        out.backward(arena.guarded(gout, shift))
        pl = [arena.guarded(t, shift).requires_grad_(True) for t in ins[:2]]
        pout = F.relu_pad(*pl)
        pout.backward(arena.guarded(gpad, shift))
        served = sum(1 for b in arena.blocks if b[4] == torch.uint8)
    for what, t in zip(NAMES + ('pad_out', 'pad_grad_x', 'pad_grad_bias'), [out.detach()] + [t.grad for t in leaves] + [pout.detach()] + [t.grad for t in pl]): assert_finite(t, what)
    differ = [n for n, x, y in zip(NAMES, [out.detach()] + [t.grad for t in leaves], [o_p] + g_p) if not torch.equal(x, y)]
    differ += [n for n, x, y in zip(('pad_out', 'pad_grad_x', 'pad_grad_bias'), [pout.detach()] + [t.grad for t in pl], [r_p] + rg_p) if not torch.equal(x, y)]
    assert not differ, f'differs from the run in plain memory in {differ}'
    assert served >= 3, f'{served} workspaces came from the arena: both directions of up_cat_gate_pad and relu_pad\'s backward at least'
    arena.check()


# ------------------------------------------------------------------------------------------------- refusals
def test_operators_refuse_wrong_operands_on_the_gpu(F):
    ins, _ = _fuse_inputs((2, 16, 8, 3, 5, 1), True, False, seed=5400)
    a, b, skip, w1, w2 = ins
    with pytest.raises(TypeError): F.up_cat_gate_pad(a.double(), skip, w1, w2)
    with pytest.raises(TypeError): F.up_cat_gate_pad(a, skip.double(), w1, w2)
    with pytest.raises(TypeError): F.up_cat_gate_pad(a, skip, w1.double(), w2.double())
    with pytest.raises(TypeError): F.relu_pad(a.double())
    with pytest.raises(RuntimeError, match='GPU'): F.up_cat_gate_pad(a, skip, w1.cpu(), w2)
    with pytest.raises(RuntimeError, match='GPU'): F.relu_pad(a, b.cpu())
    with pytest.raises(ValueError): F.up_cat_gate_pad(a, skip[:, :, :, :9], w1, w2)          # not (B,Cs,2h,2w)
    with pytest.raises(ValueError): F.up_cat_gate_pad(a, skip.transpose(2, 3), w1, w2)
    with pytest.raises(ValueError): F.up_cat_gate_pad(a, skip, w1[:, :23], w2)                # w1's C is wrong
    with pytest.raises(ValueError): F.up_cat_gate_pad(a, skip, w1, w2, b[:7])
    with pytest.raises(ValueError): F.relu_pad(a, b[:7])
    with pytest.raises(ValueError): F.relu_pad(a[:, :, :1])                                   # a one-row plane has no reflection
    out = F.up_cat_gate_pad(a, skip, w1, w2, b, 'relu')                                       # and what is right still runs
    assert out.shape == (2, 24, 8, 12) and torch.isfinite(out).all()
