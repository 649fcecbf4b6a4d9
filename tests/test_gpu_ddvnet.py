"""The DDVNet decoder on the GPU: `ddv_head` (csrc/smd_ddv.hip) against an fp64 restatement and the REFERENCE's fixture, the glued decoder against the
reference's `DDVNetDecoder` (tests/golden/net_decoder_ddvnet_64x96.npz) and against its own plain path, the example config through the trainer, and the
head in hostile memory."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as TF
import yaml

from conftest import ROOT, load_golden, parity_note, rel_to_max
from ddvnet_inputs import DDV_CASES, DDV_OVERFLOW, DDVNET_KW, NUM_BINS, ddv_case
from hostile_memory import Arena, assert_finite, hostile
from test_ddvnet_host import FLOOR, build, ddv_aten, run_and_compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def _run(fn, ins, gout, G, dtype=torch.float32):
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in ins]
    out = fn(*leaves, G)
    out.backward(gout.to(dtype))
    return out.detach(), [t.grad for t in leaves]


def _head_inputs(shape, G, mode, seed):
    """xp already padded (B,C,h+2,w+2); 'spread': logits of order 1, 'peaked': the weights x 40 (a few bins carry the softmax)."""
    B, C, h, w = shape
    g = torch.Generator().manual_seed(seed)
    xp = torch.randn(B, C, h + 2, w + 2, generator=g)
    weight = torch.randn(NUM_BINS*G, C, 3, 3, generator=g)/float(9*C)**0.5*(40.0 if mode == 'peaked' else 1.0)
    bias = 0.1*torch.randn(NUM_BINS*G, generator=g)
    return [xp.cuda(), weight.cuda(), bias.cuda()], torch.randn(B, G, h, w, generator=g).cuda()


# one and several K steps (C = 16 ... 128), heights and widths off the 4 x 64 tile, a tile wider than the image, several tiles and blocks, two groups
HEAD_SHAPES = [((1, 16, 2, 2), 1), ((2, 16, 5, 33), 1), ((1, 32, 7, 70), 1), ((3, 64, 3, 17), 1), ((1, 128, 4, 9), 1), ((1, 16, 6, 40), 2)]


@pytest.mark.parametrize('mode', ['spread', 'peaked'])
@pytest.mark.parametrize('shape,G', HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else f'g{s}')
def test_ddv_head_matches_fp64(F, shape, G, mode):
    """Output and the three gradients against the fp64 restatement.  The bound is the project's rule (test_gpu_cadepth.py): torch's own fp32 sequence
    (conv2d, softmax, multiply, sum) is compared with the same fp64 run, and the kernel gets the larger of 2e-6 of the tensor's maximum and 4 x that error.
    Two runs on the same inputs are bit-equal."""
    ins, gout = _head_inputs(shape, G, mode, seed=4000 + sum(shape) + G)
    o64, g64 = _run(ddv_aten, ins, gout, G, torch.float64)
    o32, g32 = _run(ddv_aten, ins, gout, G)
    F.set_conv_route('mfma')      # the routed gradient operators on the library's kernels wherever they serve the shape (as test_gpu_hostile_memory.py pins them): an
    try:                          # A/B on first use would hand a shape to MIOpen, whose weight gradient is not reproducible from run to run
        o, gr = _run(F.ddv_head, ins, gout, G)
        o2, gr2 = _run(F.ddv_head, ins, gout, G)
    finally: F.set_conv_route('auto')
    fails = []
    names = ('out', 'grad_xp', 'grad_w', 'grad_b')
    for what, mine, t32, ref in zip(names, [o] + gr, [o32] + g32, [o64] + g64):
        err, yard = rel_to_max(mine.double(), ref), rel_to_max(t32.double(), ref)
        parity_note(f'ddvnet_parity ddv_head {"x".join(map(str, shape)):>12} g{G} {mode:6} {what:7}: kernel {err:.2e}  torch fp32 {yard:.2e}  bound {max(FLOOR, 4*yard):.2e}')
        if not err <= max(FLOOR, 4*yard): fails.append(f'{what}: {err:.2e} vs torch fp32 {yard:.2e}')
    assert not fails, '; '.join(fails)
    differ = [n for n, a, b in zip(names, [o] + gr, [o2] + gr2) if not torch.equal(a, b)]
    assert not differ, f'two runs on the same inputs differ in {differ}'


def _fixture_case(F, g, k):
    x, weight, bias, gout = ddv_case(k)
    G = DDV_CASES[k][4]
    leaves = [t.cuda().requires_grad_(True) for t in (x, weight, bias)]
    out = F.ddv_head(TF.pad(leaves[0], (1, 1, 1, 1), mode='reflect'), leaves[1], leaves[2], G)
    out.backward(gout.cuda())
    res = {}
    for what, mine in zip(('out', 'grad_x', 'grad_w', 'grad_b'), [out.detach()] + [t.grad for t in leaves]):
        err, yard = rel_to_max(mine.cpu(), g[f'{what}_{k}']), float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])
        parity_note(f'ddvnet_parity ddv_head fixture[{k}] {what:6}: kernel vs reference {err:.2e}  reference fp32 vs fp64 {yard:.2e}')
        res[what] = (mine, err, yard)
    return res


@pytest.mark.parametrize('k', [k for k in range(len(DDV_CASES)) if k != DDV_OVERFLOW])
def test_ddv_head_matches_the_reference_fixture(F, k):
    """What the reference's conv3x3 + expected_disparity produced, at the same rule with the RECORDED fp32-vs-fp64 yardstick."""
    res = _fixture_case(F, load_golden('op_ddv_head'), k)
    for what, (_, err, yard) in res.items(): assert err <= max(FLOOR, 4*yard), f'case {k} {what}: {err:.2e}'


def test_ddv_head_does_not_overflow_where_an_unshifted_exp_would(F):
    """The fixture's case whose logits span more than 88 (exp of an unshifted row overflows fp32): finite, equal to the reference within the rule, and equal
    to fp64 within the rule measured on the same tensors."""
    g = load_golden('op_ddv_head')
    assert float(g[f'meta_logit_span_{DDV_OVERFLOW}']) > 88
    res = _fixture_case(F, g, DDV_OVERFLOW)
    for what, (mine, err, yard) in res.items():
        assert torch.isfinite(mine).all(), what
        assert err <= max(FLOOR, 4*yard), f'{what}: {err:.2e}'
    x, weight, bias, gout = ddv_case(DDV_OVERFLOW)
    G = DDV_CASES[DDV_OVERFLOW][4]
    ins = [TF.pad(x, (1, 1, 1, 1), mode='reflect').cuda(), weight.cuda(), bias.cuda()]
    o64, g64 = _run(ddv_aten, ins, gout.cuda(), G, torch.float64)
    o32, g32 = _run(ddv_aten, ins, gout.cuda(), G)
    o, gr = _run(F.ddv_head, ins, gout.cuda(), G)
    for what, mine, t32, ref in zip(('out', 'grad_xp', 'grad_w', 'grad_b'), [o] + gr, [o32] + g32, [o64] + g64):
        assert rel_to_max(mine.double(), ref) <= max(FLOOR, 4*rel_to_max(t32.double(), ref)), what


def test_ddv_head_refuses_wrong_operands_on_the_gpu(F):
    xp, w, b = torch.rand(2, 16, 6, 7).cuda(), torch.rand(NUM_BINS, 16, 3, 3).cuda(), torch.rand(NUM_BINS).cuda()
    with pytest.raises(TypeError): F.ddv_head(xp.double(), w, b)
    with pytest.raises(TypeError): F.ddv_head(xp, w, None)
    with pytest.raises(RuntimeError, match='GPU'): F.ddv_head(xp, w.cpu(), b)
    with pytest.raises(ValueError): F.ddv_head(xp, w[:, :8], b)
    only_x = [xp.clone().requires_grad_(True), w, b]                   # a gradient for the input alone, from the expanded gradient of a sum: its value is that of
    F.set_conv_route('mfma')                                           # the full backward (route pinned as in test_ddv_head_matches_fp64; every subset: test_gpu_grad_subsets.py)
    try:
        F.ddv_head(*only_x).sum().backward()
        every = [t.clone().requires_grad_(True) for t in (xp, w, b)]
        F.ddv_head(*every).backward(torch.ones(2, 1, 4, 5, device='cuda'))
    finally: F.set_conv_route('auto')
    assert only_x[0].grad is not None and torch.isfinite(only_x[0].grad).all() and torch.equal(only_x[0].grad, every[0].grad)


# ------------------------------------------------------------------------------------------------- decoder
@pytest.mark.parametrize('route', ['mfma', 'auto'])
def test_glued_decoder_matches_the_reference_decoder(F, route):
    """As test_gpu_cadepth.py::test_glued_decoder_matches_the_reference_decoder, at its bounds (2e-5 on the disparities, 2e-4 of the maximum on the
    gradients): the fixture's recorded fp32-vs-fp64 error of the reference itself is below a quarter of either."""
    g = load_golden('net_decoder_ddvnet_64x96')
    assert g['meta_ref_fp32_vs_fp64_out'] <= 2e-5/4 and g['meta_ref_fp32_vs_fp64_grad'] <= 2e-4/4
    F.set_conv_route(route)
    try: dec, out, _ = run_and_compare('cuda', 2e-5, 2e-4)
    finally: F.set_conv_route('auto')
    assert all(o.is_cuda for o in out.values()) and dec.logits == {}          # the glued path keeps no logits


def _two_paths(dec, feats, gouts):
    state, res = copy.deepcopy(dec.state_dict()), {}
    for glued in (True, False):
        dec.load_state_dict(state); dec.zero_grad(set_to_none=True)
        leaves = [f.detach().clone().requires_grad_(True) for f in feats]
        with contextlib.nullcontext() if glued else dec.plain_path(): out = dec(leaves)
        sum((out[i]*gouts[i]).sum() for i in out).backward()
        res[glued] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in leaves], {k: p.grad for k, p in dec.named_parameters()}, sorted(dec.logits))
    return res


@pytest.mark.parametrize('out_ch', [1, 2])
def test_glued_path_equals_the_plain_path(F, out_ch):
    """Two samples at 64 x 96, one and two output channels: outputs (2e-5), feature and parameter gradients (2e-4 of the maximum); `logits` filled by the
    plain path only."""
    dec, *_ = build('cuda', out_ch=out_ch)
    g = torch.Generator().manual_seed(71 + out_ch)
    feats = [torch.randn(2, c, 64//s, 96//s, generator=g).cuda() for c, s in zip(DDVNET_KW['num_ch_enc'], DDVNET_KW['enc_sc'])]
    gouts = {i: torch.randn(2, out_ch, 64 >> i, 96 >> i, generator=g).cuda() for i in DDVNET_KW['out_sc']}
    (o1, gf1, gp1, l1), (o0, gf0, gp0, l0) = (r := _two_paths(dec, feats, gouts))[True], r[False]
    assert l1 == [] and l0 == [0, 1, 2, 3] and o1[0].shape == (2, out_ch, 64, 96)
    for i in o0: assert (o1[i] - o0[i]).abs().max().item() <= 2e-5, f'output at scale {i}'
    for j, (a, b) in enumerate(zip(gf1, gf0)): assert rel_to_max(a, b) <= 2e-4, f'gradient w.r.t. feature {j}: {rel_to_max(a, b):.2e}'
    for k, b in gp0.items():
        if k == 'bins': assert b is None and gp1[k] is None
        else: assert rel_to_max(gp1[k], b) <= 2e-4, f'gradient of {k}: {rel_to_max(gp1[k], b):.2e}'


def test_glued_decoder_under_bf16_autocast_computes_in_fp32(F):
    """Under bf16 autocast the decoder returns fp32 disparities that are the fp32 run on the same (bf16-valued) features, to the 2e-5 the glued path is held to
    against the plain one (the convolutions' routes may differ between the two calls)."""
    dec, *_ = build('cuda')
    g = torch.Generator().manual_seed(73)
    feats = [torch.randn(1, c, 64//s, 96//s, generator=g).cuda() for c, s in zip(DDVNET_KW['num_ch_enc'], DDVNET_KW['enc_sc'])]
    with torch.no_grad():
        ref = dec(feats)
        with torch.autocast('cuda', dtype=torch.bfloat16): out = dec([f.bfloat16() for f in feats])
        ref_b = dec([f.bfloat16().float() for f in feats])
    for i in ref: assert out[i].dtype == torch.float32 and (out[i] - ref_b[i]).abs().max().item() <= 2e-5, f'scale {i}: {(out[i] - ref_b[i]).abs().max().item():.2e}'


# ------------------------------------------------------------------------------------------------- trainer
def test_example_config_takes_an_optimizer_step(F):
    """`cfg/kitti_ddvnet.yaml` at 2 x 64 x 96 on a synthetic batch: a finite loss and a finite gradient in every decoder parameter except `bins`."""
    from slowtv_monodepth_amd import parsers
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_ddvnet.yaml').read_text())
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    opt = parsers.get_opt(m.nets, dict(cfg['optimizer']))
    dec = m.nets['depth'].decoders['disp']
    batch = make_batch(2, 64, 96, (-1, 1), seed=42, device='cuda')
    opt.zero_grad(set_to_none=True)
    loss, ld, fwd = m.step(batch)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(v).all() for k_, v in ld.items() if k_.startswith('loss_'))
    for k_, p in dec.named_parameters():
        if k_ == 'bins': assert p.grad is None
        else: assert p.grad is not None and torch.isfinite(p.grad).all(), f'{k_} got no (finite) gradient'
    opt.step()
    assert torch.equal(dec.bins.detach().cpu().flatten(), torch.arange(NUM_BINS)/NUM_BINS)


# ------------------------------------------------------------------------------------------------- hostile memory
@pytest.mark.parametrize('shift', [0, 1])
def test_ddv_head_in_hostile_memory(F, shift):
    """`ddv_head` at (2,16,5,33) on operands in guarded, poisoned, `shift`-element-offset blocks with every buffer it allocates served from the arena,
    forward and backward: guards intact, results finite and bit-equal to the run in plain memory."""
    ins, gout = _head_inputs((2, 16, 5, 33), 1, 'peaked', seed=81)
    plain = [t.detach().clone().requires_grad_(True) for t in ins]
    arena = Arena()
    F.set_conv_route('mfma')      # (as test_gpu_hostile_memory.py pins the routed operators)
    try:
        out_p = F.ddv_head(*plain)
        out_p.backward(gout)
        with hostile(arena):
            leaves = [arena.guarded(t, shift).requires_grad_(True) for t in ins]
            go = arena.guarded(gout, shift)
            out = F.ddv_head(*leaves)
            out.backward(go)
            served = sum(1 for b in arena.blocks if b[4] == torch.uint8)
    finally: F.set_conv_route('auto')
    assert_finite(out.detach(), 'output')
    for k, t in enumerate(leaves): assert_finite(t.grad, f'gradient of operand {k}')
    differ = [n for n, a, b in zip(('out', 'grad_xp', 'grad_w', 'grad_b'), [out.detach()] + [t.grad for t in leaves], [out_p.detach()] + [t.grad for t in plain]) if not torch.equal(a, b)]
    assert not differ, f'differs from the run in plain memory in {differ}'
    assert served >= 2, f'{served} workspaces came from the arena: the packed weights and the backward\'s workspace at least'
    arena.check()
