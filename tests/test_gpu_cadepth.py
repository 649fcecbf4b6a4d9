"""The CADepth decoder on the GPU: `channel_attention` and `se_gate` (csrc/smd_attention.hip) against fp64 restatements, the glued decoder against the
REFERENCE's `CaDepthDecoder` (tests/golden/net_decoder_cadepth_64x96.npz) and against its own plain path, the example config through the trainer, and both
operators in hostile memory."""
import contextlib
import copy

import pytest
import torch
import yaml

from cadepth_inputs import CADEPTH_KW, gfeat_sample, sp_inputs, sp_out_grads
from conftest import ROOT, load_golden, parity_note, rel_to_max
from hostile_memory import Arena, assert_finite, hostile
from test_cadepth_host import ABSORBED, build, run_and_compare, se_aten, sp_aten

pytestmark = pytest.mark.gpu

FLOOR = 2e-6      # the library's bound for its fp32 operators, relative to the tensor's maximum


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


def _grad_of(fn, x, gout):
    leaf = x.detach().clone().requires_grad_(True)
    out = fn(leaf)
    out.backward(gout.to(out.dtype))
    return out.detach(), leaf.grad


def _sp_input(shape, mode, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x = x/float(shape[2]*shape[3])**0.5 if mode == 'spread' else torch.relu(x) + 0.25*torch.rand(shape, generator=g)
    return x.cuda(), torch.randn(shape, generator=g).cuda()


SP_SHAPES = [(1, 7, 1, 1), (2, 24, 3, 5), (3, 33, 2, 3), (1, 96, 12, 20), (1, 512, 6, 20), (1, 1100, 2, 3)]


@pytest.mark.parametrize('mode', ['spread', 'peaked'])
@pytest.mark.parametrize('shape', SP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_channel_attention_matches_fp64(F, shape, mode):
    """Output and input gradient against the fp64 restatement.  The bound is measured, not fixed: torch's own fp32 sequence (two bmm, max, subtraction,
    softmax, add) is compared with the same fp64 run, and the kernel gets the larger of 2e-6 of the tensor's maximum and 4 x that error (the factor allows
    for another summation order, nothing more)."""
    x, gout = _sp_input(shape, mode, seed=1000 + sum(shape))
    o64, g64 = _grad_of(sp_aten, x.double(), gout)
    o32, g32 = _grad_of(sp_aten, x, gout)
    o, g = _grad_of(F.channel_attention, x, gout)
    for what, mine, t32, ref in (('out', o, o32, o64), ('grad', g, g32, g64)):
        err, yard = rel_to_max(mine.double(), ref), rel_to_max(t32.double(), ref)
        parity_note(f'cadepth_parity channel_attention {"x".join(map(str, shape)):>12} {mode:6} {what:4}: kernel {err:.2e}  torch fp32 {yard:.2e}  bound {max(FLOOR, 4*yard):.2e}')
        assert err <= max(FLOOR, 4*yard), f'{what}: {err:.2e} vs torch fp32 {yard:.2e}'


def test_channel_attention_matches_the_reference_fixture(F):
    """The fixture's inputs against what the reference's `StructurePerception` produced, at the same rule with the RECORDED fp32-vs-fp64 yardstick."""
    g = load_golden('op_structure_perception')
    for k, (x, go) in enumerate(zip(sp_inputs(), sp_out_grads())):
        o, gx = _grad_of(F.channel_attention, x.cuda(), go.cuda())
        for what, mine, key in (('out', o, f'out_{k}'), ('grad', gx, f'grad_x_{k}')):
            err, yard = rel_to_max(mine.cpu(), g[key]), float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])
            parity_note(f'cadepth_parity channel_attention fixture[{k}] {what:4}: kernel vs reference {err:.2e}  reference fp32 vs fp64 {yard:.2e}')
            assert err <= max(FLOOR, 4*yard), f'input {k} {what}: {err:.2e}'


def test_channel_attention_is_invariant_to_the_row_shift_and_stable(F):
    """softmax(rowmax - A) = softmax(c_i - A) for any per-row constant: rows of very different scale (row maxima of A more than 80 apart, where exp of an
    unshifted row would overflow fp32) stay finite and match fp64."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 20, 3, 4, generator=g)
    x[:, ::2] *= 6.0                                          # rows of A of very different magnitude
    x = x.cuda()
    v = x.view(1, 20, -1).double()
    a = v @ v.transpose(1, 2)
    rowmax = a.amax(-1)
    assert (rowmax.max() - rowmax.min()).item() > 80 and (a.max() - a.min()).item() > 88
    out = F.channel_attention(x)
    assert torch.isfinite(out).all()
    ref = x.double() + (torch.softmax(-a, -1) @ v).view_as(x)          # no row constant at all
    ref2 = x.double() + (torch.softmax(1234.5 - a, -1) @ v).view_as(x)  # another one
    assert rel_to_max(ref2, ref) <= 1e-12
    yard = rel_to_max(sp_aten(x).double(), ref)
    assert rel_to_max(out.double(), ref) <= max(FLOOR, 4*yard)


# ------------------------------------------------------------------------------------------------- se_gate
SE_SHAPES = [(3, 5, 2, 2), (2, 12, 5, 7), (2, 96, 17, 33), (1, 512, 12, 40), (2, 16, 192, 640)]


def _se_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.relu(torch.randn(shape, generator=g))            # post-ReLU, as the decoder feeds it
    ws = [torch.randn(C, C, generator=g)/C**0.5, 0.1*torch.randn(C, generator=g), torch.randn(C, C, generator=g)/C**0.5, 0.1*torch.randn(C, generator=g)]
    return [t.cuda() for t in [x] + ws], torch.randn(shape, generator=g).cuda()


def _se_run(fn, ins, gout, dtype=torch.float32, need=(True,)*5):
    leaves = [t.detach().to(dtype).clone().requires_grad_(n) for t, n in zip(ins, need)]
    out = fn(*leaves)
    out.backward(gout.to(dtype))
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize('shape', SE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_se_gate_matches_fp64(F, shape):
    """Output and all five gradients at 2e-6 of the tensor's maximum; two runs on the same inputs are bit-equal (every sum has a fixed order)."""
    ins, gout = _se_inputs(shape, seed=2000 + sum(shape))
    o64, g64 = _se_run(se_aten, ins, gout, torch.float64)
    o, gr = _se_run(F.se_gate, ins, gout)
    o2, gr2 = _se_run(F.se_gate, ins, gout)
    names = ['x', 'w1', 'b1', 'w2', 'b2']
    errs = {'out': rel_to_max(o.double(), o64), **{f'grad_{n}': rel_to_max(a.double(), r) for n, a, r in zip(names, gr, g64)}}
    parity_note(f'cadepth_parity se_gate {"x".join(map(str, shape)):>14}: ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    for k, v in errs.items(): assert v <= FLOOR, f'{k}: {v:.2e}'
    assert torch.equal(o, o2) and all(torch.equal(a, b) for a, b in zip(gr, gr2)), 'two runs on the same inputs differ'


def test_se_gate_partial_gradients_and_the_returned_gate(F):
    ins, gout = _se_inputs((2, 12, 5, 7), seed=31)
    o64, g64 = _se_run(se_aten, ins, gout, torch.float64)
    _, g_all = _se_run(F.se_gate, ins, gout)
    _, g_par = _se_run(F.se_gate, ins, gout, need=(False, True, True, True, True))      # only the parameters
    assert g_par[0] is None and all(torch.equal(a, b) for a, b in zip(g_par[1:], g_all[1:]))
    _, g_x = _se_run(F.se_gate, ins, gout, need=(True, False, False, False, False))     # only x
    assert all(v is None for v in g_x[1:]) and torch.equal(g_x[0], g_all[0])
    assert rel_to_max(g_x[0].double(), g64[0]) <= FLOOR
    y, gate = F.se_gate(*ins, return_gate=True)
    x, w1, b1, w2, b2 = [t.double() for t in ins]
    a64 = torch.sigmoid(torch.relu(x.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)
    assert gate.shape == (2, 12) and not gate.requires_grad and rel_to_max(gate.double(), a64) <= FLOOR
    w4 = [ins[1].view(12, 12, 1, 1), ins[2], ins[3].view(12, 12, 1, 1), ins[4]]                    # the 1x1 convolutions' own weight shapes
    assert torch.equal(F.se_gate(ins[0], *w4), y)


def test_operators_refuse_wrong_operands_on_the_gpu(F):
    """What the host test cannot reach without a device: dtype, a missing operand, operands on two devices; and the shape refusals again, on GPU tensors."""
    xc, wc, bc = torch.rand(2, 6, 3, 4).cuda(), torch.rand(6, 6).cuda(), torch.rand(6).cuda()
    with pytest.raises(ValueError): F.channel_attention(xc[0])
    with pytest.raises(TypeError): F.channel_attention(xc.double())
    with pytest.raises(TypeError): F.se_gate(xc, None, bc, wc, bc)
    with pytest.raises(TypeError): F.se_gate(xc, wc, bc.double(), wc, bc)
    with pytest.raises(ValueError): F.se_gate(xc, wc[:5], bc, wc, bc)
    with pytest.raises(ValueError): F.se_gate(xc, wc, bc[:5], wc, bc)
    with pytest.raises(ValueError): F.se_gate(xc, wc, bc, torch.rand(6, 6, 3, 3).cuda(), bc)
    with pytest.raises(RuntimeError, match='GPU'): F.se_gate(xc, wc, bc.cpu(), wc, bc)
    with pytest.raises(RuntimeError, match='GPU'): F.channel_attention(xc.cpu())


# ------------------------------------------------------------------------------------------------- decoder
@pytest.mark.parametrize('route', ['mfma', 'auto', 'miopen'])
def test_glued_decoder_matches_the_reference_decoder(F, route):
    """As test_decoder_golden.py::test_decoder_kernels_match_the_reference_decoder, at its bounds (2e-5 on the disparities, 2e-4 of the maximum on the
    gradients), on the fixture's two samples, so that the training-mode BatchNorm (batch statistics, running-statistics update) is held to the reference
    across the batch: the fixture's recorded fp32-vs-fp64 error of the reference itself is 5.0e-7 / 2.8e-6, below a quarter of either.  The running statistics are
    linear in the convolutions' outputs and held to the gradients' bound."""
    g = load_golden('net_decoder_cadepth_64x96')
    assert g['meta_ref_fp32_vs_fp64_out'] <= 2e-5/4 and g['meta_ref_fp32_vs_fp64_grad'] <= 2e-4/4
    F.set_conv_route(route)
    try: out = run_and_compare('cuda', 2e-5, 2e-4, stat_tol=2e-4)
    finally: F.set_conv_route('auto')
    assert all(o.is_cuda for o in out.values())


def _two_paths(F, dec, feats, gouts, autocast=False):
    """-> {glued: (outputs, feature gradients, parameter gradients, buffers)} of the same decoder from the same state."""
    state, res = copy.deepcopy(dec.state_dict()), {}
    for glued in (True, False):
        dec.load_state_dict(state); dec.zero_grad(set_to_none=True)
        leaves = [f.detach().clone().requires_grad_(True) for f in feats]
        with contextlib.nullcontext() if glued else dec.plain_path(): out = dec(leaves)
        if gouts is not None: sum((out[i]*gouts[i]).sum() for i in out).backward()
        res[glued] = ({i: o.detach() for i, o in out.items()}, [f.grad for f in leaves], {k: p.grad for k, p in dec.named_parameters()},
                      {k: b.detach().clone() for k, b in dec.named_buffers()})
    return res


def _feats(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(b, c, h//s, w//s, generator=g).cuda() for c, s in zip(CADEPTH_KW['num_ch_enc'], CADEPTH_KW['enc_sc'])]
    return feats, g


def _compare_paths(res, out_tol, grad_tol, out_rel=False):
    (o1, gf1, gp1, b1), (o0, gf0, gp0, b0) = res[True], res[False]
    for i in o0:
        d = rel_to_max(o1[i], o0[i]) if out_rel else (o1[i] - o0[i]).abs().max().item()
        assert d <= out_tol, f'output at scale {i}: {d:.2e}'
    for j, (a, r) in enumerate(zip(gf1, gf0)):
        if r is not None: assert rel_to_max(a, r) <= grad_tol, f'gradient w.r.t. feature {j}: {rel_to_max(a, r):.2e}'
    for k, r in gp0.items():
        if r is None: continue
        assert gp1[k] is not None, f'{k} got no gradient on the glued path'
        if k.endswith(ABSORBED):
            wscale = gp0[k[:-len('bias')] + 'weight'].abs().max().item()
            assert gp1[k].abs().max().item() <= grad_tol*wscale, k
        else: assert rel_to_max(gp1[k], r) <= grad_tol, f'gradient of {k}: {rel_to_max(gp1[k], r):.2e}'
    for k, r in b0.items():
        if r.dtype == torch.int64: assert torch.equal(b1[k], r), k
        else: assert rel_to_max(b1[k], r) <= grad_tol, f'{k}: {rel_to_max(b1[k], r):.2e}'


def test_glued_path_equals_the_plain_path_in_train_mode(F):
    """Two samples at 96 x 128 (the BatchNorm statistics cross the batch): outputs, feature and parameter gradients, running statistics and batch counters."""
    dec, *_ = build('cuda')
    feats, g = _feats(2, 96, 128, seed=51)
    gouts = {i: torch.randn(2, 1, 96 >> i, 128 >> i, generator=g).cuda() for i in CADEPTH_KW['out_sc']}
    _compare_paths(_two_paths(F, dec, feats, gouts), 2e-5, 2e-4)


def test_glued_path_runs_channel_attention_below_512_channels(F, monkeypatch):
    """The routing rule sends a 512-channel deepest feature (every other decoder test here) to ATen's structure perception; with 256 channels the glued path
    calls `channel_attention` itself, and still equals the plain path: outputs, gradients, running statistics."""
    chans = [64, 64, 128, 256, 256]
    dec, *_ = build('cuda', num_ch_enc=chans)
    g = torch.Generator().manual_seed(54)
    feats = [torch.randn(2, c, 64//s, 96//s, generator=g).cuda() for c, s in zip(chans, CADEPTH_KW['enc_sc'])]
    gouts = {i: torch.randn(2, 1, 64 >> i, 96 >> i, generator=g).cuda() for i in CADEPTH_KW['out_sc']}
    calls, op = [], F.channel_attention
    monkeypatch.setattr(F, 'channel_attention', lambda x: (calls.append(tuple(x.shape)), op(x))[1])
    res = _two_paths(F, dec, feats, gouts)
    assert calls == [(2, 256, 2, 3)], calls
    _compare_paths(res, 2e-5, 2e-4)


def test_glued_path_equals_the_plain_path_in_eval_mode(F):
    dec, *_ = build('cuda')
    dec.eval()
    feats, _ = _feats(2, 64, 96, seed=52)
    before = {k: b.clone() for k, b in dec.named_buffers()}
    with torch.no_grad(): res = _two_paths(F, dec, feats, None)
    _compare_paths(res, 2e-5, 2e-4)
    for k, b in dec.named_buffers(): assert torch.equal(b, before[k]), f'{k} changed in eval mode'


@pytest.mark.parametrize('route', ['mfma', 'auto'])
def test_glued_decoder_under_bf16_autocast_stays_close_to_the_fp32_reference(F, route):
    """The bounds of test_decoder_golden.py::test_decoder_under_bf16_autocast_stays_close_to_the_fp32_reference: disparities to 1e-2, feature and weight
    gradients to 5e-2 of their sum of magnitudes.  This decoder holds them by staying in fp32 under autocast: with the Monodepth convolutions in bf16 the five
    feature gradients measured 6.0e-2, 7.4e-2, 7.6e-2, 8.7e-2, 9.2e-2 on an MI355X (ATen's autocast of the plain path: 8.8e-2 ... 14.6e-2)."""
    from cadepth_inputs import CADEPTH_BATCH
    from exact_inputs import decoder_feats, decoder_out_grads
    from slowtv_monodepth_amd.networks import checkpoint as ck
    import numpy as np
    from conftest import GOLDEN
    g = load_golden('net_decoder_cadepth_64x96')
    dec, holder, shapes, state = build('cuda')
    feats = [f.cuda().requires_grad_(True) for f in decoder_feats(seed=96, b=CADEPTH_BATCH)]
    gouts = decoder_out_grads(seed=97, b=CADEPTH_BATCH)
    F.set_conv_route(route)
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16): out = dec(feats)
        sum((out[i].float()*gouts[i].cuda()).sum() for i in out).backward()
    finally: F.set_conv_route('auto')
    for i in CADEPTH_KW['out_sc']:
        d = (out[i].detach().float().cpu() - g[f'out_{i}']).abs().max().item()
        assert d <= 1e-2, f'disparity at scale {i}: {d:.2e}'
    for j, f in enumerate(feats):
        ref = g[f'gfeat_{j}']
        e = (gfeat_sample(j, f.grad.float().cpu()) - ref).abs().sum().item()/ref.abs().sum().item()
        parity_note(f'cadepth_parity decoder bf16 autocast route {route}: gradient w.r.t. feature {j} {e:.2e} of its sum of magnitudes (bound 5e-2)')
        assert e <= 5e-2, f'gradient w.r.t. encoder feature {j}: {e:.2e} of its sum of magnitudes'
    grads = {k: v.grad for k, v in zip(ck.to_reference_state_dict(holder).keys(), holder.state_dict(keep_vars=True).values())}
    with np.load(GOLDEN/'net_decoder_cadepth_64x96.npz') as z: pkeys = [str(k) for k in z['meta_param_keys']]
    stats = g['gparam_stats']
    for n, k in enumerate(pkeys):
        if not k.endswith('.weight') or grads[k].ndim != 4 or grads[k].shape[-1] != 3: continue      # the 3x3 convolutions' weights, as the Monodepth test
        gk = grads[k].detach().double().cpu()
        assert abs(gk.abs().sum().item() - stats[n, 1].item()) <= 5e-2*stats[n, 1].item(), f'sum of |gradient| of {k}'


def test_mask_decoder_with_two_relu_channels(F):
    dec, *_ = build('cuda', out_ch=2, out_act='relu')
    feats, g = _feats(2, 64, 96, seed=53)
    gouts = {i: torch.randn(2, 2, 64 >> i, 96 >> i, generator=g).cuda() for i in CADEPTH_KW['out_sc']}
    res = _two_paths(F, dec, feats, gouts)
    assert res[True][0][0].shape == (2, 2, 64, 96) and (res[True][0][0] >= 0).all()
    _compare_paths(res, 2e-5, 2e-4, out_rel=True)


# ------------------------------------------------------------------------------------------------- trainer
def test_example_config_takes_two_optimizer_steps(F):
    """`cfg/kitti_cadepth.yaml` at 64 x 96 on synthetic batches: finite losses, the single-node loss path, a gradient in every decoder parameter, and every
    decoder parameter moved by the two steps."""
    from slowtv_monodepth_amd import parsers
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_cadepth.yaml').read_text())
    assert cfg['net']['depth']['pretrained'] is False
    torch.manual_seed(0)
    m = MonoDepthModule(copy.deepcopy(cfg)).cuda()
    opt = parsers.get_opt(m.nets, dict(cfg['optimizer']))
    dec = m.nets['depth'].decoders['disp']
    start = {k: p.detach().clone() for k, p in dec.named_parameters()}
    for k in range(2):
        batch = make_batch(2, 64, 96, (-1, 1), seed=42 + k, device='cuda')
        opt.zero_grad(set_to_none=True)
        loss, ld, fwd = m.step(batch)
        loss.backward()
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for k_, v in ld.items() if k_.startswith('loss_'))
        assert str(getattr(m.backend, 'last_path', '')).startswith('single node'), getattr(m.backend, 'last_path', None)
        for k_, p in dec.named_parameters(): assert p.grad is not None and torch.isfinite(p.grad).all(), f'{k_} got no (finite) gradient'
        opt.step()
    still = [k for k, p in dec.named_parameters() if torch.equal(p.detach(), start[k])]
    assert not still, f'parameters that did not move: {still}'


# ------------------------------------------------------------------------------------------------- hostile memory
def _hostile_case(op, ins, gout, shift, n_workspaces):
    """`op` on operands in guarded, poisoned, `shift`-element-offset blocks with every buffer it allocates served from the arena, forward and backward:
    guards intact, results finite and bit-equal to the run in plain memory, workspaces from the arena."""
    plain = [t.detach().clone().requires_grad_(True) for t in ins]
    out_p = op(*plain)
    out_p.backward(gout)
    arena = Arena()
    with hostile(arena):      # (the blocks the operators allocate stay 16-byte aligned, as the caching allocator's; only the operands are shifted)
        leaves = [arena.guarded(t, shift).requires_grad_(True) for t in ins]
        g = arena.guarded(gout, shift)
        out = op(*leaves)
        out.backward(g)
        served = sum(1 for b in arena.blocks if b[4] == torch.uint8)
    assert_finite(out.detach(), 'output')
    for k, t in enumerate(leaves): assert_finite(t.grad, f'gradient of operand {k}')
    assert torch.equal(out.detach(), out_p.detach()) and all(torch.equal(a.grad, b.grad) for a, b in zip(leaves, plain)), 'differs from the run in plain memory'
    assert served == n_workspaces, f'{served} workspaces came from the arena, expected {n_workspaces}'
    arena.check()


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('shape', [(2, 33, 2, 3), (2, 12, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_operators_in_hostile_memory(F, shape, shift):
    x, gout = _sp_input(shape, 'peaked', seed=61)
    _hostile_case(F.channel_attention, [x], gout, shift, n_workspaces=2)
    ins, gout = _se_inputs(shape, seed=62)
    _hostile_case(F.se_gate, ins, gout, shift, n_workspaces=2)
