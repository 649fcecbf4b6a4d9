"""The flip-and-blend kernel (csrc/smd_blend.hip) and what stands on it, on the GPU: `flip_blend` against the REFERENCE's fixture (tests/golden/blend_stereo.npz) at
the bound derived in test_blend_host.py (`blend_bound`), run-to-run and mirror-read bit equality, the pyramid form against per-level calls, storage-offset
operands and incoming-gradient layouts, gradient subsets in hostile memory through grad_subsets.py's checker on a local entry, `DepthNet.forward_blended` and
`BenchmarkPredictor.forward_batch(use_stereo_blend=True)` against the plain sequence.

Shapes are the fixture's (blend_inputs.BLEND_CASES), each the smallest at which something specific can break: w = 1 falls back (the mean); w = 2, 3: the ramp is
all zero / has one interior column and the middle column mirrors onto itself; w = 21: x_1 = 0.05 exactly, the clamp's edge; w = 20, 41: the 5 % edge falls between
columns; w = 67: whole four-column groups and a tail of 3; h = 1; a pyramid that ends in 1x3.  The only 16-byte vector groups of a mirrored call need w % 4 == 0
(w = 20 and the pyramid's 24 and 12); the un-mirrored calls take them at w = 41 and 67 too."""
import pytest
import torch

import grad_subsets as G
from blend_inputs import BLEND_CASES, BLEND_PYRAMID, BLEND_RANGE, BLEND_SCALED, blend_case, blend_expected
from conftest import load_golden, parity_note
from hostile_memory import Arena, assert_finite, hostile
from test_blend_host import blend_bound, scale_of

pytestmark = pytest.mark.gpu
RNG = dict(min_depth=BLEND_RANGE[0], max_depth=BLEND_RANGE[1])


@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    return functional


@pytest.fixture(scope='module')
def fixture(): return load_golden('blend_stereo')


def note(line): parity_note(f'blend_parity {line}')


def _case(k):
    """-> (l, r_raw, g) on the GPU: `r_raw` is the fixture's right input un-flipped, i.e. what a network returns for the mirrored image."""
    ins = blend_case(k)
    return ins['l'].cuda(), ins['r'].flip(-1).contiguous().cuda(), ins['g'].cuda()


def _run(F, l, r, g, need=('l', 'r'), **kw):
    """forward + backward of `flip_blend` -> (out, grad_l, grad_r) (None where the operand did not ask)."""
    l, r = l.detach().clone().requires_grad_('l' in need), r.detach().clone().requires_grad_('r' in need)
    out = F.flip_blend(l, r, **kw)
    out.backward(g)
    return out.detach(), l.grad, r.grad


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
def test_flip_blend_matches_the_reference_fixture(F, fixture, scaled):
    """Output and both gradients of every fixture case within `blend_bound` of the reference's (the gradient of r_raw is the reference's gradient of r, mirrored);
    everything finite; two runs bit-equal.  The kernel repeats ATen's operation order, so bit equality is what is expected: the count is printed."""
    kw, ks = (RNG, scale_of()) if scaled else ({}, 1.0)
    fails, same, total = [], 0, 0
    for k in (BLEND_SCALED if scaled else range(len(BLEND_CASES))):
        l, r_raw, g = _case(k)
        got, again = _run(F, l, r_raw, g, **kw), _run(F, l, r_raw, g, **kw)
        out, gl, gr = (t.cpu() for t in got)
        ref_out, ref_gl, ref_gr = blend_expected(fixture, k, scaled)
        ins = blend_case(k)
        for what, mine, ref, bound in (('out', out, ref_out, blend_bound(ins['l'], ins['r'], ks)), ('grad_l', gl, ref_gl, blend_bound(ins['g'], ins['g'], ks)),
                                       ('grad_r_raw', gr.flip(-1), ref_gr, blend_bound(ins['g'], ins['g'], ks))):
            assert torch.isfinite(mine).all(), f'case {k} {what} is not finite'
            err = (mine.double() - ref.double()).abs()
            same += int((mine == ref).sum()); total += mine.numel()
            if not (err <= bound).all(): fails.append(f'case {k} {BLEND_CASES[k]} {what}: {err.max().item():.3e} (bound {bound.max().item():.3e})')
        if BLEND_CASES[k][3] == 1 and not scaled: assert torch.equal(out, (ins['l'] + ins['r'])/2), 'w = 1 is the mean'
        assert all(torch.equal(a, b) for a, b in zip(got, again)), f'case {k}: two runs on the same inputs differ'
    note(f'flip_blend vs the reference fixture ({"scaled" if scaled else "plain"}): {same} of {total} elements bit-equal')
    assert not fails, '; '.join(fails)


def test_mirror_read_equals_the_flipped_operand_and_blend_stereo(F):
    """`flip_blend(l, r_raw)` is bit-equal to the same entry point with the mirror flag off on `r_raw.flip(-1).contiguous()`, and to `geometry.blend_stereo`, forward
    and backward; with the scaling too."""
    from slowtv_monodepth_amd import geometry
    for k in range(len(BLEND_CASES)):
        l, r_raw, g = _case(k)
        r = r_raw.flip(-1).contiguous()
        for kw in ({}, RNG):
            a, b = _run(F, l, r_raw, g, **kw), _run(F, l, r, g, mirror=False, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].flip(-1), b[2]), (k, kw)
        a0 = _run(F, l, r_raw, g)[0]
        assert torch.equal(geometry.blend_stereo(l, r), a0) and torch.equal(geometry.blend_stereo(l[0], r[0]), a0[0]) and torch.equal(geometry.blend_stereo(l[0, 0], r[0, 0]), a0[0, 0])


def test_pyramid_form_is_one_launch_bit_equal_to_per_level_calls(F, fixture):
    ins = {s: _case(k) for s, k in enumerate(BLEND_PYRAMID)}
    for kw in ({}, RNG):
        ls = {s: v[0].clone().requires_grad_(True) for s, v in ins.items()}
        rs = {s: v[1].clone().requires_grad_(True) for s, v in ins.items()}
        out = F.flip_blend_pyramid(ls, rs, **kw)
        assert list(out) == list(ls) and len({o.grad_fn for o in out.values()}) == 1, 'the levels of a pyramid are outputs of ONE autograd node: one launch'
        torch.autograd.backward(list(out.values()), [v[2] for v in ins.values()])
        for s, (l, r_raw, g) in ins.items():
            o, gl, gr = _run(F, l, r_raw, g, **kw)
            assert torch.equal(out[s], o) and torch.equal(ls[s].grad, gl) and torch.equal(rs[s].grad, gr), (s, kw)
    # a level of one column in the pyramid takes the plain path, the others the launch
    ls = {0: ins[0][0], 1: ins[0][0][..., :1].contiguous()}; rs = {0: ins[0][1], 1: ins[0][1][..., :1].contiguous()}
    out = F.flip_blend_pyramid(ls, rs)
    assert torch.equal(out[0], F.flip_blend(ls[0], rs[0])) and torch.equal(out[1], (ls[1] + rs[1])/2)
    # only some levels ask for a gradient
    ls = {s: v[0].clone().requires_grad_(s == 1) for s, v in ins.items()}; rs = {s: v[1].clone().requires_grad_(s == 2) for s, v in ins.items()}
    torch.autograd.backward(list(F.flip_blend_pyramid(ls, rs).values()), [v[2] for v in ins.values()])
    assert torch.equal(ls[1].grad, _run(F, *ins[1])[1]) and torch.equal(rs[2].grad, _run(F, *ins[2])[2]) and ls[0].grad is None and rs[0].grad is None


def _offset(t, elems=1):
    """A contiguous copy of `t` that starts `elems` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4*elems and v.is_contiguous()
    return v


@pytest.mark.parametrize('k', [BLEND_CASES.index((2, 2, 3, 20)), BLEND_CASES.index((2, 2, 3, 67)), BLEND_PYRAMID[0]], ids=['w20', 'w67', 'w24'])
def test_storage_offset_operands_and_incoming_gradient_layouts(F, k):
    """An operand one element off a 16-byte boundary (each operand in turn, and the incoming gradient), a non-contiguous and a stride-0 expanded incoming
    gradient give the bits of the aligned, contiguous run."""
    l, r_raw, g = _case(k)
    for kw in (dict(), dict(mirror=False), RNG):
        want = _run(F, l, r_raw, g, **kw)
        for shifted in ((_offset(l), r_raw, g), (l, _offset(r_raw), g), (l, r_raw, _offset(g)), (_offset(l), _offset(r_raw, 3), _offset(g, 2))):
            got = _run(F, *shifted, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), kw
        strided = g.transpose(2, 3).contiguous().transpose(2, 3)
        assert not strided.is_contiguous() or g.shape[2] == 1
        assert all(torch.equal(a, b) for a, b in zip(_run(F, l, r_raw, strided, **kw), want))
        ones = _run(F, l, r_raw, torch.ones_like(g), **kw)
        expanded = _run(F, l, r_raw, torch.ones((), device='cuda').expand_as(g), **kw)
        assert all(torch.equal(a, b) for a, b in zip(expanded, ones))


def _entry(k, kw):
    """A `grad_subsets.Entry` for case k, built locally (the table of grad_subsets.py lists the `*_ops.py` modules' Functions; this operator's module is not one)."""
    from slowtv_monodepth_amd.blend import _FlipBlend, plain_flip_blend

    def operands(gen, absent=frozenset()):
        ins = blend_case(k)
        return dict(l=ins['l'], r_raw=ins['r'].flip(-1).contiguous(), gy_out=ins['g'])
    return G.Entry(f'flip_blend{BLEND_CASES[k]}{kw}', _FlipBlend, 'flip_blend', operands, ('l', 'r_raw'), (), ('out',), lambda F, o: dict(out=F.flip_blend(o['l'], o['r_raw'], **kw)),
                   lambda o: dict(out=plain_flip_blend(o['l'], o['r_raw'], **kw)), {}, {}, (), False, {})


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('k', [BLEND_CASES.index((2, 2, 3, 20)), BLEND_CASES.index((2, 1, 1, 67)), BLEND_CASES.index((2, 2, 3, 3))], ids=['w20', 'w67h1', 'w3'])
def test_gradient_subsets_in_hostile_memory(F, k, shift):
    """grad_subsets.py's rule on a local entry: only `l`, only `r_raw` or both asking, with every operand in a guarded, poisoned block (`shift` elements off its
    alignment) and every buffer the operator allocates served from the arena: the served gradient is the BITS of the full backward's, the other is None, the forward
    output does not depend on who asks, the guards are intact, every output is fully overwritten (finite)."""
    for kw in ({}, RNG):
        e = _entry(k, kw)
        cuda = {n: t.cuda() for n, t in e.operands(None).items()}
        full = G.run_entry(e, F, cuda, frozenset(e.diff))
        for n, t in full.items(): assert_finite(t, f'{e.name} {n}')

        def in_hostile_memory(subset):
            arena = Arena()
            ops = {n: arena.guarded(t, shift) for n, t in cuda.items()}
            with hostile(arena, shift):
                out = G.run_entry(e, F, ops, subset)
                served = len(arena.blocks) - len(ops)
            assert served == 1 + len(subset), f'{served} buffers came from the arena for the subset {G.tag(subset, e.diff)}: the output and one per gradient are expected'
            arena.check()
            return out
        subsets = G.subsets_of(e.diff)
        assert len(subsets) == 3
        G.check_subsets(in_hostile_memory, full, subsets, e.diff, name=e.name)


def test_operator_refuses_wrong_operands_on_the_gpu(F):
    from slowtv_monodepth_amd.blend import plain_flip_blend
    l, r_raw, g = _case(BLEND_PYRAMID[0])
    with pytest.raises(ValueError, match='Non-matching shapes'): F.flip_blend(l, r_raw[..., :20])
    with pytest.raises(ValueError, match='Min depth'): F.flip_blend(l, r_raw, min_depth=0)
    # what the kernel does not serve runs the plain sequence: another dtype, an operand on the CPU with its partner
    assert torch.equal(F.flip_blend(l.double(), r_raw.double()), plain_flip_blend(l.double(), r_raw.double()))
    assert F.flip_blend(l.bfloat16(), r_raw.bfloat16()).dtype == torch.float32      # (the reference's promotion: an fp32 ramp times a bf16 disparity)
    assert F.flip_blend(l, r_raw).shape == l.shape


# ------------------------------------------------------------------------------------------------- the network method and the predictor
def test_forward_blended_equals_two_passes_and_the_plain_blend_and_is_differentiable(F):
    from slowtv_monodepth_amd.blend import plain_flip_blend
    from slowtv_monodepth_amd.networks.depth import DepthNet
    torch.manual_seed(4)
    net = DepthNet(enc_name='resnet18', pretrained=False).cuda().eval()
    x = torch.rand(2, 3, 64, 96, device='cuda')
    with torch.no_grad(): a, b = net(x), net(x.flip(-1))
    out = net.forward_blended(x)
    assert sorted(out) == sorted(a) and list(out['disp']) == list(a['disp'])
    for s in a['disp']:
        want = plain_flip_blend(a['disp'][s], b['disp'][s])
        err = (out['disp'][s].detach().double() - want.double()).abs()
        assert out['disp'][s].shape == a['disp'][s].shape and (err <= blend_bound(a['disp'][s], b['disp'][s])).all(), (s, err.max().item())
        note(f'forward_blended scale {s}: max |kernel - plain| {err.max().item():.2e}, {int((out["disp"][s] == want).sum())} of {want.numel()} bit-equal')
    sum(o.sum() for o in out['disp'].values()).backward()
    grads = [p.grad for p in net.encoder.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and grads[0].abs().sum().item() > 0, 'no gradient reached the encoder'


class _Conv(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 1, 3, padding=1)

    def forward(self, x): return {'disp': {0: torch.sigmoid(self.conv(x))}}


@pytest.mark.parametrize('rng', [None, (0.1, 100)], ids=['no-range', 'range'])
def test_predictor_forward_batch_with_stereo_blend_equals_the_plain_sequence(F, rng):
    from slowtv_monodepth_amd.blend import plain_flip_blend
    from slowtv_monodepth_amd.geometry import to_scaled
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor
    torch.manual_seed(8)
    net, p = _Conv().cuda().eval(), BenchmarkPredictor()
    if rng: p.min_depth, p.max_depth = rng
    x = {'imgs': torch.rand(2, 3, 5, 24)}                  # on the host: the predictor copies it, and flips it on the device
    got = p.forward_batch(x, net, torch.device('cuda'), use_stereo_blend=True)
    with torch.no_grad():
        imgs = x['imgs'].cuda()
        l, r_raw = net(imgs)['disp'][0], net(imgs.flip(-1))['disp'][0]
        want = plain_flip_blend(l, r_raw)
        if rng: want = to_scaled(want, 0.1, 100)[0]
    assert got.is_cuda and not got.requires_grad and got.shape == (2, 1, 5, 24)
    assert ((got.double() - want.double()).abs() <= blend_bound(l, r_raw, scale_of() if rng else 1.0)).all()
    preds = p(net, [(x,), (x,)], use_stereo_blend=True)
    assert preds.shape == (4, 5, 24) and torch.equal(torch.from_numpy(preds[:2]), got[:, 0].cpu())
