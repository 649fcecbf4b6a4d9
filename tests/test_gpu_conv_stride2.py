"""The encoders' 3x3 stride-2 convolutions, `conv2d(x, w (CO,C,3,3), stride=2, padding=1)`, on the split-bf16 MFMA kernels (`conv3x3_s2`,
`smd_conv3x3s2_mfma_*`): output and weight gradient against fp64 `conv2d`, repeatability, the data gradient (ATen's), operands on which nothing rounds
(tests/conv_exact.py: the fp64 result bit for bit), the fall-back for shapes the kernels turn down, and a whole ResNet-18 encoder on the kernels against
the same encoder on MIOpen."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import conv_exact as X
from conftest import rel_to_max

pytestmark = pytest.mark.gpu
KW = dict(stride=2, padding=1)


@pytest.fixture(scope='module')
def HF():
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


def _out(n): return (n - 1)//2 + 1


def _served(B, C, CO, H, W):
    from slowtv_monodepth_amd import _lib
    return _lib.lib.smd_conv3x3s2_mfma_workspace_bytes(B, C, CO, H, W) > 0


def _case(B, C, CO, H, W, seed=0):
    gen = torch.Generator(device='cuda').manual_seed(seed + B*1000 + C*10 + H + W)
    x = torch.randn(B, C, H, W, device='cuda', generator=gen)
    wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, CO, _out(H), _out(W), device='cuda', generator=gen)
    return x, wt, gy


# (B, C, CO, H, W).  16 -> 32 at 1x1, 2x2, 3x5, 5x7: odd sizes, images smaller than a tile, the Ho formula.  32 -> 64 at 8x66: a tile edge at the last
# column, an even W whose last input column no output reads, three strips of the weight gradient.  128 -> 256 at 24x80 and 256 -> 512 at 12x40: 3 x 20
# tiles, the K split (4 and 8 splits), four channel tiles per block, several channel groups of the weight gradient.  CO = 96 (a wave past CO, a channel
# group of the weight gradient past CO) and C = 48 (a channel group past C).  20 samples of 256 -> 512 at 2x2: weight-gradient blocks walk two samples each.
SHAPES = [(1, 16, 32, 1, 1), (1, 16, 32, 2, 2), (1, 16, 32, 3, 5), (1, 16, 32, 5, 7), (3, 32, 64, 8, 66), (2, 128, 256, 24, 80), (2, 256, 512, 12, 40),
          (2, 32, 96, 9, 14), (2, 48, 64, 7, 12), (20, 256, 512, 2, 2)]


@pytest.mark.parametrize('B,C,CO,H,W', SHAPES)
def test_stride2_against_fp64(HF, B, C, CO, H, W):
    """Output and weight gradient within 2e-6 of the tensor's max of fp64 `conv2d(stride=2, padding=1)` (the bound of every split-bf16 kernel here); bit for
    bit the same on a second call; the data gradient is ATen's."""
    x, wt, gy = _case(B, C, CO, H, W)
    assert _served(B, C, CO, H, W)
    wr = wt.double().clone().requires_grad_(True)
    yr = TF.conv2d(x.double(), wr, **KW); yr.backward(gy.double())
    out = []
    for _ in range(2):
        xl, wl = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        y = HF.conv3x3_s2(xl, wl); y.backward(gy)
        out.append((y.detach(), wl.grad, xl.grad))
    y, gw, gx = out[0]
    e_y, e_w = rel_to_max(y.double(), yr.detach()), rel_to_max(gw.double(), wr.grad)
    print(f'stride 2 B={B} {C}->{CO} {H}x{W}: output {e_y:.3g}, weight gradient {e_w:.3g} of the maximum')
    assert y.shape == yr.shape
    assert e_y <= 2e-6
    assert e_w <= 2e-6
    for a, b in zip(out[0][:2], out[1][:2]): assert torch.equal(a, b)          # (the data gradient is MIOpen's: it may add atomically)
    xa = x.clone().requires_grad_(True)
    TF.conv2d(xa, wt, **KW).backward(gy)
    assert rel_to_max(gx, xa.grad) < 1e-5


@pytest.mark.parametrize('which', ['weight', 'input', 'both'])
def test_stride2_gradients_asked_for(HF, which):
    """The gradient not asked for stays None; the weight gradient does not depend on whether the input's is asked for, and the input's (ATen's) is `conv2d`'s."""
    x, wt, gy = _case(2, 32, 64, 9, 14, seed=2)
    wa = wt.clone().requires_grad_(True)
    HF.conv3x3_s2(x, wa).backward(gy)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    TF.conv2d(xr, wr, **KW).backward(gy)
    xi, wi = x.clone().requires_grad_(which != 'weight'), wt.clone().requires_grad_(which != 'input')
    HF.conv3x3_s2(xi, wi).backward(gy)
    if which == 'weight': assert xi.grad is None
    else: assert rel_to_max(xi.grad, xr.grad) < 1e-5
    if which == 'input': assert wi.grad is None
    else: assert torch.equal(wi.grad, wa.grad)


# ---- operands on which nothing rounds: the fp64 result bit for bit ----
EXACT = [(1, 16, 32, 5, 7), (3, 32, 64, 8, 66), (2, 32, 96, 9, 14), (2, 48, 64, 7, 12), (2, 256, 512, 12, 40), (20, 256, 512, 2, 2)]
IDX_MAP = ('phase', 'sample', 'channel', 'y', 'x')
IDX_WGT = ('run', 'co', 'c', 'tap row', 'tap column')


@functools.lru_cache(maxsize=2)
def _layout(xshape):
    gen = torch.Generator().manual_seed(sum(xshape))
    return X.lattice_phases(xshape, 3), X.one_per_channel(xshape, 4, gen)   # (impulses three apart: no output of a 3x3 window sees two)


def _same(label, names, got, ref):
    assert got.dtype == torch.float32
    diff = X.first_difference(got, ref.float(), names)
    assert diff is None, f'{label}: {diff}'


def _grad_w(x64, w64, gy64):
    w64 = w64.clone().requires_grad_(True)
    return torch.autograd.grad(TF.conv2d(x64, w64, **KW), w64, gy64)[0]


@pytest.mark.parametrize('family', list(X.FAMILIES))
@pytest.mark.parametrize('B,C,CO,H,W', EXACT)
def test_stride2_impulses_equal_fp64(HF, B, C, CO, H, W, family):
    """Piece-built operands, one product per output element (the output: impulse lattices in x; the weight gradient: one nonzero of x per channel against a
    dense dL/dy): a tap, a column parity or a piece read from the wrong place is another number."""
    assert _served(B, C, CO, H, W)
    xshape, wshape, yshape = (B, C, H, W), (CO, C, 3, 3), (B, CO, _out(H), _out(W))
    in_ph, w_runs = _layout(xshape)
    ka, kb = X.FAMILIES[family]
    gen = torch.Generator().manual_seed(B + C + CO + H + W + ord(family[0]))
    px, pw, pg = X.draw(xshape, ka, gen), X.draw(wshape, kb, gen), X.draw(yshape, kb, gen)
    ref = None
    for scale, (ex, ew, eg) in X.SCALES.items():
        label = f'stride 2 {(B, C, CO, H, W)} family {family} scale {scale}'
        x, wt, gy = px.at(ex).cuda(), pw.at(ew).cuda(), pg.at(eg).cuda()
        xs, xo = X.impulse_stack(x, in_ph), [X.keep_only(x, idx) for idx in w_runs]
        if ref is None:                                         # (scale 'unit' comes first: exponents 0)
            w64 = wt.double()
            yr = TF.conv2d(xs.flatten(0, 1).double(), w64, **KW).unflatten(0, (len(in_ph), -1))
            gwr = torch.stack([_grad_w(t.double(), w64, gy.double()) for t in xo])
            assert (yr != 0).any() and (gwr != 0).any() and yr.shape[2:] == yshape[1:]
            ref = (yr, gwr)
        ys = torch.stack([HF.conv3x3_s2(xs[p], wt).detach() for p in range(len(in_ph))])
        _same(label + ', output', IDX_MAP, ys, ref[0]*2.0**(ex + ew))
        gws = []
        for t in xo:
            wl = wt.clone().requires_grad_(True)
            gws.append(torch.autograd.grad(HF.conv3x3_s2(t, wl), wl, gy)[0])
        _same(label + ', weight gradient', IDX_WGT, torch.stack(gws), ref[1]*2.0**(ex + eg))


@pytest.mark.parametrize('B,C,CO,H,W', EXACT + [(2, 128, 256, 24, 80)])
def test_stride2_dense_integers_equal_fp64(HF, B, C, CO, H, W):
    """Small integers everywhere: every partial sum is an integer below 2^24, so indexing, tails, K splits and sample groups show at every element."""
    assert _served(B, C, CO, H, W)
    gen = torch.Generator().manual_seed(B + C + CO + H + W)
    px, pw, pg = X.draw((B, C, H, W), 'int2', gen), X.draw((CO, C, 3, 3), 'int2', gen), X.draw((B, CO, _out(H), _out(W)), 'int2', gen)
    x64, w64, g64 = (t.at(0).cuda().double() for t in (px, pw, pg))
    w64.requires_grad_(True)
    yr = TF.conv2d(x64, w64, **KW)
    gwr, = torch.autograd.grad(yr, w64, g64)
    assert max(t.abs().max().item() for t in (yr, gwr)) < 2**24
    for scale, (ex, ew, eg) in X.SCALES.items():
        label = f'stride 2 {(B, C, CO, H, W)} family dense scale {scale}'
        x, wt, gy = px.at(ex).cuda(), pw.at(ew).cuda().requires_grad_(True), pg.at(eg).cuda()
        y = HF.conv3x3_s2(x, wt); y.backward(gy)
        _same(label + ', output', IDX_MAP[1:], y.detach(), yr.detach()*2.0**(ex + ew))
        _same(label + ', weight gradient', IDX_WGT[1:], wt.grad, gwr*2.0**(ex + eg))


# ---- shapes the kernels turn down ----
@pytest.mark.parametrize('C,CO', [(8, 32), (16, 16)])
def test_stride2_unserved_shapes_fall_back(C, CO):
    """C = 8 / CO = 16: the size query says 0, the entry points return SMD_E_UNSUPPORTED, and `conv3x3_s2` is ATen's result under every route."""
    from slowtv_monodepth_amd import _lib, functional as HF
    from slowtv_monodepth_amd._device import call, _stream
    x, wt, gy = _case(2, C, CO, 9, 14, seed=3)
    assert not _served(2, C, CO, 9, 14)
    y, gw, ws = torch.empty_like(gy), torch.empty_like(wt), torch.empty(4096, device='cuda', dtype=torch.uint8)
    with pytest.raises(_lib.Unsupported): call('smd_conv3x3s2_mfma_fwd', x.data_ptr(), ws.data_ptr(), y.data_ptr(), ws.data_ptr(), 4096, 2, C, CO, 9, 14, _stream())
    with pytest.raises(_lib.Unsupported): call('smd_conv3x3s2_mfma_bwd_weight', x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(), 4096, 2, C, CO, 9, 14, _stream())
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    yr = TF.conv2d(xr, wr, **KW); yr.backward(gy)
    try:
        for mode in ('auto', 'mfma', 'miopen'):
            HF.set_conv_route(mode)
            xl, wl = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
            y = HF.conv3x3_s2(xl, wl); y.backward(gy)
            assert rel_to_max(y, yr) < 1e-5 and rel_to_max(wl.grad, wr.grad) < 1e-5 and rel_to_max(xl.grad, xr.grad) < 1e-5, mode
            assert not [k for k in HF.conv_routes() if k[0] in ('fwd_s2', 'wgt_s2')]
    finally:
        HF.set_conv_route('auto')


# ---- a whole encoder ----
def test_resnet18_encoder_stride2_mfma_equals_miopen(HF):
    """A whole ResNet-18 encoder (fused BatchNorm on) at 2 x 3 x 64 x 96, forward and backward, route `mfma` (stem, stride-1 and stride-2 3x3 layers on the
    kernels) against route `miopen` on the same weights: the tolerances of `test_resnet18_encoder_stem_mfma_equals_miopen` (features 1e-4, gradients 2e-3
    of the maximum).  Under `auto` the routes decided include the stride-2 operators of the three transition blocks."""
    from slowtv_monodepth_amd.networks import encoders as E
    torch.manual_seed(1)
    net = E.create_encoder('resnet18', in_chans=3).cuda().train()
    x = torch.randn(2, 3, 64, 96, device='cuda')
    res = []
    try:
        for mode in ('mfma', 'miopen', 'auto'):
            HF.set_conv_route(mode)
            net.zero_grad()
            state = {k: v.clone() for k, v in net.state_dict().items()}
            feats = net(x)
            sum((f*f).mean() for f in feats).backward()
            res.append(([f.detach() for f in feats], [p.grad.clone() for p in net.parameters()]))
            net.load_state_dict(state)
        routed = {k[0]: [] for k in HF.conv_routes()}
        for k in HF.conv_routes(): routed[k[0]].append(k[1:])
    finally:
        HF.set_conv_route('mfma')
    for a, b in zip(res[0][0], res[1][0]): assert rel_to_max(a, b) < 1e-4
    for a, b in zip(res[0][1], res[1][1]): assert rel_to_max(a, b) < 2e-3
    for a, b in zip(res[2][0], res[1][0]): assert rel_to_max(a, b) < 1e-4
    for op in ('fwd_s2', 'wgt_s2'):
        assert sorted(routed.get(op, [])) == [(2, 64, 128, 16, 24), (2, 128, 256, 8, 12), (2, 256, 512, 4, 6)], (op, routed)
