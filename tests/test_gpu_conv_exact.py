"""The split-bf16 MFMA convolutions with NO tolerance: on the operands of conv_exact.py every product the kernels keep and every partial sum in any order is
an fp32 number, so output, input gradient and weight gradient must equal fp64 `conv2d` bit for bit (`torch.equal` against the fp64 result cast to the
output's type).  The tests next door hold the same kernels to 2e-6 of the tensor's maximum on Gaussian operands — the kernels' own accumulation noise, under
which one wrong piece at one tap, channel or pixel disappears; here it changes the result by more than 20 ulp against a noise of zero.

Per shape: the three piece-built families (A, B, C: between them every kept product) on the impulse layouts — forward and data gradient on a lattice of
spacing 3 (stem: 7) swept over every offset and every channel, the weight gradient on one element of x per channel against a dense dL/dy — and dense small
integers, each at unit scale and with dL/dy at 2^-30 against weights at 2^20.  The reference is computed once per family at unit scale; at the other scale
it is that result times the power of two, which is exact in fp64.

Forms: the decoder's padded form `conv3x3_mfma` (incl. the thin stage, the bf16-tensor form with one piece, and the `conv_two_tiles` knob), the encoders'
zero-padded `conv3x3_same`, the stem `conv7x7s2_stem` (forward and weight gradient: its data gradient is ATen's), and for comparison one or two shapes of
`conv3x3_thin` (f32 MFMA) and `conv3x3_head`, where a single fp32 product is exact for free.  An operator the MFMA kernels do not serve at a shape (the padded
form's data gradient needs C % 32 == 0) runs on MIOpen and is not checked here.  `smd_last_kernel_variant` names the reconstruction kernels only, not the
convolution forms (rectangular 64 x 4 and 32 x 8 tiles, row bands, the K split, the thin stage): which shape reaches which is in the comments at the same
shapes in test_gpu_parity.py, test_gpu_encoder_conv.py and test_gpu_conv_band_tiles.py, and in `conv_shape` of csrc/smd_conv_mfma.hip."""
import functools
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

import conv_exact as X

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
Served = namedtuple('Served', 'fwd data wgt')
IDX_MAP = ('phase', 'sample', 'channel', 'y', 'x')
IDX_WGT = ('run', 'co', 'c', 'tap row', 'tap column')


@pytest.fixture(scope='module')
def HF():
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


# ---- the forms: how to call one, its fp64 `conv2d`, its tensor shapes, and which operators the kernels under test serve --------------------------------
Form = namedtuple('Form', 'run kw step shapes served')


def _shapes3(grow, CO=None):
    def shapes(dims):
        B, C, co, h, w = dims if CO is None else (*dims[:2], CO, *dims[2:])
        return (B, C, h + grow, w + grow), (co, C, 3, 3), (B, co, h, w)
    return shapes


def _stem_shapes(dims):
    B, C, H, W = dims
    return (B, C, H, W), (64, C, 7, 7), (B, 64, (H - 1)//2 + 1, (W - 1)//2 + 1)


def _served_mfma(zpad):
    def served(dims):
        from slowtv_monodepth_amd import _lib
        from slowtv_monodepth_amd.conv_ops import _served
        B, C, CO, h, w = dims
        sized = not zpad or _lib.lib.smd_conv3x3z_mfma_workspace_bytes(B, C, CO, h, w) > 0
        sv = _served(C, CO, zpad, sized)
        assert sv.sized and sv.fwd and sv.wgt and (sv.data or not zpad), f'{dims}: not a shape the kernels serve'
        return Served(sv.fwd, sv.data, sv.wgt)
    return served


def _served_stem(dims):
    from slowtv_monodepth_amd import _lib
    assert _lib.lib.smd_conv7x7s2_workspace_bytes(dims[0], dims[1], 64, dims[2], dims[3]) > 0, f'{dims}: not a shape the stem kernels serve'
    return Served(True, False, True)


FORMS = {'padded': Form(lambda F, x, w: F.conv3x3_mfma(x, w), {}, 3, _shapes3(2), _served_mfma(False)),
         'same': Form(lambda F, x, w: F.conv3x3_same(x, w), dict(padding=1), 3, _shapes3(0), _served_mfma(True)),
         'stem': Form(lambda F, x, w: F.conv7x7s2_stem(x, w), dict(stride=2, padding=3), 7, _stem_shapes, _served_stem),
         'thin': Form(lambda F, x, w: F.conv3x3_thin(x, w), {}, 3, _shapes3(2, CO=16), lambda dims: Served(True, True, True)),
         'head': Form(lambda F, x, w: F.conv3x3_head(x, w, None, None), {}, 3, _shapes3(2, CO=1), lambda dims: Served(True, True, True))}


@functools.lru_cache(maxsize=2)
def _layout(xshape, yshape, step):
    """The impulse layouts of one shape, built once and shared by its families: phases of the input, phases of dL/dy, the weight gradient's runs."""
    gen = torch.Generator().manual_seed(sum(xshape) + 7*sum(yshape))
    return X.lattice_phases(xshape, step), X.lattice_phases(yshape, step), X.one_per_channel(xshape, 8 if step == 7 else 4, gen)


def _grad_w(kw, x64, w64, gy64):
    w64 = w64.clone().requires_grad_(True)
    return torch.autograd.grad(TF.conv2d(x64, w64, **kw), w64, gy64)[0]


def _grad_x(kw, xshape, w64, gy64):
    z = torch.zeros((gy64.shape[0], *xshape[1:]), dtype=torch.float64, device=gy64.device, requires_grad=True)
    return torch.autograd.grad(TF.conv2d(z, w64, **kw), z, gy64)[0]


def _same(label, names, got, ref):
    assert got.dtype in (torch.float32, BF)
    diff = X.first_difference(got, ref.to(got.dtype), names)
    assert diff is None, f'{label}: {diff}'


def _impulses(HF, form, dims, family, kinds, act=torch.float32):
    f = FORMS[form]
    xshape, wshape, yshape = f.shapes(dims)
    sv = f.served(dims)
    in_ph, out_ph, w_runs = _layout(xshape, yshape, f.step)
    gen = torch.Generator().manual_seed(sum(dims) + ord(family[0]))
    ka, kb = kinds
    px, pw, pga, pgb = X.draw(xshape, ka, gen), X.draw(wshape, kb, gen), X.draw(yshape, ka, gen), X.draw(yshape, kb, gen)

    def operands(ex, ew, eg):
        x, wt, gy_a, gy_b = (t.cuda() for t in (px.at(ex), pw.at(ew), pga.at(eg), pgb.at(eg)))
        for t in (x, gy_a, gy_b): assert torch.equal(t.to(act).float(), t)
        x, gy_a, gy_b = x.to(act), gy_a.to(act), gy_b.to(act)
        return X.impulse_stack(x, in_ph), wt, X.impulse_stack(gy_a, out_ph), [X.keep_only(x, idx) for idx in w_runs], gy_b
    xs, wt, gs, xo, gy_b = operands(0, 0, 0)
    w64 = wt.double()
    yr = TF.conv2d(xs.flatten(0, 1).double(), w64, **f.kw).unflatten(0, (len(in_ph), -1))
    gxr = _grad_x(f.kw, xshape, w64, gs.flatten(0, 1).double()).unflatten(0, (len(out_ph), -1)) if sv.data else None
    gwr = torch.stack([_grad_w(f.kw, t.double(), w64, gy_b.double()) for t in xo])
    assert (yr != 0).any() and (gwr != 0).any() and yr.shape[2:] == yshape[1:]

    for scale, (ex, ew, eg) in X.SCALES.items():
        label = f'{form} {dims} family {family} scale {scale}'
        if scale != 'unit': xs, wt, gs, xo, gy_b = operands(ex, ew, eg)
        ys, gxs = [], []
        for p in range(max(len(in_ph), len(out_ph) if sv.data else 0)):
            back = sv.data and p < len(out_ph)
            xi = xs[p % len(in_ph)].detach().requires_grad_(back)
            y = f.run(HF, xi, wt)
            if p < len(in_ph): ys.append(y.detach())
            if back: gxs.append(torch.autograd.grad(y, xi, gs[p])[0])
        _same(label + ', output', IDX_MAP, torch.stack(ys), yr*2.0**(ex + ew))
        if sv.data: _same(label + ', input gradient', IDX_MAP, torch.stack(gxs), gxr*2.0**(eg + ew))
        gws = []
        for t in xo:
            wl = wt.clone().requires_grad_(True)
            gws.append(torch.autograd.grad(f.run(HF, t, wl), wl, gy_b)[0])
        _same(label + ', weight gradient', IDX_WGT, torch.stack(gws), gwr*2.0**(ex + eg))


def _dense(HF, form, dims, kind='int2', act=torch.float32, check=('output', 'input gradient', 'weight gradient')):
    """Small integers everywhere, all three operators in one call: indexing, tails, K splits and sample groups at every element at once."""
    f = FORMS[form]
    xshape, wshape, yshape = f.shapes(dims)
    sv = f.served(dims)
    gen = torch.Generator().manual_seed(sum(dims))
    px, pw, pg = X.draw(xshape, kind, gen), X.draw(wshape, kind, gen), X.draw(yshape, kind, gen)
    x64, w64, g64 = (t.at(0).cuda().double() for t in (px, pw, pg))
    x64.requires_grad_(True); w64.requires_grad_(True)
    yr = TF.conv2d(x64, w64, **f.kw)
    gxr, gwr = torch.autograd.grad(yr, (x64, w64), g64)
    assert max(t.abs().max().item() for t in (yr, gxr, gwr)) < 2**24
    for scale, (ex, ew, eg) in X.SCALES.items():
        label = f'{form} {dims} family dense scale {scale}'
        x, wt, gy = px.at(ex).cuda().to(act), pw.at(ew).cuda(), pg.at(eg).cuda().to(act)
        x.requires_grad_(sv.data); wt.requires_grad_(True)
        y = f.run(HF, x, wt)
        y.backward(gy)
        if 'output' in check: _same(label + ', output', IDX_MAP[1:], y.detach(), yr.detach()*2.0**(ex + ew))
        if sv.data and 'input gradient' in check: _same(label + ', input gradient', IDX_MAP[1:], x.grad, gxr*2.0**(eg + ew))
        if 'weight gradient' in check: _same(label + ', weight gradient', IDX_WGT[1:], wt.grad, gwr*2.0**(ex + eg))


def _run(HF, form, dims, family):
    if family == 'dense': _dense(HF, form, dims)
    else: _impulses(HF, form, dims, family, X.FAMILIES[family])


FAMILIES = [*X.FAMILIES, 'dense']


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('B,C,CO,h,w', X.PADDED)
def test_padded_form_equals_fp64(HF, B, C, CO, h, w, family):
    """`conv3x3_mfma` (reflection-padded input, the decoder): both rectangular tiles, row bands, the K split, channel counts off the weight gradient's
    blocks, w = 1, h = 1, and the thin stage with sixteen output channels."""
    _run(HF, 'padded', (B, C, CO, h, w), family)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('B,C,CO,h,w', X.SAME)
def test_zero_padded_form_equals_fp64(HF, B, C, CO, h, w, family):
    """`conv3x3_same` (the encoders): the smallest image, bands of whole samples, w = 1 / 3 / 47 / 49, rectangular tiles, the K split, uneven sample groups."""
    _run(HF, 'same', (B, C, CO, h, w), family)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('B,C,H,W', X.STEM)
def test_stem_equals_fp64(HF, B, C, H, W, family):
    """`conv7x7s2_stem`: output and weight gradient, both channel counts, odd and tiny sizes, b = 1 / 2 / 3."""
    _run(HF, 'stem', (B, C, H, W), family)


@pytest.mark.parametrize('family', FAMILIES)
def test_two_tiles_equals_fp64(HF, knobs, family):
    """The `conv_two_tiles` launch shape (eight waves, two tiles of 32 output channels over one staged patch) at the smallest shape where `conv_shape` takes
    it for the forward and the data gradient alike."""
    assert knobs('conv_two_tiles', 1)
    _run(HF, 'padded', X.TWO_TILES, family)


@pytest.mark.parametrize('B,C,CO,h,w', X.BF16)
def test_bf16_tensors_equal_fp64(HF, B, C, CO, h, w):
    """The bf16-tensor form (one piece): bf16 integers up to 15 against fp32 weights of integers up to 15 times a power of two — every product fits
    bf16's 8 bits, so the bf16 outputs and the fp32 weight gradient are exact.  Dense: integers in {-1, 0, 1} for the bf16 outputs where their sums of
    9 C (9 CO) terms stay within 256, and always for the fp32 weight gradient."""
    dims = (B, C, CO, h, w)
    _impulses(HF, 'padded', dims, 'bf16', ('int15', 'int15'), act=BF)
    check = ['weight gradient'] + (['output'] if 9*C <= 256 else []) + (['input gradient'] if 9*CO <= 256 else [])
    _dense(HF, 'padded', dims, kind='int1', act=BF, check=tuple(check))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('form,dims', [('thin', (2, 32, 9, 33)), ('head', (3, 5, 2, 2)), ('head', (2, 32, 17, 129))])
def test_fp32_kernels_equal_fp64(HF, form, dims, family):
    """`conv3x3_thin` (f32 MFMA) and `conv3x3_head` (no activation, no bias) on the same operands: one fp32 product per element is exact there too."""
    _run(HF, form, dims, family)
