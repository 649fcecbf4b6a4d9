"""The data gradient of the encoders' 3x3 stride-2 convolutions on the split-bf16 MFMA kernel (`conv3x3_s2`'s backward, `smd_conv3x3s2d_mfma_bwd_data`):
g_x against fp64 `conv2d`'s input gradient, repeatability, operands on which nothing rounds (tests/conv_exact.py: the fp64 result bit for bit), the
gradients asked for, the fall-back for channel counts the kernel turns down, and guarded, poisoned buffers."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import conv_exact as X
from conftest import rel_to_max
from hostile_memory import Arena, assert_finite, hostile
from test_gpu_conv_exact import IDX_MAP, _grad_x, _same
from test_gpu_conv_stride2 import EXACT, KW, SHAPES, _case, _out

pytestmark = pytest.mark.gpu

# 16 -> 32 at 4x6 and 6x5: all four parity classes of the input pixel with an even and an odd last row / column
DATA_SHAPES = SHAPES + [(2, 16, 32, 4, 6), (2, 16, 32, 6, 5)]


@pytest.fixture(scope='module')
def HF():
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


def _served(B, C, CO, H, W):
    from slowtv_monodepth_amd import _lib
    return _lib.lib.smd_conv3x3s2d_mfma_workspace_bytes(B, C, CO, H, W) > 0


def _grad_input(HF, x, wt, gy, need_w=False):
    xl, wl = x.clone().requires_grad_(True), wt.clone().requires_grad_(need_w)
    HF.conv3x3_s2(xl, wl).backward(gy)
    return xl.grad, wl.grad


@pytest.mark.parametrize('B,C,CO,H,W', DATA_SHAPES)
def test_stride2_data_against_fp64(HF, B, C, CO, H, W):
    """g_x within 2e-6 of the tensor's max of fp64 `conv2d(stride=2, padding=1)`'s input gradient (the bound of every split-bf16 kernel here); bit for bit the
    same on a second call."""
    x, wt, gy = _case(B, C, CO, H, W)
    assert _served(B, C, CO, H, W)
    ref = _grad_x(KW, (B, C, H, W), wt.double(), gy.double())
    gx, _ = _grad_input(HF, x, wt, gy)
    gx2, _ = _grad_input(HF, x, wt, gy)
    e = rel_to_max(gx.double(), ref)
    print(f'stride 2 data gradient B={B} {C}->{CO} {H}x{W}: {e:.3g} of the maximum')
    assert gx.shape == ref.shape and gx.dtype == torch.float32
    assert e <= 2e-6
    assert torch.equal(gx, gx2)


# ---- operands on which nothing rounds: the fp64 result bit for bit ----
@functools.lru_cache(maxsize=2)
def _layout(yshape):
    return X.lattice_phases(yshape, 3)                          # (impulses three apart: no input pixel's taps see two)


@pytest.mark.parametrize('family', list(X.FAMILIES))
@pytest.mark.parametrize('B,C,CO,H,W', EXACT)
def test_stride2_data_impulses_equal_fp64(HF, B, C, CO, H, W, family):
    """An impulse lattice in dL/dy against piece-built weights, one product per gradient element: a tap, a parity class, a flipped index or a piece read from
    the wrong place is another number."""
    assert _served(B, C, CO, H, W)
    xshape, wshape, yshape = (B, C, H, W), (CO, C, 3, 3), (B, CO, _out(H), _out(W))
    out_ph = _layout(yshape)
    ka, kb = X.FAMILIES[family]
    gen = torch.Generator().manual_seed(B + C + CO + H + W + ord(family[0]) + 1)
    pw, pg = X.draw(wshape, kb, gen), X.draw(yshape, ka, gen)
    x = torch.zeros(xshape, device='cuda')
    ref = None
    for scale, (ex, ew, eg) in X.SCALES.items():
        label = f'stride 2 data gradient {(B, C, CO, H, W)} family {family} scale {scale}'
        wt, gs = pw.at(ew).cuda(), X.impulse_stack(pg.at(eg).cuda(), out_ph)
        if ref is None:                                         # (scale 'unit' comes first: exponents 0)
            ref = _grad_x(KW, xshape, wt.double(), gs.flatten(0, 1).double()).unflatten(0, (len(out_ph), -1))
            assert (ref != 0).any()
        gxs = torch.stack([_grad_input(HF, x, wt, gs[p])[0] for p in range(len(out_ph))])
        _same(label, IDX_MAP, gxs, ref*2.0**(eg + ew))


@pytest.mark.parametrize('B,C,CO,H,W', EXACT + [(2, 128, 256, 24, 80), (2, 16, 32, 4, 6), (2, 16, 32, 6, 5)])
def test_stride2_data_dense_integers_equal_fp64(HF, B, C, CO, H, W):
    """Small integers everywhere: every partial sum is an integer below 2^24, so indexing, tails, parity classes and K splits show at every element."""
    assert _served(B, C, CO, H, W)
    gen = torch.Generator().manual_seed(B + C + CO + H + W + 1)
    pw, pg = X.draw((CO, C, 3, 3), 'int2', gen), X.draw((B, CO, _out(H), _out(W)), 'int2', gen)
    ref = _grad_x(KW, (B, C, H, W), pw.at(0).cuda().double(), pg.at(0).cuda().double())
    assert ref.abs().max().item() < 2**24
    x = torch.zeros((B, C, H, W), device='cuda')
    for scale, (ex, ew, eg) in X.SCALES.items():
        gx, _ = _grad_input(HF, x, pw.at(ew).cuda(), pg.at(eg).cuda())
        _same(f'stride 2 data gradient {(B, C, CO, H, W)} family dense scale {scale}', IDX_MAP[1:], gx, ref*2.0**(eg + ew))


# ---- gradients asked for; shapes the kernel turns down ----
def test_stride2_data_does_not_depend_on_the_weight_gradient(HF):
    """g_x is the same bits whether or not g_w is asked for; the gradient not asked for is None."""
    x, wt, gy = _case(2, 32, 64, 9, 14, seed=2)
    gx_only, gw_none = _grad_input(HF, x, wt, gy, need_w=False)
    gx_both, gw = _grad_input(HF, x, wt, gy, need_w=True)
    assert gw_none is None and gw is not None
    assert torch.equal(gx_only, gx_both)
    xf, wl = x.clone(), wt.clone().requires_grad_(True)
    HF.conv3x3_s2(xf, wl).backward(gy)
    assert xf.grad is None and torch.equal(wl.grad, gw)


@pytest.mark.parametrize('C,CO', [(8, 32), (16, 16)])
def test_stride2_data_unserved_shapes_fall_back(C, CO):
    """C = 8 / CO = 16: the size query says 0, the entry point returns SMD_E_UNSUPPORTED, and `conv3x3_s2` gives ATen's g_x under every route."""
    from slowtv_monodepth_amd import _lib, functional as HF
    from slowtv_monodepth_amd._device import call, _stream
    x, wt, gy = _case(2, C, CO, 9, 14, seed=3)
    assert not _served(2, C, CO, 9, 14)
    gx, ws = torch.empty_like(x), torch.empty(4096, device='cuda', dtype=torch.uint8)
    with pytest.raises(_lib.Unsupported):
        call('smd_conv3x3s2d_mfma_bwd_data', gy.data_ptr(), ws.data_ptr(), gx.data_ptr(), ws.data_ptr(), 4096, 2, C, CO, 9, 14, _stream())
    xr = x.clone().requires_grad_(True)
    TF.conv2d(xr, wt, **KW).backward(gy)
    try:
        for mode in ('auto', 'mfma', 'miopen'):
            HF.set_conv_route(mode)
            got, _ = _grad_input(HF, x, wt, gy)
            assert rel_to_max(got, xr.grad) < 1e-5, mode
            assert not [k for k in HF.conv_routes() if k[0] == 'data_t2']
    finally:
        HF.set_conv_route('auto')


# ---- guarded, poisoned buffers ----
@pytest.mark.parametrize('B,C,CO,H,W', [(2, 48, 64, 7, 13), (2, 256, 512, 12, 40)])
def test_stride2_data_in_guarded_buffers(HF, B, C, CO, H, W):
    """Operands, g_x, the packed weights and the K-split workspace each in the middle of a buffer of 0xFF bytes (an odd-sized shape with a partial channel
    tile; a K-split shape): every element of g_x is written and finite, equals the friendly run's bits, and no guard byte changes."""
    x, wt, gy = _case(B, C, CO, H, W, seed=5)
    assert _served(B, C, CO, H, W)
    friendly, _ = _grad_input(HF, x, wt, gy)
    arena = Arena()
    xg, wg, gg = (arena.guarded(t) for t in (x, wt, gy))
    xg.requires_grad_(True)
    with hostile(arena):
        HF.conv3x3_s2(xg, wg).backward(gg)
    assert_finite(xg.grad, 'g_x', IDX_MAP[1:])
    assert torch.equal(xg.grad, friendly)
    arena.check()
