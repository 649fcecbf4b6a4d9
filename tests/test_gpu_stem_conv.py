"""The ResNet stem, `conv2d(x, w (64,C,7,7), stride=2, padding=3)`, on the split-bf16 MFMA kernels (`conv7x7s2_stem`, `smd_conv7x7s2_*`): output and weight
gradient against fp64 `conv2d`, repeatability, partial-gradient calls, the fall-back for shapes the kernels do not serve, and a whole ResNet-18 encoder on
the kernels against the same encoder on MIOpen."""
import pytest
import torch

from conftest import rel_to_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def HF():
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


def _case(B, C, H, W, CO=64, seed=0):
    gen = torch.Generator(device='cuda').manual_seed(seed + B*1000 + C*10 + H + W)
    x = torch.randn(B, C, H, W, device='cuda', generator=gen)
    wt = torch.randn(CO, C, 7, 7, device='cuda', generator=gen)/(7*C**0.5)
    gy = torch.randn(B, CO, (H - 1)//2 + 1, (W - 1)//2 + 1, device='cuda', generator=gen)
    return x, wt, gy


def _served(HF, B, C, H, W, CO=64):
    from slowtv_monodepth_amd import _lib
    return _lib.lib.smd_conv7x7s2_workspace_bytes(B, C, CO, H, W) > 0


def _against_fp64(HF, B, C, H, W):
    import torch.nn.functional as TF
    x, wt, gy = _case(B, C, H, W)
    assert _served(HF, B, C, H, W)
    wr = wt.double().clone().requires_grad_(True)
    yr = TF.conv2d(x.double(), wr, stride=2, padding=3); yr.backward(gy.double())
    wl = wt.clone().requires_grad_(True)
    y = HF.conv7x7s2_stem(x, wl); y.backward(gy)
    e_y, e_w = rel_to_max(y.double(), yr.detach()), rel_to_max(wl.grad.double(), wr.grad)
    print(f'stem B={B} C={C} {H}x{W}: output {e_y:.3g}, weight gradient {e_w:.3g} of the maximum')
    assert y.shape == yr.shape
    assert e_y <= 2e-6
    assert e_w <= 2e-6


# C = 3 and 6 at the cfg 2 image and a small one with b = 2; odd and tiny sizes; b = 1 and b = 3
SHAPES = [(2, 3, 192, 640), (2, 6, 192, 640), (2, 3, 96, 128), (2, 6, 96, 128),
          (2, 3, 1, 1), (2, 6, 1, 1), (2, 3, 5, 7), (2, 6, 5, 7), (2, 3, 13, 101), (2, 6, 13, 101), (2, 3, 37, 64), (2, 6, 37, 64),
          (1, 3, 37, 64), (1, 6, 13, 101), (3, 3, 13, 101), (3, 6, 37, 64)]


@pytest.mark.parametrize('B,C,H,W', SHAPES)
def test_stem_against_fp64(HF, B, C, H, W):
    """Output and weight gradient within 2e-6 of the tensor's max of fp64 `conv2d(stride=2, padding=3)` (the bound of every split-bf16 kernel here)."""
    _against_fp64(HF, B, C, H, W)


@pytest.mark.parametrize('B,C', [(12, 3), (24, 6)])
def test_stem_full_size_against_fp64(HF, B, C):
    """The cfg 2 shapes (192 x 640; depth net b = 12, pose net b = 24), where the weight gradient's K (368 640 / 737 280 pixels) is longest."""
    _against_fp64(HF, B, C, 192, 640)


@pytest.mark.parametrize('B,C,H,W', [(2, 3, 192, 640), (2, 6, 96, 128), (3, 6, 37, 64)])
def test_stem_repeatable(HF, B, C, H, W):
    x, wt, gy = _case(B, C, H, W, seed=1)
    out = []
    for _ in range(2):
        wl = wt.clone().requires_grad_(True)
        y = HF.conv7x7s2_stem(x, wl); y.backward(gy)
        out.append((y, wl.grad))
    for a, b in zip(*out): assert torch.equal(a, b)


@pytest.mark.parametrize('which', ['weight', 'input', 'both'])
def test_stem_gradients_asked_for(HF, which):
    """The gradient not asked for stays None; the weight gradient does not depend on whether the input's is asked for, and the input's (ATen's) is `conv2d`'s."""
    import torch.nn.functional as TF
    x, wt, gy = _case(2, 3, 37, 64, seed=2)
    wa = wt.clone().requires_grad_(True)
    HF.conv7x7s2_stem(x, wa).backward(gy)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    TF.conv2d(xr, wr, stride=2, padding=3).backward(gy)
    xi, wi = x.clone().requires_grad_(which != 'weight'), wt.clone().requires_grad_(which != 'input')
    HF.conv7x7s2_stem(xi, wi).backward(gy)
    if which == 'weight': assert xi.grad is None
    else: assert rel_to_max(xi.grad, xr.grad) < 1e-5
    if which == 'input': assert wi.grad is None
    else: assert torch.equal(wi.grad, wa.grad)


@pytest.mark.parametrize('C,CO', [(4, 64), (3, 32)])
def test_stem_unserved_shapes_fall_back(HF, C, CO):
    """Shapes the kernels do not serve (C = 4, CO != 64) go to MIOpen under the pinned route too, instead of raising."""
    import torch.nn.functional as TF
    x, wt, gy = _case(2, C, 21, 30, CO=CO, seed=3)
    assert not _served(HF, 2, C, 21, 30, CO)
    wl = wt.clone().requires_grad_(True)
    y = HF.conv7x7s2_stem(x, wl); y.backward(gy)
    wr = wt.clone().requires_grad_(True)
    yr = TF.conv2d(x, wr, stride=2, padding=3); yr.backward(gy)
    assert rel_to_max(y, yr) < 1e-5 and rel_to_max(wl.grad, wr.grad) < 1e-5


@pytest.mark.parametrize('in_chans', [3, 6])
def test_resnet18_encoder_stem_mfma_equals_miopen(HF, in_chans):
    """A whole ResNet-18 encoder (fused BatchNorm on), forward and backward, route `mfma` (stem and stride-1 3x3 layers on the kernels) against route
    `miopen` on the same weights: the tolerances of `test_resnet18_encoder_mfma_equals_miopen` (features 1e-4, gradients 2e-3 of the maximum)."""
    from slowtv_monodepth_amd.networks import encoders as E
    torch.manual_seed(1)
    net = E.create_encoder('resnet18', in_chans=in_chans).cuda().train()
    x = torch.randn(4, in_chans, 64, 96, device='cuda')
    res = []
    try:
        for mode in ('mfma', 'miopen'):
            HF.set_conv_route(mode)
            net.zero_grad()
            state = {k: v.clone() for k, v in net.state_dict().items()}
            feats = net(x)
            sum((f*f).mean() for f in feats).backward()
            res.append(([f.detach() for f in feats], [p.grad.clone() for p in net.parameters()]))
            net.load_state_dict(state)
    finally:
        HF.set_conv_route('mfma')
    for a, b in zip(res[0][0], res[1][0]): assert rel_to_max(a, b) < 1e-4
    for a, b in zip(res[0][1], res[1][1]): assert rel_to_max(a, b) < 2e-3
