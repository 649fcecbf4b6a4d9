"""The ResNet encoders' 3x3 stride-1 convolutions on the split-bf16 MFMA kernels with the zero padding done inside them (`conv3x3_same`,
`smd_conv3x3z_mfma_*`): output and both gradients against fp64 `conv2d(padding=1)`, repeatability, partial-gradient calls, and a whole ResNet-18
encoder on the kernels against the same encoder on MIOpen."""
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


def _case(B, C, CO, h, w, seed=0):
    gen = torch.Generator(device='cuda').manual_seed(seed + B*1000 + C*10 + CO + h + w)
    x = torch.randn(B, C, h, w, device='cuda', generator=gen)
    wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, CO, h, w, device='cuda', generator=gen)
    return x, wt, gy


# the four ResNet-18 stages at b = 2, then sizes off both tile shapes (64 x 4 and 32 x 8 pixels), the smallest image, b = 1, a K-split shape
SHAPES = [(2, 64, 64, 48, 160), (2, 128, 128, 24, 80), (2, 256, 256, 12, 40), (2, 512, 512, 6, 20),
          (2, 64, 64, 1, 1), (2, 64, 64, 5, 7), (2, 64, 64, 13, 100), (1, 128, 128, 13, 100), (1, 64, 64, 9, 33), (3, 32, 64, 7, 70), (1, 512, 512, 3, 5)]


@pytest.mark.parametrize('B,C,CO,h,w', SHAPES)
def test_conv3x3_same_against_fp64(HF, B, C, CO, h, w):
    """Output, input gradient and weight gradient within 2e-6 of the tensor's max of fp64 `conv2d(padding=1)` (the bound the padded forms are held to)."""
    import torch.nn.functional as TF
    x, wt, gy = _case(B, C, CO, h, w)
    R = [t.double().clone().requires_grad_(True) for t in (x, wt)]
    yr = TF.conv2d(R[0], R[1], padding=1); yr.backward(gy.double())
    L = [t.clone().requires_grad_(True) for t in (x, wt)]
    y = HF.conv3x3_same(L[0], L[1]); y.backward(gy)
    assert y.shape == (B, CO, h, w) and L[0].grad.shape == x.shape
    assert rel_to_max(y.double(), yr.detach()) <= 2e-6
    assert rel_to_max(L[0].grad.double(), R[0].grad) <= 2e-6
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6


@pytest.mark.parametrize('B,C,CO,h,w', [(2, 64, 64, 48, 160), (2, 512, 512, 6, 20), (1, 64, 64, 13, 100)])
def test_conv3x3_same_repeatable(HF, B, C, CO, h, w):
    x, wt, gy = _case(B, C, CO, h, w, seed=1)
    out = []
    for _ in range(2):
        L = [t.clone().requires_grad_(True) for t in (x, wt)]
        y = HF.conv3x3_same(L[0], L[1]); y.backward(gy)
        out.append((y, L[0].grad, L[1].grad))
    for a, b in zip(*out): assert torch.equal(a, b)


@pytest.mark.parametrize('which', ['input', 'weight'])
def test_conv3x3_same_one_gradient(HF, which):
    """Only the input's or only the weight's gradient asked for: the other stays None, the one asked for matches the call that computes both."""
    x, wt, gy = _case(2, 64, 64, 13, 100, seed=2)
    A = [t.clone().requires_grad_(True) for t in (x, wt)]
    HF.conv3x3_same(A[0], A[1]).backward(gy)
    xi, wi = x.clone().requires_grad_(which == 'input'), wt.clone().requires_grad_(which == 'weight')
    HF.conv3x3_same(xi, wi).backward(gy)
    if which == 'input':
        assert wi.grad is None and torch.equal(xi.grad, A[0].grad)
    else:
        assert xi.grad is None and torch.equal(wi.grad, A[1].grad)


def test_conv3x3_same_unserved_channels_fall_back(HF):
    """Channel counts the kernels do not tile (C % 16, CO % 32) go to MIOpen under the pinned route too, instead of raising."""
    import torch.nn.functional as TF
    x, wt, gy = _case(2, 24, 40, 9, 11, seed=3)
    L = [t.clone().requires_grad_(True) for t in (x, wt)]
    y = HF.conv3x3_same(L[0], L[1]); y.backward(gy)
    R = [t.clone().requires_grad_(True) for t in (x, wt)]
    yr = TF.conv2d(R[0], R[1], padding=1); yr.backward(gy)
    assert rel_to_max(y, yr) < 1e-5 and rel_to_max(L[0].grad, R[0].grad) < 1e-5 and rel_to_max(L[1].grad, R[1].grad) < 1e-5


def test_resnet18_encoder_mfma_equals_miopen(HF):
    """A whole ResNet-18 encoder (fused BatchNorm on), forward and backward, with every stride-1 3x3 convolution on the MFMA kernels against the same
    weights on MIOpen: the tolerances of the fused-BatchNorm encoder test (features 1e-4, gradients 2e-3)."""
    from slowtv_monodepth_amd.networks import encoders as E
    torch.manual_seed(1)
    net = E.create_encoder('resnet18', in_chans=3).cuda().train()
    x = torch.randn(4, 3, 64, 96, device='cuda')
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
