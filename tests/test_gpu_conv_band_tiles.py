"""Row-band pixel tiles of the split-bf16 MFMA convolution (`k_conv_mfma` with TC = 0: whole output rows of one sample, or several whole samples, per
block) and the weight gradient whose blocks walk several samples: output, input gradient and weight gradient against fp64 `conv2d`, for the coarse
shapes of cfg 2 in both operand geometries (zero-padded encoder layers; the decoder's padded form, whose data gradient is the OFF = 2 form) and for edge
shapes (bands across sample boundaries, pixel counts off 32, h = 1, w = 1 / 3 / 47 / 49, the K split on and off), plus bit-for-bit repeatability."""
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


def _case(B, C, CO, hi, wi, ho, wo, seed=0):
    gen = torch.Generator(device='cuda').manual_seed(seed + B*1000 + C*10 + CO + hi + wi)
    x = torch.randn(B, C, hi, wi, device='cuda', generator=gen)
    wt = torch.randn(CO, C, 3, 3, device='cuda', generator=gen)/(3*C**0.5)
    gy = torch.randn(B, CO, ho, wo, device='cuda', generator=gen)
    return x, wt, gy


def _check(run, ref, x, wt, gy):
    R = [t.double().clone().requires_grad_(True) for t in (x, wt)]
    yr = ref(R[0], R[1]); yr.backward(gy.double())
    L = [t.clone().requires_grad_(True) for t in (x, wt)]
    y = run(L[0], L[1]); y.backward(gy)
    assert y.shape == yr.shape and L[0].grad.shape == x.shape and L[1].grad.shape == wt.shape
    assert rel_to_max(y.double(), yr.detach()) <= 2e-6
    assert rel_to_max(L[0].grad.double(), R[0].grad) <= 2e-6
    assert rel_to_max(L[1].grad.double(), R[1].grad) <= 2e-6


# zero-padded "same" layers (C -> CO at h x w): cfg 2's layer3 / layer4 at both batch sizes, then edge shapes
SAME = [(12, 256, 256, 12, 40), (24, 256, 256, 12, 40), (12, 512, 512, 6, 20), (24, 512, 512, 6, 20),
        (12, 128, 128, 24, 80),                       # layer2 (three-row bands)
        (3, 64, 64, 5, 7),                            # bands of three whole samples, 105 pixels in all
        (5, 32, 64, 1, 49),                           # h = 1: five samples per band
        (2, 64, 64, 3, 1),                            # w = 1
        (2, 64, 32, 9, 3),                            # w = 3
        (2, 128, 64, 10, 47),                         # w = 47: five-row bands
        (2, 64, 64, 5, 49),                           # w = 49
        (1, 64, 64, 11, 49),                          # w = 49 where the rectangular tiles stay
        (1, 512, 64, 4, 20),                          # few pixels, long K: the K split on
        (5, 512, 512, 3, 5)]                          # uneven sample groups of the weight gradient


@pytest.mark.parametrize('B,C,CO,h,w', SAME)
def test_band_same_against_fp64(HF, B, C, CO, h, w):
    import torch.nn.functional as TF
    x, wt, gy = _case(B, C, CO, h, w, h, w)
    _check(HF.conv3x3_same, lambda a, b: TF.conv2d(a, b, padding=1), x, wt, gy)


# the padded form (input already padded to h + 2 x w + 2): the decoder's coarse levels, whose data gradient lands on the padded input (OFF = 2)
PADDED = [(12, 512, 256, 6, 20), (12, 512, 256, 12, 40), (12, 256, 128, 12, 40), (12, 256, 128, 24, 80),
          (3, 64, 64, 5, 7), (2, 64, 64, 1, 49), (2, 32, 64, 4, 1), (2, 128, 64, 10, 47)]


@pytest.mark.parametrize('B,C,CO,h,w', PADDED)
def test_band_padded_against_fp64(HF, B, C, CO, h, w):
    import torch.nn.functional as TF
    x, wt, gy = _case(B, C, CO, h + 2, w + 2, h, w, seed=5)
    _check(HF.conv3x3_mfma, TF.conv2d, x, wt, gy)


@pytest.mark.parametrize('B,C,CO,h,w,padded', [(12, 512, 512, 6, 20, False), (24, 256, 256, 12, 40, False), (3, 64, 64, 5, 7, False),
                                                (12, 512, 256, 12, 40, True)])
def test_band_repeatable(HF, B, C, CO, h, w, padded):
    p = 2 if padded else 0
    x, wt, gy = _case(B, C, CO, h + p, w + p, h, w, seed=1)
    run = HF.conv3x3_mfma if padded else HF.conv3x3_same
    out = []
    for _ in range(2):
        L = [t.clone().requires_grad_(True) for t in (x, wt)]
        y = run(L[0], L[1]); y.backward(gy)
        out.append((y, L[0].grad, L[1].grad))
    for a, b in zip(*out): assert torch.equal(a, b)
