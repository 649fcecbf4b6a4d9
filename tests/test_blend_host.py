"""The inference path on the host: `geometry.blend_stereo` / `blend.plain_flip_blend` against the REFERENCE's fixture (tests/golden/blend_stereo.npz) bit for
bit, the bound the GPU tests hold the kernel to (checked here on ATen's own fp32 result), the operator's argument checks, the C ABI's refusals, the predictors
on small fake networks, a checkpoint round trip through `BenchmarkPredictor.load_model`, and the `predict` entry point."""
import copy
import re

import numpy as np
import pytest
import torch
import yaml

from blend_inputs import BLEND_CASES, BLEND_PYRAMID, BLEND_RANGE, BLEND_SCALED, blend_case, blend_expected
from conftest import ROOT, load_golden
from exact_inputs import bit_checksum

EPS = 2.0**-24
NEW_SYMBOLS = ['smd_flip_blend_fwd', 'smd_flip_blend_bwd']


def blend_bound(l, r, scale=1.0):
    """The bound of the issue, per element: |out - ref| <= 8 * 2^-24 * max(|l|, |r|) [* k with the scaling].  At most eight fp32 roundings stand between the
    operands and `out` — two in m_mu = (1 - m_l) - m_r, one in l + r (halving is exact), three products, two sums — and each is at most 2^-24 of a value that
    max(|l|, |r|) bounds, because the three weights lie in [0, 1] and sum to 1; the ramp's bits are shared by both sides, so nothing else contributes.  The
    scaling multiplies everything by k = 1/min - 1/max.  (Its own two roundings are not in the issue's count; `test_aten_fp32_meets_the_bound...` checks below
    that ATen's fp32 result on the fixture inputs is inside the bound all the same.)"""
    return 8*EPS*scale*torch.maximum(l.abs(), r.abs()).double()


def scale_of(rng=BLEND_RANGE): return 1/rng[0] - 1/rng[1]


@pytest.fixture(scope='module')
def fixture():
    g = load_golden('blend_stereo')
    for k in range(len(BLEND_CASES)):
        assert sum(bit_checksum(t) for t in blend_case(k).values()) == int(g['chk'][k]), 'the seeded inputs are not the ones the fixture was made from'
    return g


# ------------------------------------------------------------------------------------------------- the operator on the CPU
@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
def test_blend_stereo_and_plain_flip_blend_reproduce_the_fixture_bit_for_bit(fixture, scaled):
    """Same torch expressions on the same CPU: outputs and both gradients are the reference's bits, through `geometry.blend_stereo` (right operand already flipped
    back) and through `plain_flip_blend` / `functional.flip_blend` (right operand as the network would return it for the mirrored image)."""
    from slowtv_monodepth_amd import functional as F, geometry as G
    from slowtv_monodepth_amd.blend import plain_flip_blend
    rng = dict(min_depth=BLEND_RANGE[0], max_depth=BLEND_RANGE[1]) if scaled else {}
    for k in (BLEND_SCALED if scaled else range(len(BLEND_CASES))):
        ins, want = blend_case(k), blend_expected(fixture, k, scaled)
        runs = {'blend_stereo': lambda l, r: (G.to_scaled(G.blend_stereo(l, r), *BLEND_RANGE)[0] if scaled else G.blend_stereo(l, r)),
                'plain_flip_blend': lambda l, r: plain_flip_blend(l, r.flip(-1), **rng), 'flip_blend': lambda l, r: F.flip_blend(l, r.flip(-1), **rng)}
        for name, run in runs.items():
            l, r = ins['l'].clone().requires_grad_(True), ins['r'].clone().requires_grad_(True)
            out = run(l, r)
            (out*ins['g']).sum().backward()
            for what, got, ref in zip(('out', 'grad_l', 'grad_r'), (out.detach(), l.grad, r.grad), want):
                assert got.dtype == torch.float32 and torch.equal(got, ref), f'case {k} {BLEND_CASES[k]} {name}: {what} differs from the reference'


def test_aten_fp32_meets_the_bound_against_fp64_on_the_fixture_inputs(fixture):
    """The yardstick of the GPU tests, derived in `blend_bound`, holds for ATen itself: the fixture's fp32 outputs and gradients against an fp64 evaluation of the
    same inputs with the same (fp32) ramp, without and with the scaling."""
    from slowtv_monodepth_amd.blend import plain_flip_blend
    for scaled in (False, True):
        rng = dict(min_depth=BLEND_RANGE[0], max_depth=BLEND_RANGE[1]) if scaled else {}
        for k in (BLEND_SCALED if scaled else range(len(BLEND_CASES))):
            ins, (out, gl, gr) = blend_case(k), blend_expected(fixture, k, scaled)
            l, r = ins['l'].double().requires_grad_(True), ins['r'].double().requires_grad_(True)
            o64 = plain_flip_blend(l, r, mirror=False, **rng)
            (o64*ins['g'].double()).sum().backward()
            ks = scale_of() if scaled else 1.0
            assert ((out.double() - o64.detach()).abs() <= blend_bound(ins['l'], ins['r'], ks)).all(), (k, scaled)
            for got, ref in ((gl, l.grad), (gr, r.grad)): assert ((got.double() - ref).abs() <= blend_bound(ins['g'], ins['g'], ks)).all(), (k, scaled)


def test_blend_stereo_takes_2d_and_3d_inputs_and_refuses_other_shapes():
    from slowtv_monodepth_amd import geometry as G
    ins = blend_case(BLEND_PYRAMID[0])
    l, r = ins['l'], ins['r']
    full = G.blend_stereo(l, r)
    assert torch.equal(G.blend_stereo(l[0, 0], r[0, 0]), full[0, 0]) and G.blend_stereo(l[0, 0], r[0, 0]).shape == (8, 24)
    assert torch.equal(G.blend_stereo(l[1], r[1]), full[1]) and G.blend_stereo(l[1], r[1]).shape == (1, 8, 24)
    with pytest.raises(ValueError, match=r'Non-matching shapes\. \(torch\.Size\(\[2, 1, 8, 24\]\) vs\. torch\.Size\(\[2, 1, 8, 23\]\)\)'): G.blend_stereo(l, r[..., :23])
    one = G.blend_stereo(l[..., :1], r[..., :1])                    # w = 1: the ramp is a single zero, the blend is the mean
    assert torch.equal(one, (l[..., :1] + r[..., :1])/2)
    assert G.blend_stereo(l.double(), r.double()).dtype == torch.float64 and 'blend_stereo' in G.__all__


def test_operator_is_reexported_and_validates_its_arguments():
    from slowtv_monodepth_amd import blend, functional as F
    assert F.flip_blend is blend.flip_blend and F.flip_blend_pyramid is blend.flip_blend_pyramid
    assert 'flip_blend' not in F.__all__ and 'flip_blend_pyramid' not in F.__all__      # (the hostile-memory case table is `__all__`; these operators' cases live in test_gpu_blend.py)
    l, r = torch.rand(2, 2, 3, 5), torch.rand(2, 2, 3, 5)
    with pytest.raises(ValueError, match=r'Min depth must be greater than 0\. \(0\)'): F.flip_blend(l, r, min_depth=0)
    with pytest.raises(ValueError, match=r'Min depth must be greater than 0\. \(-1\.5\)'): F.flip_blend(l, r, min_depth=-1.5, max_depth=None)
    with pytest.raises(ValueError, match=r'Max depth must be greater than min\. \(1 vs\. 2\)'): F.flip_blend(l, r, min_depth=2, max_depth=1)
    with pytest.raises(ValueError, match='Max depth'): F.flip_blend_pyramid({0: l}, {0: r}, min_depth=3, max_depth=2)
    with pytest.raises(ValueError, match='needs a min_depth'): F.flip_blend(l, r, max_depth=80)
    with pytest.raises(ValueError, match='Min depth'): F.flip_blend(None, None, min_depth=0)      # (raised before anything else is looked at)
    with pytest.raises(TypeError): F.flip_blend([1.0], r)
    with pytest.raises(ValueError, match='Non-matching shapes'): F.flip_blend(l, r[..., :4])
    with pytest.raises(ValueError): F.flip_blend(l[0], r[0])
    with pytest.raises(ValueError, match='keys'): F.flip_blend_pyramid({0: l}, {1: r})
    with pytest.raises(ValueError, match='share'): F.flip_blend_pyramid({0: l, 1: l[:1]}, {0: r, 1: r[:1]})
    # a maximum of 0 or None is "no maximum": the offset is 0
    assert torch.equal(F.flip_blend(l, r, min_depth=0.5, max_depth=0), F.flip_blend(l, r, min_depth=0.5)) and torch.equal(F.flip_blend(l, r, min_depth=0.5), 2.0*F.flip_blend(l, r) + 0)
    # the pyramid form on the CPU is the per-level plain sequence, in the dictionary's order
    ls, rs = {s: blend_case(k)['l'] for s, k in enumerate(BLEND_PYRAMID)}, {s: blend_case(k)['r'] for s, k in enumerate(BLEND_PYRAMID)}
    out = F.flip_blend_pyramid(ls, rs, min_depth=0.1, max_depth=100)
    assert list(out) == list(ls)
    for s in ls: assert torch.equal(out[s], blend.plain_flip_blend(ls[s], rs[s], min_depth=0.1, max_depth=100))
    assert blend.blend_ramp('cpu', 21) is blend.blend_ramp(torch.device('cpu'), 21) and blend.blend_ramp('cpu', 21)[1].item() == 0.0 and blend.blend_ramp('cpu', 21)[2].item() == 1.0


def test_header_and_prototypes_agree_on_the_new_symbols():
    from slowtv_monodepth_amd import _lib
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in the header'
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name)
    assert 'geometry.py:94-129' in header and 'geometry.py:63-76' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_blend.hip' in (ROOT/'slowtv_monodepth_amd'/'csrc'/'Makefile').read_text()
    assert 'getenv' not in (ROOT/'slowtv_monodepth_amd'/'csrc'/'smd_blend.hip').read_text()


def test_the_abi_refuses_bad_arguments_without_a_gpu():
    """Null pointers, empty levels, too many levels, unknown flags and a level of 2^31 elements are refused before anything is launched."""
    from slowtv_monodepth_amd import _lib
    p = 4096                                     # a pointer value that is never dereferenced: every call below is refused first
    arr = lambda n, v=p: _lib.ptr_array([v]*n)
    ints = _lib.int_array

    def fwd(S=2, hs=(3, 2), ws=(5, 3), planes=2, flags=3, ptrs=None):
        l, r, m, o = ptrs or (arr(S), arr(S), arr(S), arr(S))
        return _lib.call('smd_flip_blend_fwd', l, r, m, o, ints(hs), ints(ws), S, planes, flags, 1.0, 0.0, None)

    def bwd(S=2, hs=(3, 2), ws=(5, 3), planes=2, flags=3, ptrs=None):
        g, m, gl, gr = ptrs or (arr(S), arr(S), arr(S), arr(S))
        return _lib.call('smd_flip_blend_bwd', g, m, gl, gr, ints(hs), ints(ws), S, planes, flags, 1.0, None)
    for call in (fwd, bwd):
        with pytest.raises(ValueError, match='outside'): call(S=0, hs=(), ws=())
        with pytest.raises(ValueError, match='outside'): call(S=9, hs=(1,)*9, ws=(1,)*9)
        with pytest.raises(ValueError, match='invalid sizes'): call(hs=(3, 0))
        with pytest.raises(ValueError, match='invalid sizes'): call(ws=(5, -1))
        with pytest.raises(ValueError, match='invalid sizes'): call(planes=0)
        with pytest.raises(ValueError, match='invalid sizes'): call(flags=4)
        with pytest.raises(ValueError, match='2\\^31'): call(S=1, hs=(65536,), ws=(32768,), planes=1)
        with pytest.raises(ValueError, match='null'): call(ptrs=(arr(2), arr(2, None), arr(2), arr(2)))      # the ramps
        with pytest.raises(ValueError, match='null'): call(ptrs=(None, arr(2), arr(2), arr(2)))
    with pytest.raises(ValueError, match='null'): fwd(ptrs=(arr(2), arr(2), arr(2), _lib.ptr_array([p, None])))
    with pytest.raises(ValueError, match='nothing to compute'): bwd(ptrs=(arr(2), arr(2), None, None))
    with pytest.raises(ValueError, match='nothing to compute'): bwd(ptrs=(arr(2), arr(2), arr(2, None), None))


# ------------------------------------------------------------------------------------------------- predictors
class _Mean(torch.nn.Module):
    """disp = the mean over the channels: mirror-equivariant, net(flip(x)) == flip(net(x)) bit for bit."""
    def forward(self, x): return {'disp': {0: x.mean(1, keepdim=True)}}


class _Columns(torch.nn.Module):
    """disp[.., j] = j/(w-1) whatever the image: the prediction for the mirrored image is the same ramp, NOT mirrored."""
    def forward(self, x): return {'disp': {0: torch.linspace(0, 1, x.shape[-1], device=x.device).expand(x.shape[0], 1, x.shape[2], -1).contiguous()}}


class _Zero(torch.nn.Module):
    def forward(self, x): return {'disp': {0: torch.zeros_like(x[:, :1])}}


def _imgs(b=2, h=3, w=41, seed=5): return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(seed))


def test_predictor_registry_and_image_shapes():
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor, MonoDepthPredictor
    from slowtv_monodepth_amd.registry import PRED_REG
    assert PRED_REG['ours'] is BenchmarkPredictor and issubclass(BenchmarkPredictor, MonoDepthPredictor)
    with pytest.raises(TypeError): MonoDepthPredictor()                                  # abstract: load_model
    assert BenchmarkPredictor.get_img_shape('kitti') == (192, 640) and BenchmarkPredictor.get_img_shape('mapfree') == (512, 384)
    assert BenchmarkPredictor.get_img_shape('ddad') == (416, 640) and BenchmarkPredictor.get_img_shape('sintel') == (288, 640)
    assert len({BenchmarkPredictor.get_img_shape(t) for t in ('diode', 'nyud', 'tum')}) == 1
    with pytest.raises(KeyError): BenchmarkPredictor.get_img_shape('imagenet')
    assert MonoDepthPredictor.get_img_shape('kitti') is None


def test_forward_batch_blends_a_mirror_equivariant_net_onto_itself_and_a_column_ramp_to_its_closed_form():
    from slowtv_monodepth_amd.blend import blend_ramp
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor
    p, x = BenchmarkPredictor(), {'imgs': _imgs()}
    plain = p.forward_batch(x, _Mean(), 'cpu')
    assert torch.equal(plain, x['imgs'].mean(1, keepdim=True)) and not plain.requires_grad
    both = p.forward_batch(x, _Mean(), 'cpu', use_stereo_blend=True)
    assert ((both.double() - plain.double()).abs() <= blend_bound(plain, plain)).all()      # the weights sum to 1: l blended with itself is l
    w = x['imgs'].shape[-1]
    got = p.forward_batch(x, _Columns(), 'cpu', use_stereo_blend=True)
    c = torch.linspace(0, 1, w).double()
    ml = blend_ramp('cpu', w).double(); mr = ml.flip(-1)
    want = mr*c + ml*c.flip(-1) + (1 - ml - mr)*(c + c.flip(-1))/2
    assert got.shape == (2, 1, 3, w) and ((got.double() - want).abs() <= 8*EPS).all()
    assert torch.equal(p.forward_batch(x, _Columns(), 'cpu'), _Columns()(x['imgs'])['disp'][0])


def test_scaling_is_applied_iff_the_module_has_a_depth_range_and_an_own_postprocess_runs_behind_the_blend():
    from slowtv_monodepth_amd.blend import plain_flip_blend
    from slowtv_monodepth_amd.geometry import to_scaled
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor
    x = {'imgs': _imgs(seed=6)}
    raw = x['imgs'].mean(1, keepdim=True)
    blended = plain_flip_blend(raw, raw.flip(-1))        # the mirrored pass of a mirror-equivariant net returns flip(raw)
    p = BenchmarkPredictor()
    assert p.min_depth is None and p.max_depth is None
    assert torch.equal(p.forward_batch(x, _Mean(), 'cpu'), raw) and torch.equal(p.forward_batch(x, _Mean(), 'cpu', True), blended)
    for rng in ((0.5, 80), (None, 80), (0.5, None)):                       # any range switches the reference's LITERAL constants on (src/core/predictors.py:206)
        p.min_depth, p.max_depth = rng
        assert torch.equal(p.forward_batch(x, _Mean(), 'cpu'), to_scaled(raw, 0.1, 100)[0])
        assert torch.equal(p.forward_batch(x, _Mean(), 'cpu', True), to_scaled(blended, 0.1, 100)[0])

    class Squared(BenchmarkPredictor):
        def postprocess(self, pred, imgs): return pred**2
    q = Squared(); q.min_depth, q.max_depth = 0.1, 100
    assert torch.equal(q.forward_batch(x, _Mean(), 'cpu', True), blended**2)

    class Halved(BenchmarkPredictor):                                      # its own pre-process sees the flipped images, as in the reference
        def preprocess(self, imgs): return imgs*torch.linspace(0.5, 1, imgs.shape[-1])
    h = Halved()
    ramp = torch.linspace(0.5, 1, raw.shape[-1])
    l, r_raw = (x['imgs']*ramp).mean(1, keepdim=True), (x['imgs'].flip(-1)*ramp).mean(1, keepdim=True)
    assert torch.equal(h.forward_batch(x, _Mean(), 'cpu', True), plain_flip_blend(l, r_raw))


def test_call_concatenates_batches_and_refuses_an_all_zero_prediction():
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor
    p = BenchmarkPredictor()
    batches = [({'imgs': _imgs(seed=1)}, {}, {}), ({'imgs': _imgs(b=1, seed=2)},), {'imgs': _imgs(seed=3)}]
    preds = p(_Mean(), batches, device='cpu')
    assert isinstance(preds, np.ndarray) and preds.shape == (5, 3, 41) and preds.dtype == np.float32
    assert np.array_equal(preds[2], _imgs(b=1, seed=2).mean(1).numpy()[0])
    blended = p(_Mean(), batches, use_stereo_blend=True, device='cpu')
    assert blended.shape == (5, 3, 41) and np.abs(blended - preds).max() <= 8*EPS
    seen = []
    p.apply(_Mean(), batches[:2], lambda batch, pred, tag: seen.append((tag, tuple(pred.shape), pred.device.type)), False, 'cpu', 'cb')
    assert seen == [('cb', (2, 1, 3, 41), 'cpu'), ('cb', (1, 1, 3, 41), 'cpu')]
    with pytest.raises(ValueError, match='Found empty predictions at indices'): p(_Zero(), batches, device='cpu')


_CFG = yaml.safe_load((ROOT/'cfg'/'kitti_resnet18.yaml').read_text())


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    from slowtv_monodepth_amd.networks.checkpoint import reference_checkpoint
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    torch.manual_seed(3)
    m = MonoDepthModule(copy.deepcopy(_CFG))
    path = tmp_path_factory.mktemp('blend')/'last.ckpt'
    torch.save(reference_checkpoint(m, epoch=1, global_step=7), path)
    return m, path


def test_a_reference_checkpoint_round_trips_through_load_model(checkpoint):
    from slowtv_monodepth_amd.predictors import BenchmarkPredictor
    m, path = checkpoint
    p = BenchmarkPredictor()
    net = p.load_model(path)
    assert (p.min_depth, p.max_depth) == (0.1, 100) and not net.training and not any(q.requires_grad for q in net.parameters())
    x = _imgs(b=1, h=64, w=96, seed=9)
    with torch.no_grad(): want = m.nets['depth'].eval()(x)['disp'][0]
    assert torch.equal(p.forward(net, x), want)
    assert torch.equal(p.forward_batch({'imgs': x}, net, 'cpu'), p.postprocess(want, x))
    net2 = BenchmarkPredictor().load_model(path, [ROOT/'cfg'/'kitti_resnet18.yaml'])       # the cfg given instead of the carried one
    assert torch.equal(net2(x)['disp'][0], want)


def test_predict_writes_the_predictions_of_synthetic_batches(checkpoint, tmp_path, capsys):
    from slowtv_monodepth_amd import predict
    _, path = checkpoint
    out = tmp_path/'sub'/'preds.npz'
    predict.main(['--ckpt', str(path), '--stereo-blend', '--synthetic-data', '2', '--batch-size', '2', '--shape', '64', '96', '--device', 'cpu', '--out', str(out)])
    with np.load(out) as z: preds = z['preds']
    assert preds.shape == (4, 64, 96) and preds.dtype == np.float32 and np.isfinite(preds).all() and (preds >= 0.01).all() and (preds <= 10).all()
    assert 'preds (4, 64, 96)' in capsys.readouterr().out
    named = copy.deepcopy(_CFG); named['dataset'] = {'kitti_lmdb': {'split': 'eigen_zhou'}}
    cfg_file = tmp_path/'named.yaml'
    cfg_file.write_text(yaml.safe_dump(named))
    with pytest.raises(SystemExit, match=r"the cfg names dataset type\(s\) \['kitti_lmdb'\]: this package trains on synthetic triplets only \(datasets are out of scope\); pass --synthetic-data"):
        predict.main(['--ckpt', str(path), '--cfg', str(cfg_file), '--out', str(out)])


def test_forward_blended_on_the_cpu_is_two_passes_and_the_plain_blend():
    from slowtv_monodepth_amd.blend import plain_flip_blend
    from slowtv_monodepth_amd.networks.depth import DepthNet
    torch.manual_seed(4)
    net = DepthNet(enc_name='resnet18', pretrained=False).eval()
    with pytest.raises(NotImplementedError): DepthNet(enc_name='resnet18', pretrained=False, use_stereo_blend=True)      # (the constructor's refusal stands)
    x = _imgs(b=1, h=64, w=96, seed=11)
    with torch.no_grad(): a, b, out = net(x), net(x.flip(-1)), net.forward_blended(x)
    assert sorted(out) == sorted(a) and list(out['disp']) == list(a['disp'])
    for s in a['disp']: assert torch.equal(out['disp'][s], plain_flip_blend(a['disp'][s], b['disp'][s]))
    for f, g in zip(out['depth_feats'], a['depth_feats']): assert torch.equal(f, g)
