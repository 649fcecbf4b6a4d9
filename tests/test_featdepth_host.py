"""FeatDepth training on the host: the plain regularisers (`regularizers/feature.py`) and `handlers.feat_smooth` against the REFERENCE's fixture
(tests/golden/op_featreg.npz), the registry keys and `get_loss`, `AutoencoderNet`'s keys and shapes and its decoder against the reference's decoder, the
checkpoint names, the trainer's refusals with and without the network, two CPU steps of cfg/kitti_featdepth.yaml, the new C symbols and the operator's refusals.

The error bound the GPU tests hold the kernel to is defined here (`featreg_bound`), the project's 4x rule: for every fixture case the reference formula is
evaluated in fp64 on the CPU; the kernel's loss / gradient may differ from that by at most FOUR times the error of the reference's own fp32 ATen result (the
fixture) against the same fp64 values, and never less than 2 ulp of the tensor's largest magnitude (the cases where ATen is exact).  The measured errors and the
resulting bounds are in profiles/featdepth_parity.txt."""
import copy
import functools

import pytest
import torch

from conftest import ROOT, load_golden
from exact_inputs import bit_checksum, decoder_feats
from featdepth_inputs import AUTOENC_DECODER_KW, FEAT_CASES, FEAT_WEIGHTS, autoenc_decoder_state, feat_case, feat_expected, handler_case
from oracle import view_synth_oracle as O
from oracle.backend import OracleBackend
from slowtv_monodepth_amd.trainer import MonoDepthModule

NEW_SYMBOLS = ['smd_feat_regs_workspace_bytes', 'smd_feat_regs_fwd', 'smd_feat_regs_bwd']
QUANTITIES = ('l_peaky', 'l_smooth', 'g_peaky', 'g_smooth', 'g_both')


@functools.lru_cache(maxsize=None)
def fixture(): return load_golden('op_featreg')


def run_plain(feat, img, edges: bool):
    """The plain regularisers on (feat, img) in their dtype -> dict of QUANTITIES (the gradients are feat.grad under each loss alone and under the weighted sum)."""
    from slowtv_monodepth_amd.regularizers import FeatPeakReg, FeatSmoothReg
    peaky, smooth = FeatPeakReg(edges), FeatSmoothReg(edges)
    out = {}
    for tag, wp, ws in (('peaky', 1.0, 0.0), ('smooth', 0.0, 1.0), ('both', *FEAT_WEIGHTS)):
        x = feat.clone().requires_grad_(True)
        lp, ls = peaky(x, img)[0], smooth(x, img)[0]
        (lp if tag == 'peaky' else ls if tag == 'smooth' else wp*lp + ws*ls).backward()
        out[f'g_{tag}'] = x.grad
    out['l_peaky'], out['l_smooth'] = lp.detach(), ls.detach()
    return out


@functools.lru_cache(maxsize=None)
def ref64(k: int, edges: bool):
    """The reference formula in fp64 on case k (computed once, shared by the tests)."""
    ins = feat_case(k)
    return run_plain(ins['feat'].double(), ins['img'].double(), edges)


def ulp_of(v: float) -> float:
    """The spacing of float32 at magnitude v."""
    return 0.0 if v == 0 else float(torch.tensor(v, dtype=torch.float64).abs().log2().floor().exp2())*2.0**-23


def featreg_bound(k: int, edges: bool, name: str):
    """-> (bound, the fp32 ATen result's own error): max(4 * max|fixture - fp64|, 2 ulp of max|fp64|)."""
    want, aten = ref64(k, edges)[name], feat_expected(fixture(), k, edges)[name]
    own = (aten.double() - want).abs().max().item()
    return max(4*own, 2*ulp_of(want.abs().max().item())), own


def test_fixture_inputs_are_the_ones_the_reference_ran_on():
    g = fixture()
    for k in range(len(FEAT_CASES)): assert sum(bit_checksum(t) for t in feat_case(k).values()) == int(g['chk'][k]), FEAT_CASES[k]
    ins = handler_case()
    assert sum(bit_checksum(t) for v in ins.values() for t in (v if isinstance(v, list) else [v])) == int(g['hd_chk'])


@pytest.mark.parametrize('edges', [False, True], ids=['plain', 'edges'])
@pytest.mark.parametrize('k', range(len(FEAT_CASES)), ids=[n for n, _ in FEAT_CASES])
def test_plain_regularisers_reproduce_the_fixture(k, edges):
    """Same ATen sequence as the reference: the losses and the three gradients of every case bit for bit; through `featreg.feat_regs` too (CPU tensors take the
    plain path)."""
    from slowtv_monodepth_amd.featreg import feat_regs
    ins, want = feat_case(k), feat_expected(fixture(), k, edges)
    got = run_plain(ins['feat'], ins['img'], edges)
    for n in QUANTITIES: assert torch.equal(got[n], want[n]), (n, (got[n] - want[n]).abs().max().item())
    lp, ls = feat_regs(ins['feat'], ins['img'], edges, edges)
    assert torch.equal(lp, want['l_peaky']) and torch.equal(ls, want['l_smooth'])
    assert feat_regs(ins['feat'], ins['img'], edges, edges, want_smooth=False)[1] is None and feat_regs(ins['feat'], ins['img'], edges, edges, want_peaky=False)[0] is None
    if FEAT_CASES[k][0] == 'const': assert all(float(got[n].abs().max()) == 0 for n in QUANTITIES), 'a constant map has no gradient anywhere'


def test_conventions_zero_padding_and_sign_of_zero():
    """`dxx[..., w-2]` is `|dx[w-2] - 0|`, the last column / row of every difference is 0, and `abs` passes no gradient at 0."""
    from slowtv_monodepth_amd.regularizers import compute_grad, compute_laplacian
    x = torch.tensor([[[[0., 1., 3.], [0., 1., 3.]]]])
    dx, dy = compute_grad(x)
    assert dx.tolist() == [[[[1., 2., 0.], [1., 2., 0.]]]] and float(dy.abs().max()) == 0
    dxx, dyy, dxy, dyx = compute_laplacian(x)
    assert dxx.tolist() == [[[[1., 2., 0.], [1., 2., 0.]]]], 'dxx[w-2] = |dx[w-2] - 0|'
    assert dxy[0, 0, 0].tolist() == [0., 0., 0.] and dxy[0, 0, 1].tolist() == [0., 0., 0.]
    q = feat_case([n for n, _ in FEAT_CASES].index('quant'))
    dx, _ = compute_grad(q['feat'])
    assert int((dx[..., :-1] == 0).sum()) > 0, 'the quantised case has exact zeros among its differences'


def test_registry_keys_and_get_loss():
    from slowtv_monodepth_amd import parsers, registry
    from slowtv_monodepth_amd.regularizers import FeatPeakReg, FeatSmoothReg
    registry.trigger_losses(); registry.trigger_nets()
    assert registry.LOSS_REG['feat_peaky'] is FeatPeakReg and registry.LOSS_REG['feat_smooth'] is FeatSmoothReg and 'autoencoder' in registry.NET_REG
    losses, weights = parsers.get_loss({'feat_peaky': {'weight': 1e-4, 'use_edges': True}, 'feat_smooth': {'weight': 2e-4}})
    assert losses['feat_peaky'].use_edges and not losses['feat_smooth'].use_edges and not losses['feat_smooth'].edge_aware
    assert float(weights['feat_smooth']) == pytest.approx(2e-4)
    from slowtv_monodepth_amd import functional as F
    assert not {'feat_regs', 'feat_regs_pyramid'} & set(F.__all__)


@pytest.mark.parametrize('tag', ['peaky', 'smooth'])
def test_handler_feat_smooth_reproduces_the_fixture(tag):
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.regularizers import FeatPeakReg, FeatSmoothReg
    g, ins = fixture(), handler_case()
    crit = FeatPeakReg(True) if tag == 'peaky' else FeatSmoothReg(True)
    feats, supp = [f.clone().requires_grad_(True) for f in ins['feats']], [f.clone().requires_grad_(True) for f in ins['supp_feats']]
    l, ld = handlers.feat_smooth(crit, feats, ins['imgs'], supp, ins['supp_imgs'])
    assert ld == {} and torch.equal(l.detach(), g[f'hd_{tag}_loss'])
    l.backward()
    for s in range(2): assert torch.equal(feats[s].grad, g[f'hd_{tag}_g_feat_{s}']) and torch.equal(supp[s].grad, g[f'hd_{tag}_g_supp_{s}'])
    assert handlers.feat_smooth_pair(FeatPeakReg(True), FeatSmoothReg(True), ins['feats'], ins['imgs'], ins['supp_feats'], ins['supp_imgs']) is None, 'CPU tensors: no fused pair'


def test_autoencoder_net_keys_shapes_and_checkpoint_names():
    from slowtv_monodepth_amd.networks import AutoencoderNet
    from slowtv_monodepth_amd.networks.checkpoint import load_reference_state_dict, to_reference_state_dict
    torch.manual_seed(0)
    net = AutoencoderNet(enc_name='resnet18', pretrained=False, dec_name='monodepth', out_scales=[0, 1, 2, 3]).eval()
    with pytest.raises(KeyError, match='Invalid decoder'): AutoencoderNet(dec_name='nope', pretrained=False)
    assert not net.decoder.use_skip and net.decoder.out_ch == 3 and AutoencoderNet(pretrained=False, out_scales=2).out_scales == [2]
    with torch.no_grad(): out = net(torch.rand(2, 3, 64, 96))
    assert sorted(out) == ['autoenc_feats', 'autoenc_imgs'] and list(out['autoenc_imgs']) == [0, 1, 2, 3]
    assert [tuple(f.shape) for f in out['autoenc_feats']] == [(2, c, 64//s, 96//s) for c, s in zip(net.num_ch_enc, net.enc_sc)]
    for s, v in out['autoenc_imgs'].items(): assert tuple(v.shape) == (2, 3, 64 >> s, 96 >> s) and 0 <= float(v.min()) and float(v.max()) <= 1
    # the reference's names: `encoder.*` in timm's layout, `decoder.decoder.N.*` (the ModuleList of its Monodepth decoder), with and without the trainer's prefix
    ref = to_reference_state_dict(net)
    assert all(k.startswith(('encoder.', 'decoder.decoder.')) for k in ref) and 'encoder.layer1.0.conv1.weight' in ref and 'decoder.decoder.0.conv.weight' in ref
    assert ref['decoder.decoder.10.weight'].shape == (3, 16, 3, 3) and all(k in fixture()['dec_keys'] for k in ref if k.startswith('decoder.'))
    torch.manual_seed(1)
    other = AutoencoderNet(enc_name='resnet18', pretrained=False).eval()
    load_reference_state_dict(other, ref)
    for (k1, v1), (k2, v2) in zip(net.state_dict().items(), other.state_dict().items()): assert k1 == k2 and torch.equal(v1, v2)
    holder = torch.nn.Module(); holder.nets = torch.nn.ModuleDict({'autoencoder': net})
    ref = to_reference_state_dict(holder)
    assert 'nets.autoencoder.encoder.layer2.0.downsample.0.weight' in ref and 'nets.autoencoder.decoder.decoder.13.bias' in ref


def test_autoencoder_decoder_matches_the_reference_decoder():
    """The registered Monodepth decoder as `AutoencoderNet` builds it (`use_skip=False, out_ch=3`) on the reference's recorded features and weights."""
    from slowtv_monodepth_amd.networks.checkpoint import load_reference_state_dict
    from slowtv_monodepth_amd.registry import DEC_REG, trigger_decoders
    trigger_decoders()
    g = fixture()
    holder = torch.nn.Module(); holder.decoder = DEC_REG['monodepth'](**AUTOENC_DECODER_KW)
    from slowtv_monodepth_amd.networks.checkpoint import to_reference_state_dict
    shapes = {k: tuple(v.shape) for k, v in to_reference_state_dict(holder).items()}
    state = autoenc_decoder_state(shapes)
    assert sum(bit_checksum(v) for v in state.values()) == int(g['dec_chk_state'])
    load_reference_state_dict(holder, state)
    feats = [f.requires_grad_(True) for f in decoder_feats()]
    out = holder.decoder(feats)
    sum(o.sum() for o in out.values()).backward()
    for i, o in out.items():
        want = g[f'dec_out_{i}']
        got = o.detach()[:, :, ::2, ::2] if i == 0 else o.detach()
        assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-6, (i, (got - want).abs().max().item())
    assert (feats[4].grad - g['dec_gfeat_4']).abs().max().item() <= 1e-5*g['dec_gfeat_4'].abs().max().item()
    assert all(f.grad is None for f in feats[:4]), 'without skips only the deepest feature reaches the decoder'


class _Backend(OracleBackend):
    """The CPU oracle with the two autoencoder handlers the example configuration adds (oracle/view_synth_oracle.py has both)."""
    def feat_recon(self, crit, synth, depths, masks, feats, supp_feats, Ts, Ks):
        loss, ld, _ = O.feat_recon(depths, feats[-4], supp_feats[-4], Ts.float(), Ks.float(), crit.loss_name, crit.use_min, crit.use_automask, aten=self.aten)
        return loss, ld

    def autoenc_recon(self, crit, preds, targets, supp_preds, supp_targets):
        return O.autoenc_recon(preds, targets, supp_preds, supp_targets, crit.loss_name, crit.use_min, aten=self.aten), {}


_NETS = {'depth': {'enc_name': 'resnet18', 'pretrained': False, 'dec_name': 'monodepth', 'out_scales': [0]}, 'pose': {'enc_name': 'resnet18', 'pretrained': False}}


def test_trainer_refuses_the_autoencoder_losses_without_the_network_and_takes_them_with_it():
    for k, kw in (('feat_peaky', {}), ('feat_smooth', {'use_edges': True}), ('feat_recon', {'loss_name': 'l2'}), ('autoenc_recon', {})):
        cfg = {'net': copy.deepcopy(_NETS), 'loss': {'img_recon': {'weight': 1}, k: {'weight': 1, **kw}}}
        with pytest.raises(NotImplementedError, match='autoencoder') as e: MonoDepthModule(copy.deepcopy(cfg), loss_backend=OracleBackend())
        assert f'loss "{k}" needs an `autoencoder` network' in str(e.value)
        cfg['net']['autoencoder'] = {'enc_name': 'resnet18', 'pretrained': False, 'out_scales': [0]}
        assert k in MonoDepthModule(cfg, loss_backend=OracleBackend()).losses
    bad = {'net': {**copy.deepcopy(_NETS), 'autoenc': {}}, 'loss': {'img_recon': {'weight': 1}}}
    with pytest.raises((KeyError, ValueError)): MonoDepthModule(bad, loss_backend=OracleBackend())      # an unknown net key is still refused


def test_two_cpu_steps_of_the_example_config(monkeypatch, tmp_path):
    """cfg/kitti_featdepth.yaml through `python -m slowtv_monodepth_amd.train`'s `main` on synthetic data with the CPU oracle backend: two steps, every `loss_*`
    finite, both feature regularisers served, the pair cache empty afterwards."""
    import slowtv_monodepth_amd.train as T
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd import io
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_featdepth.yaml')
    assert set(cfg['loss']) == {'img_recon', 'disp_smooth', 'feat_recon', 'autoenc_recon', 'feat_peaky', 'feat_smooth'} and 'autoencoder' in cfg['net']
    torch.manual_seed(3)
    m = MonoDepthModule(copy.deepcopy(cfg), loss_backend=_Backend())
    batch = make_batch(1, 64, 96, [-1, 1], seed=5, device=torch.device('cpu'))
    opt = m.configure_optimizers()['optimizer']
    for _ in range(2):
        loss, ld, fwd = m.step(tuple(dict(d) for d in batch))
        assert set(k for k in ld if k.startswith('loss_')) == {f'loss_{k}' for k in cfg['loss']}
        assert all(torch.isfinite(v).all() for k, v in ld.items() if k.startswith('loss_')) and torch.isfinite(loss)
        assert float(ld['loss_feat_peaky'].detach()) < 0 < float(ld['loss_feat_smooth'].detach()) and m._feat_pair is None
        assert [tuple(f.shape[:2]) for f in fwd['supp_autoenc_feats']] == [(2, 1)]*5 and tuple(fwd['supp_autoenc_imgs_up'][3].shape) == (2, 1, 3, 64, 96)
        loss.backward(); opt.step(); opt.zero_grad()
    monkeypatch.setattr(T, 'MonoDepthModule', lambda c: MonoDepthModule(c, loss_backend=_Backend()))    # (the product backend needs a GPU)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    T.main(['-c', str(ROOT/'cfg'/'kitti_featdepth.yaml'), '-n', 'featdepth', '-o', str(tmp_path), '--steps', '2', '--shape', '64', '96'])
    assert (tmp_path/'featdepth'/'000'/'last.ckpt').is_file()


def test_new_c_symbols_and_abi_version():
    from slowtv_monodepth_amd import _lib
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    for name in NEW_SYMBOLS: assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name) and name in header
    assert 'smooth.py:100-176' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_featreg.hip' in (ROOT/'slowtv_monodepth_amd'/'csrc'/'Makefile').read_text()


def test_operator_refusals():
    import ctypes as C
    from slowtv_monodepth_amd import _lib
    from slowtv_monodepth_amd.featreg import _FeatRegs, feat_regs, feat_regs_pyramid
    f, i = torch.rand(2, 3, 4, 6), torch.rand(2, 3, 4, 6)
    with pytest.raises(TypeError): feat_regs([1.0], i, False, False)
    with pytest.raises(ValueError, match=r'expected \(b,c,h,w\)'): feat_regs(f[0], i, False, False)
    with pytest.raises(ValueError, match='the image resized'): feat_regs(f, i[..., :5], False, False)
    with pytest.raises(ValueError, match='the image resized'): feat_regs(f, i[:, :2], False, False)
    with pytest.raises(ValueError, match='nothing to compute'): feat_regs(f, i, True, True, want_peaky=False, want_smooth=False)
    with pytest.raises(ValueError, match='Non-matching pyramids'): feat_regs_pyramid([f, f], [i], False, False)
    with pytest.raises(ValueError, match='batch size'): feat_regs_pyramid([f, f[:1]], [i, i[:1]], False, False)
    with pytest.raises(ValueError, match='must not require a gradient'): feat_regs(f, i.clone().requires_grad_(True), False, False)
    # what the kernel does not serve runs the plain regularisers: CPU tensors (above), another dtype, an empty tensor
    lp, ls = feat_regs(f.double(), i.double(), True, True)
    assert lp.dtype == torch.float64 and ls.dtype == torch.float64
    assert all(torch.isnan(v) for v in feat_regs(f[:0], i[:0], False, False))
    # the Function itself refuses what `_check` refuses, and the C entry points their arguments, before anything is launched
    with pytest.raises(RuntimeError, match='must live on the GPU'): _FeatRegs.apply(0xc, 1, f, i)
    ints = lambda *v: (C.c_int*len(v))(*v)
    one = (C.c_void_p*1)(16)
    assert _lib.lib.smd_feat_regs_workspace_bytes(ints(3), ints(4), ints(6), 1, 2) >= 16
    assert _lib.lib.smd_feat_regs_workspace_bytes(ints(3), ints(0), ints(6), 1, 2) == 0 and _lib.lib.smd_feat_regs_workspace_bytes(ints(1 << 20), ints(1 << 10), ints(4), 1, 1) == 0
    for bad in (dict(S=0), dict(S=9), dict(B=0), dict(flags=0x3), dict(flags=0x1c), dict(h=0)):
        kw = dict(S=1, B=2, flags=0xc, h=4); kw.update(bad)
        with pytest.raises(ValueError): _lib.call('smd_feat_regs_fwd', one, one, ints(3), ints(kw['h']), ints(6), kw['S'], kw['B'], kw['flags'], 16, 16, 16, 1 << 20, None)
    with pytest.raises(ValueError, match='null pointer'): _lib.call('smd_feat_regs_fwd', one, one, ints(3), ints(4), ints(6), 1, 2, 0xc, None, 16, 16, 1 << 20, None)
    with pytest.raises(_lib.HotpathError, match='workspace too small'): _lib.call('smd_feat_regs_fwd', one, one, ints(3), ints(4), ints(6), 1, 2, 0xc, 16, 16, 16, 8, None)
    with pytest.raises(ValueError, match='nothing to compute'): _lib.call('smd_feat_regs_bwd', one, one, None, None, one, ints(3), ints(4), ints(6), 1, 2, 0xc, None)
    with pytest.raises(ValueError, match='not computed'): _lib.call('smd_feat_regs_bwd', one, one, 16, None, one, ints(3), ints(4), ints(6), 1, 2, 0x8, None)
