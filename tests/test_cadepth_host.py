"""The CADepth decoder on the host: registry and parameter names, the plain (ATen) path against what the REFERENCE's `CaDepthDecoder`, `StructurePerception`
and `DetailEmphasis` (src/networks/decoders/cadepth.py) produced (tests/golden/make_golden_cadepth.py), the new operators' surface, the example config."""
import numpy as np
import pytest
import torch
import yaml

from cadepth_inputs import CADEPTH_BATCH, CADEPTH_KW, cadepth_state, gfeat_sample, gfeat_stats, sp_inputs, sp_out_grads
from conftest import GOLDEN, ROOT, load_golden, rel_to_max
from exact_inputs import bit_checksum, decoder_feats, decoder_out_grads

ABSORBED = '.conv.0.bias'     # the bias of a convolution that feeds a training-mode BatchNorm: zero gradient in exact arithmetic, rounding noise in every run


def build(device, **over):
    from slowtv_monodepth_amd.networks import checkpoint as ck
    from slowtv_monodepth_amd.networks.decoders import CaDepthDecoder
    dec = CaDepthDecoder(**{**CADEPTH_KW, **over}).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in ck.to_reference_state_dict(holder).items()}
    state = cadepth_state(shapes)
    ck.load_reference_state_dict(holder, state, strict=True)
    holder.to(device)
    return dec, holder, shapes, state


def run_and_compare(device, out_tol, grad_tol, stat_tol=1e-5):
    """The decoder in train mode on the fixture's seeded state / features / output gradients (two samples: the BatchNorm statistics cross the batch) against
    the reference's outputs, feature and parameter gradients (as tests/test_decoder_golden.py: run_and_compare) and the BatchNorm buffers it left.  The
    gradient w.r.t. the largest feature is recorded on every second channel; all its channels are held through their per-sample sums, as the large parameter
    gradients are."""
    from slowtv_monodepth_amd.networks import checkpoint as ck
    g = load_golden('net_decoder_cadepth_64x96')
    with np.load(GOLDEN/'net_decoder_cadepth_64x96.npz') as z: keys, pkeys = [str(k) for k in z['meta_keys']], [str(k) for k in z['meta_param_keys']]
    dec, holder, shapes, state = build(device)
    assert sorted(shapes) == keys, 'the key bridge no longer yields the reference decoder\'s state-dict names'
    feats, gouts = decoder_feats(seed=96, b=CADEPTH_BATCH), decoder_out_grads(seed=97, b=CADEPTH_BATCH)
    assert sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32) == int(g['chk_state']) and sum(bit_checksum(f) for f in feats) == int(g['chk_feats']) \
        and sum(bit_checksum(v) for v in gouts.values()) == int(g['chk_gouts']), 'the seeded inputs are not the ones the fixture was made from'
    feats = [f.to(device).requires_grad_(True) for f in feats]
    out = dec(feats)
    sum((out[i]*gouts[i].to(device)).sum() for i in out).backward()
    for i in CADEPTH_KW['out_sc']:
        d = (out[i].detach().cpu() - g[f'out_{i}']).abs().max().item()
        assert d <= out_tol, f'disparity at scale {i}: {d:.2e}'
    for j, f in enumerate(feats):
        r = rel_to_max(gfeat_sample(j, f.grad.cpu()), g[f'gfeat_{j}'])
        assert r <= grad_tol, f'gradient w.r.t. encoder feature {j}: {r:.2e}'
        if f'gfeat_{j}_stats' in g:
            mine, ref = gfeat_stats(f.grad.cpu()), g[f'gfeat_{j}_stats']
            assert mine.shape == ref.shape and ((mine - ref).abs().amax(-1) <= 10*grad_tol*ref[..., 1]).all(), f'per-channel sums of the gradient w.r.t. encoder feature {j}'
    ref_sd = ck.to_reference_state_dict(holder)
    grads = {k: v.grad for k, v in zip(ref_sd.keys(), holder.state_dict(keep_vars=True).values())}
    stats = g['gparam_stats']
    for n, k in enumerate(pkeys):
        assert grads[k] is not None, f'{k} got no gradient'
        gk = grads[k].detach().double().cpu()
        if k.endswith(ABSORBED):      # no yardstick in the fixture (noise there too): held to zero at the scale of the same convolution's weight gradient
            wscale = grads[k[:-len('bias')] + 'weight'].abs().max().item()
            assert gk.abs().max().item() <= grad_tol*wscale, f'gradient of {k} (zero in exact arithmetic): {gk.abs().max().item():.2e} vs weight gradients of {wscale:.2e}'
            continue
        if f'gparam_{k}' in g:
            r = rel_to_max(gk, g[f'gparam_{k}'].double())
            assert r <= grad_tol, f'gradient of {k}: {r:.2e}'
        assert abs(gk.abs().sum().item() - stats[n, 1].item()) <= 10*grad_tol*stats[n, 1].item(), f'sum of |gradient| of {k}'
        assert abs(gk.sum().item() - stats[n, 0].item()) <= 10*grad_tol*stats[n, 1].item(), f'sum of the gradient of {k}'
    for k, v in ref_sd.items():          # running statistics and batch counters after the step
        if f'buf_{k}' not in g: continue
        ref = g[f'buf_{k}']
        if ref.dtype == torch.int64: assert int(v) == int(ref), k
        else: assert rel_to_max(v.detach().cpu(), ref) <= stat_tol, f'{k}: {rel_to_max(v.detach().cpu(), ref):.2e}'
    return out


def test_cadepth_is_registered_with_the_reference_parameter_names():
    from slowtv_monodepth_amd import DEC_REG
    from slowtv_monodepth_amd.networks import checkpoint as ck
    from slowtv_monodepth_amd.networks.decoders import CaDepthDecoder
    assert DEC_REG['cadepth'] is CaDepthDecoder and 'monodepth' in DEC_REG
    with np.load(GOLDEN/'net_decoder_cadepth_64x96.npz') as z: keys = [str(k) for k in z['meta_keys']]
    dec, holder, shapes, state = build('cpu')
    assert sorted(shapes) == keys
    for k in shapes: assert ck.to_reference_key(ck.from_reference_key(k, dec.out_sc, 'cadepth'), dec.out_sc, False, 'cadepth') == k
    # a Monodepth decoder's names are translated as before
    assert ck.from_reference_key('decoders.disp.decoder.10.weight') == 'decoders.disp.out.0.weight' and ck.from_reference_key('decoders.disp.decoder.3.conv.bias') == 'decoders.disp.up1.3.0.bias'
    with pytest.raises(KeyError): CaDepthDecoder(**{**CADEPTH_KW, 'out_act': 'bogus'})


def test_depthnet_builds_disparity_and_mask_decoders_from_the_registry_key():
    from slowtv_monodepth_amd.networks.depth import DepthNet
    net = DepthNet(enc_name='resnet18', pretrained=False, dec_name='cadepth', mask_name='uncertainty', num_ch_mask=2)
    out = net(torch.rand(1, 3, 64, 96))
    assert set(out['disp']) == set(out['mask']) == {0, 1, 2, 3}
    assert out['disp'][0].shape == (1, 1, 64, 96) and out['mask'][1].shape == (1, 2, 32, 48) and (out['mask'][0] >= 0).all()
    with pytest.raises(KeyError, match='Invalid decoder'): DepthNet(enc_name='resnet18', pretrained=False, dec_name='hrdepth')


def test_plain_path_matches_the_reference_decoder_on_the_cpu():
    """Bounds: those of test_decoder_golden.py::test_decoder_matches_the_reference_decoder_on_the_cpu (the same ATen operators in the same order)."""
    run_and_compare('cpu', 1e-6, 1e-5)


def sp_aten(x):
    b, c, h, w = x.shape
    v = x.view(b, c, -1)
    a = v @ v.transpose(1, 2)
    return x + (torch.softmax(a.amax(-1, keepdim=True) - a, -1) @ v).view_as(x)


def se_aten(x, w1, b1, w2, b2):
    mu = x.mean((2, 3))
    a = torch.sigmoid(torch.relu(mu @ w1.T + b1) @ w2.T + b2)
    return x + x*a[:, :, None, None]


def test_operator_fixtures_through_aten_restatements():
    """`sp_aten` / `se_aten` are what the GPU tests compare the kernels with (in fp64): here they, and the decoder's own plain forms, reproduce the reference."""
    from slowtv_monodepth_amd.networks.decoders import CaDepthDecoder, DetailEmphasis
    g = load_golden('op_structure_perception')
    for k, (x, go) in enumerate(zip(sp_inputs(), sp_out_grads())):
        assert torch.equal(x, g[f'in_x_{k}']) and torch.equal(go, g[f'gout_{k}'])
        for fn in (sp_aten, CaDepthDecoder.structure_perception):
            leaf = x.clone().requires_grad_(True)
            out = fn(leaf)
            (out*go).sum().backward()
            assert rel_to_max(out.detach(), g[f'out_{k}']) <= max(2e-6, 4*float(g[f'meta_ref_fp32_vs_fp64_out_{k}']))
            assert rel_to_max(leaf.grad, g[f'grad_x_{k}']) <= max(2e-6, 4*float(g[f'meta_ref_fp32_vs_fp64_grad_{k}']))
    g = load_golden('op_detail_emphasis')
    with np.load(GOLDEN/'op_detail_emphasis.npz') as z: keys = [str(k) for k in z['meta_keys']]
    de = DetailEmphasis(12).train()
    assert sorted(de.state_dict()) == keys
    de.load_state_dict({k: g[f'in_state_{k}'] for k in keys}, strict=True)
    x = g['in_x'].clone().requires_grad_(True)
    out = de(x)
    (out*g['gout']).sum().backward()
    assert rel_to_max(out.detach(), g['out']) <= 1e-6 and rel_to_max(x.grad, g['grad_x']) <= 1e-5
    for k, p in de.named_parameters():
        if k != 'conv.0.bias': assert rel_to_max(p.grad, g[f'gparam_{k}']) <= 1e-5, k
    for k, b in de.named_buffers(): assert rel_to_max(b.double(), g[f'buf_{k}'].double()) <= 1e-6, k
    # the gate alone: conv + BN + ReLU by the module, then the restatement
    y = de.conv(g['in_x'])
    ref = y + y*de.att(y)
    assert rel_to_max(se_aten(y, de.att[1].weight.view(12, 12), de.att[1].bias, de.att[3].weight.view(12, 12), de.att[3].bias), ref) <= 1e-6


def test_functional_reexports_the_attention_operators():
    from slowtv_monodepth_amd import attention_ops, functional as F
    assert F.channel_attention is attention_ops.channel_attention and F.se_gate is attention_ops.se_gate
    assert 'channel_attention' not in F.__all__ and 'se_gate' not in F.__all__      # (the hostile-memory case table is `__all__`; their cases live in test_gpu_cadepth.py)


def test_operators_refuse_cpu_tensors_and_mismatched_shapes():
    from slowtv_monodepth_amd import functional as F
    x, w, b = torch.rand(2, 6, 3, 4), torch.rand(6, 6), torch.rand(6)
    with pytest.raises(RuntimeError, match='GPU'): F.channel_attention(x)
    with pytest.raises(RuntimeError, match='GPU'): F.se_gate(x, w, b, w, b)
    with pytest.raises(TypeError): F.channel_attention([1.0])
    # shapes are refused before the device is looked at
    with pytest.raises(ValueError): F.channel_attention(x[0])
    with pytest.raises(ValueError): F.channel_attention(x[:0])
    with pytest.raises(ValueError): F.se_gate(x[0], w, b, w, b)
    with pytest.raises(ValueError): F.se_gate(x, w[:5], b, w, b)
    with pytest.raises(ValueError): F.se_gate(x, w, b[:5], w, b)
    with pytest.raises(ValueError): F.se_gate(x, w, b, torch.rand(6, 6, 3, 3), b)
    with pytest.raises(ValueError): F.se_gate(x, w, b, w.view(6, 6, 1, 1), torch.rand(7))


def test_trainer_builds_from_the_example_config():
    from slowtv_monodepth_amd.networks.decoders import CaDepthDecoder
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_cadepth.yaml').read_text())
    assert cfg['net']['depth']['dec_name'] == 'cadepth' and cfg['net']['depth']['pretrained'] is False
    m = MonoDepthModule(cfg)
    dec = m.nets['depth'].decoders['disp']
    assert isinstance(dec, CaDepthDecoder) and sorted(dec.de) == ['0', '1', '2', '3', '4']
    assert [dec.de[str(i)].conv[0].in_channels for i in range(5)] == [16, 96, 128, 256, 512]
