"""The DDVNet decoder on the host: registry, constructor errors and parameter names, the plain (ATen) path against what the REFERENCE's `DDVNetDecoder`
(src/networks/decoders/ddvnet.py) produced (tests/golden/make_golden_ddvnet.py), `ddv_head`'s surface, the C ABI's three new symbols, the example config."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
import yaml

from conftest import GOLDEN, ROOT, load_golden, rel_to_max
from ddvnet_inputs import DDV_CASES, DDVNET_BATCH, DDVNET_KW, NUM_BINS, bins, ddv_case, ddvnet_state
from exact_inputs import bit_checksum, decoder_feats, decoder_out_grads

FLOOR = 2e-6      # the library's bound for its fp32 operators, relative to the tensor's maximum


def build(device, **over):
    from slowtv_monodepth_amd.networks import checkpoint as ck
    from slowtv_monodepth_amd.networks.decoders import DDVNetDecoder
    dec = DDVNetDecoder(**{**DDVNET_KW, **over}).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in ck.to_reference_state_dict(holder).items()}
    state = ddvnet_state(shapes)
    ck.load_reference_state_dict(holder, state, strict=True)
    holder.to(device)
    return dec, holder, shapes, state


def ddv_aten(xp, weight, bias, out_ch=1):
    """The restatement the GPU tests compare `ddv_head` with (in fp64): pad already applied, conv2d + softmax + expectation per group of 128 bins."""
    logits = TF.conv2d(xp, weight, bias)
    return torch.cat([(l.softmax(1)*bins(xp.dtype).to(xp.device)).sum(1, keepdim=True) for l in logits.chunk(out_ch, 1)], 1)


def run_and_compare(device, out_tol, grad_tol, plain=False):
    """The decoder on the fixture's seeded state / features / output gradients against the reference's outputs, feature gradients and parameter gradients (in
    full where the fixture holds them, through their sum and sum of magnitudes everywhere).  -> (decoder, outputs)."""
    from slowtv_monodepth_amd.networks import checkpoint as ck
    g = load_golden('net_decoder_ddvnet_64x96')
    with np.load(GOLDEN/'net_decoder_ddvnet_64x96.npz') as z: keys, pkeys = [str(k) for k in z['meta_keys']], [str(k) for k in z['meta_param_keys']]
    dec, holder, shapes, state = build(device)
    assert sorted(shapes) == keys, 'the key bridge no longer yields the reference decoder\'s state-dict names'
    feats, gouts = decoder_feats(seed=98, b=DDVNET_BATCH), decoder_out_grads(seed=99, b=DDVNET_BATCH)
    assert sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32) == int(g['chk_state']) and sum(bit_checksum(f) for f in feats) == int(g['chk_feats']) \
        and sum(bit_checksum(v) for v in gouts.values()) == int(g['chk_gouts']), 'the seeded inputs are not the ones the fixture was made from'
    feats = [f.to(device).requires_grad_(True) for f in feats]
    if plain:
        with dec.plain_path(): out = dec(feats)
    else: out = dec(feats)
    sum((out[i]*gouts[i].to(device)).sum() for i in out).backward()
    for i in DDVNET_KW['out_sc']:
        d = (out[i].detach().cpu() - g[f'out_{i}']).abs().max().item()
        assert d <= out_tol, f'disparity at scale {i}: {d:.2e}'
    for j, f in enumerate(feats):
        r = rel_to_max(f.grad.cpu(), g[f'gfeat_{j}'])
        assert r <= grad_tol, f'gradient w.r.t. encoder feature {j}: {r:.2e}'
    grads = {k: v.grad for k, v in zip(ck.to_reference_state_dict(holder).keys(), holder.state_dict(keep_vars=True).values())}
    assert grads['decoders.disp.bins'] is None and 'decoders.disp.bins' not in pkeys
    stats = g['gparam_stats']
    for n, k in enumerate(pkeys):
        assert grads[k] is not None, f'{k} got no gradient'
        gk = grads[k].detach().double().cpu()
        if f'gparam_{k}' in g:
            r = rel_to_max(gk, g[f'gparam_{k}'].double())
            assert r <= grad_tol, f'gradient of {k}: {r:.2e}'
        assert abs(gk.abs().sum().item() - stats[n, 1].item()) <= 10*grad_tol*stats[n, 1].item(), f'sum of |gradient| of {k}'
        assert abs(gk.sum().item() - stats[n, 0].item()) <= 10*grad_tol*stats[n, 1].item(), f'sum of the gradient of {k}'
    return dec, out, g


def test_ddvnet_is_registered_and_refuses_what_the_reference_refuses():
    from slowtv_monodepth_amd import DEC_REG
    from slowtv_monodepth_amd.networks.decoders import DDVNetDecoder
    from slowtv_monodepth_amd.networks.depth import DepthNet
    assert DEC_REG['ddvnet'] is DDVNetDecoder and 'monodepth' in DEC_REG and 'cadepth' in DEC_REG
    with pytest.raises(KeyError, match='Invalid activation'): DDVNetDecoder(**{**DDVNET_KW, 'out_act': 'bogus'})
    with pytest.raises(KeyError, match='DDVNet is not compatible with mask prediction'):
        DepthNet(enc_name='resnet18', pretrained=False, dec_name='ddvnet', mask_name='uncertainty', num_ch_mask=2)
    with pytest.raises(KeyError, match='Invalid decoder'): DepthNet(enc_name='resnet18', pretrained=False, dec_name='hrdepth')
    dec = DDVNetDecoder(**{**DDVNET_KW, 'out_ch': 2, 'out_act': 'relu'})
    assert tuple(dec.bins.shape) == (1, NUM_BINS, 1, 1) and not dec.bins.requires_grad and torch.equal(dec.bins.detach(), bins())
    assert [dec.out[str(i)].out_channels for i in range(4)] == [2*NUM_BINS]*4 and [dec.out[str(i)].in_channels for i in range(4)] == [16, 32, 64, 128]
    assert dec.att.query_conv[0].in_channels == 512
    net = DepthNet(enc_name='resnet18', pretrained=False, dec_name='ddvnet')
    out = net(torch.rand(1, 3, 64, 96))
    assert set(out['disp']) == {0, 1, 2, 3} and out['disp'][0].shape == (1, 1, 64, 96) and out['disp'][3].shape == (1, 1, 8, 12)
    assert (out['disp'][0] >= 0).all() and (out['disp'][0] < 1).all()                  # an expectation over bins in [0, 127/128]


def test_plain_path_matches_the_reference_decoder_on_the_cpu():
    """The same ATen operators in the same order as the reference: held to the fixture's own yardstick rule — the larger of the library's floor and 4 x
    what the reference's fp32 run shows against its fp64 run (disparities in absolute terms: they are of order 0.5)."""
    g = load_golden('net_decoder_ddvnet_64x96')
    dec, out, g = run_and_compare('cpu', max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_out'])), max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_grad'])))
    assert sorted(dec.logits) == [0, 1, 2, 3]                                           # the plain path fills `logits`, as the reference does
    for i in range(4):
        assert tuple(dec.logits[i].shape) == tuple(int(v) for v in g[f'shape_logits_{i}']) == (DDVNET_BATCH, NUM_BINS, 64 >> i, 96 >> i)
        assert torch.equal(dec.expected_disparity(dec.logits[i]), out[i])


def test_checkpoint_keys_round_trip():
    from slowtv_monodepth_amd.networks import checkpoint as ck
    with np.load(GOLDEN/'net_decoder_ddvnet_64x96.npz') as z: keys = [str(k) for k in z['meta_keys']]
    dec, holder, shapes, state = build('cpu')
    assert sorted(shapes) == keys and 'decoders.disp.bins' in keys and 'decoders.disp.decoder.0.query_conv.0.weight' in keys
    assert ck._dec_kind(holder) == 'ddvnet'
    for k in shapes: assert ck.to_reference_key(ck.from_reference_key(k, dec.out_sc, 'ddvnet'), dec.out_sc, False, 'ddvnet') == k
    assert ck.from_reference_key('decoders.disp.decoder.11.weight', dec.out_sc, 'ddvnet') == 'decoders.disp.out.0.weight'
    assert ck.from_reference_key('decoders.disp.decoder.1.conv.bias', dec.out_sc, 'ddvnet') == 'decoders.disp.up0.4.0.bias'
    assert ck.from_reference_key('decoders.disp.decoder.0.key_conv.0.bias', dec.out_sc, 'ddvnet') == 'decoders.disp.att.key_conv.0.bias'
    back = ck.to_reference_state_dict(holder)
    assert list(back) and all(torch.equal(back[k], state[k]) for k in keys)
    # a Monodepth decoder's names are translated as before
    assert ck.from_reference_key('decoders.disp.decoder.10.weight') == 'decoders.disp.out.0.weight' and ck.from_reference_key('decoders.disp.decoder.3.conv.bias') == 'decoders.disp.up1.3.0.bias'


def test_head_fixture_through_the_aten_restatement():
    """`ddv_aten` (what the GPU tests hold `ddv_head` to, in fp64) reproduces the reference's conv3x3 + expected_disparity on the fixture's inputs."""
    g = load_golden('op_ddv_head')
    for k, (B, C, h, w, G, scale) in enumerate(DDV_CASES):
        x, weight, bias, gout = ddv_case(k)
        assert sum(bit_checksum(t) for t in (x, weight, bias, gout)) == int(g[f'chk_{k}']), 'the seeded inputs are not the ones the fixture was made from'
        leaves = [t.clone().requires_grad_(True) for t in (x, weight, bias)]
        out = ddv_aten(TF.pad(leaves[0], (1, 1, 1, 1), mode='reflect'), leaves[1], leaves[2], G)
        (out*gout).sum().backward()
        for what, mine in zip(('out', 'grad_x', 'grad_w', 'grad_b'), [out.detach()] + [t.grad for t in leaves]):
            assert rel_to_max(mine, g[f'{what}_{k}']) <= max(FLOOR, 4*float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])), f'case {k} {what}'
    assert float(g['meta_logit_span_3']) > 88


def test_ddv_head_is_reexported_and_validates_its_arguments():
    from slowtv_monodepth_amd import ddv_ops, functional as F
    assert F.ddv_head is ddv_ops.ddv_head and 'ddv_head' not in F.__all__     # (the hostile-memory case table is `__all__`; its case lives in test_gpu_ddvnet.py)
    xp, w, b = torch.rand(2, 16, 6, 7), torch.rand(NUM_BINS, 16, 3, 3), torch.rand(NUM_BINS)
    with pytest.raises(RuntimeError, match='GPU'): F.ddv_head(xp, w, b)
    with pytest.raises(TypeError): F.ddv_head([1.0], w, b)
    # shapes are refused before the device is looked at
    with pytest.raises(ValueError): F.ddv_head(xp[0], w, b)
    with pytest.raises(ValueError): F.ddv_head(xp[:0], w, b)
    with pytest.raises(ValueError): F.ddv_head(xp[:, :, :2], w, b)
    with pytest.raises(ValueError, match='multiple of 16'): F.ddv_head(torch.rand(2, 24, 6, 7), torch.rand(NUM_BINS, 24, 3, 3), b)
    with pytest.raises(ValueError): F.ddv_head(xp, w[:64], b)
    with pytest.raises(ValueError): F.ddv_head(xp, w, b[:5])
    with pytest.raises(ValueError): F.ddv_head(xp, w, b, out_ch=2)               # a weight of one group
    with pytest.raises(ValueError): F.ddv_head(xp, w, b, out_ch=0)
    with pytest.raises(ValueError): F.ddv_head(xp, w, b, out_ch=5)


def test_header_and_prototypes_agree_on_the_new_symbols():
    from slowtv_monodepth_amd import _lib
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    order = list(_lib.PROTOTYPES)
    names = ['smd_ddv_head_workspace_bytes', 'smd_ddv_head_fwd', 'smd_ddv_head_bwd_logits']
    for name in names:
        m = re.search(r'\b(size_t|int)\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        res, args = _lib.PROTOTYPES[name]
        assert (m.group(1) == 'size_t') == (res is _lib._sz)
        params = [p.strip() for p in m.group(2).split(',')]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = _lib._vp if '*' in p else _lib._sz if p.startswith('size_t') else _lib._i
            assert a is want, f'{name}: {p}'
        assert hasattr(_lib.lib, name)
    assert [order.index(n) for n in names] == list(range(order.index(names[0]), order.index(names[0]) + 3))
    assert _lib.lib.smd_abi_version() == 8
    ws = _lib.lib.smd_ddv_head_workspace_bytes
    assert ws(2, 16, 1, 5, 33) >= 2*NUM_BINS*4 and ws(2, 16, 2, 5, 33) >= 2*2*NUM_BINS*4
    assert ws(2, 24, 1, 5, 33) == 0 and ws(2, 16, 5, 5, 33) == 0 and ws(2, 16, 0, 5, 33) == 0 and ws(0, 16, 1, 5, 33) == 0 and ws(2, 16, 1, 0, 33) == 0


def test_trainer_builds_from_the_example_config():
    from slowtv_monodepth_amd.networks.decoders import DDVNetDecoder
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_ddvnet.yaml').read_text())
    assert cfg['net']['depth']['dec_name'] == 'ddvnet' and cfg['net']['depth']['pretrained'] is False
    m = MonoDepthModule(cfg)
    dec = m.nets['depth'].decoders['disp']
    assert isinstance(dec, DDVNetDecoder) and sorted(dec.out) == ['0', '1', '2', '3'] and dec.out['0'].out_channels == NUM_BINS
