"""The SuperDepth decoder on the host: registry, constructor and parameter names, `SubPixelConv`'s initialisation, the plain (ATen) path against what the
REFERENCE's `SuperdepthDecoder` (src/networks/decoders/superdepth.py) produced (tests/golden/make_golden_superdepth.py), the checkpoint bridge, the surface of
`subpixel_conv`, the C ABI's three new symbols and their refusals, the example config."""
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT, load_golden, rel_to_max
from exact_inputs import bit_checksum, decoder_feats
from superdepth_inputs import (SUBPIXEL_CASES, SUBPIXEL_NAMES, SUBPIXEL_SATURATED, SUPERDEPTH_BATCH, SUPERDEPTH_KW, subpixel_aten, subpixel_case, superdepth_out_grads,
                               superdepth_state)
from test_ddvnet_host import FLOOR

NEW_SYMBOLS = ['smd_subpixel_workspace_bytes', 'smd_subpixel_fwd', 'smd_subpixel_bwd']
ORDER = [f'upconv_{i}_{j}' for i in range(4, -1, -1) for j in (0, 1)] + [f'outconv_{k}' for k in range(4)]      # the reference's `decoder` ModuleList (superdepth.py:99)


def build(device, **over):
    from slowtv_monodepth_amd.networks import checkpoint as ck
    from slowtv_monodepth_amd.networks.decoders import SuperdepthDecoder
    dec = SuperdepthDecoder(**{**SUPERDEPTH_KW, **over}).train()
    holder = torch.nn.Module(); holder.decoders = torch.nn.ModuleDict({'disp': dec})
    shapes = {k: tuple(v.shape) for k, v in ck.to_reference_state_dict(holder).items()}
    state = superdepth_state(shapes)
    ck.load_reference_state_dict(holder, state, strict=True)
    holder.to(device)
    return dec, holder, shapes, state


def run_and_compare(device, out_tol, grad_tol, plain=False):
    """The decoder on the fixture's seeded state / features / output gradients against the reference's outputs, feature gradients and parameter gradients (in
    full where the fixture holds them, through their sum and sum of magnitudes everywhere).  -> (decoder, outputs, fixture)."""
    g = load_golden('net_decoder_superdepth_64x96')
    with np.load(GOLDEN/'net_decoder_superdepth_64x96.npz') as z: keys, pkeys = [str(k) for k in z['meta_keys']], [str(k) for k in z['meta_param_keys']]
    dec, holder, shapes, state = build(device)
    assert sorted(shapes) == keys, 'the decoder\'s state dict no longer carries the reference decoder\'s names'
    feats, gouts = decoder_feats(seed=108, b=SUPERDEPTH_BATCH), superdepth_out_grads(seed=109, b=SUPERDEPTH_BATCH)
    assert sum(bit_checksum(v) for v in state.values() if v.dtype == torch.float32) == int(g['chk_state']) and sum(bit_checksum(f) for f in feats) == int(g['chk_feats']) \
        and sum(bit_checksum(v) for v in gouts.values()) == int(g['chk_gouts']), 'the seeded inputs are not the ones the fixture was made from'
    feats = [f.to(device).requires_grad_(True) for f in feats]
    if plain:
        with dec.plain_path(): out = dec(feats)
    else: out = dec(feats)
    sum((out[i]*gouts[i].to(device)).sum() for i in out).backward()
    fails = []
    for i in SUPERDEPTH_KW['out_sc']:
        assert out[i].shape == (SUPERDEPTH_BATCH, 1, 64, 96), f'scale {i} is not full-resolution'
        d = (out[i].detach().cpu() - g[f'out_{i}']).abs().max().item()
        print(f'superdepth decoder on {device}: disparity at scale {i}: {d:.2e} (bound {out_tol:.2e})')
        if not d <= out_tol: fails.append(f'disparity at scale {i}: {d:.2e}')
    for j, f in enumerate(feats):
        r = rel_to_max(f.grad.cpu(), g[f'gfeat_{j}'])
        print(f'superdepth decoder on {device}: gradient w.r.t. encoder feature {j}: {r:.2e} (bound {grad_tol:.2e})')
        if not r <= grad_tol: fails.append(f'gradient w.r.t. encoder feature {j}: {r:.2e}')
    grads = {k: p.grad for k, p in holder.named_parameters()}
    assert sorted(grads) == pkeys
    stats = g['gparam_stats']
    for n, k in enumerate(pkeys):
        assert grads[k] is not None, f'{k} got no gradient'
        gk = grads[k].detach().double().cpu()
        if f'gparam_{k}' in g:
            r = rel_to_max(gk, g[f'gparam_{k}'].double())
            if not r <= grad_tol: fails.append(f'gradient of {k}: {r:.2e}')
        if not abs(gk.abs().sum().item() - stats[n, 1].item()) <= 10*grad_tol*stats[n, 1].item(): fails.append(f'sum of |gradient| of {k}')
        if not abs(gk.sum().item() - stats[n, 0].item()) <= 10*grad_tol*stats[n, 1].item(): fails.append(f'sum of the gradient of {k}')
    assert not fails, '; '.join(fails)
    return dec, out, g


def test_superdepth_is_registered_and_builds_on_both_trunks():
    from slowtv_monodepth_amd import DEC_REG
    from slowtv_monodepth_amd.networks.decoders import SubPixelConv, SuperdepthDecoder
    from slowtv_monodepth_amd.networks.depth import DepthNet
    assert DEC_REG['superdepth'] is SuperdepthDecoder and {'monodepth', 'cadepth', 'ddvnet', 'diffnet'} <= set(DEC_REG)
    with pytest.raises(KeyError, match='Invalid activation'): SuperdepthDecoder(**{**SUPERDEPTH_KW, 'out_act': 'bogus'})
    dec = SuperdepthDecoder(**{**SUPERDEPTH_KW, 'out_sc': [0, 2], 'out_ch': 2, 'out_act': 'relu'})
    assert list(dec.convs) == ORDER[:10] + ['outconv_0', 'outconv_2'] and all(m is dec.convs[k] for m, k in zip(dec.decoder, dec.convs))
    assert not isinstance(dec.convs, torch.nn.Module) and all(k.startswith('decoder.') for k in dec.state_dict())       # `convs` is a plain dict: registered once
    assert isinstance(dec.convs['upconv_4_0'][1], SubPixelConv) and dec.convs['upconv_4_0'][1].conv.weight.shape == (1024, 1, 3, 3)
    assert dec.convs['outconv_2'][1].conv.weight.shape == (2*16, 1, 3, 3) and dec.convs['outconv_0'][0].out_channels == 2 and isinstance(dec.activation, torch.nn.ReLU)
    assert dec.convs['upconv_0_1'].conv.in_channels == 16 and dec.convs['upconv_1_1'].conv.in_channels == 32 + 64      # no stride-1 feature: stage 0 has no skip
    net = DepthNet(enc_name='resnet18', pretrained=False, dec_name='superdepth')
    out = net(torch.rand(1, 3, 64, 96))
    assert set(out['disp']) == {0, 1, 2, 3} and all(out['disp'][i].shape == (1, 1, 64, 96) for i in range(4))             # every head is full-resolution
    assert (out['disp'][0] > 0).all() and (out['disp'][3] < 1).all()
    net = DepthNet(enc_name='convnext_tiny', pretrained=False, dec_name='superdepth', mask_name='uncertainty', num_ch_mask=2)
    out = net(torch.rand(2, 3, 64, 96))
    assert out['disp'][0].shape == (2, 1, 64, 96) and out['mask'][1].shape == (2, 2, 64, 96) and (out['mask'][0] >= 0).all()
    for bad in ('use_stereo_blend', 'use_virtual_stereo'):
        with pytest.raises(NotImplementedError): DepthNet(enc_name='resnet18', pretrained=False, dec_name='superdepth', **{bad: True})
    bil = SuperdepthDecoder(**{**SUPERDEPTH_KW, 'upsample_mode': 'bilinear', 'use_skip': False})                          # accepted and unused, as in the reference
    assert bil([torch.rand(1, c, 64//s, 96//s) for c, s in zip(SUPERDEPTH_KW['num_ch_enc'], SUPERDEPTH_KW['enc_sc'])])[2].shape == (1, 1, 64, 96)


@pytest.mark.parametrize('r', [2, 4, 8])
def test_subpixel_conv_initialisation(r):
    """Zero bias and rows equal in groups of four — the reference's literal 4 for every up-sampling factor."""
    from slowtv_monodepth_amd.networks.decoders import SubPixelConv
    torch.manual_seed(r)
    m = SubPixelConv(3, r)
    w = m.conv.weight.detach()
    assert w.shape == (3*r*r, 1, 3, 3) and m.conv.groups == 3 and isinstance(m.conv.weight, torch.nn.Parameter) and m.conv.weight.requires_grad
    assert (m.conv.bias == 0).all()
    grouped = w.view(-1, 4, 9)
    assert (grouped == grouped[:, :1]).all() and not torch.equal(grouped[0, 0], grouped[1, 0])
    x = torch.rand(2, 3, 4, 5)
    assert torch.equal(m(x), torch.nn.functional.pixel_shuffle(torch.nn.functional.conv2d(x, w, None, padding=1, groups=3), r)) and m(x).shape == (2, 3, 4*r, 5*r)


def test_plain_path_matches_the_reference_decoder_on_the_cpu():
    """The same ATen operators in the same order as the reference: held to the fixture's own yardstick rule — the larger of the library's floor and 4 x
    what the reference's fp32 run shows against its fp64 run (disparities in absolute terms: they are of order 0.5)."""
    g = load_golden('net_decoder_superdepth_64x96')
    run_and_compare('cpu', max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_out'])), max(FLOOR, 4*float(g['meta_ref_fp32_vs_fp64_grad'])))


def test_reference_keys_load_strictly_and_round_trip():
    from slowtv_monodepth_amd.networks import checkpoint as ck
    with np.load(GOLDEN/'net_decoder_superdepth_64x96.npz') as z: keys = [str(k) for k in z['meta_keys']]
    dec, holder, shapes, state = build('cpu')
    assert sorted(shapes) == keys and len(keys) == 44 and ck._dec_kind(holder) == 'superdepth'
    for want in ('decoders.disp.decoder.0.0.conv.weight', 'decoders.disp.decoder.0.1.conv.bias', 'decoders.disp.decoder.1.conv.weight', 'decoders.disp.decoder.9.conv.bias',
                 'decoders.disp.decoder.10.0.weight', 'decoders.disp.decoder.11.0.conv.bias', 'decoders.disp.decoder.13.1.conv.weight'): assert want in keys, want
    assert shapes['decoders.disp.decoder.13.1.conv.weight'] == (64, 1, 3, 3) and shapes['decoders.disp.decoder.0.1.conv.weight'] == (1024, 1, 3, 3)
    for k in keys: assert ck.from_reference_key(k, dec.out_sc, 'superdepth') == k and ck.to_reference_key(k, dec.out_sc, False, 'superdepth') == k
    back = ck.to_reference_state_dict(holder)
    assert sorted(back) == keys and all(torch.equal(back[k], state[k]) for k in keys)
    ckpt = ck.reference_checkpoint(holder)
    dec2, holder2, *_ = build('cpu')
    with torch.no_grad():
        for p in holder2.parameters(): p.zero_()
    ck.load_reference_checkpoint(holder2, ckpt)
    assert all(torch.equal(a, b) for a, b in zip(holder.state_dict().values(), holder2.state_dict().values()))
    missing = dict(state); del missing['decoders.disp.decoder.13.1.conv.bias']
    with pytest.raises(RuntimeError, match='decoder.13.1.conv.bias'): ck.load_reference_state_dict(holder, missing, strict=True)
    # the other decoders are told apart as before
    from slowtv_monodepth_amd.networks.decoders import DiffNetDecoder, MonodepthDecoder
    for cls, kind in ((MonodepthDecoder, 'monodepth'), (DiffNetDecoder, 'diffnet')):
        h = torch.nn.Module(); h.decoders = torch.nn.ModuleDict({'disp': cls(**SUPERDEPTH_KW)})
        assert ck._dec_kind(h) == kind


def test_subpixel_fixture_through_the_aten_restatement():
    """`subpixel_aten` (what the GPU tests hold the operator to, in fp64) reproduces the reference's SubPixelConv with its surroundings on the fixture's inputs."""
    g = load_golden('op_subpixel')
    for k, (B, C, Cs, h, w, r, pre, act, pad) in enumerate(SUBPIXEL_CASES):
        ins = subpixel_case(k)
        assert sum(bit_checksum(t) for t in ins.values() if t is not None) == int(g[f'chk_{k}']), 'the seeded inputs are not the ones the fixture was made from'
        leaves = {n: (t.clone().requires_grad_(True) if t is not None else None) for n, t in ins.items() if n != 'gout'}
        out = subpixel_aten(leaves['x'], leaves['pre_bias'], leaves['weight'], leaves['bias'], leaves['skip'], r, pre, act, pad)
        assert out.shape == ins['gout'].shape
        (out*ins['gout']).sum().backward()
        got = dict(out=out.detach(), **{f'grad_{n}': t.grad for n, t in leaves.items() if t is not None})
        assert sorted(got) == sorted(n for n in SUBPIXEL_NAMES if f'{n}_{k}' in g)
        for what, mine in got.items():
            assert rel_to_max(mine, g[f'{what}_{k}']) <= max(FLOOR, 4*float(g[f'meta_ref_fp32_vs_fp64_{what}_{k}'])), f'case {k} {what}'
    k = SUBPIXEL_SATURATED
    assert float(g[f'meta_pre_min_{k}']) <= -50 and float(g[f'meta_v_min_{k}']) <= -40 and float(g[f'meta_v_max_{k}']) >= 40


def test_operator_is_reexported_and_validates_its_arguments():
    from slowtv_monodepth_amd import functional as F, subpixel
    assert F.subpixel_conv is subpixel.subpixel_conv
    assert 'subpixel_conv' not in F.__all__      # (the hostile-memory case table is `__all__`; this operator's case lives in test_gpu_superdepth.py)
    x, wgt, b, pb, skip = torch.rand(2, 3, 4, 5), torch.rand(12, 1, 3, 3), torch.rand(12), torch.rand(3), torch.rand(2, 2, 8, 10)
    with pytest.raises(RuntimeError, match='GPU'): F.subpixel_conv(x, wgt, b, 2, pre_bias=pb, pre_act='elu', act='relu', skip=skip, pad=True)
    with pytest.raises(TypeError): F.subpixel_conv([1.0], wgt, b, 2)
    with pytest.raises(TypeError): F.subpixel_conv(x, None, b, 2)
    with pytest.raises(TypeError): F.subpixel_conv(x, wgt, b, 2, pre_bias=[0.0])
    with pytest.raises(TypeError): F.subpixel_conv(x, wgt, b, 2, skip=[0.0], pad=True)
    with pytest.raises(ValueError, match='up_factor'): F.subpixel_conv(x, wgt, b, 3)
    with pytest.raises(ValueError, match='pre_act'): F.subpixel_conv(x, wgt, b, 2, pre_act='relu')
    with pytest.raises(ValueError, match='act'): F.subpixel_conv(x, wgt, b, 2, act='elu')
    # shapes are refused before the device is looked at
    with pytest.raises(ValueError): F.subpixel_conv(x[0], wgt, b, 2)
    with pytest.raises(ValueError): F.subpixel_conv(x[:0], wgt, b, 2)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b, 4)                                  # weight is (C 4, ...), not (C 16, ...)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt.view(12, 3, 3), b, 2)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b[:11], 2)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b, 2, pre_bias=pb[:2])
    with pytest.raises(ValueError, match='pad'): F.subpixel_conv(x, wgt, b, 2, skip=skip)            # a skip without the padding
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b, 2, skip=skip[:, :, :7], pad=True)   # not (B,Cs,2h,2w)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b, 2, skip=skip[:1], pad=True)
    with pytest.raises(ValueError): F.subpixel_conv(x, wgt, b, 2, skip=skip[:, :0], pad=True)


def test_header_and_prototypes_agree_on_the_new_symbols():
    from slowtv_monodepth_amd import _lib
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    order = list(_lib.PROTOTYPES)
    for name in NEW_SYMBOLS:
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
    assert [order.index(n) for n in NEW_SYMBOLS] == list(range(order.index(NEW_SYMBOLS[0]), order.index(NEW_SYMBOLS[0]) + 3))
    assert 'superdepth.py:13-26' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_subpixel.hip' in (ROOT/'slowtv_monodepth_amd'/'csrc'/'Makefile').read_text()


def test_the_abi_refuses_bad_arguments_without_a_gpu():
    """Null pointers, non-positive sizes, an r that is not served, unknown activation codes, skip channels without the padding and a short workspace are
    refused before anything is launched; sizes the kernels do not serve give a workspace size of 0."""
    from slowtv_monodepth_amd import _lib
    ws = _lib.lib.smd_subpixel_workspace_bytes
    assert ws(2, 3, 2, 3, 5, 2, 1) > 0 and ws(1, 1, 0, 1, 1, 2, 1) > 0 and ws(12, 1, 0, 24, 80, 8, 0) >= 12*640*4 and ws(12, 16, 0, 96, 320, 2, 1) > 0
    for bad in ((0, 3, 2, 3, 5, 2, 1), (2, 0, 2, 3, 5, 2, 1), (2, 3, -1, 3, 5, 2, 1), (2, 3, 2, 0, 5, 2, 1), (2, 3, 2, 3, -1, 2, 1), (2, 3, 2, 3, 5, 3, 1), (2, 3, 2, 3, 5, 16, 1),
                (2, 3, 2, 3, 5, 2, 0), (2, 3, 0, 3, 5, 2, 2), (1, 1, 0, 16384, 16384, 2, 1), (1, 1, 0, 4096, 4096, 8, 0)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 0, 8000, 8000, 2, 1) > 0      # a padded plane of 2.56e8 elements is still served
    p, big = 4096, 1 << 24          # a pointer value that is never dereferenced: every call below is refused first
    fwd = lambda *sz, ptrs=(p,)*6: _lib.call('smd_subpixel_fwd', *ptrs, *sz, None)
    bwd = lambda *sz, ptrs=(p,)*11, nb=big: _lib.call('smd_subpixel_bwd', *ptrs, nb, *sz, None)
    for call in (fwd, bwd):
        with pytest.raises(ValueError, match='invalid sizes'): call(2, 3, 2, 3, 5, 3, 1, 1, 1)          # r
        with pytest.raises(ValueError, match='invalid sizes'): call(0, 3, 2, 3, 5, 2, 1, 1, 1)
        with pytest.raises(ValueError, match='invalid sizes'): call(2, 3, 2, 3, 0, 2, 1, 1, 1)
        with pytest.raises(ValueError, match='invalid sizes'): call(2, 3, 2, 3, 5, 2, 2, 1, 1)          # pre_act
        with pytest.raises(ValueError, match='invalid sizes'): call(2, 3, 2, 3, 5, 2, 1, 3, 1)          # act
        with pytest.raises(ValueError, match='invalid sizes'): call(2, 3, 2, 3, 5, 2, 1, 1, 0)          # skip channels without the padding
        with pytest.raises(ValueError, match='invalid sizes'): call(1, 1, 0, 16384, 16384, 2, 1, 1, 1)  # a padded plane of 2^30 elements
    with pytest.raises(_lib.HotpathError, match='workspace'): bwd(2, 3, 2, 3, 5, 2, 1, 1, 1, nb=16)
    for k in (0, 2, 3, 4, 5):                                                                            # x, weight, bias, skip (Cs > 0), out (pre_bias may be NULL)
        with pytest.raises(ValueError, match='null'): fwd(2, 3, 2, 3, 5, 2, 1, 1, 1, ptrs=tuple(None if j == k else p for j in range(6)))
    for k in (0, 2, 3, 4, 10):                                                                           # x, weight, out (act != none), g_out, the workspace
        with pytest.raises(ValueError, match='null'): bwd(2, 3, 2, 3, 5, 2, 1, 1, 1, ptrs=tuple(None if j == k else p for j in range(11)))
    with pytest.raises(ValueError, match='null'): bwd(2, 3, 2, 3, 5, 2, 1, 1, 1, ptrs=(p, None, p, p, p, p, p, p, p, p, p))      # g_pre_bias without pre_bias
    with pytest.raises(ValueError, match='nothing to compute'): bwd(2, 3, 2, 3, 5, 2, 1, 1, 1, ptrs=(p,)*5 + (None,)*5 + (p,))
    with pytest.raises(ValueError, match='skip gradient'): bwd(2, 3, 0, 3, 5, 2, 1, 1, 1)


def test_trainer_builds_from_the_example_config():
    from slowtv_monodepth_amd.networks.decoders import SuperdepthDecoder
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    text = (ROOT/'cfg'/'kitti_superdepth.yaml').read_text()
    cfg, base = yaml.safe_load(text), yaml.safe_load((ROOT/'cfg'/'kitti_resnet18.yaml').read_text())
    assert cfg['net']['depth']['dec_name'] == 'superdepth' and 'use_stereo_blend' in text and 'use_stereo_blend' not in cfg['net']['depth']
    base['net']['depth']['dec_name'] = 'superdepth'
    assert cfg == base
    m = MonoDepthModule(cfg)
    dec = m.nets['depth'].decoders['disp']
    assert isinstance(dec, SuperdepthDecoder) and list(dec.convs) == ORDER
