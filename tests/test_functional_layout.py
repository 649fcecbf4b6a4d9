"""`functional` is the re-export surface of the operator modules: every name it had stays, and is the object of its home module; the plumbing the
operators share is written once and does what the copies did.  Everything here runs on the host."""
import ast
from pathlib import Path

import pytest
import torch

from slowtv_monodepth_amd import _device, class_ops, conv_ops, conv_routing, functional as F, geom_ops, net_ops, recon_ops, row_skip

# `functional.__all__` of the commit before the split (2b6e44c), written out
_ALL_BEFORE = ['conv3x3_headn', 'upsample_stack', 'scale_mean', 'conv3x3_mfma', 'conv3x3_wide', 'conv3x3_same', 'set_conv_route', 'conv_routes', 'loss_path_fused',
               'crop_resize', 'disp_to_depth', 'image_recon_prep', 'PreparedFrames', 'image_recon_fused', 'image_recon_fused_disp', 'disp_smooth_fused', 'view_synth',
               'photo_error', 'recon_reduce', 'lane_shift_selftest', 'recon_flags', 'regression_loss', 'elu_pad', 'elu_up_cat_pad', 'batch_norm_act', 'max_pool3x3s2',
               'dwconv7x7', 'layer_norm_cf', 'pose_matrices', 'intrinsics', 'inv_intrinsics']
# name -> home module: the list above, the private names in use and the public ones `__all__` did not list
_HOME = {
    recon_ops: ['loss_path_fused', 'disp_to_depth', 'image_recon_prep', 'PreparedFrames', 'image_recon_fused', 'image_recon_fused_disp', 'disp_smooth_fused', 'recon_flags',
                'gaussian_blur3x3', 'disp_smooth_blurred', 'supports_per_pass'],
    row_skip: ['_RowSkipTuner', 'row_skip_tuner', 'dead_tile_shares', 'dead_wave_shares'],
    class_ops: ['upsample_stack', 'scale_mean', 'crop_resize', 'view_synth', 'photo_error', 'recon_reduce', 'lane_shift_selftest', 'regression_loss', '_ScaleMean'],
    net_ops: ['conv3x3_headn', 'conv3x3_head', 'elu_pad', 'elu_up_cat_pad', 'batch_norm_act', 'max_pool3x3s2', 'dwconv7x7', 'layer_norm_cf'],
    geom_ops: ['pose_matrices', 'intrinsics', 'inv_intrinsics'],
    conv_ops: ['conv3x3_mfma', 'conv3x3_wide', 'conv3x3_same', 'conv3x3_thin', 'conv7x7s2_stem'],
    conv_routing: ['set_conv_route', 'conv_routes', '_conv_route'],
    _device: ['call', '_stream'],
}


def test_every_name_is_the_object_of_its_home_module():
    frozen = [n for names in _HOME.values() for n in names]
    assert len(frozen) == len(set(frozen)) and set(_ALL_BEFORE) <= set(frozen)
    for home, names in _HOME.items():
        for n in names: assert hasattr(F, n) and getattr(F, n) is getattr(home, n), n
    assert set(F.__all__) >= set(_ALL_BEFORE) and len(F.__all__) == len(set(F.__all__))
    for n in F.__all__: assert hasattr(F, n) and not n.startswith('_'), n
    for n in ('conv3x3_head', 'conv3x3_thin', 'conv7x7s2_stem', 'gaussian_blur3x3', 'disp_smooth_blurred', 'supports_per_pass', 'row_skip_tuner', 'dead_tile_shares',
              'dead_wave_shares'): assert n in F.__all__, n


def test_one_tuner_table_one_mean_cache_one_tls():
    assert F.row_skip_tuner('cuda:0') is row_skip.row_skip_tuner('cuda:0') is row_skip._tuners[0]
    assert F.row_skip_tuner(torch.device('cuda', 0)) is row_skip._tuners[0]
    mods = (F, recon_ops, row_skip, class_ops, net_ops, geom_ops, conv_ops, conv_routing, _device)
    assert [m for m in mods if hasattr(m, '_tuners')] == [row_skip]
    assert [m for m in mods if hasattr(m, '_mean_ws')] == [class_ops]
    assert [m for m in mods if hasattr(m, '_tls')] == [_device]
    for m in (recon_ops, class_ops, net_ops, geom_ops, conv_ops): assert m.call is _device.call and m._stream is _device._stream and m._on is _device._on


def test_functional_defines_nothing():
    tree = ast.parse(Path(F.__file__).read_text())
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))]


def test_depth_range():
    with pytest.raises(ValueError, match=r'Min depth must be greater than 0\. \(0\)'): recon_ops._depth_range(0, 100)
    with pytest.raises(ValueError, match=r'Min depth must be greater than 0\. \(-1\.5\)'): recon_ops._depth_range(-1.5, None)
    with pytest.raises(ValueError, match=r'Max depth must be greater than min\. \(1 vs\. 2\)'): recon_ops._depth_range(2, 1)
    assert recon_ops._depth_range(None, None) == (0.0, 0.0)
    assert recon_ops._depth_range(0.1, 100) == (0.1, 100.0) and recon_ops._depth_range(2, 2) == (2.0, 2.0)
    assert recon_ops._depth_range(None, 80) == (0.0, 80.0) and recon_ops._depth_range(0.5, None) == (0.5, 0.0)
    assert recon_ops._depth_range(0.5, 0) == (0.5, 0.0)                  # max_depth 0 is "no maximum", as None is
    assert all(type(v) is float for v in recon_ops._depth_range(1, 100))
    with pytest.raises(ValueError, match='Min depth'): F.disp_to_depth([], (4, 4), min_depth=0)      # (the wrappers raise it before they look at anything else)
    with pytest.raises(ValueError, match='Max depth'): F.image_recon_fused_disp([], None, None, None, None, flags=0, min_depth=3, max_depth=2)
    with pytest.raises(ValueError, match='Max depth'): F.loss_path_fused({}, None, None, None, None, flags=0, min_depth=3, max_depth=2)


def test_frames_key_and_prepared_frames():
    imgs, supp = torch.zeros(2, 3, 8, 16), torch.zeros(1, 2, 3, 8, 16)
    flags = F.recon_flags('ssim', True, True)
    hs, ws = [8, 4], [16, 8]
    key = recon_ops._frames_key(imgs, supp, flags | 0x1000, hs, ws)      # (bits that are not the criterion's do not enter the key)
    assert key == recon_ops._frames_key(imgs, supp, flags, tuple(hs), tuple(ws))
    assert (key.imgs_ptr, key.supp_ptr, key.imgs_shape, key.supp_shape, key.flags, key.hs, key.ws) == \
        (imgs.data_ptr(), supp.data_ptr(), (2, 3, 8, 16), (1, 2, 3, 8, 16), flags, (8, 4), (16, 8))
    edge_w = torch.zeros(4, dtype=torch.uint8)
    p = F.PreparedFrames(torch.zeros(4), None, key, edge_w)
    assert p.matches(imgs, supp, flags, hs, ws)
    assert not p.matches(imgs, supp, F.recon_flags('l1', True, True), hs, ws)            # other flags
    assert not p.matches(imgs, supp, F.recon_flags('ssim', False, True), hs, ws)
    assert not p.matches(imgs[:1], supp[:, :1], flags, hs, ws)                           # other shape (same address)
    assert not p.matches(imgs.clone(), supp, flags, hs, ws) and not p.matches(imgs, supp.clone(), flags, hs, ws)   # other frames
    assert not p.matches(imgs, supp, flags, [8, 4, 2], [16, 8, 4]) and not p.matches(imgs, supp, flags, None, None)   # other pyramid / none
    assert p.edges_for(imgs, hs, ws) is edge_w and p.edges_for(imgs, tuple(hs), tuple(ws)) is edge_w
    assert p.edges_for(imgs, [8, 2], [16, 8]) is None and p.edges_for(imgs, hs, [16, 4]) is None and p.edges_for(imgs, [8], [16]) is None
    assert p.edges_for(imgs.clone(), hs, ws) is None and p.edges_for(imgs[:1], hs, ws) is None
    assert F.PreparedFrames(torch.zeros(4), None, key).edges_for(imgs, hs, ws) is None   # built without edge weights
    flat = F.PreparedFrames(torch.zeros(4), None, recon_ops._frames_key(imgs, supp, flags, None, None))
    assert flat.key.hs is None and flat.key.ws is None
    assert flat.matches(imgs, supp, flags, None, None) and not flat.matches(imgs, supp, flags, hs, ws)


def test_workspace_floor_and_passed_size():
    asked = []
    def query(*args): asked.append(args); return 100
    ws, nbytes = _device._workspace('cpu', query, 1, 2, 3, floor=256)
    assert asked == [(1, 2, 3)] and nbytes == 100 and ws.numel() == 256 and ws.dtype == torch.uint8 and ws.device.type == 'cpu'
    ws, nbytes = _device._workspace('cpu', query, 7)
    assert asked[-1] == (7,) and len(asked) == 2 and (ws.numel(), nbytes) == (100, 100)
    ws, nbytes = _device._workspace('cpu', lambda: 0)
    assert (ws.numel(), nbytes) == (0, 0)
    ws, nbytes = _device._workspace('cpu', lambda: 0, floor=256)
    assert (ws.numel(), nbytes) == (256, 0)
    ws, nbytes = _device._workspace('cpu', 1000, floor=256)              # a size already asked for: no second query
    assert (ws.numel(), nbytes) == (1000, 1000)


def test_pointer_helpers():
    t = torch.zeros(3)
    assert _device._ptr(None) is None and _device._ptr(t) == t.data_ptr()
    a = _device._ptrs([t, t[1:]])
    assert len(a) == 2 and a[0] == t.data_ptr() and a[1] == t.data_ptr() + 4
