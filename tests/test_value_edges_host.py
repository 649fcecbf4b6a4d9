"""The value-edge table (value_edges.py) checked without a GPU: it is well formed, its fp64 reference runs, its inputs are fair (ATen's own fp32 operator
on the CPU meets every bound with a factor 4 to spare, so a kernel that misses one is worse than plain fp32 arithmetic, not unlucky; where the bound is itself
4 x that fp32 operator's error, the error is capped at a quarter of YARD_CAP per slice, so no such bound is wider than 1e-3), its operands hold the regimes it
names, and its judge refuses a wrong answer that the whole-tensor measure would let through."""
import pytest
import torch

import value_edges as V
from conftest import rel_to_max
from test_gpu_cadepth import FLOOR

SPARE = 4.0


def _seed(c): return torch.Generator().manual_seed(len(c.name)*7919 + 17)


_cache = {}      # case name -> (operands, fp64 reference): computed once, never modified


def _ref64(c):
    if c.name not in _cache:
        ops = c.operands(_seed(c))
        _cache[c.name] = (ops, {k: (None if v is None else v.detach()) for k, v in c.ref(ops, V.F64).items()})
    return _cache[c.name]


def test_table_is_well_formed():
    names = [c.name for c in V.CASES]
    assert len(set(names)) == len(names)
    assert {c.op for c in V.CASES} == set(V.OPERATORS)
    for c in V.CASES:
        assert '*' in c.tol or c.tol, c.name
        assert all(b[0] in V.KINDS for b in c.tol.values()), c.name
        assert all((b[1] if b[0] == 'yard' else FLOOR) == FLOOR for b in c.tol.values()), c.name      # (the yardstick rule has one floor)


def test_batch_norm_shapes_take_the_paths_they_name():
    """The thresholds as csrc/smd_norm.hip has them: `kBnSmall` = 16384 values per channel, `f4` loads when HW % 4 == 0, and a chunk longer than the
    `kBnItemsPerBlock` = 8192 floats a block keeps in registers once N*HW exceeds `kBnMaxChunks` = 128 of them."""
    for shape, path in {**V.BN_SHAPES, **V.BN_LONG_SHAPES}.items():
        N, C, H, W = shape
        size = 'small' if N*H*W <= 16384 else 'chunked' if N*H*W <= 128*8192 else 'long'
        assert (size, 'f4' if H*W % 4 == 0 else 'scalar') == path == V.bn_path(shape), shape
        assert any(c.name.startswith(f'batch_norm_act{shape}_') for c in V.CASES), shape
    assert set(V.BN_SHAPES.values()) == {(s, v) for s in ('small', 'chunked') for v in ('scalar', 'f4')}
    assert 12*37*41 == 18204 > 16384 >= 4*6*20
    assert any(c.name.startswith('batch_norm_act(2, 3, 1, 1)') for c in V.CASES)      # M = 2


def test_edges_are_where_the_table_says():
    """The operands really hold the edges: the outlier at the stated element, zero variance, -inf windows, NaNs, one-hot positions, sigmoid levels."""
    by = {c.name: c for c in V.CASES}
    o = by['batch_norm_act(4, 8, 6, 20)_outlier300_first'].operands(torch.Generator().manual_seed(1))
    assert bool((o['x'][0, :, 0, 0] == V.BN_MEAN + 300*V.BN_SIGMA).all()) and o['x'][1:].max() < V.BN_MEAN + 6*V.BN_SIGMA
    o = by['batch_norm_act(4, 8, 6, 20)_outlier300_last'].operands(torch.Generator().manual_seed(1))
    assert bool((o['x'][-1, :, -1, -1] == V.BN_MEAN + 300*V.BN_SIGMA).all()) and o['x'][0, :, 0, 0].max() < V.BN_MEAN + 6*V.BN_SIGMA
    o = by['batch_norm_act(4, 8, 6, 20)_constant_channel'].operands(torch.Generator().manual_seed(1))
    assert o['x'][:, 1].double().var(unbiased=False).item() == 0.0
    o = by['layer_norm_cf(2, 96, 6, 20)_constant_pixel'].operands(torch.Generator().manual_seed(1))
    assert o['x'][0, :, 0, 0].double().var(unbiased=False).item() == 0.0
    x = by['max_pool3x3s2(2, 3, 5, 8)_neg_inf'].operands(torch.Generator().manual_seed(1))['x']
    y = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    assert bool((y[:, :, 0, 0] == float('-inf')).all()) and bool((y[:, :, 1, 1] == float('-inf')).all()) and bool(y.isfinite().any())
    x = by['max_pool3x3s2(1, 2, 9, 7)_nan'].operands(torch.Generator().manual_seed(1))['x']
    assert int(x.isnan().sum()) == 2 and bool(x[0, 0, 0, -1].isnan()) and bool(x[-1, -1, 4, 3].isnan())
    for shape in V.DW_SHAPES:
        x = by[f'dwconv7x7{shape}_one_hot_exact'].operands(torch.Generator().manual_seed(1))['x']
        hit = {(h, w) for h, w in V.dw_positions(*shape[2:]) if bool((x[:, :, h, w] == 1).any())}
        assert hit == set(V.dw_positions(*shape[2:])) and bool(((x == 0) | (x == 1)).all()), shape
    for c in V.CASES:
        if not c.op.startswith('conv3x3_head'): continue
        pre = V.head_pre_activation(c.operands(_seed(c)))
        for level in V.HEAD_LEVELS: assert bool(((pre - level).abs() < 3).any()), (c.name, level)
    for c in V.CASES:
        if not c.op.startswith('elu'): continue
        o = c.operands(_seed(c))
        x, b = (o['x'] if 'x' in o else o['a']), o.get('bias')
        pre = x if b is None else x + b.view(1, -1, 1, 1)
        assert bool(((pre == 0) & ~torch.signbit(pre)).any()), c.name
        if b is None: assert {float(v) for v in torch.tensor(V.PRE_ACTIVATIONS)} <= {float(v) for v in pre.flatten()} and bool(torch.signbit(pre[pre == 0]).any()), c.name
        else:
            for v in V.PRE_ACTIVATIONS: assert bool(((pre - v).abs() <= 1e-6*max(1.0, abs(v))).any()), (c.name, v)


def test_edges_of_the_second_group_are_where_the_table_says():
    """The regimes of the operators merged after the first table, on the operands in fp64."""
    cases = lambda op, tag='': [(c, c.operands(_seed(c))) for c in V.CASES if c.op == op and tag in c.name]
    for c, o in cases('channel_attention', 'one_hot'):
        p = torch.softmax(-V.attention_matrix(o), -1)
        assert p.amax(-1).min().item() >= 1 - 1e-30 and p.topk(2, -1).values[..., 1].max().item() < 1e-30, c.name      # (every off-maximum entry below 1e-30)
    for c, o in cases('channel_attention', 'ties'):
        a = V.attention_matrix(o)
        assert bool(((a == a.amin(-1, keepdim=True)).sum(-1) >= 2).all()) and bool((a == a.round()).all()) and a.abs().max() < 2**24, c.name
        assert torch.equal(o['x'][:, 0], o['x'][:, 1]), c.name
    for c, o in cases('channel_attention', 'zero'): assert not bool(o['x'].any()), c.name
    for c, o in cases('channel_attention', 'rows_1e-3_1_30'):
        top = o['x'].abs().amax((0, 2, 3))
        assert top[0::3].max() <= 1e-3 < top[1::3].max() <= 1 < top[2::3].max(), c.name
    for c, o in cases('channel_attention', 'one_channel_grad'): assert int((o['g'].abs().amax((0, 2, 3)) > 0).sum()) == 1, c.name
    for op, pre in (('se_gate', V.se_pre_activations), ('up_cat_gate_pad', lambda o: V.ucg_pre_activations(o, 'bias' in o))):
        for c, o in cases(op, '_levels'):
            gate = torch.sigmoid(pre(o)[1])
            assert 0 < gate.min().item() < 1e-38 and gate.max().item() > 1 - 1e-16 and bool(((gate - 0.5).abs() < 0.1).any()), c.name
        for c, o in cases(op, 'dead_hidden'): assert not bool(pre(o)[0].any()), c.name
        if op == 'up_cat_gate_pad':
            for c, o in cases(op, '_levels'): assert bool((pre(o)[0][:, 0] == 1).all()) and pre(o)[0][:, 1].min().item() > 1, c.name      # unit 0 carries the levels, unit 1 is alive
        for c, o in cases(op, 'zero'): assert not any(bool(o[k].any()) for k in ('x', 'a', 'skip') if k in o), c.name
        for c, o in cases(op, 'means_'):
            m = (o['x'] if op == 'se_gate' else o['skip']).double().mean((0, 2, 3))
            assert m[0] > 9e3 and 0 <= m[1] < 2e-4, c.name
    for c, o in cases('relu_pad'):
        pre = o['x'] if 'bias' not in o else o['x'] + o['bias'].view(1, -1, 1, 1)
        assert bool(((pre == 0) & ~torch.signbit(pre)).any()), c.name
        for v in V.PRE_ACTIVATIONS: assert bool(((pre - v).abs() <= 1e-6*max(1.0, abs(v))).any()), (c.name, v)
    for c, o in cases('ddv_head'):
        l = V.ddv_logits(o)
        G = l.shape[1]
        top = l.topk(3, 2).values
        if 'dominant_bin' in c.name:
            k = int(c.name.rsplit('dominant_bin', 1)[1])
            for g in range(G): assert bool((l[:, g].argmax(1) == V.ddv_bin(k, g)).all()), c.name
            assert (top[:, :, 0] - top[:, :, 1]).min().item() > 104, c.name
        elif 'tie_bins' in c.name:
            for g in range(G):
                i, j = (V.ddv_bin(k, g) for k in V.DDV_TIE)
                assert bool((l[:, g, i] == l[:, g, j]).all()) and bool((l[:, g, i] == top[:, g, 0]).all()) and (i & 4) != (j & 4), c.name
            assert bool((top[:, :, 0] == top[:, :, 1]).all()) and (top[:, :, 1] - top[:, :, 2]).min().item() > 104, c.name
        elif 'zero_logits' in c.name: assert not bool(l.any()), c.name
        else: assert l[:, :, 0::2].min().item() > 190 and l[:, :, 1::2].max().item() < -190, c.name
    for c in V.CASES:
        if c.op != 'subpixel_conv': continue
        k = next(k for k in V.SUBPIXEL_VALUE_CASES if str(V.SUBPIXEL_CASES[k]) in c.name)
        u, v = V.subpixel_pre_activations(k, c.operands(_seed(c)))
        if 'pre_activations' in c.name:
            assert bool((u == 0).any()), c.name
            for t in V.PRE_ACTIVATIONS:
                if u.numel() >= 13: assert bool(((u - t).abs() <= 1e-6*max(1.0, abs(t))).any()), (c.name, t)
        elif 'levels' in c.name:
            for t in V.HEAD_LEVELS[:min(len(V.HEAD_LEVELS), u.numel())]: assert bool(((v - t).abs() <= 0.5).any()), (c.name, t)
        else: assert not bool(v[..., 1:-1, 1:-1].any()) and bool((v == v.round()).all()) and (bool((v == 0).any()) or min(v.shape[-2:]) < 3), c.name      # (interior: all nine taps)
    for c, o in [(c, c.operands(_seed(c))) for c in V.CASES if c.op.startswith('flip_blend')]:
        for key in [k for k in o if k.startswith('l')]:
            l, r = o[key], o['r_raw' + key[1:]]
            if 'l_equals_r' in c.name or key == 'l_0': assert torch.equal(l, r.flip(-1) if 'mirror' in c.name else r), c.name
            elif 'zero_one' in c.name or key == 'l_1': assert bool(((l == 0) & (r == 1)).any()) and bool(((l == 1) & (r == 0)).any()) and bool(((l + r) == 1).all()), c.name
            else: assert {float(v) for v in l.flatten()} == set(V.BLEND_EDGE_VALUES) and (set(V.BLEND_EDGE_VALUES) if 'scaled' not in c.name else {1 - 2.0**-24, 1.0}) <= {float(v) for v in r.flatten()}, c.name
    from slowtv_monodepth_amd.regularizers.feature import compute_grad
    for c, o in cases('feat_regs', 'plateaus') + cases('feat_regs', 'eighths'):
        f = o['feat_0'].double()
        dx, dy = compute_grad(f)
        zx, zy = dx[..., :-1] == 0, dy[..., :-1, :] == 0          # exact-zero first-order differences (the appended zero column / row left out) ...
        assert bool((zx[..., :-1] & ~zx[..., 1:]).any()) and bool((zy[..., :-1, :] & ~zy[..., 1:, :]).any()), c.name      # ... next to non-zero ones
        assert bool(((dx[..., :-2] == dx[..., 1:-1]) & (dx[..., :-2] != 0)).any() or 'plateaus' in c.name), c.name       # second-order operands that tie away from 0
        assert bool((dx[..., :-2] == dx[..., 1:-1]).any()) and bool((dy[..., :-2, :] == dy[..., 1:-1, :]).any()), c.name
        if 'plateaus' in c.name: assert not bool(f[..., -1, :].any()) and not bool(f[..., :, -1].any()) and 0.7 < (f == 0).double().mean() < 0.95, c.name
    for c, o in cases('feat_regs', 'constant_image'):
        assert all(not bool(d.any()) for d in compute_grad(o['img_0'].double())), c.name
    for c, o in cases('feat_regs', 'checker_image'):
        ix, _ = compute_grad(o['img_0'], ch_mean=True)
        w = o['img_0'].shape[-1]
        assert bool((torch.exp(-ix[..., :(w + 1)//2 - 1]) == 0).all()) and torch.exp(-ix.double()).min().item() > 0, c.name
    (c, o), = cases('feat_regs', 'pyramid')
    assert o['feat_0'].abs().max() < 1e-3 and o['feat_1'].abs().max() > 1e4


@pytest.mark.parametrize('c', V.CASES, ids=[c.name for c in V.CASES])
def test_reference_runs_and_inputs_are_fair(c):
    """`ref` runs in fp64, and ATen's fp32 operator on the same operands is within a quarter of every bound of it."""
    ops, ref = _ref64(c)
    assert any(v is not None for v in ref.values())
    got = c.ref({k: v.clone() for k, v in ops.items()}, V.F32)
    for v in ops.values(): assert bool(v.isfinite().all()) or c.op == 'max_pool3x3s2', f'{c.name}: only the pool cases hold non-finite inputs'
    # A bound that is measured against the yardstick: "ATen within the rule with its own error counted half" is e <= max(FLOOR, 2e), which holds for any e.
    # What makes such a case fair is a cap on the yardstick itself: 4 x ATen's error stays within YARD_CAP, per slice, so the bound can never grow past it.
    if V.needs_yardstick(c):
        for k, y in V.yardstick_errors(c, ref, got).items():
            assert 4*y <= V.YARD_CAP, f'{c.name}: ATen in fp32 misses {k} by {y:.3g} of its maximum: the bound 4 x that would check nothing; move the values'
    for k, e in V.errors(c, got, ref, ops, got if V.needs_yardstick(c) else None, 0.5).items():
        # an output that is exactly 0 everywhere (C = 1: x_hat = 0, so g_x and g_w vanish) has no relative measure; the kernel is still held to the exact zero
        if not bool(ref[k].any()): continue
        spare = 1.0 if c.tol.get(k, c.tol.get('*'))[0] in V.YARD_KINDS else SPARE
        assert e*spare <= 1.0, f'{c.name}: ATen in fp32 is at {e:.3g} of the bound of {k}: the inputs, not the kernel, are what this case would measure'


def test_judge_refuses_an_error_inside_a_small_scale_channel():
    """One element off by 10 x the bound, in the sigma = 1e-3 channel of a tensor whose other channels reach 1e3: the whole-tensor measure accepts it, the judge does not."""
    c = next(c for c in V.CASES if c.name == 'batch_norm_act(4, 8, 6, 20)_sigma_1e-3_1_1e3')
    ops, ref = _ref64(c)
    bound = c.tol['*'][1]
    V.judge(c, {k: (None if v is None else v.clone()) for k, v in ref.items()}, ref)
    x = ops['x'].double()
    fake = dict(y=x, g_x=x.clone())
    wrong = x.clone()
    wrong[2, 0, 3, 5] += 10*bound*x[:, 0].abs().max()
    assert rel_to_max(wrong, x) <= bound                                  # what `rel_to_max` over the whole tensor would say
    assert V.excess(wrong, x, c.tol['*']) <= 1.0 < V.excess(wrong, x, c.tol['*'], 1)
    cc = c._replace(tol={'*': c.tol['*']}, split=dict(y=1, g_x=1))
    with pytest.raises(AssertionError, match='y misses its bound'): V.judge(cc, dict(y=wrong, g_x=x.clone()), fake)
    V.judge(cc, dict(y=x.clone(), g_x=x.clone()), fake)


def test_judge_refuses_an_error_inside_a_saturated_gate_channel():
    """The fp64 reference of the saturated `se_gate` case with one element of g_x off by 10 x the bound inside a channel whose gate is shut (and whose incoming
    gradient is small): the whole-tensor measure accepts it, the per-channel judge does not."""
    c = next(c for c in V.CASES if c.name == 'se_gate(2, 12, 5, 7)_b2_levels')
    ops, ref = _ref64(c)
    bound = c.tol['*'][1]
    V.judge(c, {k: v.clone() for k, v in ref.items()}, ref)
    shut = int((ops['b2'] == V.GATE_LEVELS[0]).nonzero()[0])
    assert torch.sigmoid(V.se_pre_activations(ops)[1])[:, shut].max().item() < 1e-38
    g_x = ref['g_x']
    assert g_x[:, shut].abs().max() <= g_x.abs().max()/10      # a small-scale slice
    wrong = g_x.clone()
    wrong[1, shut, 2, 3] += 10*bound*g_x[:, shut].abs().max()
    assert rel_to_max(wrong, g_x) <= bound
    assert V.excess(wrong, g_x, c.tol['*']) <= 1.0 < V.excess(wrong, g_x, c.tol['*'], c.split['g_x'])
    with pytest.raises(AssertionError, match='g_x misses its bound'): V.judge(c, dict(ref, g_x=wrong), ref)


def test_judge_compares_every_element():
    """Non-finite patterns must match, equal infinities and NaNs count as equal, and `equal` means equal."""
    inf, nan = float('inf'), float('nan')
    ref = torch.tensor([1.0, -inf, nan, 2.0])
    assert V.excess(ref.clone(), ref, V.EQUAL) == 0.0 and V.excess(ref.clone(), ref, V.TOL_POOL_GX) == 0.0
    for bad in ([1.0, inf, nan, 2.0], [1.0, -inf, 0.0, 2.0], [1.0, -inf, nan, nan], [1.0, -1e30, nan, 2.0]):
        assert V.excess(torch.tensor(bad), ref, V.EQUAL) == float('inf') and V.excess(torch.tensor(bad), ref, V.TOL_POOL_GX) == float('inf'), bad
    assert V.excess(torch.tensor([1.0, -inf, nan, 2.0 + 1e-6]), ref, V.EQUAL) == float('inf')
    assert V.excess(torch.tensor([1.0, -inf, nan, 2.0 + 1e-5]), ref, V.TOL_POOL_GX) > 1.0
