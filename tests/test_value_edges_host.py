"""The value-edge table (value_edges.py) checked without a GPU: it is well formed, its fp64 reference runs, its inputs are fair (ATen's own fp32 operator
on the CPU meets every bound with a factor 4 to spare, so a kernel that misses one is worse than plain fp32 arithmetic, not unlucky), and its judge refuses
a wrong answer that the whole-tensor measure would let through."""
import pytest
import torch

import value_edges as V
from conftest import rel_to_max

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
        assert all(b[0] in ('rel', 'close', 'equal') for b in c.tol.values()), c.name


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


@pytest.mark.parametrize('c', V.CASES, ids=[c.name for c in V.CASES])
def test_reference_runs_and_inputs_are_fair(c):
    """`ref` runs in fp64, and ATen's fp32 operator on the same operands is within a quarter of every bound of it."""
    ops, ref = _ref64(c)
    assert any(v is not None for v in ref.values())
    got = c.ref({k: v.clone() for k, v in ops.items()}, V.F32)
    for k, e in V.errors(c, got, ref).items():
        # an output that is exactly 0 everywhere (C = 1: x_hat = 0, so g_x and g_w vanish) has no relative measure; the kernel is still held to the exact zero
        if not bool(ref[k].any()): continue
        assert e*SPARE <= 1.0, f'{c.name}: ATen in fp32 is at {e:.3g} of the bound of {k}: the inputs, not the kernel, are what this case would measure'


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


def test_judge_compares_every_element():
    """Non-finite patterns must match, equal infinities and NaNs count as equal, and `equal` means equal."""
    inf, nan = float('inf'), float('nan')
    ref = torch.tensor([1.0, -inf, nan, 2.0])
    assert V.excess(ref.clone(), ref, V.EQUAL) == 0.0 and V.excess(ref.clone(), ref, V.TOL_POOL_GX) == 0.0
    for bad in ([1.0, inf, nan, 2.0], [1.0, -inf, 0.0, 2.0], [1.0, -inf, nan, nan], [1.0, -1e30, nan, 2.0]):
        assert V.excess(torch.tensor(bad), ref, V.EQUAL) == float('inf') and V.excess(torch.tensor(bad), ref, V.TOL_POOL_GX) == float('inf'), bad
    assert V.excess(torch.tensor([1.0, -inf, nan, 2.0 + 1e-6]), ref, V.EQUAL) == float('inf')
    assert V.excess(torch.tensor([1.0, -inf, nan, 2.0 + 1e-5]), ref, V.TOL_POOL_GX) > 1.0
