"""The loss-path value-edge table (value_edges_loss.py) checked without a GPU, as test_value_edges_host.py checks the first table: it is well formed, its fp64
reference runs, its inputs are fair (the oracle in fp32 meets every bound with a factor 4 to spare; where the bound is itself 4 x that yardstick's error, the
error stays within a quarter of YARD_CAP per slice), the fp32 and the fp64 evaluation take the same decision on every element (so the kernels are held to `EQUAL`
with no flip allowance), the operands hold the edges the names claim, and the judge refuses an error inside a small-scale slice of a `split` output."""
import pytest
import torch

import value_edges as V
import value_edges_loss as L
from conftest import rel_to_max
from test_gpu_cadepth import FLOOR

SPARE = 4.0
EPS = L.EPS


def _seed(c): return torch.Generator().manual_seed(len(c.name)*7919 + 17)


_cache = {}      # case name -> (operands, fp64 reference, fp32 yardstick): computed once, never modified


def _refs(c):
    if c.name not in _cache:
        ops = c.operands(_seed(c))
        det = lambda r: {k: (None if v is None else v.detach()) for k, v in r.items()}
        _cache[c.name] = (ops, det(c.ref({k: v.clone() for k, v in ops.items()}, V.F64)), det(c.ref({k: v.clone() for k, v in ops.items()}, V.F32)))
    return _cache[c.name]


def _cases(op, tag=''): return [(c, _refs(c)[0]) for c in L.CASES if c.op == op and tag in c.name]


def test_table_is_well_formed():
    names = [c.name for c in L.CASES]
    assert len(set(names)) == len(names)
    assert {c.op for c in L.CASES} == set(L.OPERATORS)
    assert not set(names) & {c.name for c in V.CASES} and not any(c in V.CASES for c in L.CASES)      # a list of its own
    assert not set(L.OPERATORS) & set(V.OPERATORS)
    for c in L.CASES:
        assert c.tol, c.name
        assert all(b[0] in V.KINDS for b in c.tol.values()), c.name
        assert all((b[1] if b[0] == 'yard' else FLOOR) == FLOOR for b in c.tol.values()), c.name      # (the yardstick rule has one floor)
    assert set(L.LOOSE) <= set(names)


@pytest.mark.parametrize('c', L.CASES, ids=[c.name for c in L.CASES])
def test_reference_runs_inputs_are_fair_and_decisions_agree(c):
    ops, ref, got = _refs(c)
    assert any(v is not None for v in ref.values())
    for k, v in ops.items(): assert not v.is_floating_point() or bool(v.isfinite().all()), f'{c.name}: {k} is not finite'
    assert {k for k, v in ref.items() if v is not None} == {k for k, v in got.items() if v is not None}
    for k in L.decisions(c):      # the zero-flip condition
        if k in ref: assert torch.equal(got[k], ref[k]), f'{c.name}: {k}: fp32 and fp64 decide differently on {int((got[k] != ref[k]).sum())} elements'
    for k, r in ref.items():      # non-finite outputs: only where the reference has them, and the yardstick has the same
        if r is not None: assert V.same_pattern(got[k].double(), r.double()), f'{c.name}: {k}: the fp32 and fp64 non-finite patterns differ'
    if V.needs_yardstick(c):
        for k, y in V.yardstick_errors(c, ref, got).items():
            assert 4*y <= V.YARD_CAP, f'{c.name}: the oracle in fp32 misses {k} by {y:.3g} of its maximum: the bound 4 x that would check nothing; move the values'
    for k, e in V.errors(c, got, ref, ops, got if V.needs_yardstick(c) else None, 0.5).items():
        if not bool(torch.nan_to_num(ref[k].double(), 0.0, 0.0, 0.0).any()): continue      # (exactly 0 everywhere: no relative measure; the kernel is still held to the exact zero)
        spare = 1.0 if c.tol.get(k, c.tol.get('*'))[0] in V.YARD_KINDS else SPARE
        assert e*spare <= 1.0, f'{c.name}: the oracle in fp32 is at {e:.3g} of the bound of {k}: the inputs, not the kernel, are what this case would measure'


def test_view_synth_edges():
    for c, o in _cases('view_synth', 'depth_regimes'):
        yz = L.vs_geometry(o)[0]
        assert bool((yz < 0).any()) and bool((yz == 0).any()) and bool((yz == EPS).any()) and bool(((yz > EPS) & (yz < 0.1)).any()), c.name
        assert bool((yz == 0.09375).any()) and bool((yz == 0.125).any()) and bool((yz == 1).any()), c.name
        assert {float(v) for v in yz.flatten()} == {d - 1 for d in L.VS_DEPTHS}, c.name      # D + tz without a rounding
        assert all(len({float(v) for v in yz[:, :, u].flatten()}) == len(L.VS_DEPTHS) for u in range(yz.shape[2])) or yz.shape[1] < 8, c.name
    for c, o in _cases('view_synth', 'shifts_off_each_side'):
        yz, px, py, sx, sy = L.vs_geometry(o)
        h, w = yz.shape[1:]
        _, ref, _ = _refs(c)
        assert bool((yz == 1).all()), c.name
        assert torch.equal(px[0], px[0].round()) and bool((px[0] == w - 1).any()) and px[0].max() == w + 2 and px[1].min() == -3 and py[2].max() == h and py[3].min() == -1, c.name
        valid = ref['valid'].bool()[:, 0]
        for b in range(4): assert bool(valid[b].any()) and not bool(valid[b].all()), c.name      # whole columns / rows off each side
        assert not bool(valid[0][px[0] == w - 1].any()), c.name
        assert bool((sx[0] == (w - 1)/2).any()) and bool(((sx[0] > w - 1) | (sx[1] < 0)).any()), c.name      # exactly on the centre pixel; beyond the borders
    for c, o in _cases('view_synth', 'on_the_borders'):
        yz, px, py, sx, sy = L.vs_geometry(o)
        assert {float(v) for v in sx[0].flatten()} == {0.0, 2.0} and {float(v) for v in sx[1].flatten()} == {-1.0, 1.0}, c.name
        assert {float(v) for v in sy[2].flatten()} == {0.0, 2.0} and {float(v) for v in sy[3].flatten()} == {-1.0, 1.0}, c.name
        valid = _refs(c)[1]['valid'].bool()[:, 0]
        assert not bool(valid.any()), c.name      # the unshifted coordinate is 0 or 1 = h - 1: |g| is exactly 1 there, which `< 1` refuses in both precisions
    for tag, d in (('depth_1e-6', 1e-6), ('depth_1e6', 1e6)):
        for c, o in _cases('view_synth', tag):
            assert bool((o['depth'] == d).all()) and bool(o['T'][:, :3, 3].all()), c.name
            assert ('g_depth' in _refs(c)[1] and _refs(c)[1]['g_K'] is not None) == (d < 1), c.name      # (the table says why not at 1e6)
    assert {c.name.split('(')[1].split(')')[0] for c in L.CASES if c.op == 'view_synth'} >= {'2,2', '5,9', '33,17'}


def test_photo_error_edges():
    for c, o in _cases('photo_error', 'pred_equals_target'):
        assert torch.equal(o['pred'], o['target']), c.name
        _, ref, _ = _refs(c)
        if '_l2_' in c.name: assert bool((ref['err'] == torch.tensor(EPS, dtype=torch.float64).sqrt()).all()) and not bool(ref['g_pred'].any()), c.name
        if '_l1_' in c.name or '_ssim_c' in c.name: assert ref['err'].abs().max() < 1e-12, c.name
    for c, o in _cases('photo_error', 'constants'):
        assert all(len({float(v) for v in o[k][i, j].flatten()}) == 1 for k in ('pred', 'target') for i in range(2) for j in range(o['pred'].shape[1])) and not torch.equal(o['pred'], o['target']), c.name
    for c, o in _cases('photo_error', 'zero_against_one'): assert not bool(o['pred'].any()) and bool((o['target'] == 1).all()), c.name
    for c, o in _cases('photo_error', 'checker_against_inverse'):
        assert bool((o['pred'] + o['target'] == 1).all()) and bool((o['pred'][..., 1:] != o['pred'][..., :-1]).all()), c.name
        if '_ssim_w1_' in c.name and '(2,2)' not in c.name: assert _refs(c)[1]['err'].max().item() > 0.5, c.name      # SSIM at its most negative
    for k in (12, 4):
        for c, o in _cases('photo_error', f'contrast_2^-{k}'):
            assert {float(v) for v in o['pred'].flatten()} <= {1.0, 1 - 2.0**-k} and o['pred'].min() < 1 and ('_ssim_c' in c.name or '_ssim_w1' in c.name) == (k == 4), c.name
    for c, o in _cases('photo_error', 'scale_1e2'): assert o['pred'].shape[1] == 5 and o['pred'].max() > 90, c.name
    modes = {m for c in L.CASES if c.op == 'photo_error' for m in L.PHOTO_MODES if f'photo_error_{m}_c' in c.name}
    assert modes == set(L.PHOTO_MODES) and {w for _, w in L.PHOTO_MODES.values()} == {0.0, 0.85, 1.0}


def test_recon_reduce_edges():
    for c, o in _cases('recon_reduce', 'identical_supports'):
        assert all(torch.equal(o['ew'][0], e) for e in o['ew']), c.name
        assert not bool(_refs(c)[1]['sel'].any()), c.name      # first index wins
    for c, o in _cases('recon_reduce', 'all_zero'): assert not bool(o['ew'].any()), c.name
    for c, o in _cases('recon_reduce', 'static_ties_warped'):
        assert torch.equal(o['ew'], o['es']) and not bool(o['noise'].any()) and not bool((_refs(c)[1]['sel'] == 255).any()), c.name
    for c, o in _cases('recon_reduce', 'static_one_ulp_smaller'):
        assert bool((o['es'] < o['ew']).all()) and torch.equal(torch.nextafter(o['es'], torch.ones_like(o['es'])*2), o['ew']) and bool((_refs(c)[1]['sel'] == 255).all()), c.name
    for c, o in _cases('recon_reduce', 'explainability'): assert {float(v) for v in o['mask'].flatten()} == {0.0, 1.0}, c.name
    for c, o in _cases('recon_reduce', 'uncertainty_levels'):
        assert [float(o['mask'][i].unique()) for i in range(o['mask'].shape[0])] == [float(torch.tensor(v)) for v in L.UNCERTAINTY_LEVELS], c.name
        assert c.split == dict(err=0, g_err_warp=1, g_mask=0), c.name
    names = [c.name for c in L.CASES if c.op == 'recon_reduce']
    assert any('_n2' in n for n in names) and any('_n3' in n for n in names) and any(n.endswith('_min') for n in names) and any(n.endswith('_mean') for n in names)


def test_regression_edges():
    for c, o in _cases('regression_loss', 'pred_equals_target'): assert torch.equal(o['pred'], o['target']), c.name
    for c, o in _cases('regression_loss', 'ties_at_max_and_delta'):
        diff = (o['pred'].double() - o['target'].double()).abs().flatten()
        assert diff.max() == 5 and int((diff == 5).sum()) == (3 if diff.numel() > 4 else 2) and int((diff == 1).sum()) >= 1, c.name
        assert 0.2*diff.max().item() == 1.0 and (torch.tensor(0.2)*torch.tensor(5.0)).item() == 1.0, c.name      # delta = 1 in both precisions
        if 'mask' in o: assert int(((diff == 5) & ~o['mask'].flatten()).sum()) == 1, c.name
    for c, o in _cases('regression_loss', 'diffs_1e-8_to_1e8'):
        assert {float(v) for v in o['pred'].abs().flatten()} == {float(torch.tensor(v)) for v in L.LOG_DIFFS[:o['pred'].numel()]}, c.name
    for c, o in _cases('regression_loss', 'to_inv_edges'):
        pairs = {(float(p), float(t)) for p, t in zip(o['pred'].flatten(), o['target'].flatten())}
        values = {float(torch.tensor(v)) for v in L.INVERT_VALUES}
        k = 6 if c.name.startswith('regression_l1(') else 5      # (1e6 under l1 only: the table says why)
        assert {p for p, _ in pairs} == {float(torch.tensor(v)) for v in L.INVERT_VALUES[:k]} and len(pairs) == k*k == o['pred'].shape[0], c.name
    for c, o in _cases('regression_loss', 'mask_all_false'):
        assert not bool(o['mask'].any()), c.name
        _, ref, _ = _refs(c)
        assert bool(ref['loss'].isnan()) and bool(ref['g_pred'].isnan().all()), c.name      # what the oracle gives: the kernel is held to this pattern


def test_depth_and_smoothness_edges():
    for c, o in _cases('disp_to_depth'):
        for k in [k for k in o if k.startswith('d')]:
            d = o[k]
            assert bool((d[0] == 1).any()) or d[0].numel() < 4, c.name
            assert len(d[1].unique()) == 1 and bool((d[2] == 0).any()) and (d[2].numel() == 1 or d[2, 0, -1, -1].item() == float(torch.tensor(1e-10))), c.name
        assert not bool(o['d0'][1].any()) and (bool((o['d1'][1] == 1).all())), c.name
        if 'None' in c.name:
            dep = _refs(c)[1]['depth_up']
            assert bool((dep == 0).any()) and dep.max().item() == 1/EPS, c.name      # d = 0 -> 0, 0 < d < eps -> 1/eps
    for c, o in _cases('disp_smooth_fused', 'constant_disp'):
        _, ref, _ = _refs(c)
        assert bool((ref['disp_grad'] == torch.tensor(EPS, dtype=torch.float64).sqrt()).all()) and not any(bool(ref[k].any()) for k in ref if k.startswith('g_d')), c.name
    for op in ('disp_smooth_fused', 'disp_smooth_blurred'):
        for c, o in _cases(op, 'zero_disp'): assert not bool(o['d0'].any()), c.name
        for c, o in _cases(op, 'disp_1e-6'): assert EPS < o['d0'].mean() < 1e-6, c.name
        for c, o in _cases(op, 'constant_image'): assert len(o['imgs'][:, 0].unique()) == 1, c.name
        for c, o in _cases(op, 'checker_image'): assert {float(v) for v in o['imgs'].flatten()} == {0.0, 1.0}, c.name
    for c, o in _cases('disp_smooth_fused', 'constant_image'):
        if 'laplacian0' in c.name: assert bool((_refs(c)[1]['image_grad'] == torch.tensor(EPS, dtype=torch.float64).sqrt()).all()), c.name      # every image difference exactly 0: edge weight exp(-0) = 1
    names = [c.name for c in L.CASES if c.op == 'disp_smooth_fused']
    assert all(any(f'edges{e}_laplacian{l}' in n for n in names) for e in (0, 1) for l in (0, 1))


def test_scale_mean_pose_and_intrinsics_edges():
    for c, o in _cases('scale_mean'):
        for x in o.values(): assert [float(x[i].unique()) for i in range(x.shape[0])] == L.MEAN_LEVELS and L.MEAN_LEVELS[3] < 1, c.name
    (c, o), = _cases('scale_mean', 'bce_ones_n1')
    _, ref, _ = _refs(c)
    assert ref['g_x0'][0].unique().item() < -1e9 and not bool(ref['g_x0'][1].any()), c.name      # ATen's clamps: log(0) -> -100, the quotient's 1e-12
    for c, o in _cases('pose_matrices'):
        assert bool(((o['aa'] != 0).sum(1) == 1).all()) and bool((o['aa'].abs().amax(1) == EPS).any()) and bool(o['inv'].any()) and not bool(o['inv'].all()), c.name
    assert not bool(_cases('pose_matrices', 't_zero')[0][1]['t'].any()) and _cases('pose_matrices', 't_1e4')[0][1]['t'].min() >= 1e4
    for c, o in _cases('intrinsics'):
        assert {float(v) for v in o['fs'].flatten()} >= {float(torch.tensor(1e-3)), 10.0} and {float(v) for v in o['cs'].flatten()} >= {float(torch.tensor(1e-3)), 10.0}, c.name


def test_image_recon_edges():
    for c, o in _cases('image_recon_fused'):
        n, b = o['T'].shape[:2]
        h, w = o['imgs'].shape[-2:]
        for s in range(o['depth'].shape[0]):
            g = dict(depth=o['depth'][s], K=o['K'])
            yz = L.vs_geometry(dict(g, T=o['T'][0]))[0]
            assert {float(v) for v in yz.flatten()} == {d - 1 for d in L.VS_DEPTHS}, c.name
            px = L.vs_geometry(dict(g, T=o['T'][1]))[1]
            assert px.max() > w - 1 and bool((px < w - 1).any()), c.name      # columns off the right side under the second support
        if 'constant_target' in c.name: assert all(len(o['imgs'][:, ch].unique()) == 1 for ch in range(3)) and len(o['supp'].unique()) > 3, c.name
        if 'supports_equal_target' in c.name: assert all(torch.equal(s, o['imgs']) for s in o['supp']), c.name
        assert not bool(_refs(c)[1]['sel'].any()), c.name
    assert any('constant_target' in c.name for c in L.CASES if c.op == 'image_recon_fused')
    assert {c.name.split(')')[0] for c in L.CASES if c.op == 'image_recon_fused'} == {'image_recon_fused(1,6,20', 'image_recon_fused(2,33,47'}


def test_judge_refuses_an_error_inside_a_small_scale_slice():
    """The gradient to the error maps under the uncertainty mask of 50 is exp(-50) of the one under the mask of 0.  One element of that slice off by 10 x the bound:
    the whole-tensor measure accepts it, the per-level judge does not."""
    c = next(c for c in L.CASES if c.name == 'recon_reduce_n2(2, 5, 7)_uncertainty_levels_mean')
    ops, ref, _ = _refs(c)
    bound = c.tol['*']
    V.judge(c, {k: (None if v is None else v.clone()) for k, v in ref.items()}, ref)
    g = ref['g_err_warp']
    assert g[:, -1].abs().max() < 1e-20*g.abs().max()
    wrong = g.clone()
    wrong[1, -1, 2, 3] += 10*bound[1]*g[:, -1].abs().max()
    assert rel_to_max(wrong, g) <= bound[1]
    assert V.excess(wrong, g, bound) <= 1.0 < V.excess(wrong, g, bound, c.split['g_err_warp'])
    with pytest.raises(AssertionError, match='g_err_warp misses its bound'): V.judge(c, dict(ref, g_err_warp=wrong), ref)
