"""The offline-evaluation kernels (csrc/smd_eval.hip) and the evaluator on the GPU: the align-and-score operator against the REFERENCE's fixture
(tests/golden/eval_reference.npz) under the bounds of test_eval_host.py (`check_case`; both errors per quantity go to profiles/eval_parity.txt through the
parity log), its resize against ATen's, the point-cloud operator against the reference's per-query distances and at the shapes where it can go wrong,
status reporting, bit reproducibility, hostile memory, and `run` end to end against the plain path.

Shapes: the fixture's 24x32 and 33x47; the point-cloud cases put n masked pixels into 24x32 (768 slots, one database slice) or 48x64 (3072 slots, two
slices): n = 256 / 257 is a database of one LDS tile / one tile + 1, n = 1 a single query that is its own neighbour's only candidate, odd and even n move
the `[::2]` boundary, n = 2100 needs three query tiles' worth of lanes in two of which nothing is left to do."""
import numpy as np
import pytest
import torch

from conftest import load_golden, parity_note
from eval_inputs import EVAL_CASES, eval_case, eval_expected, eval_kwargs
from hostile_memory import Arena, assert_finite, hostile
from test_eval_host import aligned_depth, check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def E():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import eval_metrics
    return eval_metrics


@pytest.fixture(scope='module')
def fixture(): return load_golden('eval_reference')


def _ev(k, **over):
    from slowtv_monodepth_amd.evaluator import MonoDepthEvaluator
    return MonoDepthEvaluator(**{**eval_kwargs(k), **over}, device='cuda')


def _cuda(ins):
    return (torch.from_numpy(ins['pred']).cuda(), torch.from_numpy(ins['target']).cuda(), None if ins['mask'] is None else torch.from_numpy(ins['mask']).cuda())


def _operator(E, k, fixture, **kw):
    c = EVAL_CASES[k]
    p, t, m = _cuda(eval_case(k, fixture))
    mode = c['align'] if c['align'] in ('median', 'lsqr') else 'factor'
    return E.eval_metrics(p[None, None], t[None, None], None if m is None else m[None, None], min_depth=1e-3, max_depth=c['max'], align=mode,
                          factor=c['align'] if mode == 'factor' else 1.0, **kw)


@pytest.mark.parametrize('k', range(len(EVAL_CASES)), ids=[c['name'] for c in EVAL_CASES])
def test_the_evaluator_matches_the_reference_fixture(E, fixture, k):
    """The fused path on one item: keys in the reference's merge order, every value within its bound, `{}` for the empty item; under 'median' both medians
    are the reference's bits."""
    ins = eval_case(k, fixture)
    p, t, m = _cuda(ins)
    ev = _ev(k)
    assert ev._fused(p, t)
    got = ev(p, t, list(EVAL_CASES[k]['metrics']), K=ins['K'], mask=m)
    assert check_case(k, got, fixture, 'fused') == []
    ref, _, _, med = eval_expected(fixture, k)
    r = _operator(E, k, fixture)
    if not ref: assert int(r['status'][0]) == 1 and int(r['counts'][0]) == 0 and got == {}
    elif EVAL_CASES[k]['align'] == 'median':
        mine = r['medians'][0].cpu()
        assert mine[0].numpy().tobytes() == med[0].numpy().tobytes() and mine[1].numpy().tobytes() == med[1].numpy().tobytes()
        assert float(r['values'][0, 0]) == float(med[1]/med[0])                       # the float32 ratio itself


@pytest.mark.parametrize('interp', ['bilinear', 'nearest'])
@pytest.mark.parametrize('shape', [(5, 7), (12, 16)])
def test_the_resize_is_atens(E, shape, interp):
    """-> 24x32: the up-sampled disparity bit-equal to `interpolate` for 'nearest', within one ulp for 'bilinear' (align_corners=False)."""
    g = torch.Generator().manual_seed(5)
    d = (0.05 + torch.rand(2, 1, *shape, generator=g)).cuda()
    t = (1 + torch.rand(2, 1, 24, 32, generator=g)).cuda()
    got = E.eval_metrics(d, t, align='factor', interp=interp, want_resized=True)['resized']
    kw = {} if interp == 'nearest' else {'align_corners': False}
    want = torch.nn.functional.interpolate(d, size=(24, 32), mode=interp, **kw)
    if interp == 'nearest': assert torch.equal(got, want)
    else:
        ulps = (got.view(torch.int32) - want.view(torch.int32)).abs().max().item()
        parity_note(f'eval_parity resize {shape} -> (24, 32) bilinear: at most {ulps} ulp from ATen')
        assert ulps <= 1


def _cloud_inputs(n, shape=(24, 32), b=1, seed=0, coincident=False, first=None):
    """b items with exactly n masked pixels each (`first`: the flat index of the first one; the rest are drawn), a depth 2 .. 4 and a target within 2 % of it
    (or equal to it), and one K per item."""
    h, w = shape
    g = torch.Generator().manual_seed(100 + seed)
    depth = 2 + 2*torch.rand(b, 1, h, w, generator=g)
    target = depth.clone() if coincident else depth*(1 + 0.04*(torch.rand(b, 1, h, w, generator=g) - 0.5))
    mask = torch.zeros(b, h*w, dtype=torch.bool)
    for i in range(b):
        lo = 0 if first is None else first
        idx = lo + torch.randperm(h*w - lo, generator=g)[:n]
        if first is not None: idx[0] = first
        mask[i, idx] = True
    K = torch.eye(4).repeat(b, 1, 1)
    for i in range(b): K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2] = 20.5 + 3*i, 21.25 + 2*i, w/2 - 0.25, h/2 + 0.5 + i
    return depth, target, mask.view(b, 1, h, w), K


def _cloud_check(E, depth, target, mask, K, what):
    """Operator against the plain sequence on the CPU: per-query distances to 1e-6 (float64 distances rounded to float32 there), zeros past the query count,
    counts identical unless a distance lies within 1e-5 of a threshold (then the case is mis-drawn: fail), Chamfer to 2e-6, F-Score / IoU to 1e-6."""
    from slowtv_monodepth_amd.evaluator import backproject, plain_chamfer, plain_pointcloud
    K_inv = torch.linalg.inv(K)
    nn, stats, counts = E.eval_pointcloud(depth.cuda(), target.cuda(), mask.cuda(), K_inv.cuda())
    nn, stats, counts = nn.cpu(), stats.cpu(), counts.cpu()
    assert_finite(nn, f'{what}: nn'); assert_finite(stats, f'{what}: stats')
    for i in range(depth.shape[0]):
        m = mask[i, 0].flatten()
        n = int(m.sum()); nq = (n + 1)//2
        assert int(counts[i]) == n
        want = plain_chamfer(backproject(depth[i, 0], K_inv[i])[m], backproject(target[i, 0], K_inv[i])[m])
        for d in range(2):
            assert torch.all((nn[i, d, :nq] - want[d]).abs() <= 1e-6*want[d]), f'{what}: item {i} direction {d}'
            assert not nn[i, d, nq:].any()
            for th in (0.05, 0.1, 0.2): assert ((want[d].double()/th - 1).abs() > 1e-5).all(), f'{what}: a distance within 1e-5 of {th}: draw other inputs'
        got, ref = E.pointcloud_values(stats[i].tolist(), n), plain_pointcloud(depth[i, 0], target[i, 0], mask[i, 0], K[i])
        assert list(got) == list(ref)
        for name in got: assert abs(got[name] - ref[name]) <= (2e-6 if name == 'Chamfer' else 1e-6)*abs(ref[name]), (what, i, name, got[name], ref[name])
    return nn, stats, counts


def test_the_nearest_neighbours_match_the_reference_fixture(E, fixture):
    """Per-query distances of both directions against `_chamfer_dist`'s, from the reference's aligned depth: <= 1e-6 relative (d^2 from correctly rounded
    differences carries about 4*2^-24; the reference's are float64 distances rounded to float32)."""
    worst = 0.0
    for k in range(len(EVAL_CASES)):
        ref, p_nn, t_nn, _ = eval_expected(fixture, k)
        if not ref: continue
        depth, mask, ins = aligned_depth(k, fixture)
        K_inv = torch.linalg.inv(torch.from_numpy(ins['K']))[None].cuda()
        nn, stats, counts = E.eval_pointcloud(torch.from_numpy(depth)[None, None].cuda(), torch.from_numpy(ins['target'])[None, None].cuda(),
                                              torch.from_numpy(mask)[None, None].cuda(), K_inv)
        nq = len(p_nn)
        assert int(counts[0]) == int(mask.sum()) and nq == (int(mask.sum()) + 1)//2
        for d, want in enumerate((p_nn, t_nn)):
            got = nn[0, d, :nq].cpu().numpy()
            assert np.all(np.abs(got - want) <= 1e-6*want), f'case {k} direction {d}'
            if (want > 0).all(): worst = max(worst, float(np.abs(got/want - 1).max()))
    parity_note(f'eval_parity nearest-neighbour distances against the reference\'s: at most {worst:.3e} relative (bound 1e-6)')


@pytest.mark.parametrize('n, shape', [(256, (24, 32)), (257, (24, 32)), (1, (24, 32)), (2, (24, 32)), (641, (24, 32)), (768, (24, 32)), (2100, (48, 64)),
                                      (2049, (48, 64))], ids=lambda v: str(v).replace(' ', ''))
def test_point_cloud_shapes_where_it_can_go_wrong(E, n, shape):
    _cloud_check(E, *_cloud_inputs(n, shape, seed=n), f'n = {n} in {shape}')


def test_point_cloud_first_valid_pixel_ends_a_row_and_three_intrinsics(E):
    _cloud_check(E, *_cloud_inputs(40, first=31, seed=1), 'first valid pixel = last pixel of row 0')
    _cloud_check(E, *_cloud_inputs(333, b=3, seed=2), 'b = 3 with three different K')


def test_point_cloud_coincident_points_and_the_early_return(E):
    """Equal clouds: every distance 0, P = R = 1.  Clouds 10 m apart: P = R = 0 at every threshold: `_metrics_pts` returns (0, 0)."""
    d, t, m, K = _cloud_inputs(301, coincident=True, seed=3)
    nn, stats, counts = E.eval_pointcloud(d.cuda(), t.cuda(), m.cuda(), torch.linalg.inv(K).cuda())
    assert not nn.any() and stats[0, :, 1:].cpu().tolist() == [[151.0]*3]*2
    v = E.pointcloud_values(stats[0].cpu().tolist(), int(counts[0]))
    assert v['Chamfer'] == 0 and abs(v['F-Score (10)'] - 100*2/(2 + 1e-5)) < 1e-9 and abs(v['IoU (5)'] - 100/(1 + 1e-5)) < 1e-9
    nn, stats, counts = E.eval_pointcloud(d.cuda(), (d + 10).cuda(), m.cuda(), torch.linalg.inv(K).cuda())
    v = E.pointcloud_values(stats[0].cpu().tolist(), int(counts[0]))
    assert [v[k] for k in list(v)[1:]] == [0.0]*6 and v['Chamfer'] > 1


def test_status_is_reported_and_unscored_items_leave_the_batch_alone(E, fixture):
    """A batch of a scored item, one with an empty mask and one whose disparity is all zero: status per item, zeros (never NaN) in their rows, the scored
    item's bits those of a batch of its own, `{}` from the evaluator.  SMD_EVAL_ZERO_PRED mirrors `pred_mask.sum() == 0`, which `pred > 0` in the mask
    leaves unreachable for any finite input: an all-zero prediction is reported as an empty mask, as the reference returns at its first check."""
    p, t, _ = _cuda(eval_case(0, fixture))
    ps, ts = torch.stack([p, p, torch.zeros_like(p)])[:, None], torch.stack([t, torch.zeros_like(t), t])[:, None]
    for mode in ('median', 'lsqr', 'factor'):
        r, one = E.eval_metrics(ps, ts, align=mode, want_depth=True), E.eval_metrics(ps[:1], ts[:1], align=mode, want_depth=True)
        assert r['status'].tolist() == [0, 1, 1] and r['counts'].tolist()[1:] == [0, 0] and E.STATUS[1] == 'empty mask'
        assert_finite(r['values'], 'values'); assert_finite(r['depth'], 'depth')
        assert not r['values'][1:].any() and not r['depth'][1:].any() and torch.equal(r['values'][0], one['values'][0]) and torch.equal(r['depth'][0], one['depth'][0])
    ev = _ev(0)
    assert ev._fused_group(ps[:, 0], ts[:, 0], None, None, ['eigen'])[1:] == [{}, {}]


def test_two_calls_and_a_second_stream_give_the_same_bits(E, fixture):
    k = 2
    first = _operator(E, k, fixture, want_depth=True, want_valid=True)
    again = _operator(E, k, fixture, want_depth=True, want_valid=True)
    ins = eval_case(k, fixture)
    K_inv = torch.linalg.inv(torch.from_numpy(ins['K']))[None].cuda()
    t = torch.from_numpy(ins['target'])[None, None].cuda()
    pc = E.eval_pointcloud(first['depth'], t, first['valid'], K_inv)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = _operator(E, k, fixture, want_depth=True, want_valid=True)
        pc2 = E.eval_pointcloud(other['depth'], t, other['valid'], K_inv)
    s.synchronize()
    for name in ('values', 'counts', 'status', 'medians', 'depth', 'valid'):
        assert torch.equal(first[name], again[name]) and torch.equal(first[name], other[name]), name
    for a, b in zip(pc, pc2): assert torch.equal(a, b)


@pytest.mark.parametrize('shift', [0, 1, 3], ids=['aligned', 'shifted1', 'shifted3'])
@pytest.mark.parametrize('mode', ['median', 'lsqr'])
def test_the_operators_in_hostile_memory(E, fixture, mode, shift):
    """Operands, outputs and workspaces in poisoned, guarded blocks, the operands `shift` elements off their 16-byte alignment: nothing read that nobody wrote (no NaN in any
    output), nothing written outside (guard bands intact), and the bits of an ordinary call."""
    ins = eval_case(2, fixture)                        # 33x47: no multiple of anything
    p, t, _ = _cuda(ins)
    m = (torch.rand(33, 47, generator=torch.Generator().manual_seed(9)) < 0.7).cuda()
    kw = dict(min_depth=1e-3, max_depth=5.0, align=mode, want_depth=True, want_valid=True, want_resized=True)
    K_inv = torch.linalg.inv(torch.from_numpy(ins['K']))[None].cuda()
    want = E.eval_metrics(p[None, None], t[None, None], m[None, None], **kw)
    want_pc = E.eval_pointcloud(want['depth'], t[None, None], want['valid'], K_inv)
    arena = Arena()
    gp, gt, gm, gk = (arena.guarded(v, shift) for v in (p[None, None], t[None, None], m[None, None].to(torch.uint8), K_inv))
    with hostile(arena):                               # (the blocks the operators allocate stay 16-byte aligned, as the allocator's are)
        got = E.eval_metrics(gp, gt, gm, **kw)
        got_pc = E.eval_pointcloud(got['depth'], gt, got['valid'], gk)
    arena.check()
    for name, v in got.items():
        assert_finite(v, name); assert torch.equal(v, want[name]), name
    for name, a, b in zip(('nn', 'stats', 'counts'), got_pc, want_pc):
        assert_finite(a, name); assert torch.equal(a, b), name


def test_run_end_to_end_against_the_plain_path(E, fixture, monkeypatch):
    """Five items of three (prediction, target) shape pairs, resized bilinearly, `max_items=4`: every value of the fused `run` within 1e-5 relative of the plain
    path's on the same GPU (the resize differs by an ulp of the disparity, which the means pass on; a value that is a count over n may differ by the few
    counts such an ulp can flip: 4 counts of the at least 300 queries and pixels here), and ONE device-to-host copy per shape group (counted)."""
    from slowtv_monodepth_amd import evaluator as V
    g = torch.Generator().manual_seed(11)
    shapes = [((12, 16), (24, 32)), ((24, 32), (24, 32)), ((12, 16), (24, 32)), ((17, 23), (33, 47)), ((12, 16), (24, 32))]
    preds, targets, Ks = [], [], []
    for (h, w), (H, W) in shapes:
        depth = 2 + 3*torch.rand(1, 1, h, w, generator=g)
        t = torch.nn.functional.interpolate(depth, size=(H, W), mode='bilinear', align_corners=False)[0, 0]*(1 + 0.02*(torch.rand(H, W, generator=g) - 0.5))
        t[torch.rand(H, W, generator=g) < 0.1] = 0
        preds.append((1/(1.9*depth[0, 0])).numpy()); targets.append(t.numpy())
        Ks.append(np.array([[20.5, 0, W/2, 0], [0, 21.5, H/2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32))
    data = {'depth': targets, 'K': Ks, 'cat': list('abcde'), 'subcat': list('vwxyz')}
    copies = []
    monkeypatch.setattr(V, '_to_host', lambda t: (copies.append(tuple(t.shape)), t.cpu())[1])
    kw = dict(metrics=('eigen', 'benchmark', 'pointcloud'), align_mode='median', max=10.0)
    mean, items = V.MonoDepthEvaluator(**kw, device='cuda').run(preds, data, max_items=4)
    assert sorted(copies) == [(1, 31), (1, 31), (2, 31)] and len(items) == 4 and [m['Cat'] for m in items] == list('abcd')

    class Plain(V.MonoDepthEvaluator):                 # an overridden step: the plain path, on the GPU
        def get_mask(self, target): return super().get_mask(target)
    copies.clear()
    mean2, items2 = Plain(**kw, device='cuda').run(preds, data, max_items=4)
    assert not copies and list(mean) == list(mean2)
    for a, b in zip(items, items2):
        assert list(a) == list(b)
        for name in a:
            if not isinstance(a[name], float): continue
            counted = name.startswith(('F-Score', 'IoU', '$'))
            assert abs(a[name] - b[name]) <= (100*4/300 if counted else 1e-5*abs(b[name]) + 1e-12), (name, a[name], b[name])
