"""Image logging on the GPU: the fused `rgb_from_disp`, `rgb_from_feat` and `make_grid` (csrc/smd_viz.hip) against the REFERENCE's fixture
(tests/golden/viz_reference.npz) and against plain slicing, in hostile memory, at the value edges, and `HeavyLogger.log_step` end to end.

Bounds.  rgb_from_disp: vmax bit-equal to the fixture's float32 and the same colour at every pixel (the kernel repeats numpy's float32 statements; the
generator checked that no index of these inputs hangs on a rounding) — the fixture's float64 table entries rounded to float32 are the expected bits.
rgb_from_feat: the error against `viz_inputs.pca_fp64` (the test's own float64 PCA) is at most four times the recorded error of the reference's float32
result against it; the measured errors go to the parity log.  make_grid: bit-equal to a grid built here with slicing."""
import numpy as np
import pytest
import torch

from conftest import load_golden, parity_note
from hostile_memory import Arena, hostile
from test_viz_host import GRID_CASES, grid_by_slicing
from viz_inputs import DISP_CASES, FEAT_CASES, pca_fp64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture(): return load_golden('viz_reference')


@pytest.fixture(scope='module')
def V():
    from slowtv_monodepth_amd import viz
    return viz


@pytest.mark.parametrize('k', range(len(DISP_CASES)), ids=[c[0] for c in DISP_CASES])
def test_rgb_from_disp_matches_the_reference_fixture(V, fixture, k):
    _, shape, invert = DISP_CASES[k]
    d = fixture[f'disp_in_{k}'].cuda()
    rgb, vmax = V._fused_disp(d, invert, 'turbo', 0, None)
    assert vmax.cpu().numpy().tobytes() == fixture[f'disp_vmax_{k}'].numpy().tobytes(), (vmax.tolist(), fixture[f'disp_vmax_{k}'].tolist())
    want = fixture[f'disp_out_{k}'].to(torch.float32)
    got = V.rgb_from_disp(d, invert=invert).cpu()
    assert got.dtype == torch.float32 and torch.equal(got, rgb.cpu())
    mismatches = int((got != want).any(dim=1).sum())
    print(f'viz_parity disp case {k} {DISP_CASES[k][0]}: {mismatches} of {got[:, 0].numel()} pixels with another colour')
    assert mismatches == 0
    # the accepted ranks, and a caller's vmax (a number, one per item)
    assert torch.equal(V.rgb_from_disp(d[0], invert=invert).cpu(), got[0]) and torch.equal(V.rgb_from_disp(d[0, 0], invert=invert).cpu(), got[0])
    vm = fixture[f'disp_vmax_{k}'].tolist()
    if not invert:
        assert torch.equal(V.rgb_from_disp(d, vmax=vm).cpu(), V.plain_rgb_from_disp(d.cpu(), vmax=vm).to(torch.float32))
        assert torch.equal(V.rgb_from_disp(d, vmax=0.5, vmin=0.1, cmap='magma').cpu(), V.plain_rgb_from_disp(d.cpu(), vmax=0.5, vmin=0.1, cmap='magma').to(torch.float32))


@pytest.mark.parametrize('k', range(len(FEAT_CASES)), ids=[c[0] for c in FEAT_CASES])
def test_rgb_from_feat_is_within_four_times_the_references_own_error(V, fixture, k):
    x = fixture[f'feat_in_{k}']
    exact = pca_fp64(x.numpy())
    got = V.fused_rgb_from_feat(x.cuda())             # the kernels themselves: the public name routes (1,512,3,5) to the plain path (`feat_routed_plain`)
    again = V.fused_rgb_from_feat(x.cuda())
    nc = FEAT_CASES[k][2]                              # comparable channels (c512_n3: two non-zero eigenvalues)
    e_mine = float(np.abs(got.cpu().numpy().astype(np.float64) - exact)[:, :nc].max())
    e_ref = float(np.abs(fixture[f'feat_out_{k}'].numpy().astype(np.float64) - exact)[:, :nc].max())
    line = f'viz_parity feat case {k} {FEAT_CASES[k][0]} {tuple(x.shape)}: error {e_mine:.3e} reference\'s {e_ref:.3e} (recorded {float(fixture[f"feat_err_{k}"]):.3e}, solver {fixture[f"feat_solver_{k}"]}) bound {4*e_ref:.3e}'
    parity_note(line); print(line)
    assert got.dtype == torch.float32 and got.shape == (x.shape[0], 3) + tuple(x.shape[2:])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two runs must be bit-equal'
    assert abs(e_ref - float(fixture[f'feat_err_{k}'])) <= 1e-12
    assert e_mine <= 4*e_ref
    routed = V.feat_routed_plain(x.shape[1], x.shape[0]*x.shape[2]*x.shape[3])
    assert routed == FEAT_CASES[k][0].startswith('c512')
    pub = V.rgb_from_feat(x.cuda())
    assert pub.is_cuda and pub.dtype == torch.float32
    if not routed: assert torch.equal(pub, got)
    if x.shape[0] == 1 and not routed: assert torch.equal(V.rgb_from_feat(x[0].cuda()), got[0])       # the (c,h,w) rank


@pytest.mark.parametrize('case', GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_make_grid_is_bit_equal_to_slicing(V, case):
    _, x, normalize = case
    got = V.make_grid(x.cuda(), 6, 2, normalize=normalize)
    assert torch.equal(got.cpu(), grid_by_slicing(x, 6, 2, normalize=normalize))


@pytest.mark.parametrize('shift', [0, 1, 3], ids=['aligned', 'shifted1', 'shifted3'])
def test_the_operators_in_hostile_memory(V, fixture, shift):
    """Operands in poisoned, guarded blocks `shift` elements off their alignment, outputs and workspaces in poisoned blocks: the bits of an ordinary call,
    nothing written outside."""
    d, f = fixture['disp_in_1'].cuda(), fixture['feat_in_2'].cuda()
    m = (fixture['disp_in_1'] > 0.5).cuda()
    want = (V.rgb_from_disp(d), V.rgb_from_disp(d, invert=True), V.rgb_from_feat(f), V.rgb_from_feat(fixture['feat_in_1'].cuda()), V.make_grid(d, normalize=True),
            V.make_grid(m))
    arena = Arena()
    gd, gf, gf1, gm = arena.guarded(d, shift), arena.guarded(f, shift), arena.guarded(fixture['feat_in_1'].cuda(), shift), arena.guarded(m.view(torch.uint8), shift)
    with hostile(arena):
        got = (V.rgb_from_disp(gd), V.rgb_from_disp(gd, invert=True), V.rgb_from_feat(gf), V.rgb_from_feat(gf1), V.make_grid(gd, normalize=True), V.make_grid(gm))
    for a, b in zip(got, want): assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
    arena.check()


def _same_bits_or_nan(a, b): return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_the_value_edges_follow_the_plain_path(V):
    """All-zero features (the maximum after the subtraction is 0: 0/0, NaN everywhere, as in the reference), one-hot features with distinct class counts
    (distinct eigenvalues), and a disparity of inf."""
    zeros = torch.zeros(1, 4, 3, 5)
    with pytest.warns(RuntimeWarning): want = V.plain_rgb_from_feat(zeros)
    got = V.rgb_from_feat(zeros.cuda()).cpu()
    assert torch.isnan(want).all() and torch.isnan(got).all()
    cls = torch.tensor([0]*11 + [1]*7 + [2]*4 + [3]*2).reshape(1, 4, 6)
    onehot = torch.nn.functional.one_hot(cls, 4).permute(0, 3, 1, 2).float()
    got, want = V.rgb_from_feat(onehot.cuda()).cpu(), V.plain_rgb_from_feat(onehot)
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 4e-6, float((got - want).abs().max())
    d = torch.rand(2, 1, 4, 6, generator=torch.Generator().manual_seed(3)) + 0.1
    d[0, 0, 1, 2] = float('inf'); d[1, 0, 3, :] = float('inf'); d[1, 0, 0, 0] = float('-inf')
    for invert in (False, True):
        with np.errstate(invalid='ignore'): want = V.plain_rgb_from_disp(d, invert=invert).to(torch.float32)
        assert _same_bits_or_nan(V.rgb_from_disp(d.cuda(), invert=invert).cpu(), want), invert


def test_the_fused_path_refuses_what_sklearn_refuses(V):
    with pytest.raises(ValueError, match='n_components=3'): V.rgb_from_feat(torch.zeros(1, 2, 4, 4).cuda())
    with pytest.raises(ValueError, match='n_components=3'): V.rgb_from_feat(torch.zeros(1, 8, 1, 2).cuda())
    with pytest.raises(ValueError, match='Non-matching vmax'): V.rgb_from_disp(torch.rand(2, 1, 3, 3).cuda(), vmax=[1.0])


def test_log_step_end_to_end_matches_the_plain_path(V, tmp_path):
    """`HeavyLogger.log_step` for the resnet18 configuration at b = 2, 64 x 96 (24 x 32 is below what the ResNet-18 decoder can pad) into an NpyWriter: the reference's keys, every grid finite, and each grid
    equal to the plain path's grid of the same tensors (colour maps: the same colour at every pixel; images and masks: the same bits)."""
    from test_viz_host import EXPECTED_KEYS, tiny_module_and_batch
    from slowtv_monodepth_amd.heavy_logger import HeavyLogger, NpyWriter, RecordingWriter
    module, batch = tiny_module_and_batch('resnet18', device='cuda')
    writer, rec = NpyWriter(tmp_path), RecordingWriter()
    logger = HeavyLogger(n_imgs=6, n_cols=2)
    with torch.no_grad(): _, loss_dict, fwd = module.step(tuple(dict(d) for d in batch), mode='train')
    for lg, w in ((logger, writer), (HeavyLogger(6, 2, plain=True), rec)):           # both paths on the SAME tensors
        lg.mode, lg.step, lg.writer = 'train', 3, w
        lg.log_batch(batch); lg.log_fwd(fwd); lg.log_loss(loss_dict, batch[0]['supp_idxs'])
    files = {p.name for p in tmp_path.glob('*.npy')}
    assert files == {f'train_{k.replace("/", "-")}_000003.npy' for k in EXPECTED_KEYS['resnet18']}, files
    assert (tmp_path/'text.jsonl').is_file()
    for key, grid, _ in rec.images:
        got = np.load(tmp_path/f'{key.replace("/", "-")}_000003.npy')
        assert np.isfinite(got).all() and got.shape == tuple(grid.shape), key
        if '_feats/' in key: continue      # compared below: an untrained encoder's components are not comparable between two PCA routes
        want = grid.to(torch.float32).cpu().numpy()
        assert np.array_equal(got, want), (key, float(np.abs(got - want).max()))
    # the `feats/` grids.  (1) Wiring, on the step's own encoder features, level by level: the logger's grid is `make_grid(rgb_from_feat(f))` of the same
    # tensor, bit for bit.  The deepest level (512 channels, 12 samples) is routed to the plain path (`viz.feat_routed_plain`), where sklearn's 'auto' runs
    # its randomized solver on numpy's global generator: it is seeded before both evaluations.
    assert len(fwd['depth_feats']) == 5 and V.feat_routed_plain(fwd['depth_feats'][4].shape[1], 2*2*3)
    for s_, f in enumerate(fwd['depth_feats']):
        one = RecordingWriter()
        logger.writer = one
        np.random.seed(0); logger.log_fwd({'depth_feats': [f], 'disp': {}})
        np.random.seed(0); want = V.make_grid(V.rgb_from_feat(f), 6, 2)[None]
        (key, grid, _), = one.images
        assert key == 'train_feats/target_0' and torch.equal(grid, want), s_
        assert np.array_equal(np.load(tmp_path/f'train_feats-target_{s_}_000003.npy').shape, tuple(want.shape))
    # (2) Values, on the fixture's features (separated eigenvalues, deterministic solvers: c16 and c64 run `full`): the fused logger's grid against the
    # plain logger's, within 4x the reference's recorded error (the kernels' bound) + 1x (the plain path's own), both against the same float64 PCA.
    fixture = load_golden('viz_reference')
    for k in (1, 2):
        f = fixture[f'feat_in_{k}'].cuda()
        grids = []
        for plain in (False, True):
            one = RecordingWriter()
            lg = HeavyLogger(6, 2, writer=one, plain=plain); lg.mode, lg.step = 'train', 3
            lg.log_fwd({'depth_feats': [f], 'disp': {}, 'autoenc_feats': [f]})
            assert [key for key, _, _ in one.images] == ['train_feats/target_0', 'train_feats/autoenc_0']
            grids.append(one.images[0][1].cpu())
        err = float((grids[0] - grids[1]).abs().max())
        print(f'viz_parity logger feats case {k}: fused against plain grid {err:.3e} bound {5*float(fixture[f"feat_err_{k}"]):.3e}')
        assert grids[0].shape == grids[1].shape and err <= 5*float(fixture[f'feat_err_{k}'])
    logger.writer = writer
    HeavyLogger(6, 2).log_step(module, batch, 'val', 4, writer=NpyWriter(tmp_path/'val'))
    assert len(list((tmp_path/'val').glob('*.npy'))) == len(EXPECTED_KEYS['resnet18']) - 3


def test_log_step_key_set_with_a_predictive_mask(tmp_path):
    """cfg/kitti_sfm_learner.yaml's whole step on the GPU (the CPU oracle has no masked reconstruction): the reference's keys, every grid finite."""
    from test_viz_host import EXPECTED_KEYS, tiny_module_and_batch
    from slowtv_monodepth_amd.heavy_logger import HeavyLogger, RecordingWriter
    module, batch = tiny_module_and_batch('sfm_learner', device='cuda')
    rec = RecordingWriter()
    HeavyLogger(6, 2).log_step(module, batch, 'train', 0, writer=rec)
    assert sorted(k for k, _, _ in rec.images) == [f'train_{k}' for k in EXPECTED_KEYS['sfm_learner']]
    assert all(torch.isfinite(v).all() and v.is_cuda for _, v, _ in rec.images)
