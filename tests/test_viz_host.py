"""Image logging on the CPU: the plain path of `viz` against the REFERENCE's fixture (tests/golden/viz_reference.npz), the committed colour tables against
matplotlib's, the percentile restatement against np.percentile, the grid geometry against slicing, `HeavyLogger`'s keys per configuration, the C symbols and
`train.py --log-images`."""
import importlib.util
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from viz_inputs import DISP_CASES, FEAT_CASES

NEW_SYMBOLS = ('smd_viz_disp_workspace_bytes', 'smd_viz_disp', 'smd_viz_feat_workspace_bytes', 'smd_viz_feat_moments', 'smd_viz_feat_project',
               'smd_make_grid_workspace_bytes', 'smd_make_grid')
HAVE_MPL = importlib.util.find_spec('matplotlib') is not None
HAVE_SK = importlib.util.find_spec('sklearn') is not None


def _imgs(b, c, h, w, seed): return torch.rand(b, c, h, w, generator=torch.Generator().manual_seed(seed)) - 0.25


# name, input, normalize — `n_imgs=6, n_cols=2` throughout: b = 1 (the image itself), 5 (an empty cell), 6, 7 (one image dropped), one channel, bool
GRID_CASES = [('b1', _imgs(1, 3, 5, 7, 1), False), ('b5', _imgs(5, 3, 5, 7, 2), False), ('b6', _imgs(6, 3, 4, 3, 3), False), ('b7', _imgs(7, 3, 5, 7, 4), False),
              ('b5_normalize', _imgs(5, 3, 5, 7, 5), True), ('one_channel', _imgs(5, 1, 5, 7, 6), True), ('bool', _imgs(6, 1, 5, 7, 7) > 0.2, False),
              ('uint8', (_imgs(3, 1, 5, 7, 8)*200).clamp(0).to(torch.uint8), True)]


def grid_by_slicing(x, n_imgs, nrow, normalize=False, padding=2):
    """torchvision's documented grid with plain slicing: images left to right, top to bottom, `padding` pixels of 0 around each; one image alone is returned
    as it is; normalize: the extrema of the images shown, `scale_each=False`."""
    x = x[:n_imgs].float()
    if x.shape[1] == 1: x = torch.cat([x, x, x], dim=1)
    if normalize:
        lo, hi = float(x.min()), float(x.max())
        x = (x.clamp(lo, hi) - lo)/max(hi - lo, 1e-5)
    n, _, h, w = x.shape
    if n == 1: return x[0]
    cols = min(nrow, n); rows = (n + cols - 1)//cols
    out = torch.zeros(3, rows*(h + padding) + padding, cols*(w + padding) + padding)
    for k in range(n):
        r, c = divmod(k, cols)
        out[:, padding + r*(h + padding):padding + r*(h + padding) + h, padding + c*(w + padding):padding + c*(w + padding) + w] = x[k]
    return out


@pytest.fixture(scope='module')
def fixture(): return load_golden('viz_reference')


@pytest.mark.skipif(not HAVE_MPL, reason='the plain path of rgb_from_disp needs matplotlib')
@pytest.mark.parametrize('k', range(len(DISP_CASES)), ids=[c[0] for c in DISP_CASES])
def test_the_plain_rgb_from_disp_equals_the_fixture(fixture, k):
    from slowtv_monodepth_amd import viz
    got = viz.rgb_from_disp(fixture[f'disp_in_{k}'], invert=DISP_CASES[k][2])
    assert got.dtype == torch.float64 and torch.equal(got, fixture[f'disp_out_{k}'])
    hwc = viz.rgb_from_disp(fixture[f'disp_in_{k}'].permute(0, 2, 3, 1).numpy(), invert=DISP_CASES[k][2])      # numpy: (b,h,w,1) -> (b,h,w,3)
    assert isinstance(hwc, np.ndarray) and np.array_equal(hwc, fixture[f'disp_out_{k}'].permute(0, 2, 3, 1).numpy())


@pytest.mark.skipif(not HAVE_SK, reason='the plain path of rgb_from_feat needs sklearn')
@pytest.mark.parametrize('k', range(len(FEAT_CASES)), ids=[c[0] for c in FEAT_CASES])
def test_the_plain_rgb_from_feat_equals_the_fixture(fixture, k):
    from slowtv_monodepth_amd import viz
    np.random.seed(0)                                  # c512 runs sklearn's randomized solver, which draws from numpy's global generator (as the generator seeded it)
    with np.errstate(invalid='ignore', divide='ignore'): got = viz.rgb_from_feat(fixture[f'feat_in_{k}'])
    nc = FEAT_CASES[k][2]                              # (c512_n3: the third channel is noise over noise, not recorded as comparable)
    assert got.dtype == torch.float32 and torch.equal(got[:, :nc], fixture[f'feat_out_{k}'][:, :nc]), fixture[f'feat_solver_{k}']
    assert str(fixture[f'feat_solver_{k}']) == ('covariance_eigh', 'full', 'full', 'randomized', 'full')[k]


@pytest.mark.skipif(not HAVE_MPL, reason='needs matplotlib to compare with')
def test_the_committed_tables_are_matplotlibs():
    from matplotlib import pyplot as plt
    from slowtv_monodepth_amd import viz
    for name in viz.CMAPS:
        cm = plt.get_cmap(name)
        assert np.array_equal(viz.cmap_table(name), np.asarray(cm(np.arange(cm.N)))[:, :3]), name
    with pytest.raises(KeyError, match='turbo, magma, viridis'): viz.cmap_table('jet')


@pytest.mark.parametrize('n', [1, 2, 20, 21, 1000])
def test_the_percentile_helper_is_np_percentiles(n):
    """0.95 (n - 1) integral (n = 1, 21) and fractional, t below 0.5 (n = 20: 18.05) and above (n = 2: 0.95; n = 1000: 949.05 is below, so n = 2 is the case)."""
    from slowtv_monodepth_amd.viz import percentile95
    for seed in range(4):
        x = (0.01 + 40*torch.rand(n, generator=torch.Generator().manual_seed(10*n + seed))).numpy()
        assert percentile95(x).tobytes() == np.percentile(x, 95).tobytes()


@pytest.mark.parametrize('case', GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_the_grid_geometry_is_slicings(case):
    from slowtv_monodepth_amd import viz
    _, x, normalize = case
    got = viz.make_grid(x, 6, 2, normalize=normalize)
    want = grid_by_slicing(x, 6, 2, normalize=normalize)
    assert got.shape == want.shape and torch.equal(got, want)
    n = min(6, x.shape[0])
    if n > 1: assert got.shape == (3, (x.shape[2] + 2)*((n + 1)//2) + 2, (x.shape[3] + 2)*2 + 2)


def test_the_new_symbols_are_declared_in_all_four_places():
    from slowtv_monodepth_amd import _lib, functional
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    csrc = ROOT/'slowtv_monodepth_amd'/'csrc'
    api, kernels = (csrc/'smd_api.hip').read_text(), (csrc/'smd_kernels.h').read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in the header'
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', api), f'{name} is not defined in smd_api.hip'
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name)
    for name in ('launch_viz_disp', 'launch_viz_feat_moments', 'launch_viz_feat_project', 'launch_make_grid'): assert name in kernels
    assert 'viz.py:20-74' in header and 'heavy_logger.py:35-42' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_viz.hip' in (csrc/'Makefile').read_text() and 'getenv' not in (csrc/'smd_viz.hip').read_text()
    assert not any(n in functional.__all__ for n in ('rgb_from_disp', 'rgb_from_feat', 'make_grid'))


def test_the_abi_refuses_bad_arguments_without_a_gpu():
    from slowtv_monodepth_amd import _lib
    p = 4096                                           # never dereferenced: every call below is refused first
    def disp(d=p, b=1, h=4, w=4, N=256, ws=1 << 20): return _lib.call('smd_viz_disp', d, b, h, w, 0, 1, 0.0, 1e-5, p, N, p, p, p, p, ws, None)
    for kw in (dict(d=None), dict(b=0), dict(h=0), dict(w=0), dict(N=0), dict(N=2000)):
        with pytest.raises(ValueError): disp(**kw)
    with pytest.raises(_lib.HotpathError): disp(ws=16)
    def moments(f=p, b=1, C=8, h=4, w=4): return _lib.call('smd_viz_feat_moments', f, b, C, h, w, p, p, p, 1 << 30, None)
    def project(V=p, b=1, C=8, h=4, w=4): return _lib.call('smd_viz_feat_project', p, p, V, b, C, h, w, p, p, 1 << 30, None)
    for fn in (moments, project):
        for kw in (dict(C=2), dict(C=1025), dict(h=0), dict(w=0), dict(h=1, w=2)):
            with pytest.raises(ValueError): fn(**kw)
    with pytest.raises(ValueError): moments(f=None)
    with pytest.raises(ValueError): project(V=None)
    assert _lib.lib.smd_viz_feat_workspace_bytes(1, 2, 4, 4) == 0 and _lib.lib.smd_viz_feat_workspace_bytes(1, 8, 1, 2) == 0 and _lib.lib.smd_viz_disp_workspace_bytes(1, 0, 4) == 0
    def grid(x=p, c=3, h=4, w=4, n=6, nrow=2): return _lib.call('smd_make_grid', x, 0, 2, c, h, w, n, nrow, 2, 0.0, 0, p, p, 1 << 20, None)
    for kw in (dict(x=None), dict(c=2), dict(h=0), dict(w=0), dict(n=0), dict(nrow=0)):
        with pytest.raises(ValueError): grid(**kw)


# ---------------------------------------------------------------------------------------------------------------- HeavyLogger and train.py

def _keys(supp=(-1, 1), extra=()):
    """The reference's keys (heavy_logger.py:90-210) in train mode for a ResNet-18 depth network with four disparity scales (five encoder levels), the
    reconstruction loss with warps and the edge-aware smoothness term (its two gradient images), plus what a configuration adds."""
    per_supp = [f'{p}/supp_{i}' for i in supp for p in ('imgs_aug', 'imgs', 'imgs_warp')]
    return sorted(['imgs_aug/target', 'imgs/target', *per_supp, *[f'feats/target_{s}' for s in range(5)], *[f'disp/target_{s}' for s in range(4)],
                   'grad/image', 'grad/disp', *extra])


# per configuration: resnet18 adds the automask; `mask_name` the first support's mask per scale (no automask: cfg/kitti_sfm_learner.yaml has use_automask
# False); the autoencoder its reconstructions per scale, its five feature levels and the warped features; depth hints the hints, their mask and the stereo
# partner as a third support
EXPECTED_KEYS = {'resnet18': _keys(extra=['masks/automask']),
                 'sfm_learner': _keys(extra=[f'masks/mask_0_{s}' for s in range(4)]),
                 'featdepth': _keys(extra=['masks/automask', *[f'imgs/autoenc_{s}' for s in range(4)], *[f'feats/autoenc_{s}' for s in range(5)],
                                           'feats_warp/supp_-1', 'feats_warp/supp_1']),
                 'depth_hints': _keys(supp=(-1, 1, 0), extra=['masks/automask', 'masks/hints', 'depth/hints'])}


def tiny_module_and_batch(name: str, device='cpu'):
    """A `MonoDepthModule` of configuration `name` with `trainer.log_images` and a synthetic batch at b = 2, 64 x 96 — the smallest size the suite runs the
    ResNet-18 networks at: at 24 x 32 the decoder would reflection-pad a 1 x 1 map (CPU: the oracle backend, with the handlers the other host tests add)."""
    from slowtv_monodepth_amd import io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.train import dataset_supp_idxs
    from slowtv_monodepth_amd.trainer import MonoDepthModule
    cfg = io.load_merge_yaml(ROOT/'cfg'/f'kitti_{name}.yaml')
    cfg.setdefault('trainer', {})['log_images'] = True
    torch.manual_seed(0)
    if device == 'cpu':
        from oracle.backend import OracleBackend
        if name == 'featdepth': from test_featdepth_host import _Backend as OracleBackend
        if name == 'depth_hints': from test_hints_host import _Backend as OracleBackend
        module = MonoDepthModule(cfg, loss_backend=OracleBackend())
    else: module = MonoDepthModule(cfg).to(device)
    return module, make_batch(2, 64, 96, dataset_supp_idxs(cfg), seed=1, device=torch.device(device), depth_hints=name == 'depth_hints')


@pytest.mark.skipif(not (HAVE_MPL and HAVE_SK), reason='the plain path needs matplotlib and sklearn')
@pytest.mark.parametrize('name', ['sfm_learner', 'featdepth', 'depth_hints'])
def test_heavy_logger_key_set_per_configuration(name):
    from slowtv_monodepth_amd.heavy_logger import HeavyLogger, RecordingWriter
    module, batch = tiny_module_and_batch(name)
    rec = RecordingWriter()
    if name == 'sfm_learner':
        # the CPU oracle backend has no masked reconstruction (test_gpu_viz.py runs this configuration's whole step): the networks run here, and the losses'
        # artefacts are the ones the masked handler and the smoothness term document, fed to `log_loss` directly
        x, y, _ = batch
        with torch.no_grad(): fwd = module.forward_postprocess(module.forward(x), x, y)
        lg = HeavyLogger(6, 2, writer=rec)
        lg.mode, lg.step = 'train', 1
        lg.log_batch(batch); lg.log_fwd(fwd)
        lg.log_loss({'supp_imgs_warp': y['supp_imgs'], 'image_grad': torch.rand(2, 1, 64, 96), 'disp_grad': torch.rand(2, 1, 64, 96)}, x['supp_idxs'])
    else: HeavyLogger(6, 2).log_step(module, batch, 'train', 1, writer=rec)
    assert sorted(k for k, _, _ in rec.images) == [f'train_{k}' for k in EXPECTED_KEYS[name]]
    assert all(v.ndim == 4 and v.shape[:2] == (1, 3) for _, v, _ in rec.images)


@pytest.mark.skipif(not (HAVE_MPL and HAVE_SK), reason='the plain path needs matplotlib and sklearn')
def test_heavy_logger_writes_the_references_keys_on_the_cpu(tmp_path):
    from slowtv_monodepth_amd.heavy_logger import HeavyLogger, NpyWriter, RecordingWriter, TensorBoardWriter
    module, batch = tiny_module_and_batch('resnet18')
    rec = RecordingWriter()
    HeavyLogger(6, 2).log_step(module, batch, 'train', 7, writer=rec)
    assert sorted(k for k, _, _ in rec.images) == [f'train_{k}' for k in EXPECTED_KEYS['resnet18']]
    assert all(s == 7 and v.ndim == 4 and v.shape[:2] == (1, 3) for _, v, s in rec.images) and rec.texts[0][0] == 'train_items'
    rec = RecordingWriter()
    HeavyLogger(6, 2).log_step(module, batch, 'val', 8, writer=rec)
    assert sorted(k for k, _, _ in rec.images) == [f'val_{k}' for k in EXPECTED_KEYS['resnet18'] if not k.startswith('imgs_aug/')]
    w = NpyWriter(tmp_path/'log')
    w.add_images('train_disp/target_0', rec.images[0][1], 3); w.add_text('train_items', 'a - b', 3)
    assert np.load(tmp_path/'log'/'train_disp-target_0_000003.npy').shape == tuple(rec.images[0][1].shape) and (tmp_path/'log'/'text.jsonl').read_text().count('\n') == 1
    if importlib.util.find_spec('tensorboard') is None:
        with pytest.raises(ImportError, match='tensorboard'): TensorBoardWriter(tmp_path/'tb')
    module.want_aux = False
    with pytest.raises(ValueError, match='log_images'): HeavyLogger().log_step(module, batch, 'train', 0, writer=rec)


_CHILD = '''
import sys, torch
sys.path[:0] = [{root!r}]
import slowtv_monodepth_amd.train as T
from oracle.backend import OracleBackend
from slowtv_monodepth_amd.trainer import MonoDepthModule
T.MonoDepthModule = lambda c: MonoDepthModule(c, loss_backend=OracleBackend())      # (the product backend needs a GPU)
torch.cuda.is_available = lambda: False
made = []
keep = T.make_image_logger
T.make_image_logger = lambda *a: made.append(keep(*a)) or made[-1]
args = ['-c', {cfg!r}, '-n', 'x', '-o', {out!r}, '--steps', '1', '--shape', '64', '96']
T.main(args)
loaded = [m for m in ('slowtv_monodepth_amd.heavy_logger', 'slowtv_monodepth_amd.viz', 'matplotlib', 'sklearn') if m in sys.modules]
print('WITHOUT', made, loaded)
if {with_flag!r}:
    T.main(args + ['--log-images', {log!r}, '--val-steps', '1', '--val-depth-shape', '20', '30'])
    print('WITH', type(made[-1]).__name__, type(made[-1].writer).__name__, 'slowtv_monodepth_amd.heavy_logger' in sys.modules)
'''


def test_train_builds_and_imports_no_logger_without_the_flag(tmp_path):
    """`train.main` in a fresh process on the CPU (b = 2, one step at 64 x 96): without `--log-images` `make_image_logger` returns None and neither
    `heavy_logger` nor `viz` (nor matplotlib / sklearn) is imported; with it (same process, afterwards) the last train and val batches are logged at the end
    of the epoch under the reference's keys, the val step in eval mode."""
    import subprocess
    import sys
    import yaml
    cfg = yaml.safe_load((ROOT/'cfg'/'kitti_resnet18.yaml').read_text())
    cfg['loader'] = {'batch_size': 2}; cfg['trainer']['max_epochs'] = 1
    (tmp_path/'cfg.yaml').write_text(yaml.safe_dump(cfg))
    with_flag = HAVE_MPL and HAVE_SK                   # (on the CPU the logger runs the plain path)
    code = _CHILD.format(root=str(ROOT), cfg=str(tmp_path/'cfg.yaml'), out=str(tmp_path/'runs'), log=str(tmp_path/'log'), with_flag=with_flag)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'WITHOUT [None] []' in r.stdout, r.stdout
    if with_flag:
        assert 'WITH HeavyLogger NpyWriter True' in r.stdout, r.stdout
        files = {p.name for p in (tmp_path/'log').glob('*.npy')}
        want = {f'train_{k.replace("/", "-")}_000000.npy' for k in EXPECTED_KEYS['resnet18']}
        want |= {f'val_{k.replace("/", "-")}_000000.npy' for k in EXPECTED_KEYS['resnet18'] if not k.startswith('imgs_aug/')} | {'val_depth-lidar_000000.npy'}
        assert files == want, files ^ want
