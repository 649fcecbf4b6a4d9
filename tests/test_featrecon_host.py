"""The fused feature-metric reconstruction loss (csrc/smd_featrecon.hip, featrecon.py, `handlers.feat_recon_fused`) on the host: the new C symbols and their
refusals, the operator's refusals before the device, the fused handler's plain paths (counted), `HipLossBackend.feat_recon` and the trainer's call of it, and the
cases, seeds and bounds the GPU test (tests/test_gpu_featrecon.py) runs on.

`handlers.feat_recon` runs on the un-fused HIP operators, which have no CPU implementation: for CPU tensors the plain and the fused handler refuse identically, and
with the oracle's `image_recon` behind `handlers._image_recon_generic` both return the same bits, which are held to the REFERENCE's fixture
(tests/golden/hd_feat_recon.npz) at tests/test_oracle_golden.py::test_feat_recon_handler's bounds.

Decisions.  `sel` is a chain of comparisons; the GPU test compares it with the fp64 oracle's everywhere except where the oracle's own margin between its two best
candidates is below MARGIN = 1e-5 relative (`oracle_case`), and at most MAX_LEFT_OUT = 0.5 % of a case's pixels may be left out.  The seeds below are chosen so
that the oracle alone leaves out none on the fixture and stays under the cap on every case: `test_oracle_margins_of_the_cases` checks that here, on the CPU.
One kind of pixel is no near-tie of that sort and is counted apart (`tied`): in the frame's clamped corners and edges the up-sampled map is constant, the warp
samples that same constant, and the warped and the static candidate are EQUAL before the noise is added (to TIED = 1e-12 relative in fp64: 20 of the fixture's
1920 pixels, about ten per image at any size and seed).  There the noise alone decides, by an amount of eps * |noise|: against errors of order 1 that is a margin
of about 1e-7 relative, one fp32 ulp, a hundred times below MARGIN, so no fp32 implementation (the plain path included) can be held to the fp64 decision there
and the 0.5 % rule cannot be met literally on the fixed fixture (20 / 1920 = 1.04 %).  Such a pixel has to select one of its two tied candidates, and on every
case the very selection of the plain path, which evaluates the same statements; their number is capped per case at the count the oracle gives (TIES), and
they are never counted as `near`.  Loss and gradients are then held to the fp64 values under the selection that was taken (`run_oracle(force_sel=...)`)."""
import copy
import functools
import inspect

import pytest
import torch

from conftest import ROOT, load_golden, rel_to_max
from oracle import view_synth_oracle as O
from oracle.backend import OracleBackend

NEW_SYMBOLS = ['smd_feat_recon_workspace_bytes', 'smd_feat_recon_fwd', 'smd_feat_recon_bwd']
MARGIN, MAX_LEFT_OUT, TIED = 1e-5, 5e-3, 1e-12

# name: (b, C, hf, wf, H, W, n, loss_name, use_min, use_automask, pose, seed).  pose: 'small' | 'identity' | 'far' (a third of the pixels project outside the frame)
CASES = {
    'c1': (2, 1, 6, 10, 24, 40, 2, 'l2', True, True, 'small', 11),
    'c65': (1, 65, 5, 8, 20, 32, 2, 'l2', True, True, 'small', 12),
    'w67': (1, 5, 6, 17, 22, 67, 2, 'l2', True, True, 'small', 13),             # a ragged last block of columns
    'w130': (1, 4, 3, 33, 9, 130, 2, 'l2', True, True, 'small', 14),            # a row crossing two waves' worth of columns, three blocks
    'ratio_5x7_18x26': (2, 6, 5, 7, 18, 26, 2, 'l2', True, True, 'small', 15),  # a non-integer ratio
    'ratio_1': (2, 6, 8, 12, 8, 12, 2, 'l2', True, True, 'small', 16),
    'n1': (2, 6, 6, 10, 24, 40, 1, 'l2', True, True, 'small', 17),
    'n3': (2, 6, 6, 10, 24, 40, 3, 'l2', True, True, 'small', 18),
    'l1': (2, 6, 6, 10, 24, 40, 2, 'l1', True, True, 'small', 19),
    'mean_noauto': (2, 6, 6, 10, 24, 40, 2, 'l2', False, False, 'small', 20),
    'min_noauto': (2, 6, 6, 10, 24, 40, 2, 'l2', True, False, 'small', 21),
    'border': (2, 6, 6, 10, 24, 40, 2, 'l2', True, True, 'far', 22),
    'identity': (2, 6, 6, 10, 24, 40, 2, 'l2', True, True, 'identity', 23),
}


# the structural ties of each case: the fp64 oracle's own count (it is a property of the inputs: pixels whose warped and static candidates are equal before the noise)
TIES = {'fixture': 20, 'c1': 20, 'c65': 8, 'w67': 13, 'w130': 14, 'ratio_5x7_18x26': 26, 'ratio_1': 7, 'n1': 24, 'n3': 22, 'l1': 21, 'mean_noauto': 0, 'min_noauto': 0,
        'border': 13, 'identity': 32}


def case_inputs(name):
    """The seeded operands of a case (CPU, float32): depth, feats, supp_feats, aa, t, K, noise."""
    from slowtv_monodepth_amd.synthetic import kitti_K
    b, C, hf, wf, H, W, n, *_, pose, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    depth = 1 + 9*torch.rand(b, 1, H, W, generator=g)
    feats, supp = torch.randn(b, C, hf, wf, generator=g), torch.randn(n, b, C, hf, wf, generator=g)
    supp = 0.5*supp + 0.5*feats[None]                                   # correlated with the target, as a neighbouring frame's features are
    aa, t = 0.01*torch.randn(n, b, 3, generator=g), 0.1*torch.randn(n, b, 3, generator=g)
    if pose == 'identity': aa, t = torch.zeros(n, b, 3), torch.zeros(n, b, 3)
    if pose == 'far': t[..., 0] += 1.5                                  # a sideways step of 1.5 units at depths 1 .. 10
    noise = torch.randn(b, 1, H, W, generator=g)
    return dict(depth=depth, feats=feats, supp_feats=supp, aa=aa, t=t, K=kitti_K(b, H, W), noise=noise)


def fixture_inputs():
    g = load_golden('hd_feat_recon')
    return dict(depth=g['in_depth'], feats=g['in_feats'], supp_feats=g['in_supp_feats'], aa=g['in_aa'], t=g['in_t'], K=g['in_K'], noise=g['in_noise'])


def run_oracle(ins, loss_name, use_min, use_automask, dtype=torch.float64, force_sel=None):
    """`O.feat_recon` on the case in `dtype` (`force_sel` (b,1,H,W) uint8: `O.feat_recon`'s statements with `O.image_recon`'s test aid, the decisions taken from this
    map instead of the arg-min, so that loss and gradients are the fp64 values UNDER A GIVEN SELECTION) -> dict: loss, warp, sel, g_depth, g_aa, g_t, and `near` (b,1,H,W) bool: pixels whose decision the oracle itself
    takes by less than MARGIN relative (between the two best warped errors where a warped support wins a minimum over several, between the warped and the
    static candidate under the automask), and `tied`: pixels whose warped and static candidates are equal before the noise (the module's docstring)."""
    c = {k: v.to(dtype) for k, v in ins.items()}
    depth, aa, t = (c[k].clone().requires_grad_(True) for k in ('depth', 'aa', 't'))
    n, b = aa.shape[:2]
    Ts = O.T_from_AAt(aa.flatten(0, 1), t.flatten(0, 1)).unflatten(0, (n, b))
    if force_sel is None:
        loss, ld, full = O.feat_recon({0: depth}, c['feats'], c['supp_feats'], Ts, c['K'], loss_name, use_min, use_automask, noise=c['noise'], aten=False)
    else:
        size = tuple(depth.shape[-2:])
        up_t = O.resize_bilinear(c['feats'], size)
        up_s = O.resize_bilinear(c['supp_feats'].flatten(0, 1), size).unflatten(0, (n, b))
        loss, ld, full = O.image_recon({0: depth}, up_t, up_s, Ts, c['K'], loss_name, use_min, use_automask, c['noise'], False, force_sel)
        ld = {'supp_feats_warp': ld['supp_imgs_warp']}
        assert torch.equal(full['sel'][0], force_sel), 'the oracle took the given selection'
    loss.backward()
    with torch.no_grad():
        size = tuple(depth.shape[-2:])
        tgt = O.resize_bilinear(c['feats'], size)
        warp = full['warp'].detach()                                                                            # (n,b,C,H,W)
        per = torch.stack([O.photo_error(warp[i], tgt, loss_name) for i in range(n)], 1).squeeze(2)            # (b,n,H,W)
        near = torch.zeros(b, 1, *size, dtype=torch.bool)
        tied = torch.zeros(b, 1, *size, dtype=torch.bool)
        sel = full['sel'][0]
        if use_min and n > 1:
            two = per.topk(2, dim=1, largest=False)[0]
            near |= (((two[:, 1] - two[:, 0]) < MARGIN*two[:, 1].abs())[:, None]) & (sel != 255)
        if use_automask:
            supp_up = O.resize_bilinear(c['supp_feats'].flatten(0, 1), size).unflatten(0, (n, b))
            st = torch.stack([O.photo_error(supp_up[i], tgt, loss_name) for i in range(n)], 1).squeeze(2)
            ew = per.min(1, keepdim=True)[0] if use_min else per.mean(1, keepdim=True)
            es = st.min(1, keepdim=True)[0] if use_min else st.mean(1, keepdim=True)
            scale = torch.maximum(ew.abs(), es.abs())
            tied = (ew - es).abs() <= TIED*scale
            near |= ((ew - es - O.EPS32*c['noise']).abs() < MARGIN*scale) & ~tied
    return dict(loss=loss.detach(), warp=ld['supp_feats_warp'].detach(), sel=sel, near=near, tied=tied, g_depth=depth.grad, g_aa=aa.grad, g_t=t.grad)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The fp64 oracle of a case or of the fixture ('fixture'): computed once, shared by the tests, never modified."""
    if name == 'fixture': return run_oracle(fixture_inputs(), 'l2', True, True)
    return run_oracle(case_inputs(name), *CASES[name][7:10])


@pytest.mark.parametrize('name', ['fixture', *CASES])
def test_oracle_margins_of_the_cases(name):
    """The seeds: no pixel of the fixture and at most 0.5 % of a case's pixels are decided by less than 1e-5 relative in fp64; the border case projects about a
    third of its pixels outside the frame, the identity pose moves nothing."""
    o = oracle_case(name)
    left_out = o['near'].float().mean().item()
    assert left_out <= (0 if name == 'fixture' else MAX_LEFT_OUT), (name, left_out)
    assert int(o['tied'].sum()) <= TIES[name] and not (o['tied'] & o['near']).any(), 'the structural ties: the count the oracle gives on this case, counted apart'
    assert torch.isfinite(o['loss']) and torch.isfinite(o['g_depth']).all()
    if name == 'fixture':
        g = load_golden('hd_feat_recon')
        torch.testing.assert_close(o['loss'].float(), g['out_loss'], rtol=1e-5, atol=1e-7)
    if name == 'border':
        ins = case_inputs(name)
        from slowtv_monodepth_amd.geometry import T_from_AAt
        n, b = ins['aa'].shape[:2]
        Ts = T_from_AAt(ins['aa'].flatten(0, 1), ins['t'].flatten(0, 1)).unflatten(0, (n, b))
        outside = 1 - _inside_share(ins, Ts)
        assert 0.2 <= outside <= 0.5, outside


def _inside_share(ins, Ts):
    """The share of (support, pixel) pairs whose projection lies inside the frame (pinhole projection restated in fp64)."""
    d = ins['depth'].double()
    b, _, H, W = d.shape
    K = ins['K'].double()[:, :3, :3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    pix = torch.stack((xs, ys, torch.ones_like(xs))).reshape(3, -1)
    pts = torch.linalg.inv(K) @ pix*d.reshape(b, 1, -1)
    T = Ts.double()
    cam = T[:, :, :3, :3] @ pts[None] + T[:, :, :3, 3:]
    proj = K[None] @ (cam/cam[:, :, 2:3].clamp(min=0.1))
    inside = (proj[:, :, 0] >= 0) & (proj[:, :, 0] <= W - 1) & (proj[:, :, 1] >= 0) & (proj[:, :, 1] <= H - 1)
    return inside.double().mean().item()


# ------------------------------------------------------------------------------------------------- the C ABI
def test_new_c_symbols_header_and_makefile():
    from slowtv_monodepth_amd import _lib
    header = (ROOT/'include'/'smd_hotpath.h').read_text()
    for name in NEW_SYMBOLS: assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name) and name in header, name
    assert 'handlers.py:70-119' in header and _lib.lib.smd_abi_version() == 8
    assert 'smd_featrecon.hip' in (ROOT/'slowtv_monodepth_amd'/'csrc'/'Makefile').read_text()
    src = (ROOT/'slowtv_monodepth_amd'/'csrc'/'smd_featrecon.hip').read_text()
    assert 'atomic' not in src.split('namespace smd {', 1)[1].lower() and 'gauss_noise(' in src and 'launch_pose_finalize(' in src
    assert 'gauss_noise' in (ROOT/'slowtv_monodepth_amd'/'csrc'/'smd_common.h').read_text(), 'the noise generator is the shared header\'s'


# the largest frame side the kernels serve (smd_featrecon.hip: kFrMaxSize), in four bands of about equal work
@pytest.mark.parametrize('lo,hi', [(2, 1290), (1291, 1625), (1626, 1860), (1861, 2048)])
def test_adjacent_columns_lie_at_most_one_low_resolution_column_apart(lo, hi):
    """The warp's nine-tap form (smd_featrecon.hip: `make_axis`) rests on i0(d + 1) - i0(d) being 0 or 1, i0(d) = min(int(max(fmaf(r, d + 0.5, -0.5), 0)), n_in - 1),
    r = fp32(n_in / n_out): checked here for EVERY n_out <= 2048, every n_in <= n_out and every d, d = n_out - 1 included (the warp's second tap may be the
    column past the clamp).  The fp32 fused multiply-add is restated exactly: r has 24 bits and d + 0.5 at most 12, so r (d + 0.5) - 0.5 is exact in fp64 and
    is rounded once.  (Why it holds: the exact values of two adjacent columns differ by r <= 1 - 1/2048 or by exactly 1, and half an ulp below 2048 is 2^-14.)"""
    from slowtv_monodepth_amd import _lib
    for n_out in range(lo, hi + 1):
        d = torch.arange(n_out + 1, dtype=torch.float64) + 0.5
        n_in = torch.arange(1, n_out + 1, dtype=torch.float32)
        r = (n_in/torch.tensor(float(n_out), dtype=torch.float32)).double()[:, None]
        s = (r*d - 0.5).float().clamp_(min=0)
        i0 = torch.minimum(s.int(), (n_in.int() - 1)[:, None])
        step = i0[:, 1:] - i0[:, :-1]
        assert int(step.min()) >= 0 and int(step.max()) <= 1, n_out
    ws = _lib.lib.smd_feat_recon_workspace_bytes
    assert ws(1, 1, 1, 2048, 2048, 2048, 2048) > 0 and ws(1, 1, 1, 2049, 16, 4, 4) == 0 and ws(1, 1, 1, 16, 2049, 4, 4) == 0, 'the limit the check covers is the entry points\''


FWD = ('depth', 'feat', 'supp', 'T', 'K', 'K_inv', 'noise', 'seed', 'loss', 'sel', 'warp', 'ws', 'nbytes', 'b', 'n', 'C', 'H', 'W', 'hf', 'wf', 'flags', 'stream')
BWD = ('depth', 'feat', 'supp', 'T', 'K', 'K_inv', 'sel', 'g_loss', 'g_depth', 'g_T', 'ws', 'nbytes', 'b', 'n', 'C', 'H', 'W', 'hf', 'wf', 'flags', 'stream')
L2_MIN_AUTO = 0x20 | 0x1 | 0x2


def _call(name, order, **kw):
    from slowtv_monodepth_amd import _lib
    base = dict(depth=16, feat=16, supp=16, T=16, K=16, K_inv=16, noise=None, seed=0, loss=16, sel=16, warp=None, ws=16, nbytes=1 << 22, b=2, n=2, C=6, H=24, W=40, hf=6,
                wf=10, flags=L2_MIN_AUTO, stream=None, g_loss=16, g_depth=16, g_T=16)
    base.update(kw)
    return _lib.call(name, *[base[k] for k in order])


def test_abi_refuses_bad_arguments_without_a_gpu():
    """Every check runs before any launch: null pointers one by one, zero sizes, features larger than the depth map, the element limits, flags, an undersized
    or misaligned workspace, a backward nobody asked anything of."""
    from slowtv_monodepth_amd import _lib
    ws = _lib.lib.smd_feat_recon_workspace_bytes
    blocks = 2*6*1
    assert ws(2, 2, 6, 24, 40, 6, 10) >= blocks*8 + 2*blocks*12*4 and ws(6, 3, 64, 192, 640, 48, 160) > 0 and ws(1, 1, 1, 2, 2, 1, 1) > 0
    for bad in ((0, 2, 6, 24, 40, 6, 10), (2, 0, 6, 24, 40, 6, 10), (2, 2, 0, 24, 40, 6, 10), (2, 2, 6, 1, 40, 1, 10), (2, 2, 6, 24, 40, 0, 10), (2, 9, 6, 24, 40, 6, 10),
                (2, 2, 6, 24, 40, 25, 10), (2, 2, 6, 24, 40, 6, 41), (1, 1, 1, 4096, 16, 4, 4), (1 << 10, 1, 1, 2048, 2048, 1, 1), (8, 8, 4096, 2048, 2048, 2048, 2048)):
        assert ws(*bad) == 0, bad
    for name, order, ptrs in (('smd_feat_recon_fwd', FWD, ('depth', 'feat', 'supp', 'T', 'K', 'K_inv', 'loss', 'sel', 'ws')),
                              ('smd_feat_recon_bwd', BWD, ('depth', 'feat', 'supp', 'T', 'K', 'K_inv', 'sel', 'g_loss', 'ws'))):
        for p in ptrs:
            with pytest.raises(ValueError, match='null pointer'): _call(name, order, **{p: None})
        for bad in (dict(b=0), dict(n=0), dict(C=0), dict(H=0), dict(W=1), dict(hf=0), dict(wf=0), dict(n=9), dict(H=4096), dict(flags=0x1), dict(flags=0x24), dict(flags=0x60),
                    dict(ws=20)):
            with pytest.raises(ValueError): _call(name, order, **bad)
        with pytest.raises(ValueError, match='larger than the depth map'): _call(name, order, hf=25)
        with pytest.raises(ValueError, match='larger than the depth map'): _call(name, order, wf=41)
        with pytest.raises(ValueError, match='2\\^31'): _call(name, order, b=1 << 10, H=2048, W=2048)
        with pytest.raises(_lib.HotpathError, match='workspace too small'): _call(name, order, nbytes=ws(2, 2, 6, 24, 40, 6, 10) - 1)
    with pytest.raises(ValueError, match='nothing to compute'): _call('smd_feat_recon_bwd', BWD, g_depth=None, g_T=None)


# ------------------------------------------------------------------------------------------------- the operator
def test_operator_refuses_wrong_shapes_and_types_before_the_device():
    from slowtv_monodepth_amd import functional as F
    from slowtv_monodepth_amd.featrecon import _FeatRecon, feat_recon_loss
    ins = fixture_inputs()
    n, b = ins['aa'].shape[:2]
    good = dict(depth=ins['depth'], feats=ins['feats'], supp_feats=ins['supp_feats'], Ts=torch.eye(4).expand(n, b, 4, 4).contiguous(), K=ins['K'])
    kw = dict(loss_name='l2', use_min=True, use_automask=True)
    run = lambda **over: feat_recon_loss(**{**good, **{k: v for k, v in over.items() if k in good}}, **{k: v for k, v in over.items() if k not in good}, **kw)
    with pytest.raises(KeyError): feat_recon_loss(**good, loss_name='ssim', use_min=True, use_automask=True)
    with pytest.raises(TypeError, match='must be a Tensor'): run(feats=[good['feats']])
    with pytest.raises(ValueError, match=r'expected \(b,1,H,W\)'): run(depth=good['depth'][:, 0])
    with pytest.raises(ValueError, match=r'expected \(b,1,H,W\)'): run(depth=good['depth'].expand(b, 2, 24, 40))
    with pytest.raises(ValueError, match='feats: expected'): run(feats=good['feats'][:1])
    with pytest.raises(ValueError, match='supp_feats: expected'): run(supp_feats=good['supp_feats'][:, :, :5])
    with pytest.raises(ValueError, match='supp_feats: expected'): run(supp_feats=good['supp_feats'][0])
    with pytest.raises(ValueError, match='supports'): run(supp_feats=good['supp_feats'][:1].expand(9, b, 6, 6, 10), Ts=torch.eye(4).expand(9, b, 4, 4))
    with pytest.raises(ValueError, match='larger than the depth map'): run(depth=good['depth'][..., :5, :])
    with pytest.raises(ValueError, match='Ts: expected'): run(Ts=good['Ts'][:1])
    with pytest.raises(ValueError, match='K: expected'): run(K=good['K'][:, :3, :3])
    with pytest.raises(ValueError, match='K_inv: expected'): run(K_inv=good['K'][:1])
    with pytest.raises(ValueError, match='noise: expected'): run(noise=ins['noise'][:, 0])
    with pytest.raises(TypeError, match='float32'): run(depth=good['depth'].double())
    with pytest.raises(TypeError, match='float32'): run(supp_feats=good['supp_feats'].half())
    for k in ('feats', 'supp_feats', 'K'):
        with pytest.raises(ValueError, match='must not require a gradient'): run(**{k: good[k].clone().requires_grad_(True)})
    # everything in order: the device is looked at last
    with pytest.raises(RuntimeError, match='must live on the GPU'): run(K_inv=torch.linalg.inv(good['K']))
    with pytest.raises(RuntimeError, match='must live on the GPU'): _FeatRecon.apply(good['depth'], good['feats'], good['supp_feats'], good['Ts'], good['K'], good['K'], None, 0, L2_MIN_AUTO, False)
    assert not any('feat_recon' in name for name in F.__all__), 'the operator\'s names stay out of functional.__all__'


# ------------------------------------------------------------------------------------------------- the handler
def _oracle_generic(crit, depths, imgs, supp_imgs, Ts, Ks, K_inv, noise, want_warp, masks=None):
    """`handlers._image_recon_generic` on the CPU oracle (ATen up-sampling and grid_sample, as the reference runs them)."""
    loss, ld, _ = O.image_recon(depths, imgs, supp_imgs, Ts, Ks, crit.loss_name, crit.use_min, crit.use_automask, noise=noise, aten=True)
    return loss, ld


def test_fused_handler_on_the_cpu_is_the_plain_handler(monkeypatch):
    from slowtv_monodepth_amd import handlers
    from slowtv_monodepth_amd.geometry import T_from_AAt
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    assert list(inspect.signature(handlers.feat_recon_fused).parameters)[:9] == list(inspect.signature(handlers.feat_recon).parameters)
    assert 'feat_recon_fused' in handlers.__all__ and list(inspect.signature(handlers.feat_recon_fused).parameters)[9:] == ['want_warp']
    g, ins = load_golden('hd_feat_recon'), fixture_inputs()
    n, b = ins['aa'].shape[:2]

    def run(fn, **kw):
        depth, aa, t = (ins[k].clone().requires_grad_(True) for k in ('depth', 'aa', 't'))
        Ts = T_from_AAt(aa.flatten(0, 1), t.flatten(0, 1)).unflatten(0, (n, b))
        crit = ReconstructionLoss(loss_name='l2', use_min=True, use_automask=True)
        l, ld = fn(crit, None, {0: depth}, None, ins['feats'], ins['supp_feats'], Ts, ins['K'], noise=ins['noise'], **kw)
        l.backward()
        return l.detach(), ld, depth.grad, aa.grad, t.grad
    msgs = []
    for fn in (handlers.feat_recon, handlers.feat_recon_fused):      # the un-fused operators are GPU-only: both refuse, identically
        with pytest.raises(RuntimeError, match='must live on the GPU') as e: run(fn)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    monkeypatch.setattr(handlers, '_image_recon_generic', _oracle_generic)
    plain, fused = run(handlers.feat_recon), run(handlers.feat_recon_fused, want_warp=False)
    assert torch.equal(plain[0], fused[0]) and all(torch.equal(a, c) for a, c in zip(plain[2:], fused[2:])), 'CPU tensors: the plain handler\'s bits'
    assert torch.equal(plain[1]['supp_feats_warp'], fused[1]['supp_feats_warp']), 'the plain path returns what the plain handler returns'
    torch.testing.assert_close(fused[0], g['out_loss'], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(fused[1]['supp_feats_warp'], g['out_supp_feats_warp'], rtol=1e-4, atol=1e-5)
    for k, v in zip(('depth', 'aa', 't'), fused[2:]): assert rel_to_max(v, g[f'grad_{k}']) < 1e-3, k
    # the encoder's feature lists: entry [-4]
    lists = run(lambda c, s, d, m, f, sf, *a, **k: handlers.feat_recon_fused(c, s, d, m, [f*0, f, f*0, f*0, f*0], [sf*0, sf, sf*0, sf*0, sf*0], *a, **k))
    assert torch.equal(lists[0], plain[0])


def test_every_fallback_condition_takes_the_plain_path(monkeypatch):
    """Counted: CPU tensors, a predictive mask, a criterion with `mask_name`, 'ssim', intrinsics that require a gradient, features larger than the depth map, a
    subclass of the criterion, another dtype of the depth, sizes the kernel does not serve.  `served` is asked on tensors that claim to be on the GPU."""
    from slowtv_monodepth_amd import featrecon, handlers
    from slowtv_monodepth_amd.losses import ReconstructionLoss
    calls = []
    monkeypatch.setattr(handlers, 'feat_recon', lambda *a, **k: calls.append((a, k)) or ('plain', {}))
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))      # every tensor claims the GPU: only the rules decide
    monkeypatch.setattr(featrecon, 'feat_recon_loss', lambda *a, **k: pytest.fail('a declined call reached the kernel\'s operator'))
    ins = fixture_inputs()
    n, b = ins['aa'].shape[:2]
    Ts = torch.eye(4).expand(n, b, 4, 4).contiguous()
    crit = ReconstructionLoss(loss_name='l2', use_min=True, use_automask=True)
    ok = dict(crit=crit, depths={0: ins['depth']}, masks=None, feats=ins['feats'], supp_feats=ins['supp_feats'], Ts=Ts, Ks=ins['K'])
    assert featrecon.served(**ok), 'the fixture on a GPU is served'
    assert featrecon.served(**{**ok, 'feats': ins['feats'].half(), 'supp_feats': ins['supp_feats'].half()}), 'bf16 / fp16 features are converted at the low resolution'
    assert featrecon.served(**{**ok, 'Ts': Ts.clone().requires_grad_(True)}) and featrecon.served(**{**ok, 'crit': ReconstructionLoss('l1')})

    class Sub(ReconstructionLoss): pass
    declined = {
        'predictive mask': {'masks': {0: torch.rand(b, n, 24, 40)}},
        'mask_name': {'crit': ReconstructionLoss('l2', mask_name='explainability')},
        'ssim': {'crit': ReconstructionLoss('ssim', use_min=True)},
        'learned K': {'Ks': ins['K'].clone().requires_grad_(True)},
        'features larger than the depth map': {'depths': {0: ins['depth'][..., :5, :8]}},
        'subclass': {'crit': Sub('l2')},
        'depth dtype': {'depths': {0: ins['depth'].double()}},
        'sizes': {'depths': {0: ins['depth'].expand(b, 1, 24, 40)[..., :1, :]}},
    }
    for why, over in declined.items():
        args = {**ok, **over}
        assert not featrecon.served(**args), why
        before = len(calls)
        out = handlers.feat_recon_fused(args['crit'], None, args['depths'], args['masks'], args['feats'], args['supp_feats'], args['Ts'], args['Ks'], noise=None, want_warp=False)
        assert out == ('plain', {}) and len(calls) == before + 1, why
        assert calls[-1][1] == {'noise': None}, 'the plain handler takes no `want_warp`'
    monkeypatch.undo()
    monkeypatch.setattr(handlers, 'feat_recon', lambda *a, **k: calls.append((a, k)) or ('plain', {}))
    assert not featrecon.served(**ok), 'CPU tensors'
    before = len(calls)
    assert handlers.feat_recon_fused(crit, None, ok['depths'], None, ok['feats'], ok['supp_feats'], Ts, ok['Ks']) == ('plain', {}) and len(calls) == before + 1
    assert crit.noise_seed == 0, 'a declined call draws no seed: the plain handler draws its own'


# ------------------------------------------------------------------------------------------------- the trainer
class _Backend(OracleBackend):
    def autoenc_recon(self, crit, preds, targets, supp_preds, supp_targets):
        return O.autoenc_recon(preds, targets, supp_preds, supp_targets, crit.loss_name, crit.use_min, aten=self.aten), {}


def test_backend_has_feat_recon_and_the_module_calls_it(monkeypatch):
    """`HipLossBackend.feat_recon` exists with the handler's eight arguments and sends them to `handlers.feat_recon_fused` with `want_warp` = the module's
    `log_images`; the cfg/kitti_featdepth.yaml module built on the CPU calls the backend's method, not the plain handler."""
    from slowtv_monodepth_amd import handlers, io
    from slowtv_monodepth_amd.synthetic import make_batch
    from slowtv_monodepth_amd.trainer import HipLossBackend, MonoDepthModule
    assert list(inspect.signature(HipLossBackend.feat_recon).parameters)[1:] == list(inspect.signature(handlers.feat_recon).parameters)[:8]
    assert not hasattr(OracleBackend, 'feat_recon'), 'other backends keep their signature'
    seen = []

    def fused(crit, synth, depths, masks, feats, supp_feats, Ts, Ks, *, noise=None, want_warp=True):
        seen.append((want_warp, isinstance(feats, list), tuple(feats[-4].shape), Ts.requires_grad))
        loss, ld, _ = O.feat_recon(depths, feats[-4], supp_feats[-4], Ts.float(), Ks.float(), crit.loss_name, crit.use_min, crit.use_automask, aten=True)
        return loss, (ld if want_warp else {})
    monkeypatch.setattr(handlers, 'feat_recon_fused', fused)

    class Backend(_Backend):
        feat_recon = HipLossBackend.feat_recon
    cfg = io.load_merge_yaml(ROOT/'cfg'/'kitti_featdepth.yaml')
    batch = make_batch(1, 64, 96, [-1, 1], seed=5, device=torch.device('cpu'))
    for log_images in (False, True):
        c = copy.deepcopy(cfg); c.setdefault('trainer', {})['log_images'] = log_images
        torch.manual_seed(3)
        m = MonoDepthModule(c, loss_backend=Backend())
        assert m.backend.log_images is log_images
        loss, ld, _ = m.step(tuple(dict(d) for d in batch))
        assert torch.isfinite(loss) and torch.isfinite(ld['loss_feat_recon']) and ('supp_feats_warp' in ld) == log_images
        assert seen[-1] == (log_images, True, (1, 64, 16, 24), True)
    assert len(seen) == 2
    assert HipLossBackend().feat_recon.__func__ is HipLossBackend.feat_recon and getattr(HipLossBackend(), 'log_images', True) is True
