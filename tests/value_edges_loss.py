"""Value-edge cases for the loss-path operators (`view_synth`, `photo_error`, `recon_reduce`, `regression_loss`, `disp_to_depth`, `disp_smooth_fused`,
`disp_smooth_blurred`, `scale_mean`, `pose_matrices`, `intrinsics` / `inv_intrinsics`, `image_recon_fused`): the table.  Device-agnostic; test_value_edges_loss_host.py
checks it on the CPU, test_gpu_value_edges_loss.py runs it.  `Case`, the judge and the helpers are value_edges.py's; the list of cases and `OPERATORS` are this file's own.

These kernels are dense with comparisons on VALUES: the transformed depth against 0, eps and 0.1, the border clamp of the sampling coordinate, the clamp of the
SSIM error to [0, 1], `sqrt(max(e2, eps))`, first-index-wins minima, the strict automask, `to_inv`'s `x > 0` against `x >= eps`, berHu's `diff <= delta` and its
ties at the maximum, a division by the mask sum, `max(mean, eps)`, a logarithm of exactly 0.  None of them is met on `rand` / `randn` data.

Reference and yardstick: `ref(ops, dtype)` is oracle/view_synth_oracle.py on the CPU; in float64 it is the reference, in float32 (the oracle's `aten=True` form where
it has one) the yardstick.  `scale_mean` has no oracle entry and is restated from test_gpu_masks.py::test_scale_mean_matches_fp64.  `recon_reduce` takes error maps
where the oracle's `recon_loss` takes images: the oracle runs with its photometric stage replaced by the identity (`_errors_as_images`), everything behind it
(`apply_mask`, the reductions, the automask, `sel`) is the oracle's own.

No tolerance is introduced: every output takes the named bound test_gpu_hostile_memory.py lists for that operator and output.  Where the fp32 yardstick cannot
meet an operator's absolute bound AT the edge the case says so and takes value_edges.py's ('yard', FLOOR) rule.

Decisions (`sel`, `valid`, and through the outputs every clamp gate) are the same comparison in fp32 and fp64 by construction: dyadic operands, identity rotation
with dyadic intrinsics (the third row of K R K^-1 is exactly (0, 0, 1), so the transformed depth is `D + tz` in one rounding-free step), integer pixel shifts,
tz = -1 against the depths of VS_DEPTHS.  The threshold 0.1 has no common fp32 / fp64 representation and is approached from both sides (0.09375, 0.125).  The
host test asserts that the yardstick's decisions equal the reference's on every element: the GPU test holds them to `EQUAL` with no allowance.

What cannot be built.  The sampling coordinate is sx = p w/(w - 1) - 0.5 (the reference normalises by w - 1 and grid_sample un-normalises by w), which is exact only
where w/(w - 1) is dyadic (w - 1 a power of two: 2, 5, 9, 17, 33); and p = (k + 0.5)(w - 1)/w is a dyadic number for the borders k = 0 and k = w - 1 only at
w = 2.  So samples land exactly ON x = 0 and x = w - 1 in the 2 x 2 cases, and exactly on interior pixel centres in the others (VS_SHAPES)."""
import contextlib

import torch
import torch.nn.functional as TF

import value_edges as V
from value_edges import F32, F64, Case, TOL_YARD, _dyadic, _pattern
from oracle import view_synth_oracle as O
from test_gpu_hostile_memory import (EQUAL, SWEEP_ERR_ATOL, SWEEP_GRAD, SWEEP_LOSS, TOL_BLURRED_GRAD, TOL_BLURRED_LOSS, TOL_K, TOL_K0_DEPTH, TOL_K0_GRAD, TOL_K0_LOSS,
                                     TOL_K_GRAD, TOL_KINV, TOL_MASKED_GRAD, TOL_MASKED_LOSS, TOL_MEAN_GRAD, TOL_MEAN_LOSS, TOL_PHOTO_ERR, TOL_PHOTO_GRAD, TOL_PHOTO_GRAD_C,
                                     TOL_POSE_GAA, TOL_POSE_GT, TOL_POSE_T, TOL_REGR, TOL_REGR_GRAD, TOL_SMOOTH_AUX, TOL_VS_DWARP, TOL_VS_GRAD, TOL_VS_WARP)

OPERATORS = ('view_synth', 'photo_error', 'recon_reduce', 'regression_loss', 'disp_to_depth', 'disp_smooth_fused', 'disp_smooth_blurred', 'scale_mean', 'pose_matrices',
             'intrinsics', 'image_recon_fused')
EPS = O.EPS32
CASES = []
LOOSE = {}      # case name -> outputs accumulated with float atomics: between two runs they are held to their bound, not to bit-equality


def case(name, op, operands, run, ref, tol, split=None, check=None, loose=()):
    CASES.append(Case(name, op, operands, run, ref, tol, split or {}, check))
    if loose: LOOSE[name] = tuple(loose)


def decisions(c): return [k for k, b in c.tol.items() if b == EQUAL]


def _leaf(t): return t.detach().clone().requires_grad_(True)
def _to(dtype): return lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
def _c(t, dtype): return t.detach().cpu().to(dtype)
def _cycle(values, shape, step=1): return torch.tensor(values, dtype=F32)[(torch.arange(torch.Size(shape).numel())*step) % len(values)].view(shape)
def _eighths(shape, gen, lo=0, hi=9): return torch.randint(lo, hi, shape, generator=gen).float()/8


def _scalar_rel(bound):
    """A ('close', rtol, 0) bound on a scalar is ('rel', rtol): |a - b| <= rtol |b| either way (value_edges.py's `close` wants an absolute part)."""
    assert bound[0] == 'close' and bound[2] == 0
    return ('rel', bound[1])


# ---- view_synth ---------------------------------------------------------------------------------------------------------------------------------------------
# (h, w): h - 1 and w - 1 are powers of two, so w/(w - 1) and h/(h - 1) are dyadic and every coordinate below is exact in fp32.  561 pixels: three blocks of 256.
VS_SHAPES = [(5, 9), (33, 17)]
# The transformed depth is D + tz = D - 1: negative, exactly 0, exactly eps, between eps and 0.1, either side of 0.1, above it (0.25 and 1: exact reciprocals).
VS_DEPTHS = [0.5, 1.0, 1 + 2.0**-23, 1.0625, 1.09375, 1.125, 1.25, 2.0]
VS_K = [[2.0, 0, 1.0, 0], [0, 2.0, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]      # dyadic: K^-1 is exact, K K^-1 = I exactly


def _vs_T(ts):
    T = torch.eye(4).repeat(len(ts), 1, 1)
    T[:, :3, 3] = torch.tensor(ts, dtype=F32)
    return T


def vs_geometry(o):
    """-> (yz, px, py, sx, sy) of a `view_synth` case in fp64: the transformed depth, the projected pixel and the sampling coordinate before the border clamp."""
    depth, T, K = o['depth'].double(), o['T'].double(), o['K'].double()
    sx, sy, _, _ = O.sample_coords(depth, T, K)
    B, _, h, w = depth.shape
    v, u = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing='ij')
    X = (torch.linalg.inv(K)[:, :3, :3] @ torch.stack([u, v, torch.ones_like(u)]).reshape(1, 3, h*w))*depth.reshape(B, 1, h*w)
    Y = T[:, :3, :3] @ X + T[:, :3, 3:4]
    yz = Y[:, 2].reshape(B, h, w)
    p = (K[:, :3, :3] @ (Y/Y[:, 2:3].clamp(min=EPS).clamp(min=0.1))).reshape(B, 3, h, w)
    return yz, p[:, 0], p[:, 1], sx, sy


def _vs_regimes(C, h, w, gen):
    """tz = -1 under the depths of VS_DEPTHS, one per pixel in turn (a step of 3 against 8 values: every column and row meets every regime)."""
    return dict(depth=_cycle(VS_DEPTHS, (2, 1, h, w), 3), T=_vs_T([[0, 0, -1.0], [0.25, -0.125, -1.0]]))


def _vs_shifts(C, h, w, gen):
    """Constant depth 1, tz = 0: p = (u + 3, v) / (u - 3, v) / (u, v + 1) / (u, v - 1).  Whole columns (rows) leave the image on each side: border clamp, `valid` = 0, zero
    coordinate gradient; p = w - 1 exactly is met (not valid: |gx| = 1); u + 3 = (w - 1)/2 lands on the centre pixel exactly (sx = (w - 1)/2: 4 and 8)."""
    return dict(depth=torch.ones(4, 1, h, w), T=_vs_T([[1.5, 0, 0], [-1.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]))


def _vs_borders(C, h, w, gen):
    """h = w = 2: sx = 2 p - 0.5.  Shifts of +-0.25: p in {0.25, 1.25} -> sx in {0, 2}, p in {-0.25, 0.75} -> sx in {-1, 1}: exactly ON x = 0 and x = w - 1 (valid, but the
    clamp's gradient is 0 there: borders count as outside) and beyond them; the same in y."""
    assert (h, w) == (2, 2)
    return dict(depth=torch.ones(4, 1, h, w), T=_vs_T([[0.125, 0, 0], [-0.125, 0, 0], [0, 0.125, 0], [0, -0.125, 0]]))


def _vs_extreme(depth):
    """One depth everywhere under a translation: 1e-6 (the translation is everything: every pixel samples one point) or 1e6 (it is nothing: the identity warp up to
    1e-6 of a pixel)."""
    return lambda C, h, w, gen: dict(depth=torch.full((2, 1, h, w), depth), T=_vs_T([[0.125, 0.0625, 0.5], [-0.25, 0.125, 0.25]]))


def _view_synth(tag, C, h, w, fill, tol=None, split=None, grads=('inp', 'depth', 'T', 'K')):
    def operands(gen):
        o = fill(C, h, w, gen)
        B = o['depth'].shape[0]
        return dict(o, inp=_eighths((B, C, h, w), gen), K=torch.tensor(VS_K).repeat(B, 1, 1), gw=_dyadic((B, C, h, w), gen), gd=_dyadic((B, 1, h, w), gen))

    def go(o, leaf, fn):
        L = {k: (leaf(o[k]) if k in grads else leaf(o[k]).detach()) for k in ('inp', 'depth', 'T', 'K')}
        warp, dwarp, valid = fn(L['inp'], L['depth'], L['T'], L['K'])
        ((warp*o['gw'].to(warp)).sum() + (dwarp*o['gd'].to(warp)).sum()).backward()
        g = {k: L[k].grad for k in grads}
        return dict(warp=warp, dwarp=dwarp, valid=valid.to(torch.uint8), g_input=g.get('inp'), g_depth=g.get('depth'), g_T=g['T'][..., :3, :] if 'T' in g else None, g_K=g.get('K'))

    def run(F, o): return go(o, _leaf, F.view_synth)
    def ref(o, dtype): return go(o, _to(dtype), lambda i, d, T, K: O.view_synth(i, d, T, K, aten=dtype == F32))
    case(f'view_synth_c{C}({h},{w})_{tag}', 'view_synth', operands, run, ref,
         tol or {'warp': TOL_VS_WARP, 'dwarp': TOL_VS_DWARP, 'valid': EQUAL, '*': TOL_VS_GRAD}, split=split, loose=['g_input'] if 'inp' in grads else ())


for _C in (1, 5):
    for _h, _w in VS_SHAPES:
        _view_synth('depth_regimes', _C, _h, _w, _vs_regimes); _view_synth('shifts_off_each_side', _C, _h, _w, _vs_shifts)
    _view_synth('on_the_borders', _C, 2, 2, _vs_borders)
    _view_synth('depth_1e-6', _C, 5, 9, _vs_extreme(1e-6))
    # At depth 1e6 the gradients to the depth and to K are differences of terms 1e6 times their size (the warp does not depend on either in the limit): no fp32
    # evaluation resolves them, the oracle's included, so they are not outputs of this case
    _view_synth('depth_1e6', _C, 5, 9, _vs_extreme(1e6), grads=('inp', 'T'))


# ---- photo_error --------------------------------------------------------------------------------------------------------------------------------------------
PHOTO_SHAPES = [(2, 2), (5, 7), (33, 47)]
PHOTO_MODES = {'ssim': ('ssim', 0.85), 'ssim_w0': ('ssim', 0.0), 'ssim_w1': ('ssim', 1.0), 'l1': ('l1', 0.85), 'l2': ('l2', 0.85)}


def _checker(shape): return ((torch.arange(shape[-2]).view(-1, 1) + torch.arange(shape[-1]).view(1, -1)) % 2).float().expand(shape).clone()


def _ph_equal(shape, gen):
    x = _eighths(shape, gen)
    return x, x.clone()


def _ph_contrast(k):
    """Near 1 with a contrast of 2^-k.  k = 12: 9 sxx - sx^2 is 81 times a variance of 1e-8 between two numbers of size 81, below one fp32 rounding of either: the
    oracle's fp32 SSIM error map is wrong by its whole size there, so no fp32 bound exists and SSIM takes k = 4 (at k = 6 the oracle's fp32 is still at 8e-4 of the map's maximum, over a quarter of YARD_CAP)."""
    return lambda shape, gen: (1 - 2.0**-k*torch.randint(0, 2, shape, generator=gen).float(), 1 - 2.0**-k*torch.randint(0, 2, shape, generator=gen).float())


PHOTO_VALUES = {'pred_equals_target': _ph_equal,
                'constants': lambda shape, gen: (torch.full(shape, 0.25) + _cycle([0, 0.125, 0.25], shape[:2]).view(*shape[:2], 1, 1), torch.full(shape, 0.75)),
                'zero_against_one': lambda shape, gen: (torch.zeros(shape), torch.ones(shape)),
                'checker_against_inverse': lambda shape, gen: (_checker(shape), 1 - _checker(shape)),
                'contrast_2^-12': _ph_contrast(12), 'contrast_2^-4': _ph_contrast(4),
                'scale_1e2': lambda shape, gen: (100*torch.rand(shape, generator=gen), 100*torch.rand(shape, generator=gen))}


def _photo(tag, C, h, w, mode, fill, tol):
    loss_name, w_ssim = PHOTO_MODES[mode]

    def operands(gen):
        pred, target = fill((2, C, h, w), gen)
        return dict(pred=pred, target=target, ge=_pattern((2, 1, h, w)))

    def go(o, leaf, fn):
        pred = leaf(o['pred'])
        err = fn(pred, leaf(o['target']).detach()); err.backward(o['ge'].to(err))
        return dict(err=err, g_pred=pred.grad)
    case(f'photo_error_{mode}_c{C}({h},{w})_{tag}', 'photo_error', operands, lambda F, o: go(o, _leaf, lambda p, t: F.photo_error(p, t, loss_name, w_ssim)),
         lambda o, dtype: go(o, _to(dtype), lambda p, t: O.photo_error(p, t, loss_name, aten=dtype == F32, weight_ssim=w_ssim)), tol)


def _photo_tol(tag, mode, C):
    """The bounds of a photo_error case, or None where the combination is not a case."""
    ssim = PHOTO_MODES[mode] in (('ssim', 0.85), ('ssim', 1.0))      # (the modes in which the SSIM term is evaluated)
    grad = TOL_PHOTO_GRAD if C == 3 else TOL_PHOTO_GRAD_C
    # scale 1e2 (features, not images; C = 5): C1 and C2 are 1e-8 of the window sums and the error map reaches 1e2, where one fp32 rounding is the whole of
    # TOL_PHOTO_ERR's absolute part: the yardstick rule
    if tag == 'scale_1e2': return {'*': TOL_YARD} if C == 5 else None
    # Constant windows under SSIM: the variance 9 sxx - sx^2 is exactly 0, and what fp32 leaves of it stands over C2 = 9e-4.  The error map meets its bound; the
    # oracle's fp32 gradient is at up to 0.65 x TOL_PHOTO_GRAD: the yardstick rule for the gradient (the cancellation edge forces it)
    if tag == 'constants' and ssim: return dict(err=TOL_PHOTO_ERR, g_pred=TOL_YARD)
    # The contrasts: 2^-12 where SSIM is not evaluated, 2^-4 where it is (`_ph_contrast`), the latter under the yardstick rule (the oracle's fp32 is at up to 40 x
    # TOL_PHOTO_ERR at 2^-6 already).  SSIM AT 2^-12 has no fp32 reference: test_gpu_value_edges_loss.py holds it to what needs none (SSIM_UNRESOLVED)
    if tag == 'contrast_2^-4': return {'*': TOL_YARD} if ssim else None
    if tag == 'contrast_2^-12' and ssim: return None
    # C = 5 is held relative to the gradient's maximum: where pred == target the SSIM gradient is 0 up to rounding in fp64 too, and has no such measure
    if tag == 'pred_equals_target' and ssim and C == 5: return None
    return dict(err=TOL_PHOTO_ERR, g_pred=grad)


for _tag, _fill in PHOTO_VALUES.items():
    for _h, _w in PHOTO_SHAPES:
        for _mode in PHOTO_MODES:
            for _C in (3, 5):
                if _photo_tol(_tag, _mode, _C) is not None: _photo(_tag, _C, _h, _w, _mode, _fill, _photo_tol(_tag, _mode, _C))
# SSIM at a contrast of 2^-12, the issue's cancellation in 9 sxx - sx^2: (weight_ssim, C) of the runs test_gpu_value_edges_loss.py::test_ssim_at_contrast_2_12 makes
SSIM_UNRESOLVED = [(0.85, 3), (1.0, 3), (0.85, 5), (1.0, 5)]


# ---- recon_reduce -------------------------------------------------------------------------------------------------------------------------------------------
RR_SHAPES = [(2, 2, 2), (2, 5, 7), (2, 33, 47)]      # (B, h, w): 6188 elements take 25 blocks
UNCERTAINTY_LEVELS = [0.0, 1e-7, 1.0, 10.0, 50.0]
# The incoming gradient, a power of two: under the mask of 50 the gradient to an error map is exp(-50)/(n B h w) = 1e-26 of it, and `rel_to_max` measures a slice
# against no less than 1e-20
RR_GRAD_SCALE = 2.0**24


@contextlib.contextmanager
def _errors_as_images():
    """`recon_loss` on error maps: its photometric stage is the identity for the duration."""
    keep = O.photo_error
    O.photo_error = lambda pred, target, *a, **k: pred
    try: yield
    finally: O.photo_error = keep


def _rr_maps(n, shape, gen): return 0.125 + _eighths((n, *shape), gen, 0, 8)      # eighths in [0.125, 1]: sums over three supports are exact


def _rr_identical(n, shape, gen):
    e = _rr_maps(1, shape, gen).expand(n, *shape).clone()
    return dict(ew=e)


def _rr_tie_static(n, shape, gen):
    e = _rr_maps(n, shape, gen)
    return dict(ew=e, es=e.clone(), noise=torch.zeros(shape[0], 1, *shape[1:]))


def _rr_ulp_static(n, shape, gen):
    e = _rr_maps(n, shape, gen)
    return dict(ew=e, es=torch.nextafter(e, torch.zeros_like(e)), noise=torch.zeros(shape[0], 1, *shape[1:]))


def _rr_explain(n, shape, gen):
    return dict(ew=_rr_maps(n, shape, gen), mask=torch.randint(0, 2, (shape[0], n, *shape[1:]), generator=gen).float())


def _rr_uncertain(n, shape, gen):
    """One level per sample (B = 5): the error map, the gradients and the mask's gradient are judged per level."""
    shape = (len(UNCERTAINTY_LEVELS), *shape[1:])
    return dict(ew=_rr_maps(n, shape, gen), mask=torch.tensor(UNCERTAINTY_LEVELS).view(-1, 1, 1, 1).expand(shape[0], n, *shape[1:]).clone())


def _recon_reduce(tag, n, shape, fill, use_min, mask_name=None, split=None):
    def operands(gen): return fill(n, shape, gen)

    def go(o, leaf, fn):
        ew, mask = leaf(o['ew']), (leaf(o['mask']) if 'mask' in o else None)
        loss, err, sel = fn(ew, leaf(o['es']).detach() if 'es' in o else None, o.get('noise'), mask)
        (loss*RR_GRAD_SCALE).backward()
        return dict(loss=loss, err=err, sel=sel, g_err_warp=ew.grad, g_mask=None if mask is None else mask.grad)

    def run(F, o): return go(o, _leaf, lambda ew, es, noise, mask: F.recon_reduce(ew, es, use_min=use_min, noise=noise, mask=mask, mask_name=mask_name))

    def ref(o, dtype):
        def fn(ew, es, noise, mask):
            with _errors_as_images():
                loss, out = O.recon_loss(ew.unsqueeze(2), torch.zeros_like(ew[0]).unsqueeze(1), source=None if es is None else es.unsqueeze(2), loss_name='l1', use_min=use_min,
                                         use_automask=es is not None, noise=None if noise is None else noise.to(ew), mask=mask, mask_name=mask_name)
            return loss, out['err'], out['sel']
        return go(o, _to(dtype), fn)
    case(f'recon_reduce_n{n}{shape}_{tag}{"_min" if use_min else "_mean"}', 'recon_reduce', operands, run, ref,
         {'loss': TOL_MASKED_LOSS, 'err': ('close', 0, SWEEP_ERR_ATOL), 'sel': EQUAL, '*': TOL_MASKED_GRAD}, split=split)


for _n in (2, 3):
    for _shape in RR_SHAPES:
        for _um in (True, False):
            _recon_reduce('identical_supports', _n, _shape, _rr_identical, _um)
            _recon_reduce('all_zero', _n, _shape, lambda n, shape, gen: dict(ew=torch.zeros(n, *shape)), _um)
            _recon_reduce('static_ties_warped', _n, _shape, _rr_tie_static, _um)
            _recon_reduce('explainability_0_1', _n, _shape, _rr_explain, _um, 'explainability')
        # one ulp under the minimum: under the mean (a + b + c)/3 two roundings could close the gap in one precision and not in the other
        _recon_reduce('static_one_ulp_smaller', _n, _shape, _rr_ulp_static, True)
        # the mean over the supports: no decision between two differently masked errors.  With `use_min`: identical supports under identical masks (all ties)
        _recon_reduce('uncertainty_levels', _n, _shape, _rr_uncertain, False, 'uncertainty', split=dict(err=0, g_err_warp=1, g_mask=0))
        _recon_reduce('uncertainty_levels_identical_supports', _n, _shape, lambda n, shape, gen: dict(_rr_uncertain(n, shape, gen), ew=_rr_identical(n, (5, *shape[1:]), gen)['ew']),
                      True, 'uncertainty', split=dict(err=0, g_err_warp=1, g_mask=0))


# ---- regression_loss ----------------------------------------------------------------------------------------------------------------------------------------
REGR_SHAPES = [(1, 1, 2, 2), (2, 1, 5, 7), (2, 1, 33, 47)]      # 3102 elements: four blocks of 1024
LOG_DIFFS = [1e-8, 1e-4, 1.0, 1e4, 1e8]
INVERT_VALUES = [0.0, -1.0, EPS, 1e-10, 1.0, 1e6]


def _rg_mask(shape, gen): return torch.rand(shape, generator=gen) < 0.7


def _rg_equal(shape, gen):
    x = 0.125 + _eighths(shape, gen)
    return dict(pred=x, target=x.clone())


def _rg_berhu_ties(shape, gen):
    """Differences in eighths below 5, the maximum 5 at three elements (the first, the last and a middle one, which the mask leaves out), every fifth element at exactly
    1 = delta (0.2 x 5 rounds to 1 in fp32 and in fp64)."""
    n = torch.Size(shape).numel()
    diff = _eighths((n,), gen, 0, 40)
    diff[::5] = 1.0
    sign = 1 - 2.0*torch.randint(0, 2, (n,), generator=gen)
    mask = torch.ones(n, dtype=torch.bool)
    if n > 4: diff[0] = diff[-1] = diff[n//2] = 5.0; mask[n//2] = False; mask[3::7] = False
    else: diff[0] = diff[-1] = 5.0; diff[1] = 1.0; mask[-1] = False
    target = _eighths((n,), gen)
    return dict(pred=(target + sign*diff).view(shape), target=target.view(shape), mask=mask.view(shape))


def _rg_log(shape, gen):
    n = torch.Size(shape).numel()
    return dict(pred=(_cycle(LOG_DIFFS, (n,))*(1 - 2.0*(torch.arange(n) % 2))).view(shape), target=torch.zeros(shape))


def _rg_invert(values):
    """Every pair (pred, target) of `values`, one pair per index of dim 0 of a (k k, m) tensor: to_inv gives 0 for 0 and the negative, 1/eps for eps and for 1e-10.
    Pairs at 1/eps stand beside pairs at 1; TOL_REGR and TOL_REGR_GRAD are per-element bounds, so neither hides the other."""
    def fill(shape, gen):
        k = len(values)
        assert shape[0] == k*k
        v, i = torch.tensor(values), torch.arange(k*k)
        return dict(pred=v[i % k].view(-1, 1).expand(shape).clone(), target=v[i//k].view(-1, 1).expand(shape).clone())
    return fill


def _regression(tag, shape, loss_name, fill, invert=False, masked=False, tol=None, split=None):
    def operands(gen):
        o = fill(shape, gen)
        if masked == 'none': o['mask'] = torch.zeros(o['pred'].shape, dtype=torch.bool)
        elif masked and 'mask' not in o: o['mask'] = _rg_mask(o['pred'].shape, gen)
        elif not masked: o.pop('mask', None)
        return o

    def go(o, leaf, fn):
        pred = leaf(o['pred'])
        loss, err = fn(pred, leaf(o['target']).detach(), o.get('mask')); loss.backward()
        return dict(loss=loss, err=err, g_pred=pred.grad)

    def ref(o, dtype):
        def fn(p, t, m):
            loss, out = O.regression_loss(p, t, None if m is None else m.to(p.dtype), loss_name, invert)
            return loss, out['err_regr']
        return go(o, _to(dtype), fn)
    case(f'regression_{loss_name}{shape}_{tag}{"_invert" if invert else ""}{"_mask" if masked is True else "_mask_all_false" if masked else ""}', 'regression_loss', operands,
         lambda F, o: go(o, _leaf, lambda p, t, m: F.regression_loss(p, t, m, loss_name=loss_name, invert=invert)), ref, tol or {'g_pred': TOL_REGR_GRAD, '*': TOL_REGR}, split=split)


for _shape in REGR_SHAPES:
    for _name in ('l1', 'log_l1', 'berhu'):
        for _masked in (False, True):
            _regression('pred_equals_target', _shape, _name, _rg_equal, masked=_masked)
        # sum(mask) = 0: the oracle's loss is 0/0 and its gradient 0 x inf; the kernel is held to the oracle's pattern, whatever it is
        _regression('dyadic', _shape, _name, lambda shape, gen: dict(pred=_eighths(shape, gen), target=_eighths(shape, gen)), masked='none')
    for _masked in (False, True): _regression('ties_at_max_and_delta', _shape, 'berhu', _rg_berhu_ties, masked=_masked)
    _regression('diffs_1e-8_to_1e8', _shape, 'log_l1', _rg_log)


for _name in ('l1', 'log_l1', 'berhu'):
    # 1e6 under l1 only.  berHu: 1/eps - 1e-6 IS 1/eps in fp32: the pair (eps, 1e6) would attain the maximum in fp32 and not in fp64, and the count of ties is a
    # decision.  log_l1: `(1 + diff).log()` at diff = 1e-6 is 5 % off in any fp32 evaluation (1 + 1e-6 rounds first), half of TOL_REGR's absolute part: no room to spare
    _values = INVERT_VALUES if _name == 'l1' else INVERT_VALUES[:5]
    for _m in (1, 3, 87):      # (k k, m): 36 x 87 elements are four blocks of 1024
        for _masked in (False, True): _regression('to_inv_edges', (len(_values)**2, _m), _name, _rg_invert(_values), invert=True, masked=_masked)


# ---- disp_to_depth ------------------------------------------------------------------------------------------------------------------------------------------
# (size, pyramid): the smallest; an integer ratio; the non-integer ratios of test_k0_and_smoothness_at_non_integer_ratios
K0_PYRAMIDS = [((2, 2), [(2, 2), (1, 1)]), ((6, 20), [(6, 20), (3, 10)]), ((33, 47), [(33, 47), (16, 23), (8, 11)])]


def _k0_operands(size, lows, gen):
    """Sample 0: quarters in [0.25, 1] (exact ones); sample 1: constant planes (0 at the first scale, 1 at the second, 0.5 below); sample 2: as sample 0 with pixels of
    exactly 0 and one of 1e-10.  The gradients are judged per sample: sample 2's reach depth^2 = 1/eps^2."""
    o = dict(gup=_dyadic((len(lows), 3, 1, *size), gen))
    for s, (hs, ws) in enumerate(lows):
        d = torch.randint(1, 5, (3, 1, hs, ws), generator=gen).float()/4
        d[1] = [0.0, 1.0, 0.5][min(s, 2)]
        d[2].flatten()[::3] = 0.0
        if hs*ws > 1: d[2, 0, -1, -1] = 1e-10
        o[f'd{s}'] = d
    return o


def _disp_to_depth(size, lows, mn, mx):
    S = len(lows)

    def go(o, leaf, fn):
        d = {s: leaf(o[f'd{s}']) for s in range(S)}
        dep = fn(d)
        (dep*o['gup'].to(dep)).sum().backward()
        return dict(depth_up=dep, **{f'g_d{s}': v.grad for s, v in d.items()})

    def run(F, o): return go(o, _leaf, lambda d: F.disp_to_depth(list(d.values()), size, mn, mx)[0])
    def ref(o, dtype): return go(o, _to(dtype), lambda d: torch.stack(list(O.disp_to_depth_up(d, size, mn, mx, aten=dtype == F32)[1].values())))
    # At a non-integer ratio the interpolation weight next to a pixel of exactly 0 is all there is of the disparity, and in fp32 it carries the rounding of a source
    # coordinate of up to 47: the oracle's fp32 is at 1.6 x TOL_K0_DEPTH there.  The yardstick rule, per sample (the zero pixels force it)
    integer = all(size[0] % hs == 0 and size[1] % ws == 0 for hs, ws in lows)
    case(f'disp_to_depth{size}_{len(lows)}_scales_range_{mn}_{mx}', 'disp_to_depth', lambda gen: _k0_operands(size, lows, gen), run, ref,
         {'depth_up': TOL_K0_DEPTH if integer else TOL_YARD, '*': TOL_K0_GRAD}, split=dict({f'g_d{s}': 0 for s in range(S)}, **({} if integer else {'depth_up': 1})))


for _size, _lows in K0_PYRAMIDS:
    for _mn, _mx in ((0.1, 100), (None, None)): _disp_to_depth(_size, _lows, _mn, _mx)


# ---- disp_smooth_fused / disp_smooth_blurred ----------------------------------------------------------------------------------------------------------------
def _sm_rand(shape, gen): return 0.05 + 0.9*torch.rand(shape, generator=gen)
def _sm_img(shape, gen): return torch.rand(shape[0], 3, *shape[2:], generator=gen)


SMOOTH_VALUES = {      # tag -> (disparity, image)
    'constant_disp': (lambda shape, gen: torch.full(shape, 0.5), _sm_img),                       # mean exactly 0.5, d/mean exactly 1: every difference 0, aux maps sqrt(eps)
    'zero_disp': (lambda shape, gen: torch.zeros(shape), _sm_img),                                # mean < eps: the clamp is active, the mean term off
    'disp_1e-6': (lambda shape, gen: 1e-6*_sm_rand(shape, gen), _sm_img),
    'constant_image': (_sm_rand, lambda shape, gen: torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1).expand(shape[0], 3, *shape[2:]).clone()),      # edge weight exactly 1
    'checker_image': (_sm_rand, lambda shape, gen: _checker((shape[0], 3, *shape[2:])))}
SMOOTH_PYRAMIDS = [[(2, 2)], [(6, 20), (3, 10)], [(33, 47), (16, 23)]]


def _smooth_operands(lows, tag, gen):
    fd, fi = SMOOTH_VALUES[tag]
    o = {f'd{s}': fd((2, 1, hs, ws), gen) for s, (hs, ws) in enumerate(lows)}
    o['imgs'] = fi((2, 1, *lows[0]), gen)
    return o


def _smooth_go(S):
    def go(o, leaf, fn):
        d = {s: leaf(o[f'd{s}']) for s in range(S)}
        loss, dg, ig = fn(d, leaf(o['imgs']).detach()); loss.backward()
        return dict(loss=loss, disp_grad=dg, image_grad=ig, **{f'g_d{s}': v.grad for s, v in d.items()})
    return go


def _disp_smooth(tag, lows, edges, lap):
    go = _smooth_go(len(lows))

    def ref(o, dtype):
        def fn(d, imgs):
            ls = {s: O.smooth_reg(v, O.resize_bilinear(imgs, v.shape[-2:], aten=dtype == F32), edges, use_laplacian=lap) for s, v in d.items()}      # (`O.disp_smooth` with the second-order form)
            return torch.stack([v[0]/2**s for s, v in ls.items()]).mean(), ls[0][1]['disp_grad'], ls[0][1]['image_grad']
        return go(o, _to(dtype), fn)
    case(f'disp_smooth_fused{lows}_{tag}_edges{int(edges)}_laplacian{int(lap)}', 'disp_smooth_fused', lambda gen: _smooth_operands(lows, tag, gen),
         lambda F, o: go(o, _leaf, lambda d, imgs: F.disp_smooth_fused(d, imgs, use_edges=edges, want_aux=True, use_laplacian=lap)), ref,
         {'loss': TOL_K0_LOSS, 'disp_grad': TOL_SMOOTH_AUX, 'image_grad': TOL_SMOOTH_AUX, '*': TOL_K0_GRAD})


def _disp_smooth_blurred(tag, size, edges):
    """One scale (the form test_blurred_smoothness pins).  No constant disparity here: its blur is constant up to the rounding of the three weights, and the sign
    of that rounding would be the whole gradient, in fp64 as well."""
    go = _smooth_go(1)

    def ref(o, dtype):
        def fn(d, imgs):
            loss, ld = O.smooth_reg(d[0], imgs, edges, use_blur=True)
            return loss, ld['disp_grad'], ld['image_grad']
        return go(o, _to(dtype), fn)
    case(f'disp_smooth_blurred{size}_{tag}_edges{int(edges)}', 'disp_smooth_blurred', lambda gen: _smooth_operands([size], tag, gen),
         lambda F, o: go(o, _leaf, lambda d, imgs: F.disp_smooth_blurred(d, imgs, use_edges=edges, want_aux=True)), ref,
         {'loss': TOL_BLURRED_LOSS, 'disp_grad': TOL_SMOOTH_AUX, 'image_grad': TOL_SMOOTH_AUX, '*': TOL_BLURRED_GRAD})


for _tag in SMOOTH_VALUES:
    for _lows in SMOOTH_PYRAMIDS:
        for _edges in (False, True):
            for _lap in (False, True): _disp_smooth(_tag, _lows, _edges, _lap)
            if _tag != 'constant_disp': _disp_smooth_blurred(_tag, _lows[0], _edges)


# ---- scale_mean ---------------------------------------------------------------------------------------------------------------------------------------------
MEAN_LEVELS = [0.0, 1.0, 2.0**-24, 1 - 2.0**-24, 0.5, 0.25]      # one per index of dim 0: the gradient at 0 is -1e12 (ATen's 1e-12 under the quotient), at 1 exactly 0
MEAN_SHAPES = [(5, 7), (2, 2), (33, 47)]                         # per tensor (6, n, h, w): 9306 n elements are 3 n blocks of 4096


def _scale_mean(mode, n):
    S = len(MEAN_SHAPES)

    def operands(gen): return {f'x{s}': torch.tensor(MEAN_LEVELS).view(-1, 1, 1, 1).expand(len(MEAN_LEVELS), n, *hw).clone() for s, hw in enumerate(MEAN_SHAPES)}

    def go(o, leaf, fn):
        L = [leaf(o[f'x{s}']) for s in range(S)]
        loss = fn(L); (2.5*loss).backward()
        return dict(loss=loss, **{f'g_x{s}': x.grad for s, x in enumerate(L)})

    def ref(o, dtype):      # `TF.binary_cross_entropy` clamps the logarithm at -100, and its backward divides by max((1 - x) x, 1e-12)
        def fn(R):
            if mode == 'bce_ones': return torch.stack([TF.binary_cross_entropy(r, torch.ones_like(r)) for r in R]).mean()
            return torch.stack([(r.mean() if mode == 'identity' else -r.mean()) for r in R]).mean()
        return go(o, _to(dtype), fn)
    case(f'scale_mean_{mode}_n{n}_levels', 'scale_mean', operands, lambda F, o: go(o, _leaf, lambda L: F.scale_mean(L, mode)), ref,
         {'loss': _scalar_rel(TOL_MEAN_LOSS), '*': TOL_MEAN_GRAD}, split={f'g_x{s}': 0 for s in range(S)})


for _mode in ('bce_ones', 'identity', 'negate'):
    for _n in (1, 3): _scale_mean(_mode, _n)


# ---- pose_matrices / intrinsics -----------------------------------------------------------------------------------------------------------------------------
POSE_ANGLES = [0.5, -1.0, EPS, 2.0**-10]      # about one axis at a time, the other two components exactly 0: W has exact zeros; |aa| exactly eps: the clamp's edge


def _pose(tag, t_of):
    N = 3*len(POSE_ANGLES)

    def operands(gen):
        aa = torch.zeros(N, 3)
        for i, a in enumerate(POSE_ANGLES):
            for ax in range(3): aa[3*i + ax, ax] = a
        return dict(aa=aa, t=t_of(N, gen), inv=(torch.arange(N) % 2).to(torch.uint8), gT=_dyadic((N, 4, 4), gen))

    def go(o, leaf, fn):
        aa, t = leaf(o['aa']), leaf(o['t'])
        T = fn(aa, t, o['inv']); T.backward(o['gT'].to(T))
        return dict(T=T, g_aa=aa.grad, g_t=t.grad)

    def ref(o, dtype):
        def fn(aa, t, inv):
            T = O.T_from_AAt(aa, t)
            return torch.stack([torch.linalg.inv(Ti) if f else Ti for Ti, f in zip(T, inv)])
        return go(o, _to(dtype), fn)
    case(f'pose_matrices_single_axis_{tag}', 'pose_matrices', operands, lambda F, o: go(o, _leaf, F.pose_matrices), ref, dict(T=TOL_POSE_T, g_aa=TOL_POSE_GAA, g_t=TOL_POSE_GT))


_pose('t_zero', lambda N, gen: torch.zeros(N, 3))
_pose('t_unit', lambda N, gen: _dyadic((N, 3), gen))
_pose('t_1e4', lambda N, gen: 1e4*(1 + _eighths((N, 3), gen)))


def _intrinsics(size):
    def operands(gen):
        v = torch.tensor([1e-3, 10.0, 0.5])
        fs, cs = torch.cartesian_prod(v, v), torch.cartesian_prod(v, v).flip(0)
        return dict(fs=fs, cs=cs, gK=_dyadic((len(fs), 4, 4), gen), gKi=_dyadic((len(fs), 4, 4), gen))

    def go(o, leaf, fn, inv):
        fs, cs = leaf(o['fs']), leaf(o['cs'])
        K, Ki = fn(fs, cs); ((K*o['gK'].to(K)).sum() + (Ki*o['gKi'].to(K)).sum()).backward()
        Ks = K.detach().clone(); Ks[:, 0, 1] = 0.5*Ks[:, 0, 0]      # a caller's K with skew: the adjugate inverse
        return dict(K=K, K_inv=Ki, g_fs=fs.grad, g_cs=cs.grad, skew_inv=inv(Ks))

    def ref(o, dtype):
        def fn(fs, cs):
            K = O.resize_K(O.build_K(fs, cs), size)
            return K, torch.linalg.inv(K)
        return go(o, _to(dtype), fn, torch.linalg.inv)
    # c/f reaches 1e4: the LU inverse of the oracle's fp32 is at up to 4.8 x TOL_KINV.  The yardstick rule for the two inverses, per sample (fs = 1e-3 beside cs = 10 forces it)
    case(f'intrinsics{size}_fs_cs_1e-3_10', 'intrinsics', operands, lambda F, o: go(o, _leaf, lambda fs, cs: F.intrinsics(fs, cs, size), F.inv_intrinsics), ref,
         dict(K=TOL_K, K_inv=TOL_YARD, skew_inv=TOL_YARD, g_fs=TOL_K_GRAD, g_cs=TOL_K_GRAD), split=dict(K_inv=0, skew_inv=0))


_intrinsics((2, 2)); _intrinsics((96, 320))


# ---- image_recon_fused --------------------------------------------------------------------------------------------------------------------------------------
def _image_recon(b, h, w, identical, constant=False):
    """The fused kernels' own copies of the geometry (`issue`, `finish_depth`) at the depth regimes and the border-crossing translation of the `view_synth` cases: the
    mean over two supports, no automask (no decision; `sel` is 0).  Support 0: tz = -1 under VS_DEPTHS; support 1: three pixels to the left at tz = 0."""
    n, S = 2, 2

    def operands(gen):
        imgs = _eighths((b, 3, h, w), gen)
        if w == 47:      # (and the images are ramps, one slope per channel and sample in 1/128: a ramp's bilinear derivative is the same on both sides of a centre)
            v, u = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
            imgs = 0.125 + (torch.randint(0, 3, (b, 3, 1, 1), generator=gen).float()*u + torch.randint(0, 3, (b, 3, 1, 1), generator=gen).float()*v)/128
        # The bilinear derivative jumps where a sample lands exactly on a pixel centre, and with w/(w - 1) not dyadic fp32 and fp64 land on different sides of it.
        # At w = 47 the one dyadic p that does is 23: cx = 23.25 and a shift of 2.75 pixels keep every (D u - cx)/z and u + 2.75/D off it (at h = 33 the scale is dyadic).
        cx, shift = (w//2, 3.0) if w != 47 else (23.25, 2.75)
        # A constant target: every window's variance 9 syy - sy^2 is exactly 0.  The fused forward forms the target's term as fmaf(9, syy, 81 C2) - sy^2 (the order
        # `photo_error` had before its fix), which puts the rounding of 81 sy^2 over 81 C2 = 0.07: at most 3e-5 of a channel's error, a tenth of SWEEP_ERR_ATOL (measured: 2.3e-6, profiles/value_edges_loss.txt)
        if constant: imgs = torch.tensor([0.75, 0.5, 0.375]).view(1, 3, 1, 1).expand(b, 3, h, w).clone()
        K = torch.tensor([[16.0, 0, cx, 0], [0, 4.0, h//2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).repeat(b, 1, 1)
        T = torch.stack([_vs_T([[0, 0, -1.0]]*b), _vs_T([[shift/16, 0, 0]]*b)])
        depth = torch.stack([_cycle(VS_DEPTHS, (b, 1, h, w), 3), _cycle(VS_DEPTHS, (b, 1, h, w), 5)])
        return dict(imgs=imgs, supp=imgs[None].repeat(n, 1, 1, 1, 1) if identical else (_eighths((n, b, 3, h, w), gen) if w != 47 else imgs[None].flip(3) + _eighths((n, b, 3, 1, 1), gen)/4), depth=depth, T=T, K=K)

    def go(o, leaf, fn):
        d, T = leaf(o['depth']), leaf(o['T'])
        loss, err, sel = fn(d, leaf(o['imgs']).detach(), leaf(o['supp']).detach(), T, leaf(o['K']).detach()); loss.backward()
        return dict(loss=loss, err=err, sel=sel, g_depth=d.grad, g_T=T.grad[..., :3, :])

    def run(F, o): return go(o, _leaf, lambda d, i, s, T, K: F.image_recon_fused(d, i, s, T, K, flags=F.recon_flags('ssim', False, False))[:3])

    def ref(o, dtype):
        def fn(d, i, s, T, K):
            loss, _, full = O.image_recon({k: d[k] for k in range(S)}, i, s, T, K, 'ssim', False, False, aten=dtype == F32)
            return loss, full['err'], full['sel']
        return go(o, _to(dtype), fn)
    case(f'image_recon_fused({b},{h},{w})_depth_regimes{"_supports_equal_target" if identical else ""}{"_constant_target" if constant else ""}', 'image_recon_fused', operands, run, ref,
         {'loss': SWEEP_LOSS, 'err': ('close', 0, SWEEP_ERR_ATOL), 'sel': EQUAL, '*': ('rel', SWEEP_GRAD)})


for _dims in [(1, 6, 20), (2, 33, 47)]:
    for _identical in (False, True): _image_recon(*_dims, _identical)
_image_recon(1, 6, 20, False, constant=True)      # (at 33 x 47 the supports are ramps of the target: under a constant target they carry no gradient to judge)
