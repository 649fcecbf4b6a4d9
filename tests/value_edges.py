"""Value-edge cases for the encoder / decoder operators (`batch_norm_act`, `layer_norm_cf`, `max_pool3x3s2`, `dwconv7x7`, `elu_pad`, `elu_up_cat_pad`,
`conv3x3_head`, `conv3x3_headn`) and, since they were merged, `channel_attention`, `se_gate`, `relu_pad`, `up_cat_gate_pad`, `ddv_head`, `subpixel_conv`, `flip_blend`,
`flip_blend_pyramid` and `feat_regs`: the table and the judge.  Device-agnostic; test_value_edges_host.py checks the table on the CPU, test_gpu_value_edges.py runs it.

The suite's other families sweep shapes, memory and gradient subsets on Gaussian or uniform data.  Here the VALUES are the edge: one element far off a channel's
mean (at the first position, and at the last as a control), mean >> sigma, zero variance, scales that differ by 1e6 between channels, -inf / NaN / full ties in
the pool, pre-activations from 1e-7 to 1e4 through ELU and the sigmoid, one-hot images smaller than the 7x7 window on exact integer operands.  For the second
group: one-hot, uniform and tied softmax rows, gates saturated at +-200, dead hidden layers, all-zero operands, channel means 1e8 apart, disparities of exactly 0
and 1, feature plateaus, image contrasts whose edge weight is exactly 1 or underflows to 0 (no NaN and no infinity there: only the pool cases carry them).

No tolerance is introduced: every output is held to the named bound of the operator's own parity test (test_gpu_hostile_memory.py lists them).  Two
refinements keep a large-scale part of a tensor from hiding a small-scale part: BatchNorm tensors shaped like `x` are judged per channel and LayerNorm
tensors per sample (`split`), each slice relative to its own maximum.  No element is left out of any comparison; where the reference is not finite (the
pool's -inf and NaN cases) the pattern has to be identical.

Case: name; op; operands(gen) -> {name: CPU tensor}; run(F, ops) -> {name: tensor} (outputs and all gradients, on the operands' device);
ref(ops, dtype) -> the same operation on plain ATen on the CPU in `dtype` (float64: the reference; float32: the yardstick of the host test);
tol: {name: bound, '*': default} (the kinds: `KINDS` below); split: {name: dim or (dim, size)} (slices judged one by one); check: None or f(out) with the case's extra assertions."""
from collections import namedtuple

import torch
import torch.nn.functional as TF

from conftest import rel_to_max
from ddvnet_inputs import NUM_BINS
from superdepth_inputs import SUBPIXEL_CASES, subpixel_aten
from test_blend_host import blend_bound, scale_of
from test_cadepth_host import se_aten, sp_aten
from test_ddvnet_host import ddv_aten
from test_diffnet_host import fuse_aten, relu_pad_aten
from test_featdepth_host import FEAT_WEIGHTS, ulp_of
from test_gpu_cadepth import FLOOR
from test_gpu_hostile_memory import (EQUAL, TOL_BF16_OUT, TOL_BN, TOL_CONV_F32, TOL_DWCONV, TOL_GLUE_BIAS, TOL_GLUE_GA, TOL_GLUE_GX, TOL_GLUE_OUT, TOL_LN,
                                     TOL_LN_BF16_GRAD, TOL_LN_BF16_OUT, TOL_POOL_GX)

BF = torch.bfloat16
F64, F32 = torch.float64, torch.float32
OPERATORS = ('batch_norm_act', 'layer_norm_cf', 'max_pool3x3s2', 'dwconv7x7', 'elu_pad', 'elu_up_cat_pad', 'conv3x3_head', 'conv3x3_headn',
             'channel_attention', 'se_gate', 'relu_pad', 'up_cat_gate_pad', 'ddv_head', 'subpixel_conv', 'flip_blend', 'flip_blend_pyramid', 'feat_regs')
# The bounds of the second group's own parity tests.  FLOOR (test_gpu_cadepth.py; test_ddvnet_host.py's, which test_gpu_ddvnet.py, test_gpu_diffnet.py and
# test_gpu_superdepth.py import, is the same number): `se_gate` is held to it as it stands (test_se_gate_matches_fp64), the others to max(FLOOR, 4 x yardstick).
TOL_SE = ('rel', FLOOR)           # test_gpu_cadepth.py::test_se_gate_matches_fp64
TOL_YARD = ('yard', FLOOR)        # test_channel_attention_matches_fp64, test_ddv_head_matches_fp64, test_gpu_diffnet.py::_hold, test_subpixel_conv_matches_the_reference_fixture
TOL_FEATREG = ('yard_ulp',)       # test_featdepth_host.py::featreg_bound

# The two thresholds of csrc/smd_norm.hip's BatchNorm, restated: one block per channel up to BN_SMALL values per channel (`kBnSmall`), else the chunked
# sweeps; `f4` loads when HW % 4 == 0.  Above BN_KEPT values per channel (`kBnMaxChunks*kBnItemsPerBlock`) a chunk holds more than a thread keeps in registers.
BN_SMALL, BN_KEPT = 16384, 128*8192


def bn_path(shape):
    N, _, H, W = shape
    return ('small' if N*H*W <= BN_SMALL else 'chunked' if N*H*W <= BN_KEPT else 'long'), ('f4' if (H*W) % 4 == 0 else 'scalar')


Case = namedtuple('Case', 'name op operands run ref tol split check')
CASES = []


def case(name, op, operands, run, ref, tol, split=None, check=None):
    CASES.append(Case(name, op, operands, run, ref, tol, split or {}, check))


# ---- the judge ----------------------------------------------------------------------------------------------------------------------------------------
# Bounds.  ('rel', b): max error over the tensor's (or slice's) maximum; ('close', rtol, atol); ('equal',); and, for the operators whose own parity tests use them:
# ('yard', floor): the rule of test_gpu_cadepth.py / test_gpu_ddvnet.py / test_gpu_diffnet.py / test_gpu_superdepth.py — relative to the maximum, at most the larger of
#   `floor` and 4 x the error of ATen's fp32 sequence (`c.ref(ops, F32)`, the yardstick) against the same fp64 reference, per slice where the output is split;
# ('yard_ulp',): `featreg_bound` of test_featdepth_host.py — in absolute terms, the larger of 4 x the yardstick's error and 2 ulp of the reference's largest magnitude;
# ('elem', f): f(ops) -> a per-element absolute bound (`blend_bound` of test_blend_host.py); where it is 0 the element has to be exact.
# The yardstick is ATen's output on the case's operands, never the kernel's.
YARD_KINDS = ('yard', 'yard_ulp')
KINDS = ('rel', 'close', 'equal', 'elem') + YARD_KINDS


def needs_yardstick(c): return any(b[0] in YARD_KINDS for b in c.tol.values())


def yardstick(c, ops):
    """ATen's fp32 sequence on the case's operands (None where no bound of the case is measured against it)."""
    return {k: v.detach() for k, v in c.ref({k: v.clone() for k, v in ops.items()}, F32).items() if v is not None} if needs_yardstick(c) else None


def same_pattern(got, ref):
    """Non-finite elements: NaN where the reference has NaN, the same infinity where it has one, finite everywhere else."""
    return bool(((got.isnan() == ref.isnan()) & (got.isinf() == ref.isinf()) & (~ref.isinf() | (got == ref))).all())


def _slices(t, how):
    """how: a dim (one slice per index) or (dim, size) (slices of `size` along dim: the bin groups of a weight)."""
    return t.unbind(how) if isinstance(how, int) else t.split(how[1], how[0])


def _ratio(err, bound):
    """err/bound with 0/0 = 0: an exact zero meets a zero bound, nothing else does."""
    return 0.0 if err == 0 else float('inf') if bound == 0 else err/bound


FLT_MIN = 2.0**-126      # float32's smallest normal number
YARD_CAP = 1e-3          # the widest relative bound an fp32 gradient has in this suite (TOL_VS_GRAD, TOL_MASKED_GRAD, TOL_CHAIN_GRAD of test_gpu_hostile_memory.py)


def below_fp32(ref): return ref.abs().max().item() < FLT_MIN


def _yard_excess(got, ref, yard, floor, yard_scale):
    """One tensor or slice under max(floor, 4 x yardstick), never wider than YARD_CAP: a yardstick that ATen's fp32 misses by more says the inputs are beyond
    fp32, and the host test refuses such a case instead of letting its bound grow.  A reference whose largest magnitude is below float32's smallest normal
    number (the gradients behind a softmax or a gate saturated past exp(-87)) has no relative measure in fp32: there the result has to be that small too."""
    if below_fp32(ref): return _ratio((got - ref).abs().max().item(), FLT_MIN)
    return rel_to_max(got, ref)/min(YARD_CAP, max(floor, 4*yard_scale*rel_to_max(yard, ref)))


def yardstick_errors(c, ref, yard):
    """-> {output: the worst slice's error of the yardstick relative to the slice's maximum} over the outputs held to ('yard', floor); slices below fp32 left out."""
    res = {}
    for k, r in ref.items():
        if r is None or c.tol.get(k, c.tol.get('*'))[0] != 'yard': continue
        r, y = r.detach().double().cpu(), yard[k].detach().double().cpu().reshape(r.shape)
        parts = [(y, r)] if k not in c.split else zip(_slices(y, c.split[k]), _slices(r, c.split[k]))
        res[k] = max([rel_to_max(a, b) for a, b in parts if not below_fp32(b)], default=0.0)
    return res


def excess(got, ref, bound, dim=None, yard=None, yard_scale=1.0, ops=None):
    """The error of `got` against `ref` in units of `bound` (<= 1 holds it); with `dim`, the worst slice along it, each relative to its own maximum.
    Every element takes part: a non-finite pattern that differs is an infinite excess, identical non-finite elements are equal.  `yard`: the yardstick's
    output for the yardstick bounds, counted `yard_scale` times (the host test halves it for ATen itself)."""
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu().reshape(got.shape)
    if not same_pattern(got, ref): return float('inf')
    if bound[0] == 'equal': return 0.0 if bool(((got == ref) | ref.isnan()).all()) else float('inf')
    fin = ref.isfinite()
    got, ref = torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, ref, torch.zeros_like(ref))      # (identical there: they add no error)
    if bound[0] == 'close':
        assert bound[2] > 0, 'every `close` bound of these operators has an absolute part'
        return ((got - ref).abs()/(bound[2] + bound[1]*ref.abs())).max().item()
    if bound[0] == 'elem':
        err, b = (got - ref).abs(), bound[1](ops).double().cpu().reshape(got.shape)
        return max(_ratio(e, v) for e, v in zip(err.flatten().tolist(), b.flatten().tolist()))
    if bound[0] in YARD_KINDS:
        assert yard is not None, 'a yardstick bound needs the yardstick'
        yard = yard.detach().double().cpu().reshape(got.shape)
    if bound[0] == 'yard_ulp':
        own = (yard - ref).abs().max().item()
        return _ratio((got - ref).abs().max().item(), max(4*yard_scale*own, 2*ulp_of(ref.abs().max().item())))
    if bound[0] == 'yard':
        parts = [(got, ref, yard)] if dim is None else zip(_slices(got, dim), _slices(ref, dim), _slices(yard, dim))
        return max(_yard_excess(g, r, y, bound[1], yard_scale) for g, r, y in parts)
    if dim is None: return rel_to_max(got, ref)/bound[1]
    return max(rel_to_max(g, r) for g, r in zip(_slices(got, dim), _slices(ref, dim)))/bound[1]


def errors(c, out, ref, ops=None, yard=None, yard_scale=1.0):
    """-> {output: excess} over every output of the case that has a bound."""
    res = {}
    for k, v in out.items():
        if v is None: continue
        bound = c.tol.get(k, c.tol.get('*'))
        assert bound is not None, f'{c.name}: no bound for {k}'
        res[k] = excess(v, ref[k], bound, c.split.get(k), None if yard is None else yard.get(k), yard_scale, ops)
    return res


def judge(c, out, ref, ops=None, yard=None):
    assert {k for k, v in out.items() if v is not None} == {k for k, v in ref.items() if v is not None}, f'{c.name}: outputs {sorted(out)} against {sorted(ref)}'
    for k, e in errors(c, out, ref, ops, yard).items():
        bound = c.tol.get(k, c.tol.get('*'))
        assert e <= 1.0, f'{c.name}: {k} misses its bound {bound} by a factor {e:.3g}' + (f' (worst slice along dim {c.split[k]})' if k in c.split else '')
    if c.check is not None: c.check(out)


def _dyadic(shape, gen): return torch.randint(-8, 9, shape, generator=gen).float()/8       # gradients whose sums are exact
def _leaf(t): return t.detach().clone().requires_grad_(True)
def _g(t): return None if t is None else t.grad


def _cast(dtype):
    """Operand -> a fresh CPU leaf in `dtype` (bf16 operands keep their rounded values)."""
    return lambda t: None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_(True)


# ---- batch_norm_act ---------------------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = {(3, 5, 7, 9): ('small', 'scalar'), (4, 8, 6, 20): ('small', 'f4'), (12, 6, 37, 41): ('chunked', 'scalar'), (5, 4, 64, 64): ('chunked', 'f4')}
BN_LONG_SHAPES = {(1, 2, 1023, 1027): ('long', 'scalar'), (1, 2, 1024, 1028): ('long', 'f4')}      # chunks longer than a thread's registers: read twice
BN_MEAN, BN_SIGMA = 2.0, 0.5


def _bn_base(shape, gen, mean=BN_MEAN, sigma=BN_SIGMA): return mean + sigma*torch.randn(*shape, generator=gen)


def _bn_outlier(K, where):
    def fill(shape, gen):
        x = _bn_base(shape, gen)
        if where == 'first': x[0, :, 0, 0] = BN_MEAN + K*BN_SIGMA
        else: x[-1, :, -1, -1] = BN_MEAN + K*BN_SIGMA
        return dict(x=x)
    return fill


def _bn_constant(shape, gen):
    """Variance exactly 0 in fp64 too: invstd = 1/sqrt(eps) = 316.  The constants are small against the bias: ATen's fp32 operator folds the mean into the offset
    (x*a + (bias - mean*a)), which costs it half an ulp of |mean|*316*gamma, and the yardstick has to hold the bound itself."""
    x, b = _bn_base(shape, gen), torch.randn(shape[1], generator=gen)
    x[:, 1] = 0.0; x[:, 2] = 2.0**-10
    b[1], b[2] = 1.0, -0.5
    return dict(x=x, b=b)


def _bn_scales(shape, gen):
    C = shape[1]
    sigma = torch.tensor([1e-3, 1.0, 1e3])[torch.arange(C) % 3].view(1, C, 1, 1)
    return dict(x=sigma*(BN_MEAN + torch.randn(*shape, generator=gen)))      # (each channel's mean scales with it: BN_MEAN_OVER_SIGMA below)


def _bn_dead(shape, gen):
    C = shape[1]
    k = torch.arange(C) % 3      # gamma = beta = 0: y exactly 0; beta = -50: dead; the third kind lives
    w, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    return dict(x=_bn_base(shape, gen), w=torch.where(k == 0, torch.zeros(C), w), b=torch.where(k == 0, torch.zeros(C), torch.where(k == 1, torch.full((C,), -50.0), b)))


BN_VALUES = {f'outlier{K}_{where}': _bn_outlier(K, where) for K in (5, 30, 300) for where in ('first', 'last')}
# mean >> sigma.  What fp32 can resolve is limited by the mean itself: BatchNorm hands the mean to its backward as ONE float, off by up to half an ulp =
# 6e-8*|mean|, i.e. 6e-8*mean/sigma of a standard deviation in every x - mean, and the same share of g_weight.  A quarter of TOL_BN (the room the host test
# asks the fp32 yardstick to leave) is 5e-6, reached at mean/sigma = 83; at mean/sigma = 1e4 every fp32 BatchNorm, ATen's included, is at 30 times the bound.
BN_MEAN_OVER_SIGMA = 50.0
BN_VALUES.update({'mean_50_sigma': lambda shape, gen: dict(x=_bn_base(shape, gen, 100.0, 100.0/BN_MEAN_OVER_SIGMA)), 'constant_channel': _bn_constant, 'sigma_1e-3_1_1e3': _bn_scales})


def _batch_norm(tag, shape, fill, relu, res):
    N, C, H, W = shape

    def operands(gen):
        o = dict(w=torch.rand(C, generator=gen) + 0.5, b=torch.randn(C, generator=gen), g=torch.randn(*shape, generator=gen), rm=torch.zeros(C), rv=torch.ones(C))
        if res: o['r'] = torch.randn(*shape, generator=gen)
        o.update(fill(shape, gen))
        return o

    def go(o, leaf, fn):
        x, w, b, r = leaf(o['x']), leaf(o['w']), leaf(o['b']), (leaf(o['r']) if res else None)
        rm, rv = o['rm'].detach().clone().to(x), o['rv'].detach().clone().to(x)
        y = fn(x, w, b, rm, rv, r); y.backward(o['g'].to(x))
        return dict(y=y, g_x=x.grad, g_weight=w.grad, g_bias=b.grad, g_residual=_g(r), running_mean=rm, running_var=rv)

    def run(F, o): return go(o, _leaf, lambda x, w, b, rm, rv, r: F.batch_norm_act(x, w, b, rm, rv, residual=r, momentum=0.1, eps=1e-5, relu=relu))

    def ref(o, dtype):
        def f(x, w, b, rm, rv, r):
            y = TF.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
            if res: y = y + r
            return TF.relu(y) if relu else y
        return go(o, _cast(dtype), f)
    case(f'batch_norm_act{shape}_{tag}{"_relu" if relu else ""}{"_res" if res else ""}', 'batch_norm_act', operands, run, ref, {'*': TOL_BN},
         split=dict(y=1, g_x=1, g_residual=1))


for _shape in BN_SHAPES:
    for _tag, _fill in BN_VALUES.items():
        for _relu, _res in [(False, False), (True, True)]: _batch_norm(_tag, _shape, _fill, _relu, _res)
    _batch_norm('dead_relu', _shape, _bn_dead, True, False)      # (a residual would revive the dead channels)
# M = 2: the unbiased factor of running_var.  Two values a few sqrt(eps) apart: further apart, x_hat is +-1 and g_x cancels to rounding noise in any precision
for _relu, _res in [(False, False), (True, True)]: _batch_norm('two_values', (2, 3, 1, 1), lambda shape, gen: dict(x=_bn_base(shape, gen, 0.1, 4e-3)), _relu, _res)
# (no ReLU on two million elements: some land within an fp32 rounding of 0, where the mask of any fp32 evaluation differs from the fp64 one)
# (and a sparse incoming gradient, 1 element in 64 in eighths: the fp32 yardstick sums g and g*x_hat sequentially, a million terms would be its error, not the kernel's)
def _bn_long(shape, gen): return dict(_bn_outlier(30, 'first')(shape, gen), g=_dyadic(shape, gen)*(torch.rand(*shape, generator=gen) < 1/64))


for _shape in BN_LONG_SHAPES: _batch_norm('outlier30_first', _shape, _bn_long, False, True)


# ---- layer_norm_cf ----------------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(2, 96, 6, 20), (1, 7, 33, 65), (2, 1030, 5, 7), (2, 1, 3, 3)]


def _ln_outlier(ch):
    def fill(shape, gen):
        x = 0.1*torch.randn(*shape, generator=gen)
        x[:, ch] = 50.0
        return x
    return fill


def _ln_constant_pixel(shape, gen):
    x = torch.randn(*shape, generator=gen)
    x[0, :, 0, 0] = 1.25; x[-1, :, -1, -1] = -7.0; x[0, :, shape[2]//2, 1] = 0.0       # variance 0: rstd = rsqrt(eps) (values whose fp32 sums over C are exact)
    return x


# A common offset: as for BatchNorm, the float that carries the mean to the backward bounds what fp32 can resolve (6e-8*offset/sigma against a quarter of TOL_LN)
LN_OFFSET = 20.0
LN_VALUES = {'outlier_first': _ln_outlier(0), 'outlier_last': _ln_outlier(-1), 'offset_20': lambda shape, gen: LN_OFFSET + torch.randn(*shape, generator=gen),
             'constant_pixel': _ln_constant_pixel, 'scale_1e-4': lambda shape, gen: 1e-4*torch.randn(*shape, generator=gen)}


def _layer_norm(tag, shape, fill, bf=False):
    C = shape[1]

    def operands(gen):
        o = dict(x=fill(shape, gen), w=torch.rand(C, generator=gen) + 0.5, b=torch.randn(C, generator=gen), g=_dyadic(shape, gen))
        if bf: o['g'] = o['g'].to(BF)
        return o

    def go(o, leaf, fn):
        x, w, b = leaf(o['x']), leaf(o['w']), leaf(o['b'])
        y = fn(x, w, b); y.backward(o['g'].to(y))
        return dict(y=y, g_x=x.grad, g_w=w.grad, g_b=b.grad)

    def run(F, o): return go(o, _leaf, lambda x, w, b: F.layer_norm_cf(x, w, b, 1e-6, out_dtype=BF if bf else F32))
    def ref(o, dtype): return go(o, _cast(dtype), lambda x, w, b: TF.layer_norm(x.permute(0, 2, 3, 1), (C,), w, b, 1e-6).permute(0, 3, 1, 2))
    case(f'layer_norm_cf{shape}_{tag}{"_bf16" if bf else ""}', 'layer_norm_cf', operands, run, ref, {'y': TOL_LN_BF16_OUT, '*': TOL_LN_BF16_GRAD} if bf else {'*': TOL_LN},
         split=dict(y=0, g_x=0))


for _shape in LN_SHAPES:
    for _tag, _fill in LN_VALUES.items(): _layer_norm(_tag, _shape, _fill)
_layer_norm('outlier_first', (2, 96, 6, 20), _ln_outlier(0), bf=True)


# ---- max_pool3x3s2 ----------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 3, 5, 8), (1, 2, 4, 4), (1, 1, 1, 1), (1, 2, 9, 7)]
_NEG_INF = float('-inf')


def _pool_neg_inf(shape, gen):
    N, C, H, W = shape
    x = torch.randn(*shape, generator=gen)
    x.flatten()[::3] = _NEG_INF
    x[:, :, :2, :2] = _NEG_INF                              # the corner window (2x2 valid taps, the rest padding) is all -inf
    if H >= 4 and W >= 4: x[:, :, 1:4, 1:4] = _NEG_INF      # ... and so is the interior window (1, 1)
    return x


def _pool_nan(shape, gen):
    N, C, H, W = shape
    x = torch.randn(*shape, generator=gen)
    x[0, 0, 0, W - 1] = float('nan')                        # on the border
    x[-1, -1, H//2, W//2] = float('nan')                    # in the interior (where the plane has one)
    return x


POOL_VALUES = {'all_negative': lambda shape, gen: -1 - torch.rand(*shape, generator=gen), 'constant': lambda shape, gen: torch.full(shape, -2.5),
               'neg_inf': _pool_neg_inf, 'nan': _pool_nan}


def _max_pool(tag, shape, fill):
    ho, wo = (shape[2] - 1)//2 + 1, (shape[3] - 1)//2 + 1

    def operands(gen):      # the incoming gradient: integers, so that the <= 4 windows that meet in one pixel add up exactly
        return dict(x=fill(shape, gen), g=torch.randint(-8, 9, (shape[0], shape[1], ho, wo), generator=gen).float())

    def go(o, leaf, fn):
        x = leaf(o['x'])
        y = fn(x); y.backward(o['g'].to(y))
        return dict(y=y, g_x=x.grad)

    def run(F, o): return go(o, _leaf, F.max_pool3x3s2)
    def ref(o, dtype): return go(o, _cast(dtype), lambda x: TF.max_pool2d(x, 3, 2, 1))
    case(f'max_pool3x3s2{shape}_{tag}', 'max_pool3x3s2', operands, run, ref, dict(y=EQUAL, g_x=EQUAL if tag == 'constant' else TOL_POOL_GX))


for _shape in POOL_SHAPES:
    for _tag, _fill in POOL_VALUES.items(): _max_pool(_tag, _shape, _fill)


# ---- dwconv7x7 --------------------------------------------------------------------------------------------------------------------------------------------
DW_SHAPES = [(1, 2, 3, 5), (1, 1, 1, 1), (9, 2, 7, 7), (2, 3, 9, 70)]      # the first two: smaller than the window


def dw_positions(H, W):
    """The four corners, the four edge midpoints and the centre."""
    return [(h, w) for h in (0, H//2, H - 1) for w in (0, W//2, W - 1)]


def _dw_exact(shape, gen):
    N, C, H, W = shape
    x = torch.zeros(*shape)
    pos = dw_positions(H, W)
    for k in range(max(N*C, len(pos))):      # one position per (sample, channel) pair while the pairs last, then further ones on top
        n, c = divmod(k % (N*C), C)
        x[n, c][pos[k % len(pos)]] = 1.0
    w = torch.arange(1, 50, dtype=F32).view(1, 1, 7, 7) + 64.0*torch.arange(C, dtype=F32).view(C, 1, 1, 1)
    return dict(x=x, w=w, b=torch.randint(-4, 5, (C,), generator=gen).float(), g=torch.randint(-8, 9, shape, generator=gen).float())


def _dw_dense(shape, gen):
    C = shape[1]
    return dict(x=torch.randn(*shape, generator=gen), w=torch.randn(C, 1, 7, 7, generator=gen)*0.2, b=torch.randn(C, generator=gen), g=torch.randn(*shape, generator=gen))


def _dwconv(tag, shape, fill, tol):
    def go(o, leaf, fn):
        x, w, b = leaf(o['x']), leaf(o['w']), leaf(o['b'])
        y = fn(x, w, b); y.backward(o['g'].to(y))
        return dict(y=y, g_x=x.grad, g_w=w.grad, g_b=b.grad)

    def run(F, o): return go(o, _leaf, F.dwconv7x7)
    def ref(o, dtype): return go(o, _cast(dtype), lambda x, w, b: TF.conv2d(x, w, b, padding=3, groups=shape[1]))
    case(f'dwconv7x7{shape}_{tag}', 'dwconv7x7', lambda gen: fill(shape, gen), run, ref, {'*': tol})


for _shape in DW_SHAPES: _dwconv('one_hot_exact', _shape, _dw_exact, EQUAL)
_dwconv('dense', (1, 2, 3, 5), _dw_dense, TOL_DWCONV)


# ---- elu_pad / elu_up_cat_pad -----------------------------------------------------------------------------------------------------------------------------
PRE_ACTIVATIONS = [0.0, -0.0, -1e-7, -1e-4, -1e-2, -20.0, -87.0, -90.0, -104.0, -1e4, 1e-7, 1e4]


def _glue_x(shape, bias, gen):
    """The list tiled over the tensor; with a bias, x = v - bias (so that x + bias is v up to one rounding) and every 13th element x = -bias: the sum is exactly 0."""
    n = torch.Size(shape).numel()
    x = torch.tensor(PRE_ACTIVATIONS)[torch.arange(n) % len(PRE_ACTIVATIONS)].view(shape)
    if bias is not None:
        bc = bias.view(1, -1, *[1]*(len(shape) - 2)).expand(shape)
        x = torch.where((torch.arange(n) % 13 == 12).view(shape), -bc, x - bc)
    return x


def _finite(out):
    for k, v in out.items(): assert v is None or bool(v.isfinite().all()), f'{k} is not finite'


def _elu_pad(shape, bias):
    B, C, h, w = shape

    def operands(gen):
        b = torch.randn(C, generator=gen) if bias else None
        o = dict(x=_glue_x(shape, b, gen), gy=_dyadic((B, C, h + 2, w + 2), gen))
        if bias: o['bias'] = b
        return o

    def go(o, leaf, fn):
        x, b = leaf(o['x']), (leaf(o['bias']) if bias else None)
        out = fn(x, b); out.backward(o['gy'].to(out))
        return dict(out=out, g_x=x.grad, g_bias=_g(b))

    def run(F, o): return go(o, _leaf, lambda x, b: F.elu_pad(x, b, True))
    def ref(o, dtype): return go(o, _cast(dtype), lambda x, b: TF.pad(TF.elu(x + b[None, :, None, None] if bias else x), (1, 1, 1, 1), mode='reflect'))
    case(f'elu_pad{shape}{"_bias" if bias else ""}', 'elu_pad', operands, run, ref, {'*': TOL_GLUE_BIAS} if bias else dict(out=TOL_GLUE_OUT, g_x=TOL_GLUE_GX), check=_finite)


def _elu_up_cat_pad(B, Ca, Cs, h, w, bias):
    def operands(gen):
        b = torch.randn(Ca, generator=gen) if bias else None
        o = dict(a=_glue_x((B, Ca, h, w), b, gen), skip=_glue_x((B, Cs, 2*h, 2*w), None, gen), gy=_dyadic((B, Ca + Cs, 2*h + 2, 2*w + 2), gen))
        if bias: o['bias'] = b
        return o

    def go(o, leaf, fn):
        a, s, b = leaf(o['a']), leaf(o['skip']), (leaf(o['bias']) if bias else None)
        out = fn(a, s, b); out.backward(o['gy'].to(out))
        return dict(out=out, g_a=a.grad, g_skip=s.grad, g_bias=_g(b))

    def run(F, o): return go(o, _leaf, lambda a, s, b: F.elu_up_cat_pad(a, s, bias=b))

    def ref(o, dtype):
        def f(a, s, b):
            up = TF.interpolate(TF.elu(a + b[None, :, None, None] if bias else a), scale_factor=2, mode='nearest')
            return TF.pad(torch.cat((up, s), 1), (1, 1, 1, 1), mode='reflect')
        return go(o, _cast(dtype), f)
    case(f'elu_up_cat_pad({B},{Ca},{Cs},{h},{w}){"_bias" if bias else ""}', 'elu_up_cat_pad', operands, run, ref,
         {'*': TOL_GLUE_BIAS} if bias else dict(out=TOL_GLUE_OUT, g_a=TOL_GLUE_GA, g_skip=TOL_GLUE_GX), check=_finite)


for _bias in (False, True):
    _elu_pad((2, 3, 7, 9), _bias); _elu_up_cat_pad(2, 5, 2, 6, 9, _bias)


# ---- conv3x3_head / conv3x3_headn ---------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, 5, 2, 2), (2, 32, 17, 129)]
HEAD_LEVELS = [0.0, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0]      # the pre-activations the sigmoid has to cover
# Per channel.  No level + bias cancels to 0 from further out than 0.5: the sum would carry the rounding of its large partial sums (half an ulp of 20 is 1e-6, 288 times) into
# the steepest part of the sigmoid, in any fp32 convolution.  The incoming gradient of the large shape is sparse (1 pixel in 16), so that the fp32 yardstick's
# sequential sum for the weight gradient has a few hundred terms, not 4386.
HEAD_BIAS = [0.25, -0.5, 45.0, -130.0]


def _head(B, C, h, w, n=None, bf=False):
    """Channel 0 of the padded input carries a map of HEAD_LEVELS that the centre tap of every output channel passes through unscaled; the other channels are
    Gaussians under weights scaled to a unit sum: pre-activation = level + N(0, ~1) + bias[channel].  n None: `conv3x3_head`, else `conv3x3_headn`."""
    co = n or 1

    def operands(gen):
        xp = torch.randn(B, C, h + 2, w + 2, generator=gen)
        k = torch.arange(B).view(B, 1, 1) + torch.arange(h + 2).view(1, h + 2, 1)*3 + torch.arange(w + 2).view(1, 1, w + 2)
        xp[:, 0] = torch.tensor(HEAD_LEVELS)[k % len(HEAD_LEVELS)]
        wt = torch.randn(co, C, 3, 3, generator=gen)/(3*C**0.5)
        wt[:, 0] = 0.0; wt[:, 0, 1, 1] = 1.0
        o = dict(xp=xp.to(BF) if bf else xp, w=wt, bias=torch.tensor(HEAD_BIAS[:co]), gy=torch.randn(B, co, h, w, generator=gen)*(torch.rand(B, co, h, w, generator=gen) < 1/16 if h*w > 64 else 1))
        return o

    def go(o, leaf, fn):
        xp, wt, b = leaf(o['xp']), leaf(o['w']), leaf(o['bias'])
        y = fn(xp, wt, b); y.backward(o['gy'].to(y))
        return dict(y=y, g_xp=xp.grad, g_w=wt.grad, g_bias=b.grad)

    def run(F, o): return go(o, _leaf, lambda xp, wt, b: (F.conv3x3_headn if n else F.conv3x3_head)(xp, wt, b, 'sigmoid'))
    def ref(o, dtype): return go(o, _cast(dtype), lambda xp, wt, b: torch.sigmoid(TF.conv2d(xp, wt, b)))

    def check(out):
        _finite(out)
        assert bool(((out['y'] >= 0) & (out['y'] <= 1)).all()), 'y leaves [0, 1]'
    nm = f'conv3x3_headn{n}' if n else 'conv3x3_head'
    case(f'{nm}({B},{C},{h},{w})_sigmoid_levels{"_bf16" if bf else ""}', 'conv3x3_headn' if n else 'conv3x3_head', operands, run, ref,
         {'*': TOL_CONV_F32, 'g_xp': TOL_BF16_OUT if bf else TOL_CONV_F32}, check=check)


for _dims in HEAD_SHAPES:
    for _n in (None, 1, 4): _head(*_dims, n=_n)
_head(2, 32, 17, 129, bf=True)


def head_pre_activation(o):
    """The pre-activation of a head case's operands in fp64 (the host test checks that it covers HEAD_LEVELS)."""
    return TF.conv2d(o['xp'].double(), o['w'].double(), o['bias'].double())


# =============================================================================================================================================================
# The operators merged after the first table.  None of them addresses memory by data: every value below is finite.
def _pattern(shape, mod=17):
    """A dyadic gradient that depends on nothing but the shape (eighths in [-1, 1]): a `check` can restate it."""
    return (((torch.arange(torch.Size(shape).numel()) * 7) % mod).float().view(shape) - mod//2)/8


# ---- channel_attention --------------------------------------------------------------------------------------------------------------------------------------
# (C, h, w): C below / at / above one 16-row tile and off every multiple of 4; 2 and 5 column tiles over the four waves (idle waves, a wave with two tiles);
# n = h w = 1, 12 (a multiple of 4, not of 8) and 35 (of neither)
CA_SHAPES = [(5, 1, 1), (5, 3, 4), (16, 3, 4), (20, 5, 7), (70, 1, 1), (70, 5, 7)]
CA_BATCH = 2


def _ca_one_hot(shape, gen):
    """Post-ReLU rows of norms 8, 32, 56, ...: channel c is (8 + 24 c) u_c with u_c a positive unit map.  Every row's minimum of A is its entry at channel 0,
    and the next entry is further than 104 above it (row 0: 8 (32 cos - 8) with cos >= 0.7; n = 1: 8 x 24), so exp(rowmin - A) is exactly 0 off the minimum
    in fp32 and below 1e-45 in fp64: P is one-hot, dE = P o (dP - rowsum) vanishes, g_x = g + P^T g."""
    C, h, w = shape
    v = torch.relu(torch.randn(CA_BATCH, C, h*w, generator=gen)) + 0.5
    v = v/v.norm(dim=-1, keepdim=True)*(8.0 + 24.0*torch.arange(C).view(1, C, 1))
    return dict(x=v.view(CA_BATCH, C, h, w), g=torch.randn(CA_BATCH, C, h, w, generator=gen))


def _ca_ties(shape, gen):
    """Small integers (A is exact in fp32).  Channels 2 and 3 are the same NEGATIVE multiple (-3) of the all-ones map and every other channel is non-negative:
    the rows of the other channels reach their minimum at both.  Channels 0 and 1 are identical and have the largest sum there is (2 and 1 alternating, the rest
    are 0 or 1): two equal columns in every row, and where the rows of channels 2 and 3 reach theirs.  (-3 against 2 and 1: out = x + P V of channels 2 and 3 is
    -3 + (2 or 1), not a cancellation to 0, which would leave the slice nothing to be relative to.)"""
    C, h, w = shape
    x = torch.randint(0, 2, (CA_BATCH, C, h, w), generator=gen).float()
    x[:, 0] = 2.0 - (torch.arange(h*w) % 2).float().view(h, w); x[:, 1] = x[:, 0]
    if C > 3: x[:, 2] = -3.0; x[:, 3] = -3.0
    return dict(x=x, g=_dyadic((CA_BATCH, C, h, w), gen))


def _ca_scales(shape, gen):
    """Rows at 1e-3, 1 and 30 by c % 3.  (30, not 1e3: A reaches 900 n, and the fp32 yardstick's own exp(rowmax - A) of a rounded A is what the rule measures against.)"""
    C, h, w = shape
    s = torch.tensor([1e-3, 1.0, 30.0])[torch.arange(C) % 3].view(1, C, 1, 1)
    return dict(x=s*torch.rand(CA_BATCH, C, h, w, generator=gen), g=torch.randn(CA_BATCH, C, h, w, generator=gen))


def _ca_sparse_grad(shape, gen):
    C, h, w = shape
    g = torch.zeros(CA_BATCH, C, h, w)
    g[:, C//2] = _dyadic((CA_BATCH, h, w), gen)
    return dict(x=torch.relu(torch.randn(CA_BATCH, C, h, w, generator=gen)) + 0.25*torch.rand(CA_BATCH, C, h, w, generator=gen), g=g)      # ('peaked' of test_gpu_cadepth.py)


CA_VALUES = {'zero': lambda shape, gen: dict(x=torch.zeros(CA_BATCH, *shape), g=_pattern((CA_BATCH, *shape))), 'one_hot': _ca_one_hot, 'ties': _ca_ties,
             'rows_1e-3_1_30': _ca_scales, 'one_channel_grad': _ca_sparse_grad}


def attention_matrix(o):
    """A = V V^T of a `channel_attention` case in fp64."""
    v = o['x'].double().flatten(2)
    return v @ v.transpose(1, 2)


def _channel_attention(tag, shape, fill):
    def go(o, leaf, fn):
        x = leaf(o['x'])
        out = fn(x); out.backward(o['g'].to(out))
        return dict(out=out, g_x=x.grad)

    def check(out):
        _finite(out)
        if tag != 'zero': return
        g = _pattern((CA_BATCH, *shape)).double()      # P is uniform and V = 0: out = x, g_x = g + P^T g = g + mean_c g
        assert bool((out['out'] == 0).all()), 'x = 0: out = x'
        assert rel_to_max(out['g_x'].double().cpu(), g + g.mean(1, keepdim=True)) <= FLOOR, 'x = 0: g_x = g + mean_c(g)'
    case(f'channel_attention{shape}_{tag}', 'channel_attention', lambda gen: fill(shape, gen), lambda F, o: go(o, _leaf, F.channel_attention),
         lambda o, dtype: go(o, _cast(dtype), sp_aten), {'*': TOL_YARD}, split=dict(out=1, g_x=1), check=check)


for _shape in CA_SHAPES:
    for _tag, _fill in CA_VALUES.items(): _channel_attention(_tag, _shape, _fill)


# ---- se_gate ------------------------------------------------------------------------------------------------------------------------------------------------
SE_VALUE_SHAPES = [(3, 5, 2, 2), (2, 12, 5, 7)]      # SE_SHAPES[:2] of test_gpu_cadepth.py: HW % 4 == 0 and not
GATE_LEVELS = [-200.0, -90.0, -20.0, 0.0, 20.0, 90.0, 200.0]      # the gate's pre-activation, by 3 c % 7: with five channels -200, 0, 200, -20, 90


def gate_levels(C): return torch.tensor(GATE_LEVELS)[(3*torch.arange(C)) % 7]


def _se_base(shape, gen):
    C = shape[1]
    return dict(x=torch.relu(torch.randn(shape, generator=gen)), w1=torch.randn(C, C, generator=gen)/C**0.5, b1=0.1*torch.randn(C, generator=gen),
                w2=torch.randn(C, C, generator=gen)/C**0.5, b2=0.1*torch.randn(C, generator=gen), g=_dyadic(shape, gen))


def _se_saturated(shape, gen):
    """b2 = gate_levels(C) under a small w2, x in eighths: only the channels at level 0 carry the parameter gradients, and with a dyadic g their plane sums of
    g x are exact (in Gaussians they cancel to a few ulp of their largest term, in ATen's fp32 as well, and that error would be the whole of g_w2).  The channels whose gate is shut at -200 also receive a gradient 64 times smaller, as they would from a
    consumer behind the shut gate: a small-scale slice of g_x that only the per-channel judge sees."""
    o, C = _se_base(shape, gen), shape[1]
    o['x'] = torch.relu(_dyadic(shape, gen))
    o['w2'] = 0.01*o['w2']; o['b2'] = gate_levels(C)
    o['g'][:, o['b2'] == GATE_LEVELS[0]] /= 64
    return o


def _se_means(shape, gen):
    """Channel 0 at 1e4, channel 1 at 1e-4, and the columns of w1 that read them scaled the other way: the hidden layer sees both at unit scale.  (With w1 left
    alone the pre-activation is 1e4 w: half an ulp of the fp32 mean moves it by 1e-3, which no fp32 evaluation of the gate holds to FLOOR.)"""
    o = _se_base(shape, gen)
    o['x'][:, 0] = 1e4*(1 + 0.125*torch.rand(shape[0], *shape[2:], generator=gen)); o['x'][:, 1] *= 1e-4
    o['w1'][:, 0] *= 1e-4; o['w1'][:, 1] *= 1e4
    return o


SE_VALUES = {'b2_levels': _se_saturated, 'dead_hidden': lambda shape, gen: dict(_se_base(shape, gen), b1=torch.full((shape[1],), -50.0)),
             'zero': lambda shape, gen: dict(_se_base(shape, gen), x=torch.zeros(shape)), 'means_1e4_1e-4': _se_means}
SE_NAMES = ('x', 'w1', 'b1', 'w2', 'b2')


def se_pre_activations(o):
    """-> (hidden, z) of an `se_gate` case in fp64: hidden = relu(W1 mean + b1), z = W2 hidden + b2."""
    x, w1, b1, w2, b2 = (o[n].double() for n in SE_NAMES)
    hidden = torch.relu(x.mean((2, 3)) @ w1.T + b1)
    return hidden, hidden @ w2.T + b2


def _se_gate(tag, shape, fill):
    def go(o, leaf, fn):
        ins = [leaf(o[n]) for n in SE_NAMES]
        out = fn(*ins); out.backward(o['g'].to(out))
        return dict(out=out, **{f'g_{n}': t.grad for n, t in zip(SE_NAMES, ins)})
    case(f'se_gate{shape}_{tag}', 'se_gate', lambda gen: fill(shape, gen), lambda F, o: go(o, _leaf, F.se_gate), lambda o, dtype: go(o, _cast(dtype), se_aten),
         {'*': TOL_SE}, split=dict(out=1, g_x=1), check=_finite)


for _shape in SE_VALUE_SHAPES:
    for _tag, _fill in SE_VALUES.items(): _se_gate(_tag, _shape, _fill)


# ---- up_cat_gate_pad ----------------------------------------------------------------------------------------------------------------------------------------
# (B, Ca, Cs, h, w, R, bias and 'relu'): FUSE_CASES[0] and [1] of the DiffNet fixture — `a` planes of 15 elements beside `skip` planes of 60, and 24 beside 96
UCG_SHAPES = [(2, 16, 16, 3, 5, 2, True), (1, 40, 24, 4, 6, 4, False)]


def _ucg_base(shape, gen):
    B, Ca, Cs, h, w, R, bias = shape
    C = Ca + Cs
    o = dict(a=torch.randn(B, Ca, h, w, generator=gen) + torch.randn(1, Ca, 1, 1, generator=gen), skip=torch.rand(B, Cs, 2*h, 2*w, generator=gen) + torch.rand(1, Cs, 1, 1, generator=gen),
             w1=torch.randn(R, C, generator=gen)/C**0.5, w2=torch.randn(C, R, generator=gen)/R**0.5, gy=_dyadic((B, C, 2*h + 2, 2*w + 2), gen))
    if bias: o['bias'] = 0.5*torch.randn(Ca, generator=gen)
    return o


def _ucg_saturated(shape, gen):
    """No b2 here: the last skip channel is the constant 1 (its mean is exactly 1), hidden unit 0 reads that channel alone (hidden_0 = 1), and
    w2[:, 0] = gate_levels(C); the other hidden units keep a small w2.  Hidden unit 1 is kept ALIVE (w1[1] >= 0 with 4 on the constant channel): the channels at
    level 0 have w2[:, 0] = 0, so through unit 0 alone g_w1 and the shut channels' g_skip would consist of the saturated channels' exp(-|z|) terms only, which
    ATen's fp32 a (1 - a) misses by many times their size; through unit 1 they stand beside the live channels' terms, as they do in a trained gate."""
    o, C = _ucg_base(shape, gen), shape[1] + shape[2]
    o['skip'][:, -1] = 1.0
    o['w1'][0] = 0.0; o['w1'][0, -1] = 1.0
    o['w1'][1] = o['w1'][1].abs(); o['w1'][1, -1] += 4.0
    o['w2'] *= 0.01; o['w2'][:, 0] = gate_levels(C)
    return o


def _ucg_dead(shape, gen):
    """Non-negative channel means under w1 <= 0: every hidden unit is dead and the gate is exactly 0.5.  (`a` is made positive: without 'relu' its means could be negative.)"""
    o = _ucg_base(shape, gen)
    o['a'] = o['a'].abs() + 0.25
    if 'bias' in o: o['bias'] = o['bias'].abs()
    o['w1'] = -o['w1'].abs()
    return o


def _ucg_zero(shape, gen):
    o = _ucg_base(shape, gen)
    o['a'], o['skip'] = torch.zeros_like(o['a']), torch.zeros_like(o['skip'])
    if 'bias' in o: o['bias'] = torch.zeros_like(o['bias'])
    return o


def _ucg_means(shape, gen):
    """As `_se_means`: skip channel 0 at 1e4 and 1 at 1e-4, w1's columns the other way."""
    o, Ca = _ucg_base(shape, gen), shape[1]
    o['skip'][:, 0] = 1e4*(1 + 0.125*torch.rand_like(o['skip'][:, 0])); o['skip'][:, 1] *= 1e-4
    o['w1'][:, Ca] *= 1e-4; o['w1'][:, Ca + 1] *= 1e4
    return o


UCG_VALUES = {'w2_levels': _ucg_saturated, 'dead_hidden': _ucg_dead, 'zero': _ucg_zero, 'means_1e4_1e-4': _ucg_means}


def ucg_pre_activations(o, act):
    """-> (hidden, z) of an `up_cat_gate_pad` case in fp64."""
    x = o['a'].double() + (o['bias'].double().view(1, -1, 1, 1) if 'bias' in o else 0)
    mean = torch.cat(((TF.relu(x) if act else x).mean((2, 3)), o['skip'].double().mean((2, 3))), 1)
    hidden = torch.relu(mean @ o['w1'].double().T)
    return hidden, hidden @ o['w2'].double().T


def _up_cat_gate_pad(tag, shape, fill):
    bias = shape[6]
    act = 'relu' if bias else None

    def go(o, leaf, fn):
        a, b, s, w1, w2 = leaf(o['a']), (leaf(o['bias']) if bias else None), leaf(o['skip']), leaf(o['w1']), leaf(o['w2'])
        out = fn(a, b, s, w1, w2); out.backward(o['gy'].to(out))
        return dict(out=out, g_a=a.grad, g_bias=_g(b), g_skip=s.grad, g_w1=w1.grad, g_w2=w2.grad)
    case(f'up_cat_gate_pad{shape[:6]}_{tag}{"_bias_relu" if bias else ""}', 'up_cat_gate_pad', lambda gen: fill(shape, gen),
         lambda F, o: go(o, _leaf, lambda a, b, s, w1, w2: F.up_cat_gate_pad(a, s, w1, w2, b, act)), lambda o, dtype: go(o, _cast(dtype), lambda a, b, s, w1, w2: fuse_aten(a, b, s, w1, w2, act)),
         {'*': TOL_YARD}, split=dict(out=1, g_a=1, g_skip=1), check=_finite)


for _shape in UCG_SHAPES:
    for _tag, _fill in UCG_VALUES.items(): _up_cat_gate_pad(_tag, _shape, _fill)


# ---- relu_pad -----------------------------------------------------------------------------------------------------------------------------------------------
def _relu_pad(shape, bias):
    B, C, h, w = shape

    def operands(gen):
        b = torch.randn(C, generator=gen) if bias else None
        o = dict(x=_glue_x(shape, b, gen), gy=_dyadic((B, C, h + 2, w + 2), gen))
        if bias: o['bias'] = b
        return o

    def go(o, leaf, fn):
        x, b = leaf(o['x']), (leaf(o['bias']) if bias else None)
        out = fn(x, b); out.backward(o['gy'].to(out))
        return dict(out=out, g_x=x.grad, g_bias=_g(b))
    case(f'relu_pad{shape}{"_bias" if bias else ""}', 'relu_pad', operands, lambda F, o: go(o, _leaf, F.relu_pad), lambda o, dtype: go(o, _cast(dtype), relu_pad_aten),
         {'*': TOL_YARD}, check=_finite)


for _bias in (False, True):
    _relu_pad((2, 3, 7, 9), _bias); _relu_pad((1, 2, 5, 7), _bias)


# ---- ddv_head -----------------------------------------------------------------------------------------------------------------------------------------------
DDV_C = 16
# (B, G, h, w): one pixel; a second pixel fragment partly outside the image; a second 64-column tile of one column, two groups
DDV_SHAPES = [(1, 1, 1, 1), (2, 1, 5, 33), (1, 2, 5, 33), (1, 2, 4, 65)]
DDV_MARGIN = 120.0
DDV_DOMINANT = (0, 1, 63, 64, 127)
DDV_TIE = (3, 4)      # registers r & 3 of one half-wave and + 4 g of the other (the layout comment of k_ddv_head)


def ddv_bin(k, g):
    """The bin of group g that a case names by its bin k of group 0 (mirrored in the second group, so that both ends of the layout are hit in one case)."""
    return k if g == 0 else NUM_BINS - 1 - k


def _ddv_base(shape, gen):
    """Channel 0 of the padded input is 1 everywhere: the centre tap of a bin's weight on that channel adds itself to the bin's logit at every pixel.  The other
    channels are Gaussians under weights scaled to a unit sum: logit = centre tap + N(0, ~1) + bias."""
    B, G, h, w = shape
    xp = torch.randn(B, DDV_C, h + 2, w + 2, generator=gen)
    xp[:, 0] = 1.0
    wt = torch.randn(NUM_BINS*G, DDV_C, 3, 3, generator=gen)/(3*DDV_C**0.5)
    wt[:, 0] = 0.0
    return dict(xp=xp, w=wt, bias=0.1*torch.randn(NUM_BINS*G, generator=gen), gy=torch.randn(B, G, h, w, generator=gen))


def _ddv_peaks(bins_of_group0):
    def fill(shape, gen):
        o = _ddv_base(shape, gen)
        for g in range(shape[1]):
            rows = [g*NUM_BINS + ddv_bin(k, g) for k in bins_of_group0]
            o['w'][rows] = 0.0; o['bias'][rows] = 0.0      # (the peaks carry no noise: two of them tie exactly)
            o['w'][rows[0], 0, 1, 1] = DDV_MARGIN
            # the second peak of a tie stands in the bias: with both in the weights g_xp would be 120 (g_logit_3 + g_logit_4), an exact cancellation whose
            # rounding residue has nothing to be relative to
            for r in rows[1:]: o['bias'][r] = DDV_MARGIN
        return o
    return fill


def _ddv_zero(shape, gen):
    o = _ddv_base(shape, gen)
    return dict(o, w=torch.zeros_like(o['w']), bias=torch.zeros_like(o['bias']))


def _ddv_alternating(shape, gen):
    o = _ddv_base(shape, gen)
    o['bias'] = o['bias'] + 200.0*(1 - 2.0*(torch.arange(o['bias'].numel()) % 2))
    return o


DDV_VALUES = {**{f'dominant_bin{k}': _ddv_peaks((k,)) for k in DDV_DOMINANT}, 'zero_logits': _ddv_zero, f'tie_bins{DDV_TIE[0]}_{DDV_TIE[1]}': _ddv_peaks(DDV_TIE),
              'bias_pm200': _ddv_alternating}


def ddv_logits(o):
    """The logits of a `ddv_head` case in fp64, (B, G, 128, h, w)."""
    l = TF.conv2d(o['xp'].double(), o['w'].double(), o['bias'].double())
    return l.view(l.shape[0], -1, NUM_BINS, *l.shape[2:])


def _ddv_head(tag, shape, fill):
    B, G, h, w = shape

    def go(o, leaf, fn):
        xp, wt, b = leaf(o['xp']), leaf(o['w']), leaf(o['bias'])
        y = fn(xp, wt, b); y.backward(o['gy'].to(y))
        return dict(y=y, g_xp=xp.grad, g_w=wt.grad, g_bias=b.grad)

    def run(F, o):
        F.set_conv_route('mfma')      # as test_ddv_head_matches_fp64 pins it: an A/B on first use could hand the gradient GEMMs to a library whose sums are not reproducible
        try: return go(o, _leaf, lambda xp, wt, b: F.ddv_head(xp, wt, b, G))
        finally: F.set_conv_route('auto')

    def check(out):
        _finite(out)
        assert bool(((out['y'] >= 0) & (out['y'] <= (NUM_BINS - 1)/NUM_BINS)).all()), 'disp leaves [0, 127/128]'
        if tag == 'zero_logits': assert bool((out['y'] == 63.5/NUM_BINS).all()), 'all-equal logits: disp = 63.5/128 exactly'
    case(f'ddv_head{shape}_{tag}', 'ddv_head', lambda gen: fill(shape, gen), run, lambda o, dtype: go(o, _cast(dtype), lambda xp, wt, b: ddv_aten(xp, wt, b, G)),
         {'*': TOL_YARD}, split=dict(g_w=(0, NUM_BINS), g_bias=(0, NUM_BINS)), check=check)


for _shape in DDV_SHAPES:
    for _tag, _fill in DDV_VALUES.items(): _ddv_head(_tag, _shape, _fill)


# ---- subpixel_conv ------------------------------------------------------------------------------------------------------------------------------------------
SUBPIXEL_VALUE_CASES = (0, 1, 2, 7)      # of SUBPIXEL_CASES, the shapes only: pad + skip, one pixel, r = 4 without pad, the sigmoid behind a pad
SUBPIXEL_OPS = ('x', 'pre_bias', 'weight', 'bias', 'skip')


def _sp_base(k, gen):
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]
    o = dict(x=torch.randn(B, C, h, w, generator=gen), pre_bias=0.5*torch.randn(C, generator=gen), weight=torch.randn(C*r*r, 1, 3, 3, generator=gen)/3.0,
             bias=0.5*torch.randn(C*r*r, generator=gen), gy=_dyadic((B, C + Cs, r*h + 2, r*w + 2) if pad else (B, C, r*h, r*w), gen))
    if Cs: o['skip'] = torch.randn(B, Cs, r*h, r*w, generator=gen)
    return o


def _sp_pre(k, gen):
    """x + pre_bias runs through PRE_ACTIVATIONS (and is exactly 0 at every 13th element): `_glue_x`.  The weights are scaled down by the 1e4 the list reaches."""
    o = _sp_base(k, gen)
    o['x'] = _glue_x(o['x'].shape, o['pre_bias'], gen)
    return o


def _sp_levels(k, gen):
    """The output's pre-activation v runs through HEAD_LEVELS: x > 0 passes ELU unchanged, the centre tap is 1 and the other taps 0, so v = level + bias with
    a small bias; as `_head` builds them.  x + pre_bias = 256 + level is exact in fp32 for a pre_bias in eighths."""
    o = _sp_base(k, gen)
    n = o['x'].numel()
    o['pre_bias'] = torch.randint(-8, 9, o['pre_bias'].shape, generator=gen).float()/8
    o['x'] = 256.0 + torch.tensor(HEAD_LEVELS)[torch.arange(n) % len(HEAD_LEVELS)].view(o['x'].shape) - o['pre_bias'].view(1, -1, 1, 1)
    o['weight'] = torch.zeros_like(o['weight']); o['weight'][:, 0, 1, 1] = 1.0
    o['bias'] = -256.0 + torch.randint(-4, 5, o['bias'].shape, generator=gen).float()/8
    return o


def _sp_relu_zero(k, gen):
    """Integer operands whose sum cancels: x + pre_bias = 2 everywhere (ELU passes it), weights in {-1, 0, 1} with nine taps, bias = -2 sum(w) in the interior,
    so v is exactly 0 on every interior pixel in any precision and relu'(0) = 0 there; the border pixels see fewer taps and stay live."""
    o = _sp_base(k, gen)
    o['pre_bias'] = torch.randint(-2, 3, o['pre_bias'].shape, generator=gen).float()
    o['x'] = 2.0 - o['pre_bias'].view(1, -1, 1, 1).expand_as(o['x']).clone()
    o['weight'] = torch.randint(-1, 2, o['weight'].shape, generator=gen).float()
    o['bias'] = -2.0*o['weight'].sum((1, 2, 3))
    return o


def subpixel_pre_activations(k, o):
    """-> (u, v) in fp64: u = x + pre_bias in front of the ELU, v the convolution's output in front of `act`."""
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]
    u = o['x'].double() + o['pre_bias'].double().view(1, -1, 1, 1)
    return u, TF.conv2d(TF.elu(u), o['weight'].double(), o['bias'].double(), padding=1, groups=C)


def _subpixel(tag, k, fill):
    B, C, Cs, h, w, r, pre, act, pad = SUBPIXEL_CASES[k]
    assert pre == 'elu'

    def go(o, leaf, fn):
        L = {n: (leaf(o[n]) if n in o else None) for n in SUBPIXEL_OPS}
        out = fn(L); out.backward(o['gy'].to(out))
        return dict(out=out, **{f'g_{n}': _g(L[n]) for n in SUBPIXEL_OPS})

    def run(F, o): return go(o, _leaf, lambda L: F.subpixel_conv(L['x'], L['weight'], L['bias'], r, pre_bias=L['pre_bias'], pre_act=pre, act=act, skip=L['skip'], pad=pad))
    def ref(o, dtype): return go(o, _cast(dtype), lambda L: subpixel_aten(L['x'], L['pre_bias'], L['weight'], L['bias'], L['skip'], r, pre, act, pad))
    case(f'subpixel_conv{SUBPIXEL_CASES[k]}_{tag}', 'subpixel_conv', lambda gen: fill(k, gen), run, ref, {'*': TOL_YARD}, check=_finite)


for _k in SUBPIXEL_VALUE_CASES:
    _subpixel('pre_activations', _k, _sp_pre); _subpixel('levels', _k, _sp_levels)
    if SUBPIXEL_CASES[_k][7] == 'relu': _subpixel('relu_zero', _k, _sp_relu_zero)


# ---- flip_blend / flip_blend_pyramid ------------------------------------------------------------------------------------------------------------------------
BLEND_WIDTHS = (2, 3, 21, 64)      # the ramp all 0 / 1; one interior column that mirrors onto itself; x_1 = 0.05 exactly, the clamp's edge; whole 16-byte groups
BLEND_LEAD = (2, 2, 3)             # (b, c, h)
BLEND_DEPTHS = dict(min_depth=0.1, max_depth=100)
BLEND_EDGE_VALUES = [0.0, 2.0**-24, 1 - 2.0**-24, 1.0]


def _blend_equal(shape, gen, scaled):
    """l == r, powers of two from 1/4 (under the depth range: 1/2) to 1.  `blend_bound` counts eight roundings and a quarter of it leaves ATen's fp32 two: with one-bit operands the three
    products with the 24-bit ramp are exact, and what rounds is the ramp's own 1 - m_l - m_r and the two sums.  (Under the depth range the offset 1/max is added,
    whose rounding the bound does not count: the operands stay large against it.)"""
    l = 2.0**-torch.randint(0, 2 if scaled else 3, shape, generator=gen).float()
    return l, l.clone()


def _blend_zero_one(shape, gen, scaled):
    k = (torch.arange(shape[0]*shape[1]).view(shape[0], shape[1], 1, 1) % 2).float().expand(shape)      # l = 0, r = 1 on even planes, the reverse on odd ones
    return k.clone(), (1 - k).clone()


def _blend_edges(shape, gen, scaled):
    """Every pair of BLEND_EDGE_VALUES.  Under the depth range a pair of two small values becomes (small, 1): the bound is 8 eps k max(|l|, |r|) and the scaled
    output carries the rounding of the offset 1/max = 0.01 whatever the operands are, which no fp32 evaluation holds to a bound of 1e-13."""
    n = torch.Size(shape).numel()
    v = torch.tensor(BLEND_EDGE_VALUES)
    l, r = v[torch.arange(n) % 4].view(shape), v[(torch.arange(n)//4) % 4].view(shape)
    if scaled: r = torch.where(torch.maximum(l, r) < 0.5, torch.ones_like(r), r)
    return l.clone(), r.clone()


BLEND_VALUES = {'l_equals_r': _blend_equal, 'zero_one': _blend_zero_one, 'edge_values': _blend_edges}


def _blend_operands(shape, fill, scaled, mirror, gen):
    """l, r_raw (what the operator takes: the right prediction un-flipped when `mirror`) and a dyadic gradient."""
    l, r = fill(shape, gen, scaled)      # r: already flipped back
    return dict(l=l, r_raw=r.flip(-1).contiguous() if mirror else r, g=_dyadic(shape, gen))


def _blend_tol(scaled, mirror, key=''):
    ks = scale_of() if scaled else 1.0
    back = (lambda t: t.flip(-1)) if mirror else (lambda t: t)
    return {f'out{key}': ('elem', lambda o: blend_bound(o[f'l{key}'], back(o[f'r_raw{key}']), ks)), f'g_l{key}': ('elem', lambda o: blend_bound(o[f'g{key}'], o[f'g{key}'], ks)),
            f'g_r_raw{key}': ('elem', lambda o: blend_bound(back(o[f'g{key}']), back(o[f'g{key}']), ks))}


def _flip_blend(tag, w, fill, scaled, mirror):
    shape = (*BLEND_LEAD, w)
    kw = dict(BLEND_DEPTHS if scaled else {}, mirror=mirror)

    def go(o, leaf, fn):
        l, r = leaf(o['l']), leaf(o['r_raw'])
        out = fn(l, r, **kw); out.backward(o['g'].to(out))
        return dict(out=out, g_l=l.grad, g_r_raw=r.grad)

    def ref(o, dtype):
        from slowtv_monodepth_amd.blend import plain_flip_blend
        return go(o, _cast(dtype), plain_flip_blend)
    case(f'flip_blend{shape}_{tag}{"_scaled" if scaled else ""}{"_mirror" if mirror else ""}', 'flip_blend', lambda gen: _blend_operands(shape, fill, scaled, mirror, gen),
         lambda F, o: go(o, _leaf, F.flip_blend), ref, _blend_tol(scaled, mirror), check=_finite)


for _i, _w in enumerate(BLEND_WIDTHS):
    for _j, (_tag, _fill) in enumerate(BLEND_VALUES.items()):
        for _scaled in ((False, True) if _w in (3, 64) else ((_i + _j) % 2 == 1,)): _flip_blend(_tag, _w, _fill, _scaled, mirror=(_i + _j + _scaled) % 2 == 0)


def _flip_blend_pyramid():
    """Three levels in one launch, one value generator each, under the depth range."""
    shapes = [(2, 1, 6, 24), (2, 1, 3, 12), (2, 1, 2, 3)]
    fills = list(BLEND_VALUES.values())

    def operands(gen):
        o = {}
        for s, (shape, fill) in enumerate(zip(shapes, fills)): o.update({f'{n}_{s}': t for n, t in _blend_operands(shape, fill, True, True, gen).items()})
        return o

    def go(o, leaf, fn):
        ls, rs = {s: leaf(o[f'l_{s}']) for s in range(3)}, {s: leaf(o[f'r_raw_{s}']) for s in range(3)}
        out = fn(ls, rs)
        torch.autograd.backward([out[s] for s in range(3)], [o[f'g_{s}'].to(out[s]) for s in range(3)])
        return {**{f'out_{s}': out[s] for s in range(3)}, **{f'g_l_{s}': ls[s].grad for s in range(3)}, **{f'g_r_raw_{s}': rs[s].grad for s in range(3)}}

    def ref(o, dtype):
        from slowtv_monodepth_amd.blend import plain_flip_blend
        return go(o, _cast(dtype), lambda ls, rs: {s: plain_flip_blend(ls[s], rs[s], **BLEND_DEPTHS) for s in ls})
    tol = {}
    for s in range(3): tol.update(_blend_tol(True, True, f'_{s}'))
    case('flip_blend_pyramid_3_levels_scaled_mirror', 'flip_blend_pyramid', operands, lambda F, o: go(o, _leaf, lambda ls, rs: F.flip_blend_pyramid(ls, rs, **BLEND_DEPTHS)), ref, tol, check=_finite)


_flip_blend_pyramid()


# ---- feat_regs ----------------------------------------------------------------------------------------------------------------------------------------------
FEAT_SHAPES = [(2, 3, 7, 67), (1, 2, 4, 6)]      # '7x67' (with 3 channels) and 'const' of the fixture's shape list
FEAT_IMG_STEP = 400.0                            # exp(-400) underflows in fp32 (and exp(-400/3) in a kernel that keeps the channel sum)


def _img(shape, gen): return torch.rand(shape[0], 3, *shape[2:], generator=gen)


def _feat_plateaus(shape, gen):
    """relu(randn - 1): about 84 % exact zeros, in patches that touch live pixels on every side; the last row and the last column are plateaus too."""
    f = torch.relu(torch.randn(shape, generator=gen) - 1)
    f[..., -1, :] = 0.0; f[..., :, -1] = 0.0
    return dict(feat=f, img=_img(shape, gen))


def _feat_eighths(shape, gen):
    """Eighths in [0, 0.5]: five levels, so neighbouring first-order differences tie exactly all over the interior (second-order sign(0))."""
    return dict(feat=torch.randint(0, 5, shape, generator=gen).float()/8, img=_img(shape, gen))


def _feat_const_img(shape, gen):
    img = torch.empty(shape[0], 3, *shape[2:])
    img[:] = torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1)
    return dict(feat=torch.randn(shape, generator=gen), img=img)


def _feat_checker_img(shape, gen):
    """0 / 400 per pixel on the left half of the image, uniform noise on the right: every first-order image difference on the left is 400 (weight exp(-400) = 0
    in fp32, 1e-174 in fp64) and every interior second-order one 0 (weight exactly 1).  The right half keeps the losses at their usual scale, which is what the
    bound is relative to."""
    B, _, h, w = shape
    img = _img(shape, gen)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    left = (xx < (w + 1)//2).expand(B, 3, h, w)
    return dict(feat=torch.randn(shape, generator=gen), img=torch.where(left, FEAT_IMG_STEP*((yy + xx) % 2).float().expand(B, 3, h, w), img))


FEAT_VALUES = {'plateaus': _feat_plateaus, 'eighths': _feat_eighths, 'constant_image': _feat_const_img, 'checker_image': _feat_checker_img}


def _feat_regs(name, fills, flags, unit_weights=False):
    """`fills`: one (shape, generator) per pyramid level; outputs: both losses and, per level, the gradient of FEAT_WEIGHTS[0] l_peaky + FEAT_WEIGHTS[1] l_smooth.
    `unit_weights`: the image is constant, every edge weight is exp(-0) = 1 exactly: the losses without the edge terms are outputs too, and have to be the same bits."""
    S = len(fills)

    def operands(gen):
        o = {}
        for s, (shape, fill) in enumerate(fills): o.update({f'{n}_{s}': t for n, t in fill(shape, gen).items()})
        return o

    def go(o, leaf, fn):
        feats, imgs = [leaf(o[f'feat_{s}']) for s in range(S)], [o[f'img_{s}'].detach().to(dtype=leaf(o['img_0']).dtype) for s in range(S)]
        lp, ls = fn(feats, imgs, flags)
        (FEAT_WEIGHTS[0]*lp + FEAT_WEIGHTS[1]*ls).backward()
        out = dict(l_peaky=lp, l_smooth=ls, **{f'g_feat_{s}': feats[s].grad for s in range(S)})
        if unit_weights: out['l_peaky_no_edges'], out['l_smooth_no_edges'] = (l.detach() for l in fn([f.detach() for f in feats], imgs, (False, False)))
        return out

    def run(F, o):
        from slowtv_monodepth_amd.featreg import feat_regs, feat_regs_pyramid
        return go(o, _leaf, (lambda f, i, fl: feat_regs(f[0], i[0], *fl)) if S == 1 else (lambda f, i, fl: feat_regs_pyramid(f, i, *fl)))

    def ref(o, dtype):
        from slowtv_monodepth_amd.featreg import plain_feat_regs
        return go(o, _cast(dtype), lambda f, i, fl: plain_feat_regs(f, i, *fl))

    def check(out):
        _finite(out)
        if unit_weights: assert torch.equal(out['l_peaky'], out['l_peaky_no_edges']) and torch.equal(out['l_smooth'], out['l_smooth_no_edges']), 'a constant image: every weight is exactly 1'
    case(name, 'feat_regs', operands, run, ref, {'*': TOL_FEATREG}, check=check)


for _shape in FEAT_SHAPES:
    for _tag, _fill in FEAT_VALUES.items():
        for _flags in ([(False, False), (False, True), (True, False), (True, True)] if _tag == 'plateaus' else [(True, True)]):
            _feat_regs(f'feat_regs{_shape}_{_tag}_edges{int(_flags[0])}{int(_flags[1])}', [(_shape, _fill)], _flags, unit_weights=_tag == 'constant_image')


def _feat_scaled(scale): return lambda shape, gen: dict(feat=scale*torch.randn(shape, generator=gen), img=_img(shape, gen))


# two levels of one pyramid at 1e-4 and 1e4: each level's gradient is an output of its own, so the small one is judged at its own scale
_feat_regs('feat_regs_pyramid_levels_1e-4_1e4', [((2, 3, 8, 12), _feat_scaled(1e-4)), ((2, 4, 4, 6), _feat_scaled(1e4))], (True, True))
