"""Value-edge cases for the encoder / decoder operators (`batch_norm_act`, `layer_norm_cf`, `max_pool3x3s2`, `dwconv7x7`, `elu_pad`, `elu_up_cat_pad`,
`conv3x3_head`, `conv3x3_headn`): the table and the judge.  Device-agnostic; test_value_edges_host.py checks the table on the CPU, test_gpu_value_edges.py runs it.

The suite's other families sweep shapes, memory and gradient subsets on Gaussian or uniform data.  Here the VALUES are the edge: one element far off a channel's
mean (at the first position, and at the last as a control), mean >> sigma, zero variance, scales that differ by 1e6 between channels, -inf / NaN / full ties in
the pool, pre-activations from 1e-7 to 1e4 through ELU and the sigmoid, one-hot images smaller than the 7x7 window on exact integer operands.

No tolerance is introduced: every output is held to the named bound of the operator's own parity test (test_gpu_hostile_memory.py lists them).  Two
refinements keep a large-scale part of a tensor from hiding a small-scale part: BatchNorm tensors shaped like `x` are judged per channel and LayerNorm
tensors per sample (`split`), each slice relative to its own maximum.  No element is left out of any comparison; where the reference is not finite (the
pool's -inf and NaN cases) the pattern has to be identical.

Case: name; op; operands(gen) -> {name: CPU tensor}; run(F, ops) -> {name: tensor} (outputs and all gradients, on the operands' device);
ref(ops, dtype) -> the same operation on plain ATen on the CPU in `dtype` (float64: the reference; float32: the yardstick of the host test);
tol: {name: bound, '*': default}; split: {name: dim} (slices judged one by one); check: None or f(out) with the case's extra assertions."""
from collections import namedtuple

import torch
import torch.nn.functional as TF

from conftest import rel_to_max
from test_gpu_hostile_memory import (EQUAL, TOL_BF16_OUT, TOL_BN, TOL_CONV_F32, TOL_DWCONV, TOL_GLUE_BIAS, TOL_GLUE_GA, TOL_GLUE_GX, TOL_GLUE_OUT, TOL_LN,
                                     TOL_LN_BF16_GRAD, TOL_LN_BF16_OUT, TOL_POOL_GX)

BF = torch.bfloat16
F64, F32 = torch.float64, torch.float32
OPERATORS = ('batch_norm_act', 'layer_norm_cf', 'max_pool3x3s2', 'dwconv7x7', 'elu_pad', 'elu_up_cat_pad', 'conv3x3_head', 'conv3x3_headn')

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
def same_pattern(got, ref):
    """Non-finite elements: NaN where the reference has NaN, the same infinity where it has one, finite everywhere else."""
    return bool(((got.isnan() == ref.isnan()) & (got.isinf() == ref.isinf()) & (~ref.isinf() | (got == ref))).all())


def excess(got, ref, bound, dim=None):
    """The error of `got` against `ref` in units of `bound` (<= 1 holds it); with `dim`, the worst slice along it, each relative to its own maximum.
    Every element takes part: a non-finite pattern that differs is an infinite excess, identical non-finite elements are equal."""
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu().reshape(got.shape)
    if not same_pattern(got, ref): return float('inf')
    if bound[0] == 'equal': return 0.0 if bool(((got == ref) | ref.isnan()).all()) else float('inf')
    fin = ref.isfinite()
    got, ref = torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, ref, torch.zeros_like(ref))      # (identical there: they add no error)
    if bound[0] == 'close':
        assert bound[2] > 0, 'every `close` bound of these operators has an absolute part'
        return ((got - ref).abs()/(bound[2] + bound[1]*ref.abs())).max().item()
    if dim is None: return rel_to_max(got, ref)/bound[1]
    return max(rel_to_max(g, r) for g, r in zip(got.unbind(dim), ref.unbind(dim)))/bound[1]


def errors(c, out, ref):
    """-> {output: excess} over every output of the case that has a bound."""
    res = {}
    for k, v in out.items():
        if v is None: continue
        bound = c.tol.get(k, c.tol.get('*'))
        assert bound is not None, f'{c.name}: no bound for {k}'
        res[k] = excess(v, ref[k], bound, c.split.get(k))
    return res


def judge(c, out, ref):
    assert {k for k, v in out.items() if v is not None} == {k for k, v in ref.items() if v is not None}, f'{c.name}: outputs {sorted(out)} against {sorted(ref)}'
    for k, e in errors(c, out, ref).items():
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
