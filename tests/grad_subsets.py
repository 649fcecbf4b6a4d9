"""Every `torch.autograd.Function` of the package with only SOME of its operands asking for a gradient (test_grad_subsets_host.py checks the table and the
checker on the CPU, test_gpu_grad_subsets.py runs the operators).

The rule: an operator asked for a subset of its gradients returns, for those, the BITS of the full backward, and nothing for the rest; its forward outputs do
not depend on who asks.  Each `needs_input_grad` branch changes what reaches the C ABI (NULL outputs, workspaces that are not allocated, launches that are
skipped, scratch tensors standing in for outputs nobody asked for), and none of that may change another output's bits.

One `Entry` per case: the Function class, the public wrapper, the operands at a small shape, the ordered differentiable operands, the optional ones, a
restatement in plain torch (run in fp64 on the CPU: ATen, or oracle/view_synth_oracle.py) and the bounds.  No tolerance is introduced here: every bound is a
named constant of test_gpu_hostile_memory.py (each taken there from the family's parity test); the CADepth, DDVNet and DiffNet operators take those files'
rule, max(FLOOR, 4 x the error of torch's own fp32 sequence against fp64) (`yard=True`).

`loose`: the gradients that are NOT held to bit-equality between a subset and the full backward, each with the kernel and the reason; they are held to the
reference at the family's bound instead.  Nothing else may stand there."""
import itertools
from collections import namedtuple

import torch
import torch.nn.functional as TF

import conv_exact as X
from conftest import load_golden, rel_to_max
from hostile_memory import first_nan
from test_ddvnet_host import FLOOR, ddv_aten
from test_cadepth_host import se_aten, sp_aten
from test_diffnet_host import fuse_aten, relu_pad_aten
from test_gpu_hostile_memory import (EQUAL, SWEEP_ERR_ATOL, TOL_BLUR, TOL_BLUR_GRAD, TOL_BN, TOL_CHAIN_DEPTH, TOL_CHAIN_GRAD, TOL_CHAIN_LOSS, TOL_CONV_F32, TOL_DWCONV,
                                     TOL_GLUE_BIAS, TOL_GLUE_GA, TOL_GLUE_GX, TOL_GLUE_OUT, TOL_K, TOL_K0_DEPTH, TOL_K0_GRAD, TOL_K0_LOSS, TOL_K_GRAD, TOL_KINV, TOL_LN,
                                     TOL_MASKED_GRAD, TOL_MASKED_LOSS, TOL_MEAN_GRAD, TOL_MEAN_LOSS, TOL_PHOTO_ERR, TOL_PHOTO_GRAD, TOL_POOL_GX, TOL_POSE_GAA,
                                     TOL_POSE_GT, TOL_POSE_T, TOL_REGR, TOL_REGR_GRAD, TOL_SMOOTH_AUX, TOL_UP_GRAD, TOL_UP_OUT, TOL_VS_DWARP, TOL_VS_GRAD, TOL_VS_WARP,
                                     _K, close, rel)

# name; fn: the Function class; wrapper: the public name in `functional`; operands(gen, absent) -> {name: CPU tensor}, `gy_<output>` the incoming gradient of
# a differentiable output, the optional operands in `absent` left out; diff: the differentiable operands in the Function's order; optional: the operands that
# may be None; outputs: the differentiable outputs; call(F, o) / ref(o) -> {name: tensor} (every output, differentiable or not) from the kernels / plain torch;
# tol: {name: bound | None (not compared with the reference), '*': default}, or tol(o) -> such a dict; loose: {gradient: kernel and reason};
# groups: further subsets a training configuration produces; yard: the bound is max(FLOOR, 4 x torch fp32's own error); views: {name: slice compared with the reference}
Entry = namedtuple('Entry', 'name fn wrapper operands diff optional outputs call ref tol loose groups yard views')
TABLE = []

# Functions with ONE differentiable operand and no optional one: there is no subset to leave out.  They stand in the table all the same, for the
# gradient-layout axis (and their one subset is run like any other).
EXEMPT = {
    '_MaxPool3x3s2': 'one differentiable operand (x), no optional one', '_ChannelAttention': 'one differentiable operand (x), no optional one',
    '_Blur3': 'one differentiable operand (x), no optional one', '_PhotoError': 'one differentiable operand (pred; target gets no gradient), no optional one'}


def entry(name, fn, wrapper, operands, diff, outputs, call, ref, tol, optional=(), loose=None, groups=(), yard=False, views=None):
    def ops(gen, absent=frozenset()):
        o = operands(gen, frozenset(absent)) if 'absent' in operands.__code__.co_varnames[:operands.__code__.co_argcount] else operands(gen)
        return {k: v for k, v in o.items() if k not in absent}
    TABLE.append(Entry(name, fn, wrapper, ops, tuple(diff), tuple(optional), tuple(outputs), call, ref, tol, dict(loose or {}), tuple(frozenset(g) for g in groups), yard,
                       dict(views or {})))


def functions_of_the_package():
    """{class name: class} of every `torch.autograd.Function` subclass DEFINED in a `slowtv_monodepth_amd/*_ops.py` module."""
    import importlib
    import pkgutil
    import slowtv_monodepth_amd as P
    out = {}
    for m in pkgutil.iter_modules(P.__path__):
        if not m.name.endswith('_ops'): continue
        mod = importlib.import_module(f'{P.__name__}.{m.name}')
        for k, v in vars(mod).items():
            if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v is not torch.autograd.Function and v.__module__ == mod.__name__: out[k] = v
    return out


# ---- the subsets, the runs, the checker (pure torch: CPU tensors work) -------------------------------------------------------------------------------------
def subsets_of(diff, groups=()):
    """k <= 3 operands: all 2^k - 1 non-empty subsets.  More: each alone, each left out alone, and `groups`.  -> list of frozensets, no repeats, never the full set
    twice (the full set is the run every subset is compared with, and is itself run as a subset once: its bits must reproduce)."""
    diff = tuple(diff)
    if len(diff) <= 3: out = [frozenset(c) for r in range(1, len(diff) + 1) for c in itertools.combinations(diff, r)]
    else: out = [frozenset([d]) for d in diff] + [frozenset(diff) - {d} for d in diff] + [frozenset(g) for g in groups] + [frozenset(diff)]
    seen, uniq = set(), []
    for s in out:
        if s and s not in seen and s <= frozenset(diff): seen.add(s); uniq.append(s)
    return uniq


def tag(subset, diff): return '{' + ', '.join(d for d in diff if d in subset) + '}'


def run_entry(e, F, o, subset, gy=None, unused=()):
    """One forward + backward: the operands of `subset` are leaves, the others plain tensors.  `gy`: {output: incoming gradient} instead of the operands' `gy_*`;
    `unused`: differentiable outputs that take no part in the backward.  -> {output: tensor, 'g_<operand>': gradient or None}."""
    o, leaves = dict(o), {}
    for k in e.diff:
        if k in o and k in subset: o[k] = leaves[k] = o[k].detach().requires_grad_(True)
    out = e.call(F, o)
    outs = [n for n in e.outputs if n not in unused]
    torch.autograd.backward([out[n] for n in outs], [(gy or {}).get(n, o.get(f'gy_{n}')) for n in outs])
    res = {k: (v.detach() if v is not None else None) for k, v in out.items()}
    res.update({f'g_{k}': (o[k].grad if k in leaves else None) for k in e.diff if k in o})
    return res


def run_reference(e, o, dtype=torch.float64):
    """The restatement with every differentiable operand a leaf, in `dtype` on the CPU."""
    o = {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach()) for k, v in o.items()}
    leaves = {k: o[k].clone().requires_grad_(True) for k in e.diff if k in o}
    o.update(leaves)
    out = e.ref(o)
    torch.autograd.backward([out[n] for n in e.outputs], [o[f'gy_{n}'] for n in e.outputs])
    res = {k: v.detach() for k, v in out.items() if v is not None}
    res.update({f'g_{k}': v.grad for k, v in leaves.items()})
    return res


def error_of(got, ref, bound):
    """-> (figure, passed) of `got` against `ref` under a bound of test_gpu_hostile_memory.py."""
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu().reshape(got.shape)
    if bound[0] == 'equal': return float((got != ref).sum()), torch.equal(got, ref)
    if bound[0] == 'rel': r = rel_to_max(got, ref); return r, r <= bound[1]
    d = (got - ref).abs()
    return float(d.max()) if d.numel() else 0.0, bool((d <= bound[2] + bound[1]*ref.abs()).all())


def bounds_of(e, o, ref, ref32=None):
    """{name: bound} for one run: the entry's table, or the yardstick rule from torch's own fp32 run."""
    tol = e.tol(o) if callable(e.tol) else e.tol
    if not e.yard: return {k: tol.get(k, tol.get('*')) for k in ref}
    return {k: (tol[k] if k in tol else rel(max(FLOOR, 4*rel_to_max(ref32[k].double(), ref[k])))) for k in ref}


def check_full(name, full, ref, bounds, views=None, figures=None):
    """The full run (or any run) against the reference: every output and gradient the reference has, finite and within its bound."""
    fails = []
    for k, r in ref.items():
        assert full.get(k) is not None, f'{name}: {k} is missing'
        msg = first_nan(full[k])
        if msg: fails.append(f'{k}: {msg}'); continue
        if bounds.get(k) is None: continue
        v = (views or {}).get(k, lambda t: t)
        fig, ok = error_of(v(full[k]), v(r), bounds[k])
        if figures is not None: figures[k] = fig
        if not ok: fails.append(f'{k}: {fig:.3e} against the reference (bound {bounds[k]})')
    assert not fails, f'{name}: ' + '; '.join(fails)


def check_subsets(run, full, subsets, diff, *, name='', loose=(), hold=None):
    """`run(subset) -> {name: tensor | None}` for each subset against `full`, the run in which every operand of `diff` asked:
    forward outputs bit-equal, every requested gradient bit-equal (the `loose` ones: `hold(what, key, tensor)` instead), every operand left out without a
    gradient, everything finite.  Every failure names the operand and the subset."""
    fails = []
    for s in subsets:
        got, t = run(s), tag(s, diff)
        for k, f in full.items():
            g = got.get(k)
            if k.startswith('g_') and k[2:] in diff:
                if k[2:] not in s:
                    if g is not None: fails.append(f'operand {k[2:]} got a gradient nobody asked for (subset {t})')
                    continue
                if g is None: fails.append(f'operand {k[2:]}: no gradient although asked for (subset {t})'); continue
                what = f'gradient of operand {k[2:]} (subset {t})'
            else:
                if f is None: continue
                if g is None: fails.append(f'output {k} is missing (subset {t})'); continue
                what = f'output {k} (subset {t})'
            msg = first_nan(g)
            if msg: fails.append(f'{what}: {msg}'); continue
            if k in loose:
                if hold is not None: hold(what, k, g)
            elif not torch.equal(g, f):
                fails.append(f'{what} differs from the full backward: {X.first_difference(g, f, [f"d{i}" for i in range(g.ndim)])}')
    assert not fails, f'{name}: ' + '; '.join(fails)


# ---- decoder glue ------------------------------------------------------------------------------------------------------------------------------------------
def _rn(gen, *shape): return torch.randn(*shape, generator=gen)
def _bc(b): return b[None, :, None, None]
def _pad(x): return TF.pad(x, (1, 1, 1, 1), mode='reflect')


def _elu_pad(shape):
    B, C, h, w = shape
    from slowtv_monodepth_amd.net_ops import _EluPad
    entry(f'elu_pad{shape}', _EluPad, 'elu_pad', lambda gen: dict(x=_rn(gen, *shape), bias=_rn(gen, C), gy_out=_rn(gen, B, C, h + 2, w + 2)), ['x', 'bias'], ['out'],
          lambda F, o: dict(out=F.elu_pad(o['x'], o.get('bias'), True)), lambda o: dict(out=_pad(TF.elu(o['x'] + _bc(o['bias']) if 'bias' in o else o['x']))),
          lambda o: {'*': TOL_GLUE_BIAS} if 'bias' in o else dict(out=TOL_GLUE_OUT, g_x=TOL_GLUE_GX), optional=['bias'])


def _elu_up_cat_pad(B, Ca, Cs, h, w):
    from slowtv_monodepth_amd.net_ops import _EluUpCatPad

    def operands(gen, absent):
        cs = 0 if 'skip' in absent else Cs
        o = dict(a=_rn(gen, B, Ca, h, w), bias=_rn(gen, Ca), gy_out=_rn(gen, B, Ca + cs, 2*h + 2, 2*w + 2))
        if cs: o['skip'] = _rn(gen, B, cs, 2*h, 2*w)
        return o

    def ref(o):
        up = TF.interpolate(TF.elu(o['a'] + _bc(o['bias']) if 'bias' in o else o['a']), scale_factor=2, mode='nearest')
        return dict(out=_pad(torch.cat((up, o['skip']), 1) if 'skip' in o else up))
    entry(f'elu_up_cat_pad({B},{Ca},{Cs},{h},{w})', _EluUpCatPad, 'elu_up_cat_pad', operands, ['a', 'bias', 'skip'] if Cs else ['a', 'bias'], ['out'],
          lambda F, o: dict(out=F.elu_up_cat_pad(o['a'], o.get('skip'), bias=o.get('bias'))), ref,
          lambda o: {'*': TOL_GLUE_BIAS} if 'bias' in o else dict(out=TOL_GLUE_OUT, g_a=TOL_GLUE_GA, g_skip=TOL_GLUE_GX), optional=['bias', 'skip'] if Cs else ['bias'])


def _head(B, C, h, w, n=None):
    """n None: `conv3x3_head` (one channel); else `conv3x3_headn`."""
    from slowtv_monodepth_amd.net_ops import _Conv3x3Head, _Conv3x3HeadN
    co, nm = n or 1, f'conv3x3_headn' if n else 'conv3x3_head'
    entry(f'{nm}{n or ""}({B},{C},{h},{w})', _Conv3x3HeadN if n else _Conv3x3Head, nm,
          lambda gen: dict(xp=_rn(gen, B, C, h + 2, w + 2), w=_rn(gen, co, C, 3, 3)/(3*C**0.5), bias=_rn(gen, co), gy_y=_rn(gen, B, co, h, w)), ['xp', 'w', 'bias'], ['y'],
          lambda F, o: dict(y=getattr(F, nm)(o['xp'], o['w'], o.get('bias'), 'sigmoid')), lambda o: dict(y=torch.sigmoid(TF.conv2d(o['xp'], o['w'], o.get('bias')))),
          {'*': TOL_CONV_F32}, optional=['bias'])


_elu_pad((2, 3, 7, 9))
_elu_up_cat_pad(2, 5, 2, 6, 9); _elu_up_cat_pad(2, 3, 0, 1, 1)
for _dims in [(3, 5, 2, 2), (2, 32, 17, 129)]:
    _head(*_dims)
    for _n in (1, 4): _head(*_dims, n=_n)


# ---- convolutions (the routed ones pinned to the MFMA kernels by the GPU module's fixture) ----------------------------------------------------------------------
def _conv(name, fn, wrapper, xs, ws, ys, kw):
    entry(name, fn, wrapper, lambda gen: dict(x=_rn(gen, *xs), w=_rn(gen, *ws)/(ws[2]*ws[1]**0.5), gy_y=_rn(gen, *ys)), ['x', 'w'], ['y'],
          lambda F, o: dict(y=getattr(F, wrapper)(o['x'], o['w'])), lambda o: dict(y=TF.conv2d(o['x'], o['w'], **kw)), {'*': TOL_CONV_F32})


def _convs():
    from slowtv_monodepth_amd.conv_ops import _Conv3x3s2, _Conv3x3Thin, _Conv3x3Wide, _Conv7x7s2Stem
    pad = lambda d: ((d[0], d[1], d[3] + 2, d[4] + 2), (d[2], d[1], 3, 3), (d[0], d[2], d[3], d[4]))
    for dims in [(2, 16, 32, 5, 7), (2, 16, 16, 7, 70)]: _conv(f'conv3x3_mfma{dims}', _Conv3x3Wide, 'conv3x3_mfma', *pad(dims), {})      # (the second: the thin stage)
    _conv('conv3x3_wide(2, 16, 32, 5, 7)', _Conv3x3Wide, 'conv3x3_wide', *pad((2, 16, 32, 5, 7)), {})
    _conv('conv3x3_thin(2, 16, 16, 7, 70)', _Conv3x3Thin, 'conv3x3_thin', *pad((2, 16, 16, 7, 70)), {})
    for B, C, CO, h, w in X.SAME[:2]: _conv(f'conv3x3_same{(B, C, CO, h, w)}', _Conv3x3Wide, 'conv3x3_same', (B, C, h, w), (CO, C, 3, 3), (B, CO, h, w), dict(padding=1))
    for B, C, H, W in X.STEM[:2]:
        _conv(f'conv7x7s2_stem{(B, C, H, W)}', _Conv7x7s2Stem, 'conv7x7s2_stem', (B, C, H, W), (64, C, 7, 7), (B, 64, (H - 1)//2 + 1, (W - 1)//2 + 1), dict(stride=2, padding=3))
    for B, C, CO, H, W in [(2, 16, 32, 4, 6), (2, 32, 96, 9, 14)]:      # (shapes of test_gpu_conv_stride2_data.py: the smallest two-sample one; odd sizes with a wave past CO)
        _conv(f'conv3x3_s2{(B, C, CO, H, W)}', _Conv3x3s2, 'conv3x3_s2', (B, C, H, W), (CO, C, 3, 3), (B, CO, (H - 1)//2 + 1, (W - 1)//2 + 1), dict(stride=2, padding=1))


_convs()


# ---- encoder layers ----------------------------------------------------------------------------------------------------------------------------------------
def _batch_norm(shape):
    from slowtv_monodepth_amd.net_ops import _BatchNormAct
    N, C, H, W = shape

    def operands(gen, absent):
        o = dict(x=_rn(gen, *shape)*2 + 3*_rn(gen, 1, C, 1, 1), residual=_rn(gen, *shape), w=torch.rand(C, generator=gen) + 0.5, b=_rn(gen, C), gy_y=_rn(gen, *shape))
        if 'running' not in absent: o.update(rm=torch.zeros(C), rv=torch.ones(C))
        return o

    def go(fn, o):
        rm, rv = (o['rm'].clone(), o['rv'].clone()) if 'rm' in o else (None, None)         # updated in place: a copy per run
        return dict(y=fn(o['x'], o['w'], o['b'], rm, rv, o.get('residual')), **(dict(running_mean=rm, running_var=rv) if rm is not None else {}))

    def ref_fn(x, w, b, rm, rv, r):
        y = TF.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
        return TF.relu(y + r if r is not None else y)
    entry(f'batch_norm_act{shape}', _BatchNormAct, 'batch_norm_act', operands, ['x', 'residual', 'w', 'b'], ['y'],
          lambda F, o: go(lambda x, w, b, rm, rv, r: F.batch_norm_act(x, w, b, rm, rv, residual=r, momentum=0.1, eps=1e-5, relu=True), o), lambda o: go(ref_fn, o),
          {'*': TOL_BN}, optional=['residual', 'running'], groups=[{'x', 'residual'}, {'w', 'b'}])


def _simple(name, fn, wrapper, operands, diff, call, ref, tol, **kw):
    entry(name, fn, wrapper, operands, diff, ['y'], lambda F, o: dict(y=call(F, o)), lambda o: dict(y=ref(o)), tol, **kw)


def _layers():
    from slowtv_monodepth_amd.net_ops import _DwConv7x7, _LayerNormCF, _MaxPool3x3s2
    for shape in [(3, 5, 7, 9), (2, 130, 3, 5)]: _batch_norm(shape)
    sp = (3, 4, 9, 7)
    _simple(f'max_pool3x3s2{sp}', _MaxPool3x3s2, 'max_pool3x3s2', lambda gen: dict(x=torch.relu(_rn(gen, *sp)), gy_y=_rn(gen, sp[0], sp[1], 5, 4)), ['x'],
            lambda F, o: F.max_pool3x3s2(o['x']), lambda o: TF.max_pool2d(o['x'], 3, 2, 1), dict(y=EQUAL, g_x=TOL_POOL_GX))
    sd = (2, 5, 6, 20)
    _simple(f'dwconv7x7{sd}', _DwConv7x7, 'dwconv7x7', lambda gen: dict(x=_rn(gen, *sd), w=_rn(gen, sd[1], 1, 7, 7)*0.2, b=_rn(gen, sd[1]), gy_y=_rn(gen, *sd)), ['x', 'w', 'b'],
            lambda F, o: F.dwconv7x7(o['x'], o['w'], o.get('b')), lambda o: TF.conv2d(o['x'], o['w'], o.get('b'), padding=3, groups=sd[1]), {'*': TOL_DWCONV}, optional=['b'])
    N, C, H, W = s = (1, 7, 33, 65)
    _simple(f'layer_norm_cf{s}', _LayerNormCF, 'layer_norm_cf',
            lambda gen: dict(x=_rn(gen, *s)*2 + 3*_rn(gen, N, 1, H, W), w=torch.rand(C, generator=gen) + 0.5, b=_rn(gen, C), gy_y=_rn(gen, *s)), ['x', 'w', 'b'],
            lambda F, o: F.layer_norm_cf(o['x'], o['w'], o['b'], 1e-6), lambda o: TF.layer_norm(o['x'].permute(0, 2, 3, 1), (C,), o['w'], o['b'], 1e-6).permute(0, 3, 1, 2),
            {'*': TOL_LN})


_layers()


# ---- the CADepth, DDVNet and DiffNet operators: the yardstick rule of their test files --------------------------------------------------------------------------
def _attention():
    from slowtv_monodepth_amd.attention_ops import _ChannelAttention, _SeGate
    from slowtv_monodepth_amd.ddv_ops import NUM_BINS, _DdvHead
    from slowtv_monodepth_amd.fusion_ops import _ReluPad, _UpCatGatePad
    for s in [(3, 33, 2, 3), (2, 24, 3, 5)]:
        _simple(f'channel_attention{s}', _ChannelAttention, 'channel_attention', lambda gen, s=s: dict(x=_rn(gen, *s)/float(s[2]*s[3])**0.5, gy_y=_rn(gen, *s)), ['x'],
                lambda F, o: F.channel_attention(o['x']), lambda o: sp_aten(o['x']), {}, yard=True)
    for s in [(2, 12, 5, 7), (2, 96, 17, 33)]:      # (the second: several chunks per plane and more channels than a wave)
        C = s[1]
        entry(f'se_gate{s}', _SeGate, 'se_gate',
              lambda gen, s=s, C=C: dict(x=torch.relu(_rn(gen, *s)), w1=_rn(gen, C, C)/C**0.5, b1=0.1*_rn(gen, C), w2=_rn(gen, C, C)/C**0.5, b2=0.1*_rn(gen, C), gy_y=_rn(gen, *s)),
              ['x', 'w1', 'b1', 'w2', 'b2'], ['y'], lambda F, o: dict(zip(('y', 'gate'), F.se_gate(o['x'], o['w1'], o['b1'], o['w2'], o['b2'], return_gate=True))),
              lambda o: dict(y=se_aten(o['x'], o['w1'], o['b1'], o['w2'], o['b2']), gate=torch.sigmoid(torch.relu(o['x'].mean((2, 3)) @ o['w1'].T + o['b1']) @ o['w2'].T + o['b2'])),
              {'*': rel(FLOOR)}, groups=[{'x'}, {'w1', 'b1', 'w2', 'b2'}])       # (test_se_gate_matches_fp64: FLOOR itself, no yardstick)
    (B, C, h, w), G = (2, 16, 5, 33), 1
    entry(f'ddv_head({B},{C},{h},{w})g{G}', _DdvHead, 'ddv_head',
          lambda gen: dict(xp=_rn(gen, B, C, h + 2, w + 2), w=_rn(gen, NUM_BINS*G, C, 3, 3)/float(9*C)**0.5, b=0.1*_rn(gen, NUM_BINS*G), gy_y=_rn(gen, B, G, h, w)),
          ['xp', 'w', 'b'], ['y'], lambda F, o: dict(y=F.ddv_head(o['xp'], o['w'], o['b'], G)), lambda o: dict(y=ddv_aten(o['xp'], o['w'], o['b'], G)), {}, yard=True)
    for B, Ca, Cs, h, w, R in [(2, 16, 8, 3, 5, 1), (2, 16, 16, 33, 70, 2)]:
        Cc = Ca + Cs
        entry(f'up_cat_gate_pad({B},{Ca},{Cs},{h},{w},{R})', _UpCatGatePad, 'up_cat_gate_pad',
              lambda gen, B=B, Ca=Ca, Cs=Cs, h=h, w=w, R=R, Cc=Cc: dict(a=_rn(gen, B, Ca, h, w) + _rn(gen, 1, Ca, 1, 1), bias=0.5*_rn(gen, Ca), skip=_rn(gen, B, Cs, 2*h, 2*w) + _rn(gen, 1, Cs, 1, 1),
                                                                      w1=_rn(gen, R, Cc)/float(Cc)**0.5, w2=_rn(gen, Cc, R)/float(R)**0.5, gy_out=_rn(gen, B, Cc, 2*h + 2, 2*w + 2)),
              ['a', 'bias', 'skip', 'w1', 'w2'], ['out'], lambda F, o: dict(out=F.up_cat_gate_pad(o['a'], o['skip'], o['w1'], o['w2'], o.get('bias'), 'relu')),
              lambda o: dict(out=fuse_aten(o['a'], o.get('bias'), o['skip'], o['w1'], o['w2'], 'relu')), {}, optional=['bias'], yard=True,
              groups=[{'a', 'skip'}, {'bias', 'w1', 'w2'}, {'w1', 'w2'}])
    B, C, h, w = s = (2, 16, 5, 33)
    entry(f'relu_pad{s}', _ReluPad, 'relu_pad', lambda gen: dict(x=_rn(gen, *s), bias=0.5*_rn(gen, C), gy_out=_rn(gen, B, C, h + 2, w + 2)), ['x', 'bias'], ['out'],
          lambda F, o: dict(out=F.relu_pad(o['x'], o.get('bias'))), lambda o: dict(out=relu_pad_aten(o['x'], o.get('bias'))), {}, optional=['bias'], yard=True)


_attention()


# ---- class-level operators ------------------------------------------------------------------------------------------------------------------------------------
def _oracle():
    from oracle import view_synth_oracle as O
    return O


def _regression(name, loss_name, operands):
    from slowtv_monodepth_amd.class_ops import _Regression

    def ref(o):
        loss, out = _oracle().regression_loss(o['pred'], o['target'], o['mask'].to(o['pred'].dtype) if 'mask' in o else None, loss_name)
        return dict(loss=loss, err=out['err_regr'])
    # g_target is the mirrored arithmetic of g_pred (k_regr_bwd): it takes g_pred's bound
    entry(f'regression_{name}', _Regression, 'regression_loss', operands, ['pred', 'target'], ['loss'],
          lambda F, o: dict(zip(('loss', 'err'), F.regression_loss(o['pred'], o['target'], o.get('mask'), loss_name=loss_name))), ref,
          dict(loss=TOL_REGR, err=TOL_REGR, g_pred=TOL_REGR_GRAD, g_target=TOL_REGR_GRAD), optional=['mask'])


def _regr_fixture(fixture):
    def operands(gen):
        g = load_golden(fixture)
        return dict(pred=g['in_pred'], target=g['in_target'], gy_loss=torch.ones(()), **({'mask': g['in_mask'].bool()} if 'in_mask' in g else {}))
    return operands


def _regr_blocks(gen):      # 3102 elements: four blocks of 1024 with a ragged tail
    s = (2, 1, 33, 47)
    return dict(pred=0.1 + 5*torch.rand(*s, generator=gen), target=0.1 + 5*torch.rand(*s, generator=gen), mask=torch.rand(*s, generator=gen) > 0.3, gy_loss=torch.tensor(0.75))


_regression('op_regr_berhu_mask', 'berhu', _regr_fixture('op_regr_berhu_mask')); _regression('op_regr_log_l1', 'log_l1', _regr_fixture('op_regr_log_l1'))
_regression('berhu(2, 1, 33, 47)', 'berhu', _regr_blocks); _regression('log_l1(2, 1, 33, 47)', 'log_l1', _regr_blocks)


def _class_ops():
    from slowtv_monodepth_amd.class_ops import _PhotoError, _ReconReduce, _ScaleMean, _UpsampleStack, _ViewSynth
    from slowtv_monodepth_amd.geom_ops import _Intrinsics, _PoseMatrices
    from slowtv_monodepth_amd.recon_ops import _Blur3

    def vs_operands(gen):
        O, g = _oracle(), load_golden('op_view_synth')
        return dict(inp=g['in_input'], depth=g['in_depth'], T=O.T_from_AAt(g['in_aa'], g['in_t']).contiguous(), K=g['in_K'], K_inv=torch.linalg.inv(g['in_K']),
                    gy_warp=g['in_gw'], gy_dwarp=g['in_gd'])
    # g_input: float atomicAdd in k_view_synth_bwd (csrc/smd_unfused.hip), no fixed sum order: `loose` in the hostile table too
    entry('view_synth_c5', _ViewSynth, 'view_synth', vs_operands, ['inp', 'depth', 'T', 'K', 'K_inv'], ['warp', 'dwarp'],
          lambda F, o: dict(zip(('warp', 'dwarp', 'valid'), F.view_synth(o['inp'], o['depth'], o['T'], o['K'], o.get('K_inv')))),
          lambda o: dict(zip(('warp', 'dwarp', 'valid'), _oracle().view_synth(o['inp'], o['depth'], o['T'], o['K'], o.get('K_inv')))),
          {'warp': TOL_VS_WARP, 'dwarp': TOL_VS_DWARP, 'valid': None, '*': TOL_VS_GRAD}, optional=['K_inv'],
          loose={'g_inp': 'k_view_synth_bwd (csrc/smd_unfused.hip) accumulates g_input with float atomicAdd: its sum order is not fixed from run to run'},
          groups=[{'depth', 'T'}, {'K', 'K_inv'}, {'inp', 'depth', 'T'}, {'depth'}, {'T'}], views={'g_T': lambda g: g[..., :3, :]})

    def photo_operands(gen):
        g = load_golden('op_photo_error')
        return dict(pred=g['in_pred'], target=g['in_target'], gy_y=g['in_ge'])
    _simple('photo_error_ssim', _PhotoError, 'photo_error', photo_operands, ['pred'], lambda F, o: F.photo_error(o['pred'], o['target'], 'ssim'),
            lambda o: _oracle().photo_error(o['pred'], o['target'], 'ssim'), dict(y=TOL_PHOTO_ERR, g_pred=TOL_PHOTO_GRAD))

    n, B, h, w = 3, 2, 33, 47

    def rr_operands(gen):      # random error maps: the decisions (minimum over the supports, automask) are taken by margins far above the 1e-7 tie-break noise
        return dict(err_warp=torch.rand(n, B, h, w, generator=gen), err_static=torch.rand(n, B, h, w, generator=gen), mask=0.5*_rn(gen, B, n, h, w), noise=_rn(gen, B, 1, h, w),
                    gy_loss=torch.tensor(1.25))

    def rr_ref(o):
        O, name = _oracle(), ('uncertainty' if 'mask' in o else None)
        red = lambda e: O.apply_mask(e.permute(1, 0, 2, 3), o.get('mask'), name).min(dim=1, keepdim=True)[0]
        err = red(o['err_warp'])
        sel = O.apply_mask(o['err_warp'].permute(1, 0, 2, 3), o.get('mask'), name).argmin(dim=1, keepdim=True)
        if 'err_static' in o:
            st = red(o['err_static']) + (O.EPS32*o['noise'] if 'noise' in o else 0)
            sel = torch.where(err <= st, sel, torch.full_like(sel, 255)); err = torch.minimum(err, st)
        return dict(loss=err.mean(), err=err[:, 0], sel=sel[:, 0].to(torch.uint8))
    entry(f'recon_reduce({n},{B},{h},{w})', _ReconReduce, 'recon_reduce', rr_operands, ['err_warp', 'mask'], ['loss'],
          lambda F, o: dict(zip(('loss', 'err', 'sel'), F.recon_reduce(o['err_warp'], o.get('err_static'), use_min=True, noise=o.get('noise'), seed=5, mask=o.get('mask'),
                                                                   mask_name='uncertainty' if 'mask' in o else None))), rr_ref,
          {'loss': TOL_MASKED_LOSS, 'err': close(0, SWEEP_ERR_ATOL), 'sel': EQUAL, '*': TOL_MASKED_GRAD}, optional=['err_static', 'mask', 'noise'])

    b, nn, size, sizes = 1, 4, (33, 47), [(33, 47), (17, 23), (5, 9), (1, 1)]
    xs = [f'x{s}' for s in range(len(sizes))]
    entry(f'upsample_stack({b},{nn},{size})', _UpsampleStack, 'upsample_stack',
          lambda gen: dict({f'x{s}': torch.rand(b, nn, hs, ws, generator=gen) for s, (hs, ws) in enumerate(sizes)}, gy_up=_rn(gen, len(sizes), b, nn, *size)), xs, ['up'],
          lambda F, o: dict(up=F.upsample_stack([o[k] for k in xs], size)),
          lambda o: dict(up=torch.stack([TF.interpolate(o[k], size=size, mode='bilinear', align_corners=False) for k in xs])), {'up': TOL_UP_OUT, '*': TOL_UP_GRAD},
          groups=[{'x0', 'x1'}])
    shapes = [(2, 1, 33, 47), (1, 1, 1, 1), (3, 1, 64, 64)]      # sizes off the 4096-element blocks (test_scale_mean_matches_fp64)
    ms = [f'x{s}' for s in range(len(shapes))]
    entry('scale_mean_bce_ones', _ScaleMean, 'scale_mean', lambda gen: dict({f'x{s}': torch.sigmoid(3*_rn(gen, *sh)) for s, sh in enumerate(shapes)}, gy_loss=torch.tensor(2.5)),
          ms, ['loss'], lambda F, o: dict(loss=F.scale_mean([o[k] for k in ms], 'bce_ones')),
          lambda o: dict(loss=torch.stack([TF.binary_cross_entropy(o[k], torch.ones_like(o[k])) for k in ms]).mean()), {'loss': TOL_MEAN_LOSS, '*': TOL_MEAN_GRAD})

    N = 9

    def pose_operands(gen):
        aa = _rn(gen, N, 3)*0.3
        aa[0] = 0.0; aa[1] = aa[1]*1e-4/aa[1].norm()       # the clip branch and the |aa| < eps branch (test_inverted_pose_matches_general_inverse)
        return dict(aa=aa, t=_rn(gen, N, 3), inv=torch.tensor([0, 1, 1, 0, 1, 0, 1, 1, 0], dtype=torch.uint8), gy_T=_rn(gen, N, 4, 4))

    def pose_ref(o):
        T = _oracle().T_from_AAt(o['aa'], o['t'])
        return dict(T=torch.stack([torch.linalg.inv(Ti) if f else Ti for Ti, f in zip(T, o['inv'])]))
    entry('pose_matrices_inverted', _PoseMatrices, 'pose_matrices', pose_operands, ['aa', 't'], ['T'], lambda F, o: dict(T=F.pose_matrices(o['aa'], o['t'], o['inv'])), pose_ref,
          dict(T=TOL_POSE_T, g_aa=TOL_POSE_GAA, g_t=TOL_POSE_GT))

    bk, sz = 5, (96, 320)

    def k_ref(o):
        O = _oracle()
        K = O.resize_K(O.build_K(o['fs'], o['cs']), sz)
        return dict(K=K, K_inv=torch.linalg.inv(K))
    entry('intrinsics', _Intrinsics, 'intrinsics',
          lambda gen: dict(fs=torch.rand(bk, 2, generator=gen) + 0.5, cs=torch.rand(bk, 2, generator=gen)*0.2 + 0.4, gy_K=_rn(gen, bk, 4, 4), gy_K_inv=_rn(gen, bk, 4, 4)),
          ['fs', 'cs'], ['K', 'K_inv'], lambda F, o: dict(zip(('K', 'K_inv'), F.intrinsics(o['fs'], o['cs'], sz))), k_ref, dict(K=TOL_K, K_inv=TOL_KINV, g_fs=TOL_K_GRAD, g_cs=TOL_K_GRAD))
    s = (3, 2, 33, 70)
    _simple(f'gaussian_blur3x3{s}', _Blur3, 'gaussian_blur3x3', lambda gen: dict(x=torch.rand(*s, generator=gen), gy_y=_rn(gen, *s)), ['x'], lambda F, o: F.gaussian_blur3x3(o['x']),
            lambda o: _oracle().gaussian_blur3x3(o['x']), dict(y=TOL_BLUR, g_x=TOL_BLUR_GRAD))


_class_ops()


# ---- the reconstruction operators: b=2, h=33, w=47, n=3 and the pyramid of the hostile `_loss_path` cases; mean over the supports, no automask (no decision to flip) ------
RB, RH, RW, RN, LOWS = 2, 33, 47, 3, [(33, 47), (16, 23), (8, 11)]
DS = [f'd{s}' for s in range(len(LOWS))]


def _recon_operands(gen):
    O = _oracle()
    imgs = torch.rand(RB, 3, RH, RW, generator=gen)
    aa, t = 0.01*_rn(gen, RN*RB, 3), 0.05*_rn(gen, RN*RB, 3)
    fs, cs = torch.tensor([0.58, 1.92])[None].repeat(RB, 1)*(1 + 0.05*_rn(gen, RB, 2)), 0.5 + 0.03*_rn(gen, RB, 2)
    K = O.resize_K(O.build_K(fs, cs), (RH, RW))
    o = dict(imgs=imgs, supp=(imgs[None] + 0.15*_rn(gen, RN, RB, 3, RH, RW)).clamp(0, 1), aa=aa, t=t, fs=fs, cs=cs, T=O.T_from_AAt(aa, t).unflatten(0, (RN, RB)).contiguous(),
             K=K, K_inv=torch.linalg.inv(K), depth=1 + 10*torch.rand(len(LOWS), RB, 1, RH, RW, generator=gen), gy_loss=torch.tensor(1.5),
             gy_depth_up=1e-3*_rn(gen, len(LOWS), RB, 1, RH, RW))
    o.update({f'd{s}': 0.05 + 0.9*torch.rand(RB, 1, hs, ws, generator=gen) for s, (hs, ws) in enumerate(LOWS)})
    return o


def _only(*keep):
    """The operands of `_recon_operands` an entry uses (the others would only be copied to the device)."""
    return lambda gen: {k: v for k, v in _recon_operands(gen).items() if k in keep}


def _recon_ref(depth_up, o):
    """`oracle.image_recon` with an explicit `K_inv` (the oracle's handler always inverts K itself): view synthesis of every support at every scale, the
    photometric error against the target, the mean over the supports.  depth_up {s: (b,1,h,w)} -> loss."""
    O, S = _oracle(), len(depth_up)
    dep = torch.stack(list(depth_up.values())).flatten(0, 1)
    ex = lambda t, tail: t.expand(RN, S, RB, *tail).flatten(0, 2)
    Ki = o['K_inv'] if 'K_inv' in o else torch.linalg.inv(o['K'])
    warp = O.view_synth(ex(o['supp'][:, None], (3, RH, RW)), dep[None].expand(RN, *dep.shape).flatten(0, 1), ex(o['T'][:, None], (4, 4)), ex(o['K'][None, None], (4, 4)),
                        ex(Ki[None, None], (4, 4)))[0]
    return O.recon_loss(warp.unflatten(0, (RN, S*RB)), o['imgs'][None].expand(S, *o['imgs'].shape).flatten(0, 1), use_min=False, use_automask=False)[0]


def _depth_up(o): return _oracle().disp_to_depth_up({s: o[k] for s, k in enumerate(DS)}, (RH, RW), 0.1, 100)[1]


def _recon():
    from slowtv_monodepth_amd.recon_ops import _DispSmooth, _DispToDepth, _ImageRecon, _ImageReconDisp, _LossPath
    flags = lambda F: F.recon_flags('ssim', False, False)
    KK = [{'K', 'K_inv'}, {'K'}, {'K_inv'}]
    entry('disp_to_depth', _DispToDepth, 'disp_to_depth', _only(*DS, 'gy_depth_up'), DS, ['depth_up'],
          lambda F, o: dict(zip(('depth_up', 'disp_up'), F.disp_to_depth([o[k] for k in DS], (RH, RW), 0.1, 100, want_disp_up=True))),
          lambda o: dict(depth_up=torch.stack(list(_depth_up(o).values()))), {'depth_up': TOL_K0_DEPTH, '*': TOL_K0_GRAD})
    entry('disp_smooth_fused', _DispSmooth, 'disp_smooth_fused', _only(*DS, 'imgs', 'gy_loss'), DS, ['loss'],
          lambda F, o: dict(zip(('loss', 'disp_grad', 'image_grad'), F.disp_smooth_fused({s: o[k] for s, k in enumerate(DS)}, o['imgs'], use_edges=True, want_aux=True))),
          lambda o: (lambda l, aux: dict(loss=l, disp_grad=aux['disp_grad'], image_grad=aux['image_grad']))(*_oracle().disp_smooth({s: o[k] for s, k in enumerate(DS)}, o['imgs'], True)),
          {'loss': TOL_K0_LOSS, 'disp_grad': TOL_SMOOTH_AUX, 'image_grad': TOL_SMOOTH_AUX, '*': TOL_K0_GRAD})
    entry('image_recon_fused', _ImageRecon, 'image_recon_fused', _only('depth', 'imgs', 'supp', 'T', 'K', 'K_inv', 'gy_loss'), ['depth', 'T', 'K', 'K_inv'], ['loss'],
          lambda F, o: dict(zip(('loss', 'err', 'sel'), F.image_recon_fused(o['depth'], o['imgs'], o['supp'], o['T'], o['K'], o.get('K_inv'), flags=flags(F))[:3])),
          lambda o: dict(loss=_recon_ref({s: o['depth'][s] for s in range(len(LOWS))}, o)), {'loss': TOL_CHAIN_LOSS, '*': TOL_CHAIN_GRAD}, optional=['K_inv'],
          groups=[{'depth'}, {'T'}, {'depth', 'T'}, *KK], views={'g_T': lambda g: g[..., :3, :]})
    entry('image_recon_fused_disp', _ImageReconDisp, 'image_recon_fused_disp', _only(*DS, 'imgs', 'supp', 'T', 'K', 'K_inv', 'gy_loss', 'gy_depth_up'), ['T', 'K', 'K_inv', *DS],
          ['loss', 'depth_up'],
          lambda F, o: dict(zip(('loss', 'err', 'sel', 'warp0', 'depth_up'), F.image_recon_fused_disp([o[k] for k in DS], o['imgs'], o['supp'], o['T'], o['K'], o.get('K_inv'), flags=flags(F),
                                                                                                 min_depth=0.1, max_depth=100))),
          lambda o: (lambda dep: dict(loss=_recon_ref(dep, o), depth_up=torch.stack(list(dep.values()))))(_depth_up(o)),
          {'loss': TOL_CHAIN_LOSS, 'depth_up': TOL_CHAIN_DEPTH, '*': TOL_CHAIN_GRAD}, optional=['K_inv'], groups=[set(DS), {'T'}, {'T', *DS}, *KK], views={'g_T': lambda g: g[..., :3, :]})

    def lp_ref(o):
        dep = _depth_up(o)
        l_rec, l_sm = _recon_ref(dep, o), _oracle().disp_smooth({s: o[k] for s, k in enumerate(DS)}, o['imgs'], True)[0]
        return dict(loss=l_rec + 0.001*l_sm, l_rec=l_rec, l_sm=l_sm, depth_up=torch.stack(list(dep.values())))
    lp_tol = {'loss': TOL_CHAIN_LOSS, 'l_rec': TOL_CHAIN_LOSS, 'l_sm': TOL_CHAIN_LOSS, 'depth_up': TOL_CHAIN_DEPTH, '*': TOL_CHAIN_GRAD}
    lp_names = ('loss', 'l_rec', 'l_sm', 'sel', 'depth_up')
    lp_kw = dict(min_depth=0.1, max_depth=100, seed=11, w_recon=1.0, w_smooth=0.001)
    entry('loss_path_fused', _LossPath, 'loss_path_fused', _only(*DS, 'imgs', 'supp', 'T', 'K', 'K_inv', 'gy_loss'), ['T', 'K', 'K_inv', *DS], ['loss'],
          lambda F, o: dict(zip(lp_names, F.loss_path_fused({s: o[k] for s, k in enumerate(DS)}, o['imgs'], o['supp'], o['T'], o['K'], o.get('K_inv'), flags=flags(F), **lp_kw))), lp_ref,
          lp_tol, optional=['K_inv'], groups=[set(DS), {'T'}, {'T', *DS}, *KK], views={'g_T': lambda g: g[..., :3, :]})

    def lp_pose(F, o):      # `Ts`, `K`, `K_inv` from the leaves, taken as values: the gradients go to (aa, t) and (fs, cs) directly
        Ts = F.pose_matrices(o['aa'], o['t']).unflatten(0, (RN, RB)); K, K_inv = F.intrinsics(o['fs'], o['cs'], (RH, RW))
        return dict(zip(lp_names, F.loss_path_fused({s: o[k] for s, k in enumerate(DS)}, o['imgs'], o['supp'], Ts, K, K_inv, pose=(o['aa'], o['t'], None), intrinsics=(o['fs'], o['cs']),
                                                    flags=flags(F), **lp_kw)))

    def lp_pose_ref(o):
        O = _oracle()
        K = O.resize_K(O.build_K(o['fs'], o['cs']), (RH, RW))
        return lp_ref({**o, 'T': O.T_from_AAt(o['aa'], o['t']).unflatten(0, (RN, RB)), 'K': K, 'K_inv': torch.linalg.inv(K)})
    entry('loss_path_fused_pose_leaves', _LossPath, 'loss_path_fused', _only(*DS, 'imgs', 'supp', 'aa', 't', 'fs', 'cs', 'gy_loss'), ['aa', 't', 'fs', 'cs', *DS], ['loss'], lp_pose, lp_pose_ref,
          lp_tol, groups=[set(DS), {'aa', 't'}, {'fs', 'cs'}, {'aa', 't', *DS}, {'aa', 't', 'fs', 'cs'}])


_recon()
BY_NAME = {e.name: e for e in TABLE}
