"""Who serves a convolution operator, the split-bf16 MFMA kernels or the reference (MIOpen; for the thin last stage the f32-MFMA kernels): the decision only,
no autograd, no launches of its own, testable without a GPU (`conv_ops` builds the operators on `serve`).  A same-box A/B decides the first time an (operator,
shape) pair is seen: both run on the call's own tensors, interleaved, a few times each; the faster one is cached for the process.  `set_conv_route('mfma' |
'miopen')` pins the choice; inside a HIP-graph capture nothing is timed and `RULES` stands in.  Operator names, the keys of `RULES` and of `conv_routes()`:
`<fwd | data | wgt>[_<family suffix>]`."""
from __future__ import annotations

import torch

from ._lib import Unsupported

_MODE = 'auto'
_ROUTES: dict = {}                       # (op, B, C, CO, h, w) -> (use_mfma, us_mfma, us_ref)
_AB_WARMUPS, _AB_ROUNDS, _AB_MARGIN = 2, 5, 0.97
_DECLINED = (Unsupported, ValueError)    # what the kernel path raises where it turns a shape down: the reference serves the call instead


def set_conv_route(mode: str = 'auto'):
    """'auto' (A/B on first use), 'mfma' or 'miopen' for every routed convolution; clears the cached decisions."""
    global _MODE
    if mode not in ('auto', 'mfma', 'miopen'): raise ValueError(mode)
    _MODE = mode
    _ROUTES.clear()


def conv_routes() -> dict:
    """The decisions taken so far: {(op, B, C, CO, h, w): (use_mfma, us_mfma, us_miopen)}."""
    return dict(_ROUTES)


# ---- the static rule, the stand-in where nothing may be timed (graph capture).  Per operator: the MFMA kernels serve a shape that meets EVERY bound of ANY
# one clause (`_BOUNDS`; px = B h w, thin: CO == 16, coarse: the row-band tiles' levels, w <= 80 with C >= 256); no clause: never the kernels.  h x w and
# the profile that filled the clauses, per family of operator names:
#   fwd / data / wgt     fp32 tensors, reflection-padded input (the decoder), h x w the OUTPUT size: the shapes that won on an MI355X at cfg 2,
#                        profiles/r06_decoder_convs.txt; the coarse levels on the row-band tiles (1.18-1.59 x forward, 1.09-1.74 x data gradient,
#                        0.92-1.37 x weight gradient): profiles/r08_coarse_convs.txt
#   *_bf16               the same layers on bf16 tensors, the OUTPUT size: MIOpen's bf16 kernels serve the wide layers; the thin stage is the stencil-like
#                        case (profiles/r06_decoder_convs.txt)
#   *_z                  the zero-padded encoder layers (C = CO), the OUTPUT size (= the input's), profiles/r08_coarse_convs.txt: the data gradient wins at
#                        every stage (1.4-1.7 x); forward and weight gradient win 1.13-1.6 x from 64 to 256 channels and at 512 channels with b = 24 (2880
#                        pixels), and are even with MIOpen at 512 channels with b = 12 (1440)
#   fwd_s / wgt_s        the 7x7 stride-2 stems, the INPUT size: profiles/stem_convs.txt (the data gradient is ATen's: no route)
#   fwd_s2 / wgt_s2      the strided 3x3 layers (`conv3x3_s2`), the INPUT size, profiles/s2_convs.txt (cfg 2, b = 12 / 24): the forward wins at all three
#                        transition blocks (1.27-2.06 x, the smallest 5760 input pixels per channel); the weight gradient loses at all of them (0.30-0.44 x)
#   data_t2              their data gradient (a transposed convolution), the layer's INPUT size, the gradient's own: profiles/s2_data_convs.txt (cfg 2,
#                        b = 12 / 24), the clause filled from what won there
_COARSE_W_MAX, _COARSE_C_MIN = 80, 256
_Z_FWD_WGT = [dict(px_min=1000, ch_max=511), dict(px_min=2400)]
RULES = {
    'fwd': [dict(thin=True), dict(thin=False, px_min=20000, c_co_max=128*64), dict(thin=False, coarse=True, px_min=1000)],
    'data': [dict(thin=True), dict(thin=False, px_min=5000, c_max=256), dict(thin=False, coarse=True, px_min=1000)],
    'wgt': [dict(thin=False, px_min=20000, co_max=64), dict(thin=False, coarse=True, px_min=2400)],
    'fwd_bf16': [dict(thin=True)], 'data_bf16': [dict(thin=True)], 'wgt_bf16': [dict(thin=True)],
    'fwd_z': _Z_FWD_WGT, 'data_z': [dict(px_min=1000)], 'wgt_z': _Z_FWD_WGT,
    'fwd_s': [dict(px_min=20000)], 'wgt_s': [dict(px_min=20000)],
    'fwd_s2': [dict(px_min=5000)], 'wgt_s2': [],
    'data_t2': [dict(px_min=5000)],
}
_BOUNDS = {'px_min': lambda v, B, C, CO, h, w: B*h*w >= v,
           'c_max': lambda v, B, C, CO, h, w: C <= v,
           'co_max': lambda v, B, C, CO, h, w: CO <= v,
           'c_co_max': lambda v, B, C, CO, h, w: C*CO <= v,
           'ch_max': lambda v, B, C, CO, h, w: max(C, CO) <= v,
           'thin': lambda v, B, C, CO, h, w: (CO == 16) == v,
           'coarse': lambda v, B, C, CO, h, w: (w <= _COARSE_W_MAX and C >= _COARSE_C_MIN) == v}


def static_rule(op, B, C, CO, h, w) -> bool:
    """`RULES[op]` evaluated for one shape (`KeyError`: an operator no family has)."""
    return any(all(_BOUNDS[name](v, B, C, CO, h, w) for name, v in clause.items()) for clause in RULES[op])


def may_serve(key, unknown=True) -> bool:
    """What `_conv_route` would say of `key` = (op, B, C, CO, h, w) without timing anything: the pinned mode, the cached decision, the static rule under
    capture; `unknown` where the shape's A/B has not been run yet."""
    if _MODE != 'auto': return _MODE == 'mfma'
    r = _ROUTES.get(key)
    if r is None: return static_rule(*key) if torch.cuda.is_initialized() and _capturing() else unknown   # (no capture without an initialised device)
    return r[0]


# ---- the A/B and the dispatcher ---------------------------------------------------------------------------------------------------------------------
_capturing = torch.cuda.is_current_stream_capturing


def _time_interleaved(run_mfma, run_ref, rounds):
    """Microseconds of `rounds` runs of each, interleaved: a box's clocks drift over the first milliseconds, whatever is timed first looks slower."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(rounds)]
    for e in ev:
        e[0].record(); run_mfma(); e[1].record(); run_ref(); e[2].record()
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1])*1e3 for e in ev], [e[1].elapsed_time(e[2])*1e3 for e in ev]


def _conv_route(op, B, C, CO, h, w, run_mfma, run_ref) -> bool:
    """Pinned mode, cached decision, static rule under capture (not cached), or an A/B now: two warm-ups, five interleaved timings, medians, a 3 % margin."""
    if _MODE != 'auto': return _MODE == 'mfma'
    key = (op, B, C, CO, h, w)
    r = _ROUTES.get(key)
    if r is None:
        if _capturing(): return static_rule(op, B, C, CO, h, w)
        for _ in range(_AB_WARMUPS): run_mfma(); run_ref()
        us_m, us_r = _time_interleaved(run_mfma, run_ref, _AB_ROUNDS)
        t_m, t_r = sorted(us_m)[_AB_ROUNDS//2], sorted(us_r)[_AB_ROUNDS//2]
        r = _ROUTES[key] = (t_m < _AB_MARGIN*t_r, t_m, t_r)
    return r[0]


def serve(key, run_mfma, run_ref, *, eligible, force=False):
    """Run the operator `key` = (op, B, C, CO, h, w) on the MFMA kernels or the reference; returns what the one that served it returned.  Not `eligible` (a shape
    the kernels do not take): the reference, under `force` too; `run_mfma` is never called, nothing is cached.  `force`: the kernels, their errors propagate.  Else
    as `_conv_route` says; where the kernel path declines (`_DECLINED`: in the A/B, then cached as (False, nan, nan), or in the call) the reference serves it."""
    if not eligible: return run_ref()
    if force: return run_mfma()
    try:
        use = _conv_route(*key, run_mfma, run_ref)
    except _DECLINED:
        _ROUTES[key] = (False, float('nan'), float('nan'))
        use = False
    if use:
        try:
            return run_mfma()
        except _DECLINED:
            pass
    return run_ref()
