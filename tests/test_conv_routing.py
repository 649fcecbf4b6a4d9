"""`conv_routing`: the dispatcher's branches with fake callables and an injected timer, the one rule table's structure, and the static rule on the shapes the
project runs and on the grid recorded before the three tables became one (tests/golden/make_golden_conv_skeleton.py).  No GPU."""
import math

import numpy as np
import pytest

import conv_skeleton_cases as K
from conftest import GOLDEN

from slowtv_monodepth_amd import _lib, conv_routing as R

KEY = ('fwd', 12, 64, 32, 48, 160)


class Fakes:
    """`run_mfma` / `run_ref` that count their calls and return a tag; `raises`: what `run_mfma` raises instead."""
    def __init__(self, raises=None):
        self.n_mfma = self.n_ref = 0
        self.raises = raises

    def run_mfma(self):
        self.n_mfma += 1
        if self.raises is not None: raise self.raises
        return 'mfma'

    def run_ref(self):
        self.n_ref += 1
        return 'ref'

    def serve(self, **kw):
        kw.setdefault('eligible', True)
        return R.serve(KEY, self.run_mfma, self.run_ref, **kw)


@pytest.fixture
def timer(monkeypatch):
    """Replaces the event timer and the capture probe: `timer.us = (mfma, ref)`, `timer.capturing`; counts the timings taken.  Like the real timer it
    runs both callables `rounds` times."""
    class T:
        us, capturing, calls = (10.0, 20.0), False, 0
    def fake(run_mfma, run_ref, rounds):
        T.calls += 1
        for _ in range(rounds): run_mfma(); run_ref()
        return [T.us[0]]*rounds, [T.us[1]]*rounds
    monkeypatch.setattr(R, '_time_interleaved', fake)
    monkeypatch.setattr(R, '_capturing', lambda: T.capturing)
    R.set_conv_route('auto')
    yield T
    R.set_conv_route('auto')


def test_force_runs_the_kernels_and_propagates_their_errors(timer):
    f = Fakes()
    assert f.serve(force=True) == 'mfma' and (f.n_mfma, f.n_ref) == (1, 0)
    for exc in (_lib.Unsupported('no'), ValueError('no')):
        f = Fakes(exc)
        with pytest.raises(type(exc)): f.serve(force=True)
        assert f.n_ref == 0
    assert R.conv_routes() == {} and timer.calls == 0


@pytest.mark.parametrize('mode', ['auto', 'mfma', 'miopen'])
@pytest.mark.parametrize('force', [False, True])
def test_ineligible_never_calls_the_kernels_and_caches_nothing(timer, mode, force):
    R.set_conv_route(mode)
    f = Fakes()
    assert f.serve(eligible=False, force=force) == 'ref'
    assert (f.n_mfma, f.n_ref) == (0, 1) and R.conv_routes() == {} and timer.calls == 0


def test_pinned_miopen_takes_the_reference(timer):
    R.set_conv_route('miopen')
    f = Fakes()
    assert f.serve() == 'ref' and (f.n_mfma, f.n_ref) == (0, 1) and R.conv_routes() == {}


@pytest.mark.parametrize('exc', [None, _lib.Unsupported('no'), ValueError('no')])
def test_pinned_mfma_runs_the_kernels_and_falls_back_where_they_decline(timer, exc):
    R.set_conv_route('mfma')
    f = Fakes(exc)
    assert f.serve() == ('mfma' if exc is None else 'ref')
    assert (f.n_mfma, f.n_ref) == (1, 0 if exc is None else 1) and R.conv_routes() == {} and timer.calls == 0


def test_pinned_mfma_does_not_swallow_other_errors(timer):
    R.set_conv_route('mfma')
    with pytest.raises(_lib.HotpathError): Fakes(_lib.HotpathError('launch failed')).serve()


@pytest.mark.parametrize('us, use', [((10.0, 20.0), True), ((20.0, 10.0), False), ((96.9, 100.0), True), ((97.0, 100.0), False), ((99.0, 100.0), False)])
def test_auto_times_once_and_caches_the_decision(timer, us, use):
    timer.us = us
    f = Fakes()
    assert f.serve() == ('mfma' if use else 'ref')
    assert timer.calls == 1 and R.conv_routes() == {KEY: (use, us[0], us[1])}
    assert (f.n_mfma, f.n_ref) == (2 + 5 + use, 2 + 5 + (not use))      # two warm-ups, five timings, the call itself
    g = Fakes()                                                          # second call: the cached decision, no timing
    assert g.serve() == ('mfma' if use else 'ref')
    assert timer.calls == 1 and (g.n_mfma, g.n_ref) == (int(use), int(not use))


def test_auto_takes_the_median_of_the_timings(timer, monkeypatch):
    monkeypatch.setattr(R, '_time_interleaved', lambda m, r, rounds: ([500.0, 9.0, 10.0, 400.0, 11.0], [1.0, 20.0, 19.0, 300.0, 2.0]))
    assert Fakes().serve() == 'mfma' and R.conv_routes() == {KEY: (True, 11.0, 19.0)}


@pytest.mark.parametrize('exc', [_lib.Unsupported('no'), ValueError('no')])
def test_failed_ab_is_cached_as_not_served(timer, exc):
    f = Fakes(exc)
    assert f.serve() == 'ref'
    (use, t_m, t_r), = R.conv_routes().values()
    assert use is False and math.isnan(t_m) and math.isnan(t_r) and list(R.conv_routes()) == [KEY]
    assert (f.n_mfma, f.n_ref) == (1, 1) and timer.calls == 0            # (the first warm-up raised)
    g = Fakes(exc)
    assert g.serve() == 'ref' and (g.n_mfma, g.n_ref) == (0, 1)


@pytest.mark.parametrize('exc', [_lib.Unsupported('no'), ValueError('no')])
def test_cached_mfma_still_falls_back_where_the_call_declines(timer, exc):
    assert Fakes().serve() == 'mfma'
    f = Fakes(exc)
    assert f.serve() == 'ref' and (f.n_mfma, f.n_ref) == (1, 1)
    assert R.conv_routes()[KEY][0] is True                               # (the decision stays)


def test_capture_uses_the_static_rule_and_caches_nothing(timer):
    timer.capturing = True
    assert R.static_rule(*KEY) is True
    f = Fakes()
    assert f.serve() == 'mfma' and (f.n_mfma, f.n_ref) == (1, 0)
    key = ('wgt', 12, 32, 16, 96, 320)
    assert R.static_rule(*key) is False
    g = Fakes()
    assert R.serve(key, g.run_mfma, g.run_ref, eligible=True) == 'ref' and (g.n_mfma, g.n_ref) == (0, 1)
    assert R.conv_routes() == {} and timer.calls == 0
    timer.us = (20.0, 10.0)                                              # a decision cached before the capture wins over the rule
    timer.capturing = False
    assert Fakes().serve() == 'ref'
    timer.capturing = True
    assert Fakes().serve() == 'ref' and timer.calls == 1


def test_set_conv_route_clears_the_cache_and_rejects_unknown_modes(timer):
    Fakes().serve()
    assert len(R.conv_routes()) == 1
    with pytest.raises(ValueError): R.set_conv_route('cudnn')
    assert len(R.conv_routes()) == 1                                     # (a rejected mode changes nothing)
    R.set_conv_route('auto')
    assert R.conv_routes() == {}
    assert Fakes().serve() == 'mfma' and timer.calls == 2


def test_functional_keeps_its_surface():
    from slowtv_monodepth_amd import _device, conv_ops, functional as F
    assert F.set_conv_route is R.set_conv_route and F.conv_routes is R.conv_routes and F._conv_route is R._conv_route
    for name in ('conv3x3_thin', 'conv3x3_mfma', 'conv3x3_wide', 'conv3x3_same', 'conv7x7s2_stem', 'conv3x3_s2'): assert getattr(F, name) is getattr(conv_ops, name)
    assert F.call is conv_ops.call is _device.call and F._stream is conv_ops._stream is _device._stream     # one `_tls` behind all of them
    assert not hasattr(F, '_tls') and not hasattr(conv_ops, '_tls')


# The static rule on the shapes the project runs — the decoder (fp32 and bf16 tensors), the encoders' 3x3 stride-1 layers (depth net: B = b; pose net: B = 2 b)
# and the stems of a ResNet-18 depth net and pose net.  The expected values are those of `_conv_static_rule` of the commit before the rule became a table
# (c0e17d7), written out; per row (family, B, C, CO, h, w, (fwd, data, wgt)), the stem (fwd, wgt).
_OPS = {'padded': ('fwd', 'data', 'wgt'), 'bf16': ('fwd_bf16', 'data_bf16', 'wgt_bf16'), 'zpad': ('fwd_z', 'data_z', 'wgt_z'), 'stem': ('fwd_s', 'wgt_s')}
_EXPECTED = [
    # 192 x 640, b = 12
    ('padded', 12, 512, 256, 6, 20, (True, True, False)),
    ('padded', 12, 512, 256, 12, 40, (True, True, True)),
    ('padded', 12, 256, 128, 12, 40, (True, True, True)),
    ('padded', 12, 256, 128, 24, 80, (True, True, True)),
    ('padded', 12, 128, 64, 24, 80, (True, True, True)),
    ('padded', 12, 128, 64, 48, 160, (True, True, True)),
    ('padded', 12, 64, 32, 48, 160, (True, True, True)),
    ('padded', 12, 96, 32, 96, 320, (True, True, True)),
    ('padded', 12, 32, 16, 96, 320, (True, True, False)),
    ('padded', 12, 16, 16, 192, 640, (True, True, False)),
    ('bf16', 12, 512, 256, 6, 20, (False, False, False)),
    ('bf16', 12, 512, 256, 12, 40, (False, False, False)),
    ('bf16', 12, 256, 128, 12, 40, (False, False, False)),
    ('bf16', 12, 256, 128, 24, 80, (False, False, False)),
    ('bf16', 12, 128, 64, 24, 80, (False, False, False)),
    ('bf16', 12, 128, 64, 48, 160, (False, False, False)),
    ('bf16', 12, 64, 32, 48, 160, (False, False, False)),
    ('bf16', 12, 96, 32, 96, 320, (False, False, False)),
    ('bf16', 12, 32, 16, 96, 320, (True, True, True)),
    ('bf16', 12, 16, 16, 192, 640, (True, True, True)),
    ('zpad', 12, 64, 64, 48, 160, (True, True, True)),
    ('zpad', 12, 128, 128, 24, 80, (True, True, True)),
    ('zpad', 12, 256, 256, 12, 40, (True, True, True)),
    ('zpad', 12, 512, 512, 6, 20, (False, True, False)),
    ('zpad', 24, 64, 64, 48, 160, (True, True, True)),
    ('zpad', 24, 128, 128, 24, 80, (True, True, True)),
    ('zpad', 24, 256, 256, 12, 40, (True, True, True)),
    ('zpad', 24, 512, 512, 6, 20, (True, True, True)),
    ('stem', 12, 3, 64, 192, 640, (True, True)),
    ('stem', 24, 6, 64, 192, 640, (True, True)),
    # 192 x 640, b = 24
    ('padded', 24, 512, 256, 6, 20, (True, True, True)),
    ('padded', 24, 512, 256, 12, 40, (True, True, True)),
    ('padded', 24, 256, 128, 12, 40, (True, True, True)),
    ('padded', 24, 256, 128, 24, 80, (True, True, True)),
    ('padded', 24, 128, 64, 24, 80, (True, True, True)),
    ('padded', 24, 128, 64, 48, 160, (True, True, True)),
    ('padded', 24, 64, 32, 48, 160, (True, True, True)),
    ('padded', 24, 96, 32, 96, 320, (True, True, True)),
    ('padded', 24, 32, 16, 96, 320, (True, True, False)),
    ('padded', 24, 16, 16, 192, 640, (True, True, False)),
    ('bf16', 24, 512, 256, 6, 20, (False, False, False)),
    ('bf16', 24, 512, 256, 12, 40, (False, False, False)),
    ('bf16', 24, 256, 128, 12, 40, (False, False, False)),
    ('bf16', 24, 256, 128, 24, 80, (False, False, False)),
    ('bf16', 24, 128, 64, 24, 80, (False, False, False)),
    ('bf16', 24, 128, 64, 48, 160, (False, False, False)),
    ('bf16', 24, 64, 32, 48, 160, (False, False, False)),
    ('bf16', 24, 96, 32, 96, 320, (False, False, False)),
    ('bf16', 24, 32, 16, 96, 320, (True, True, True)),
    ('bf16', 24, 16, 16, 192, 640, (True, True, True)),
    ('zpad', 24, 64, 64, 48, 160, (True, True, True)),
    ('zpad', 24, 128, 128, 24, 80, (True, True, True)),
    ('zpad', 24, 256, 256, 12, 40, (True, True, True)),
    ('zpad', 24, 512, 512, 6, 20, (True, True, True)),
    ('zpad', 48, 64, 64, 48, 160, (True, True, True)),
    ('zpad', 48, 128, 128, 24, 80, (True, True, True)),
    ('zpad', 48, 256, 256, 12, 40, (True, True, True)),
    ('zpad', 48, 512, 512, 6, 20, (True, True, True)),
    ('stem', 24, 3, 64, 192, 640, (True, True)),
    ('stem', 48, 6, 64, 192, 640, (True, True)),
    # 384 x 640, b = 12
    ('padded', 12, 512, 256, 12, 20, (True, True, True)),
    ('padded', 12, 512, 256, 24, 40, (True, True, True)),
    ('padded', 12, 256, 128, 24, 40, (True, True, True)),
    ('padded', 12, 256, 128, 48, 80, (True, True, True)),
    ('padded', 12, 128, 64, 48, 80, (True, True, True)),
    ('padded', 12, 128, 64, 96, 160, (True, True, True)),
    ('padded', 12, 64, 32, 96, 160, (True, True, True)),
    ('padded', 12, 96, 32, 192, 320, (True, True, True)),
    ('padded', 12, 32, 16, 192, 320, (True, True, False)),
    ('padded', 12, 16, 16, 384, 640, (True, True, False)),
    ('bf16', 12, 512, 256, 12, 20, (False, False, False)),
    ('bf16', 12, 512, 256, 24, 40, (False, False, False)),
    ('bf16', 12, 256, 128, 24, 40, (False, False, False)),
    ('bf16', 12, 256, 128, 48, 80, (False, False, False)),
    ('bf16', 12, 128, 64, 48, 80, (False, False, False)),
    ('bf16', 12, 128, 64, 96, 160, (False, False, False)),
    ('bf16', 12, 64, 32, 96, 160, (False, False, False)),
    ('bf16', 12, 96, 32, 192, 320, (False, False, False)),
    ('bf16', 12, 32, 16, 192, 320, (True, True, True)),
    ('bf16', 12, 16, 16, 384, 640, (True, True, True)),
    ('zpad', 12, 64, 64, 96, 160, (True, True, True)),
    ('zpad', 12, 128, 128, 48, 80, (True, True, True)),
    ('zpad', 12, 256, 256, 24, 40, (True, True, True)),
    ('zpad', 12, 512, 512, 12, 20, (True, True, True)),
    ('zpad', 24, 64, 64, 96, 160, (True, True, True)),
    ('zpad', 24, 128, 128, 48, 80, (True, True, True)),
    ('zpad', 24, 256, 256, 24, 40, (True, True, True)),
    ('zpad', 24, 512, 512, 12, 20, (True, True, True)),
    ('stem', 12, 3, 64, 384, 640, (True, True)),
    ('stem', 24, 6, 64, 384, 640, (True, True)),
]


def test_static_rule_on_the_shapes_the_project_runs():
    assert len(_EXPECTED) == 3*(2*10 + 2*4 + 2)
    for family, B, C, CO, h, w, expected in _EXPECTED:
        assert len(expected) == len(_OPS[family])
        for op, e in zip(_OPS[family], expected):
            assert R.static_rule(op, B, C, CO, h, w) is e, (op, B, C, CO, h, w)


def test_rules_is_one_table_keyed_by_the_operator_names():
    """Forward, data and weight gradient plain and as `_bf16` and `_z`; the stem and the stride-2 layers' forward and weight gradient; the stride-2 data
    gradient: fourteen operators (the stem has no `data_s`), each under its own key of the one table."""
    names = {k + s for k in ('fwd', 'data', 'wgt') for s in ('', '_bf16', '_z')} | {'fwd_s', 'wgt_s', 'fwd_s2', 'wgt_s2', 'data_t2'}
    assert set(R.RULES) == names == set(K.OPS) == {op for ops in _OPS.values() for op in ops} | {'fwd_s2', 'wgt_s2', 'data_t2'} and len(names) == 14
    for name in ('STATIC_RULES', 'STRIDED_RULES', 'TRANSPOSED_RULES', '_FAMILY_OF_SUFFIX'): assert not hasattr(R, name), name


def test_every_clause_names_known_bounds_and_only_wgt_s2_has_none():
    for op, clauses in R.RULES.items():
        assert all(set(c) <= set(R._BOUNDS) for c in clauses), op
        assert bool(clauses) is (op != 'wgt_s2'), op              # `wgt_s2`: never the kernels under capture (MIOpen's wins at every transition block)
    assert not any(R.static_rule('wgt_s2', *p[1:]) for p in K.grid() if p[0] == 'wgt_s2')


@pytest.mark.parametrize('op', K.NO_SUCH_OP)
def test_static_rule_raises_for_an_operator_no_family_has(op):
    assert set(K.NO_SUCH_OP) == {'data_s', 'data_s2', 'fwd_t2', 'fwd_s3'}
    with pytest.raises(KeyError): R.static_rule(op, 12, 64, 128, 48, 160)


def test_static_rule_equals_the_recording_on_every_grid_point():
    """Every operator x batch size x channel pair x size of conv_skeleton_cases.grid() (the networks' layers at both resolutions and one step on either side of
    every bound): the booleans `static_rule` returned before the tables were merged."""
    with np.load(GOLDEN/'conv_skeleton_rules.npz') as z: n, served = int(z['n']), np.unpackbits(z['served'])
    pts = K.grid()
    assert len(pts) == n == len(K.OPS)*len(K.BATCHES)*len(K.CHANNELS)*len(K.sizes()) and {p[0] for p in pts} == set(R.RULES)
    bad = [p for p, e in zip(pts, served[:n]) if R.static_rule(*p) is not bool(e)]
    assert not bad, f'{len(bad)} of {n} decisions changed, the first: {bad[:5]}'
