"""The routed convolutions launch what they launched before their three operators became one skeleton: per case of conv_skeleton_cases.py, route ('mfma',
'miopen', and 'auto' with the timer of test_conv_routing.py, which also pins the count of warm-up and timing runs; there the case runs twice: the A/B,
then the cached decision) and gradient subset ({x}, {w}, {x, w}), the library entry points in order with their sizes, counts and which pointers are NULL, as
recorded through the `call` seam by tests/golden/make_golden_conv_skeleton.py at the commit before.  Under 'mfma' also the bits (as SHA-256 digests) of the
output and of every gradient the kernels write: the same calls on the same library give the same bits, whoever asks for a gradient."""
import json

import pytest
import torch

import conv_skeleton_cases as K
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
REC = json.loads((GOLDEN/'conv_skeleton_calls.json').read_text())


def test_recording_covers_every_case():
    assert set(REC['sequences']) == {c.name for c in K.CASES} and len(K.CASES) == 16
    for c in K.CASES:
        assert set(REC['sequences'][c.name]) == set(K.MODES) and all(set(s) == set(K.SUBSETS) for s in REC['sequences'][c.name].values()), c.name
        assert set(REC['bits'].get(c.name, {})) == set(c.bits), c.name
    unserved = [c.name for c in K.CASES if not c.bits]            # per family one shape the size query turns down (C = 8): no forward on the kernels
    assert len(unserved) == 4 and not any('_fwd(' in REC['launches'][i] for n in unserved for s in REC['sequences'][n].values() for q in s.values() for i in q)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('case', K.CASES, ids=[c.name for c in K.CASES])
def test_launches_and_bits_equal_the_recording(case, mode):
    from slowtv_monodepth_amd import conv_routing as R, functional as F
    for subset in K.SUBSETS:
        log, out = K.record_case(F, R, case, mode, subset)
        want = [REC['launches'][i] for i in REC['sequences'][case.name][mode][subset]]
        assert log == want, f'{case.name}, route {mode}, gradients of {subset}: launched {log}, recorded {want}'
        assert (out['g_x'] is None) == ('x' not in subset) and (out['g_w'] is None) == ('w' not in subset)
        if mode != 'mfma': continue
        for k in case.bits:
            if out[k] is not None: assert K.digest(out[k]) == REC['bits'][case.name][k], f'{case.name}, gradients of {subset}: {k} has other bits than recorded'
    assert F.conv_routes() == {}
