"""What make_golden_conv_skeleton.py records and the tests replay (conv_skeleton_rules.npz, conv_skeleton_calls.json): the grid of the static rule, the
routed convolutions' cases with their seeded operands, and the recorder around the one `call` seam.  Only the public names of `functional` /
`conv_routing`, `_device.call` and `conv_routing._time_interleaved` are used: the recording was taken at the commit BEFORE the rule tables and the operators
were merged into one table and one skeleton, with this file as it stands."""
import contextlib
import hashlib
import importlib
import itertools
import math
import zlib
from collections import namedtuple

import torch

# ---- the static rule's grid ---------------------------------------------------------------------------------------------------------------------------------
OPS = ('fwd', 'data', 'wgt', 'fwd_bf16', 'data_bf16', 'wgt_bf16', 'fwd_z', 'data_z', 'wgt_z', 'fwd_s', 'wgt_s', 'fwd_s2', 'wgt_s2', 'data_t2')
NO_SUCH_OP = ('data_s', 'data_s2', 'fwd_t2', 'fwd_s3')             # `static_rule` raises KeyError
BATCHES = (1, 2, 12, 24, 48)
# the decoder's layers, the encoders' stride-1 and stride-2 layers, the stems; then one step on either side of `_COARSE_C_MIN` / c_max (256), co_max (64),
# c_co_max (128*64) and ch_max (511)
CHANNELS = ((512, 256), (256, 128), (128, 64), (64, 32), (96, 32), (32, 16), (16, 16), (64, 64), (128, 128), (256, 256), (512, 512), (64, 128), (128, 256),
            (256, 512), (3, 64), (6, 64), (255, 128), (257, 128), (128, 63), (128, 65), (129, 64), (511, 511), (510, 512))
_PX_MIN = (1000, 2400, 5000, 20000)                                # every `px_min` of the tables


def sizes():
    """(h, w): the pyramid levels of 192 x 640 and 384 x 640; per batch size and `px_min`, the two sizes on either side of B h w = px_min, as one row and as
    rows of 80 columns (the widest the coarse clauses take); 79 / 80 / 81 columns around `_COARSE_W_MAX`."""
    out = [(H >> s, 640 >> s) for H in (192, 384) for s in range(6)]
    for B, v in itertools.product(BATCHES, _PX_MIN):
        n, rows = math.ceil(v/B), math.ceil(v/(B*80))
        out += [(1, n - 1), (1, n), (rows - 1, 80), (rows, 80)]
    out += [(h, w) for h in (1, 6, 30) for w in (79, 80, 81)]
    return sorted({(h, w) for h, w in out if h > 0 and w > 0})


def grid():
    """Every (op, B, C, CO, h, w) of the recording, in its order."""
    return [(op, B, C, CO, h, w) for op in OPS for B in BATCHES for C, CO in CHANNELS for h, w in sizes()]


# ---- the operators' cases ---------------------------------------------------------------------------------------------------------------------------------------
# name; wrapper: the name in `functional`; xs, ws: the shapes of x and the weight; extra: further arguments (`ddv_head`: bias shape, out_ch); bf16: x as bfloat16;
# bits: which of y, g_x, g_w the kernels write under route 'mfma' (the others are MIOpen's, whose solver choice is not ours: not recorded)
Case = namedtuple('Case', 'name wrapper xs ws bias bf16 bits')
SUBSETS = ('x', 'w', 'xw')
MODES = ('mfma', 'miopen', 'auto')


def _c3(wrapper, dims, grow, bits, bf16=False):
    B, C, CO, h, w = dims
    return Case(f'{wrapper}{"_bf16" if bf16 else ""}{dims}', wrapper, (B, C, h + grow, w + grow), (CO, C, 3, 3), None, bf16, bits)


def _stem(dims, bits):
    B, C, H, W = dims
    return Case(f'conv7x7s2_stem{dims}', 'conv7x7s2_stem', (B, C, H, W), (64, C, 7, 7), None, False, bits)


ALL, NONE = ('y', 'g_x', 'g_w'), ()
CASES = [
    _c3('conv3x3_mfma', (2, 16, 32, 5, 7), 2, ('y', 'g_w')),        # (C = 16: the data gradient is MIOpen's)
    _c3('conv3x3_mfma', (2, 16, 16, 7, 70), 2, ALL),                # the thin stage
    _c3('conv3x3_wide', (2, 16, 32, 5, 7), 2, ('y', 'g_w')),
    _c3('conv3x3_wide', (2, 16, 16, 7, 70), 2, ALL),                # the thin stage: the references are the f32-MFMA kernels
    _c3('conv3x3_wide', (2, 16, 16, 7, 70), 2, ALL, bf16=True),
    _c3('conv3x3_wide', (2, 8, 32, 5, 7), 2, NONE),                 # C = 8: the size query turns it down
    _c3('conv3x3_same', (2, 64, 64, 1, 1), 0, ALL),
    _c3('conv3x3_same', (3, 64, 64, 5, 7), 0, ALL),
    _c3('conv3x3_same', (2, 8, 32, 5, 7), 0, NONE),
    _stem((2, 3, 1, 1), ('y', 'g_w')),                              # (the stem's data gradient is ATen's)
    _stem((2, 3, 5, 7), ('y', 'g_w')),
    _stem((2, 8, 5, 7), NONE),
    _c3('conv3x3_s2', (1, 16, 32, 1, 1), 0, ALL),
    _c3('conv3x3_s2', (2, 16, 32, 4, 6), 0, ALL),
    _c3('conv3x3_s2', (2, 8, 32, 9, 14), 0, NONE),
    Case('ddv_head(1, 16, 2, 2)', 'ddv_head', (1, 16, 4, 4), (128, 16, 3, 3), (128,), False, ALL),
]


def operands(case):
    """-> (x, weight, bias or None, generator) on the CPU; the generator goes on to draw dL/dy once the output's shape is known."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    x = torch.randn(*case.xs, generator=gen)
    wt = torch.randn(*case.ws, generator=gen)/(case.ws[2]*case.ws[1]**0.5)
    bias = torch.randn(*case.bias, generator=gen) if case.bias else None
    return (x.bfloat16() if case.bf16 else x), wt, bias, gen


def run_case(F, case, subset):
    """One forward and backward with the operands of `subset` asking for a gradient -> {'y', 'g_x', 'g_w'}, None where not asked for."""
    x, wt, bias, gen = operands(case)
    x, wt = x.cuda().requires_grad_('x' in subset), wt.cuda().requires_grad_('w' in subset)
    y = getattr(F, case.wrapper)(x, wt, *([bias.cuda(), 1] if bias is not None else []))
    y.backward(torch.randn(*y.shape, generator=gen).to(y.dtype).cuda())
    torch.cuda.synchronize()
    return dict(y=y.detach(), g_x=x.grad, g_w=wt.grad)


def digest(t):
    """The SHA-256 of a tensor's bits, with its type and shape: equal digests, equal bit patterns."""
    b = t.detach().cpu().contiguous()
    return f'{str(b.dtype).rpartition(".")[2]}{list(b.shape)}:' + hashlib.sha256(b.view(torch.uint8).numpy().tobytes()).hexdigest()


# ---- the recorder ---------------------------------------------------------------------------------------------------------------------------------------------------
def _arg(a):
    """Sizes, counts and flags as they are; a pointer (a tensor's, the stream's) as 'p', NULL as '-': which operands a launch is handed, not where they live."""
    if a is None: return '-'
    return str(a) if isinstance(a, int) and abs(a) < 2**32 else 'p'


@contextlib.contextmanager
def recording(log):
    """Every launch the convolution modules make through `call` (they bind `_device.call` by name: the binding of each is wrapped), as 'entry(arguments)'."""
    from slowtv_monodepth_amd import _device
    real, mods = _device.call, []
    for name in ('conv_ops', 'conv_s2', 'ddv_ops'):
        try: mods.append(importlib.import_module(f'slowtv_monodepth_amd.{name}'))
        except ModuleNotFoundError: pass

    def spy(entry, *args):
        log.append(f'{entry}({",".join(_arg(a) for a in args)})')
        return real(entry, *args)
    for m in mods:
        assert m.call is real, m.__name__
        m.call = spy
    try: yield
    finally:
        for m in mods: m.call = real


def fake_timer(run_mfma, run_ref, rounds):
    """The stand-in of tests/test_conv_routing.py for `conv_routing._time_interleaved`: runs both `rounds` times, the kernels win."""
    for _ in range(rounds): run_mfma(); run_ref()
    return [10.0]*rounds, [20.0]*rounds


def record_case(F, R, case, mode, subset):
    """The launches of one case under one route (set anew: the cache is empty), and its results.  'auto': the timer is the fake, and the case runs twice,
    the first call taking the A/B and the second the cached decision."""
    log, real = [], R._time_interleaved
    F.set_conv_route(mode)
    try:
        if mode == 'auto': R._time_interleaved = fake_timer
        with recording(log):
            out = run_case(F, case, subset)
            if mode == 'auto': run_case(F, case, subset)
    finally:
        R._time_interleaved = real
        F.set_conv_route('auto')
    return log, out
