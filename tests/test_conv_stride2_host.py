"""Host side of the stride-2 3x3 convolutions (`conv3x3_s2`): the C prototypes, the size query, the Makefile (the static stand-in of its routes:
test_conv_routing.py)."""
import ctypes as C
import re
from pathlib import Path

from slowtv_monodepth_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
# (B, C, CO, H, W) of the transition blocks' conv1, H x W its INPUT: cfg 2 (192 x 640; depth net b = 12, pose net b = 24) and the 384 x 640 counterparts
CFG2 = [(b, c, 2*c, 48*64//c, 160*64//c) for b in (12, 24) for c in (64, 128, 256)]
TALL = [(b, c, co, 2*h, w) for b, c, co, h, w in CFG2]


def test_header_prototypes_match_ctypes_and_the_abi_stays():
    header = re.sub(r'/\*.*?\*/', ' ', (ROOT/'include'/'smd_hotpath.h').read_text(), flags=re.S)
    found = dict(re.findall(r'\b(smd_conv3x3s2_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header, flags=re.S))
    assert set(found) == {'smd_conv3x3s2_mfma_workspace_bytes', 'smd_conv3x3s2_mfma_fwd', 'smd_conv3x3s2_mfma_bwd_weight'}
    for name, params in found.items():
        kinds = ['p' if '*' in q else 'i' for q in params.replace('\n', ' ').split(',')]
        res, args = _lib.PROTOTYPES[name]
        assert ['p' if t in (C.c_void_p, C.c_char_p) else 'i' for t in args] == kinds, name
        assert res is (C.c_size_t if name.endswith('_bytes') else C.c_int)
        assert hasattr(_lib.lib, name)
    assert _lib.lib.smd_abi_version() == 8


def test_workspace_query_states_what_is_served():
    q = _lib.lib.smd_conv3x3s2_mfma_workspace_bytes
    for dims in CFG2 + TALL + [(1, 16, 32, 1, 1), (2, 48, 96, 7, 9)]: assert q(*dims) > 0 and q(*dims) % 256 == 0, dims
    for dims in [(2, 8, 32, 9, 14), (2, 16, 16, 9, 14), (2, 24, 32, 9, 14), (2, 16, 48, 9, 14), (0, 16, 32, 9, 14), (2, 16, 32, 0, 14), (2, 16, 32, 9, 0)]: assert q(*dims) == 0, dims


def test_makefile_lists_the_source():
    mk = (ROOT/'slowtv_monodepth_amd'/'csrc'/'Makefile').read_text()
    srcs = re.search(r'^SRCS := (.*)$', mk, flags=re.M).group(1).split()
    assert 'smd_conv_s2.hip' in srcs and (ROOT/'slowtv_monodepth_amd'/'csrc'/'smd_conv_s2.hip').is_file()
