"""Host side of the stride-2 3x3 convolutions' data gradient (`smd_conv3x3s2d_*`): the C prototypes, the size query, `may_serve` (the static stand-in of its
route: test_conv_routing.py)."""
import ctypes as C
import re
from pathlib import Path

from slowtv_monodepth_amd import _lib, conv_routing as R

ROOT = Path(__file__).resolve().parents[1]
# (B, C, CO, H, W) of the transition blocks' conv1, H x W its INPUT: cfg 2 (192 x 640; depth net b = 12, pose net b = 24) and the 384 x 640 counterparts
CFG2 = [(b, c, 2*c, 48*64//c, 160*64//c) for b in (12, 24) for c in (64, 128, 256)]
TALL = [(b, c, co, 2*h, w) for b, c, co, h, w in CFG2]


def test_header_prototypes_match_ctypes_and_the_abi_stays():
    header = re.sub(r'/\*.*?\*/', ' ', (ROOT/'include'/'smd_hotpath.h').read_text(), flags=re.S)
    found = dict(re.findall(r'\b(smd_conv3x3s2d_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header, flags=re.S))
    assert set(found) == {'smd_conv3x3s2d_mfma_workspace_bytes', 'smd_conv3x3s2d_mfma_bwd_data'}
    for name, params in found.items():
        kinds = ['p' if '*' in q else 'i' for q in params.replace('\n', ' ').split(',')]
        res, args = _lib.PROTOTYPES[name]
        assert ['p' if t in (C.c_void_p, C.c_char_p) else 'i' for t in args] == kinds, name
        assert res is (C.c_size_t if name.endswith('_bytes') else C.c_int)
        assert hasattr(_lib.lib, name)
    assert _lib.lib.smd_abi_version() == 8


def test_workspace_query_states_what_is_served():
    q = _lib.lib.smd_conv3x3s2d_mfma_workspace_bytes
    for dims in CFG2 + TALL + [(1, 16, 32, 1, 1), (2, 48, 96, 7, 9)]: assert q(*dims) > 0 and q(*dims) % 256 == 0, dims
    for dims in [(2, 8, 32, 9, 14), (2, 16, 16, 9, 14), (2, 24, 32, 9, 14), (2, 16, 48, 9, 14), (0, 16, 32, 9, 14), (2, 16, 32, 0, 14), (2, 16, 32, 9, 0)]: assert q(*dims) == 0, dims


def test_packed_image_holds_whole_channel_tiles():
    """The data-gradient image is tiles of 32 input channels: the pack's size query counts C up to a multiple of 32."""
    q = _lib.lib.smd_conv3x3_mfma_packed_bytes
    assert q(48, 64, 3) == q(64, 64, 3) and q(16, 32, 3) == q(32, 32, 3) and q(64, 128, 3) >= 64*128*9*3*2


def test_may_serve_follows_the_mode_and_the_cache():
    key = ('data_t2', 12, 64, 128, 48, 160)
    try:
        R.set_conv_route('miopen'); assert not R.may_serve(key)
        R.set_conv_route('mfma'); assert R.may_serve(key)
        R.set_conv_route('auto'); assert R.may_serve(key) and not R.may_serve(key, unknown=False)
        R._ROUTES[key] = (False, 2.0, 1.0); assert not R.may_serve(key)
        R._ROUTES[key] = (True, 1.0, 2.0); assert R.may_serve(key)
    finally:
        R.set_conv_route('auto')
