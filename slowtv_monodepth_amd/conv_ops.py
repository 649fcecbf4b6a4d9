"""The routed convolutions as `torch.autograd.Function`s: every operator (forward, data gradient, weight gradient) runs on the split-bf16 MFMA kernels
(`smd_conv3x3_mfma_*`, `smd_conv3x3z_mfma_*`, `smd_conv7x7s2_*`, `smd_conv3x3s2[d]_mfma_*`) or on its reference, as `conv_routing.serve` decides.  What differs
between the families is a `_Family` record; `_forward` and `_backward` are written once.  `functional` re-exports the wrappers."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._device import _check, _check_fb, _on, _ptr, _stream, _workspace, call
from .conv_routing import may_serve, serve

_BF = torch.bfloat16


def _thin_bwd(xp, weight, g_y, want_x, want_w):
    """The f32-MFMA kernels of the last stage (`smd_conv3x3_thin_bwd`; fp32 tensors only): (g_xp, g_w), None where not wanted."""
    if not (want_x or want_w): return None, None
    B, C, H, W = xp.shape
    g_xp = torch.empty_like(xp) if want_x else None
    g_w = torch.empty_like(weight) if want_w else None
    ws, nbytes = _workspace(xp.device, _lib.lib.smd_conv3x3_thin_workspace_bytes, B, C, H - 2, W - 2, floor=256) if want_w else (None, 0)
    call('smd_conv3x3_thin_bwd', xp.data_ptr(), weight.data_ptr(), g_y.data_ptr(), _ptr(g_xp), _ptr(g_w), _ptr(ws), nbytes, B, C, H - 2, W - 2, _stream())
    return g_xp, g_w


class _Conv3x3Thin(torch.autograd.Function):
    """`conv3x3_thin`: the f32 MFMA (`smd_conv3x3_thin_*`: `v_mfma_f32_16x16x4_f32`, operands staged through LDS); `conv3x3_wide` routes to it per operator."""
    @staticmethod
    def forward(ctx, xp, weight):
        xp = _check('xp', xp)
        if xp.ndim != 4 or xp.shape[2] < 4 or xp.shape[3] < 4: raise ValueError(f'expected a padded (B,C,h+2,w+2) with h, w >= 2, got {tuple(xp.shape)}')
        B, C, H, W = xp.shape
        weight = _check('weight', weight, (16, C, 3, 3))
        y = torch.empty((B, 16, H - 2, W - 2), device=xp.device, dtype=torch.float32)
        call('smd_conv3x3_thin_fwd', xp.data_ptr(), weight.data_ptr(), y.data_ptr(), B, C, H - 2, W - 2, _stream())
        ctx.save_for_backward(xp, weight)
        return y

    @staticmethod
    def backward(ctx, g_y):
        xp, weight = ctx.saved_tensors
        _on(xp)
        B, C, H, W = xp.shape
        g_y = _check('grad(y)', g_y, (B, 16, H - 2, W - 2))
        return _thin_bwd(xp, weight, g_y, *ctx.needs_input_grad)


def conv3x3_thin(xp, weight):
    """`F.conv2d(xp, weight)` for sixteen output channels and an input that is already reflection-padded: the thin up-convolution of the decoder's last
    stage (src/networks/decoders/monodepth.py:45-50, 80-84), bias-free (the next glue kernel adds it).  xp (B,C,h+2,w+2), weight (16,C,3,3) -> (B,16,h,w);
    C = 16 or 32 (`_lib.Unsupported` otherwise)."""
    return _Conv3x3Thin.apply(xp, weight)


_Served = namedtuple('_Served', 'fwd data wgt thin sized')


def _served(C, CO, zpad, sized) -> _Served:
    """What the 3x3 MFMA kernels serve for one layer — the Python statement of `smd::conv_mfma_served` (csrc/smd_kernels.h), made once per forward and read
    by the backward; thin: the last stage (its reference is the f32-MFMA kernel); sized: the workspace query took the sizes (or `force`)."""
    thin = CO == 16 and C in (16, 32) and not zpad
    return _Served(fwd=(C % 16 == 0 and CO % 32 == 0) or thin,
                   data=(CO % 16 == 0 and C % 32 == 0) or (C == 16 and CO == 16 and not zpad),   # the data gradient's own operand order
                   wgt=CO % 32 == 0 or thin, thin=thin, sized=sized)


def pack_weights(weight, C, CO, pieces, want_fwd, want_bwd):
    """`smd_conv3x3_mfma_pack`: the weights' pieces in the operand order of the forward and of the data gradient, (wf, wb), None where not wanted."""
    nbytes = _lib.lib.smd_conv3x3_mfma_packed_bytes(C, CO, pieces)
    wf = _workspace(weight.device, nbytes, floor=256)[0] if want_fwd else None
    wb = _workspace(weight.device, nbytes, floor=256)[0] if want_bwd else None
    call('smd_conv3x3_mfma_pack', weight.data_ptr(), _ptr(wf), _ptr(wb), C, CO, pieces, _stream())
    return wf, wb


def _stem_pack(weight, C, CO, pieces, want_fwd, want_bwd):
    wp, _ = _workspace(weight.device, _lib.lib.smd_conv7x7s2_packed_bytes, C, CO)
    call('smd_conv7x7s2_pack', weight.data_ptr(), wp.data_ptr(), C, CO, _stream())
    return wp, None


# A family of routed operators.  ops: the names `serve` routes forward, data gradient and weight gradient under (None: no kernel, the reference serves it
# unrouted); entries: their entry points; query, query_data: the size queries of forward and weight gradient and (None: the same one) of the data gradient,
# 0 = sizes the kernels do not take, the reference serves every operator; k, stride, pad: the convolution, as ATen is handed it; out_dims: h x w of the
# operator's key and of the library calls is the OUTPUT size (else the input's); pack: the weights' operand images; pieces_arg / fwd_ws: the entry points
# take `pieces` / the forward takes a workspace
_Family = namedtuple('_Family', 'ops entries query query_data k stride pad out_dims pack pieces_arg fwd_ws')
_PADDED = _Family(('fwd', 'data', 'wgt'), ('smd_conv3x3_mfma_fwd', 'smd_conv3x3_mfma_bwd_data', 'smd_conv3x3_mfma_bwd_weight'),
                  'smd_conv3x3_mfma_workspace_bytes', None, 3, 1, 0, True, pack_weights, True, True)
_BF16 = _PADDED._replace(ops=('fwd_bf16', 'data_bf16', 'wgt_bf16'))
_ZPAD = _Family(('fwd_z', 'data_z', 'wgt_z'), ('smd_conv3x3z_mfma_fwd', 'smd_conv3x3z_mfma_bwd_data', 'smd_conv3x3z_mfma_bwd_weight'),
                'smd_conv3x3z_mfma_workspace_bytes', None, 3, 1, 1, True, pack_weights, True, True)
_STEM = _Family(('fwd_s', None, 'wgt_s'), ('smd_conv7x7s2_fwd', None, 'smd_conv7x7s2_bwd_weight'),
                'smd_conv7x7s2_workspace_bytes', None, 7, 2, 3, False, _stem_pack, False, False)
_S2 = _Family(('fwd_s2', 'data_t2', 'wgt_s2'), ('smd_conv3x3s2_mfma_fwd', 'smd_conv3x3s2d_mfma_bwd_data', 'smd_conv3x3s2_mfma_bwd_weight'),
              'smd_conv3x3s2_mfma_workspace_bytes', 'smd_conv3x3s2d_mfma_workspace_bytes', 3, 2, 1, False, pack_weights, False, True)


def _dims(fam, x, weight):
    """-> (B, C, CO, h, w) of the family's keys and library calls, and the output's (ho, wo)."""
    B, C, H, W = x.shape
    ho, wo = (H + 2*fam.pad - fam.k)//fam.stride + 1, (W + 2*fam.pad - fam.k)//fam.stride + 1
    return (B, C, weight.shape[0], *((ho, wo) if fam.out_dims else (H, W))), (ho, wo)


def _launch(fam, entry, a, b, out, nws, dims, pieces):
    """`entry` into `out` (returned) on a workspace of its own (`nws` None: the entry point takes none)."""
    ws = () if nws is None else _workspace(out.device, nws, floor=256)
    call(entry, a.data_ptr(), b.data_ptr(), out.data_ptr(), *((ws[0].data_ptr(), ws[1]) if ws else ()), *dims, *((pieces,) if fam.pieces_arg else ()), _stream())
    return out


def _forward(ctx, fam, x, weight, pieces=3, force=False):
    """The forward of every routed family on checked tensors: the kernels (the pack included) or the reference as `serve` says; leaves on `ctx` what
    `_backward` reads.  bfloat16 tensors: one piece, routed under the `_bf16` names."""
    bf = x.dtype == _BF
    if bf: fam, pieces = _BF16, 1
    dims, (ho, wo) = _dims(fam, x, weight)
    B, C, CO = dims[:3]
    nws = nwd = getattr(_lib.lib, fam.query)(*dims)          # (0: sizes the kernels do not take — the reference serves every operator)
    if fam.query_data: nwd = getattr(_lib.lib, fam.query_data)(*dims) if ctx.needs_input_grad[0] else 0
    sv = _served(C, CO, fam is _ZPAD, force or nws > 0) if fam.stride == 1 else _Served(nws > 0, fam.ops[1] is not None and nwd > 0, nws > 0, False, True)
    if force and not sv.fwd:
        raise _lib.Unsupported(f'the MFMA forward serves C % 16 == 0 with CO % 32 == 0{"" if fam is _ZPAD else ", or CO = 16 with C = 16 | 32"}, not C={C} CO={CO}')
    # The data gradient's operand image rides in the forward's pack launch.  The stride-2 layers: only where the backward may read it and the kernels are
    # known to serve this forward, so that the forward's own A/B times the forward's pack alone (the second image costs 2 - 12 us, profiles/s2_data_convs.txt)
    want_bwd = sv.data
    if fam is _S2: want_bwd = nwd > 0 and may_serve((fam.ops[1], *dims)) and may_serve((fam.ops[0], *dims), unknown=False)
    y = torch.empty((B, CO, ho, wo), device=x.device, dtype=x.dtype)
    packed = {}

    def run_mfma():                                          # the pack included: production pays it on every call, so the A/B times it too
        wf, packed['wb'] = fam.pack(weight, C, CO, pieces, True, want_bwd)
        return _launch(fam, fam.entries[0], x, wf, y, nws if fam.fwd_ws else None, dims, pieces)

    def run_ref():
        if sv.thin and not bf: call('smd_conv3x3_thin_fwd', x.data_ptr(), weight.data_ptr(), y.data_ptr(), B, C, ho, wo, _stream()); return y
        return torch.conv2d(x, weight.to(_BF) if bf else weight, None, fam.stride, fam.pad)
    out = serve((fam.ops[0], *dims), run_mfma, run_ref, eligible=sv.fwd and sv.sized, force=force)
    ctx.save_for_backward(x, weight, packed.get('wb'))
    ctx.plan = dict(fam=fam, pieces=pieces, force=force, sv=sv, nws=nws, nwd=nwd)
    return out


def _backward(x, weight, wp_bwd, g_y, need_x, need_w, *, fam, pieces, force, sv, nws, nwd, deterministic_ref=False):
    """(g_x, g_w) of every routed family for dL/dy = g_y, None where not needed: each operator on the MFMA kernels or its reference, as `serve` says.
    `wp_bwd`: the data gradient's operand image where the forward's pack made it (else it is packed here, inside the timed call).  `deterministic_ref`: where
    MIOpen serves an operator it is asked for its deterministic solvers (left to itself it may pick one that accumulates with atomics: other bits on every run)."""
    _on(x)
    dims, (ho, wo) = _dims(fam, x, weight)
    B, C, CO = dims[:3]
    bf = x.dtype == _BF
    g_y = _check_fb('grad(y)', g_y.to(x.dtype), (B, CO, ho, wo))
    g_x = g_w = None
    w_ref = weight.to(_BF) if bf else weight

    def cb(mask):
        aten = lambda: torch.ops.aten.convolution_backward(g_y, x, w_ref, None, [fam.stride]*2, [fam.pad]*2, [1, 1], False, [0, 0], 1, mask)
        if not deterministic_ref: return aten()
        # ONLY `torch.backends.cudnn.deterministic` is set, and restored (`torch.backends.cudnn.flags(...)` would also switch `enabled` off and with it
        # MIOpen itself: ATen's im2col fallback would serve the call)
        det, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
        try: return aten()
        finally: torch.backends.cudnn.deterministic = det
    thin_ref = sv.thin and not bf                            # (the last stage in fp32: the reference is the f32-MFMA kernel)
    if need_x:                                               # (the stem: no kernel, not eligible — `serve` hands it straight to ATen and caches no route)
        ok = sv.data and sv.sized
        g_x = torch.empty_like(x) if ok else None
        packed = {'wb': wp_bwd}

        def run_data():                                      # (MIOpen served the forward, or the route was not known then: the pack is paid here)
            if packed['wb'] is None: packed['wb'] = fam.pack(weight, C, CO, pieces, False, True)[1]
            return _launch(fam, fam.entries[1], g_y, packed['wb'], g_x, nwd, dims, pieces)
        ref_data = (lambda: _thin_bwd(x, weight, g_y, True, False)[0]) if thin_ref else (lambda: cb([True, False, False])[0])
        g_x = serve((fam.ops[1], *dims), run_data, ref_data, eligible=ok, force=force)
    if need_w:
        ok = sv.wgt and sv.sized
        g_w = torch.empty_like(weight) if ok else None
        run_wgt = lambda: _launch(fam, fam.entries[2], x, g_y, g_w, nws, dims, pieces)
        ref_wgt = (lambda: _thin_bwd(x, weight, g_y, False, True)[1]) if thin_ref else (lambda: cb([False, True, False])[1].float())
        g_w = serve((fam.ops[2], *dims), run_wgt, ref_wgt, eligible=ok, force=force)
    return g_x, g_w


def _ctx_backward(ctx, g_y):
    x, weight, wp_bwd = ctx.saved_tensors
    return _backward(x, weight, wp_bwd, g_y, *ctx.needs_input_grad[:2], **ctx.plan)


def conv3x3_wide_backward(xp, weight, g_y, *, need_x, need_w, deterministic_ref=False):
    """(g_xp, g_w) of `conv3x3_wide(xp, weight)` for a dL/dy made elsewhere, without its forward: the tail of `ddv_ops.ddv_head`'s backward, whose dL/dy is
    the recomputed logit gradient."""
    dims, _ = _dims(_PADDED, xp, weight)
    nws = _lib.lib.smd_conv3x3_mfma_workspace_bytes(*dims)
    return _backward(xp, weight, None, g_y, need_x, need_w, fam=_PADDED, pieces=3, force=False, sv=_served(dims[1], dims[2], False, nws > 0), nws=nws, nwd=nws,
                     deterministic_ref=deterministic_ref)


class _Conv3x3Wide(torch.autograd.Function):
    """`F.conv2d(xp, weight (CO,C,3,3))` on an already reflection-padded input; each of the three operators (forward, data gradient, weight gradient) runs
    on the bf16 matrix cores (`smd_conv3x3_mfma_*`) or through the alternative — MIOpen, or for the 16-channel last stage in fp32 the f32-MFMA kernels
    `smd_conv3x3_thin_*` — as `conv_routing.serve` says (`force`: always the MFMA kernels).  fp32 tensors: every operand split into three bf16 pieces, fp32-class
    results.  bfloat16 tensors (bf16 autocast): one piece, bf16 in and out, the weights as their bf16 rounding, fp32 accumulation and an fp32 weight gradient.
    `zpad`: the zero-padded "same" layer on the UNPADDED x instead (`conv3x3_same`; fp32 only), routed under `fwd_z` / `data_z` / `wgt_z`."""
    @staticmethod
    def forward(ctx, xp, weight, pieces, force, zpad=False):
        xp = _check_fb('xp', xp)
        if zpad and xp.dtype != torch.float32: raise TypeError(f'the zero-padded convolution takes float32 tensors, got {xp.dtype}')
        if xp.ndim != 4 or (not zpad and (xp.shape[2] < 3 or xp.shape[3] < 3)):
            raise ValueError(f'expected {"(B,C,h,w)" if zpad else "a padded (B,C,h+2,w+2)"}, got {tuple(xp.shape)}')
        return _forward(ctx, _ZPAD if zpad else _PADDED, xp, _check_weight(weight, xp.shape[1], 3), pieces, force)

    @staticmethod
    def backward(ctx, g_y): return (*_ctx_backward(ctx, g_y), None, None, None)


def _check_weight(weight, C, k):
    if weight.ndim != 4 or tuple(weight.shape[1:]) != (C, k, k): raise ValueError(f'weight: expected (CO,{C},{k},{k}), got {tuple(weight.shape)}')
    return _check('weight', weight, (weight.shape[0], C, k, k))


def conv3x3_mfma(xp, weight, pieces: int = 3):
    """`F.conv2d(xp, weight)` for an input that is already reflection-padded, ALWAYS through the split-bf16 MFMA kernels (`smd_conv3x3_mfma_*`): the wide
    up-convolutions of the decoder (src/networks/decoders/monodepth.py:40-50, 71-84), bias-free (the next glue kernel adds it).  xp (B,C,h+2,w+2) fp32,
    weight (CO,C,3,3) fp32 -> (B,CO,h,w) fp32; C % 16 == 0 and CO % 32 == 0, or the thin stage CO = 16 with C = 16 | 32 (`_lib.Unsupported` otherwise).  Every fp32 operand is split exactly into three
    bf16 pieces and six products are kept per fp32 product (`pieces=3`: fp32-class error, see csrc/smd_conv_mfma.hip; `pieces=2` is an experiment setting)."""
    return _Conv3x3Wide.apply(xp, weight, int(pieces), True)


def conv3x3_wide(xp, weight):
    """The same convolution, each operator through whichever of the MFMA kernels and MIOpen won this box's A/B for its shape (`conv_routing.serve`)."""
    return _Conv3x3Wide.apply(xp, weight, 3, False)


def conv3x3_same(x, weight):
    """`F.conv2d(x, weight (CO,C,3,3), padding=1)`, bias-free, zero padding: the ResNet encoders' 3x3 stride-1 convolutions (the timm blocks built at
    src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,h,w) fp32 -> (B,CO,h,w) fp32.  Each operator runs on the split-bf16 MFMA kernels
    (`smd_conv3x3z_mfma_*`, the padding done inside them) or MIOpen, as `conv_routing.serve` says under `fwd_z` / `data_z` / `wgt_z`
    (`set_conv_route('mfma')` pins the kernels); channel counts or sizes the kernels do not take go to MIOpen."""
    return _Conv3x3Wide.apply(x, weight, 3, False, True)


class _Conv7x7s2Stem(torch.autograd.Function):
    """`conv7x7s2_stem`.  The input is normally the image; a data gradient, where asked for, is ATen's."""
    @staticmethod
    def forward(ctx, x, weight):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (B,C,H,W), got {tuple(x.shape)}')
        return _forward(ctx, _STEM, x, _check_weight(weight, x.shape[1], 7))

    @staticmethod
    def backward(ctx, g_y): return _ctx_backward(ctx, g_y)


def conv7x7s2_stem(x, weight):
    """`F.conv2d(x, weight (CO,C,7,7), stride=2, padding=3)`, bias-free: the ResNet encoders' stem (`conv1` of the timm ResNets built at
    src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,H,W) fp32 -> (B,CO,(H-1)//2+1,(W-1)//2+1) fp32.  CO = 64 with C = 3 or 6: forward and
    weight gradient on the split-bf16 MFMA kernels (`smd_conv7x7s2_*`) or MIOpen, per operator and shape (`conv_routing.serve`, ops `fwd_s` / `wgt_s`;
    `set_conv_route('mfma')` pins the kernels); any other channel count goes to MIOpen."""
    return _Conv7x7s2Stem.apply(x, weight)


class _Conv3x3s2(torch.autograd.Function):
    """`conv3x3_s2`.  Each of the three operators on the kernels or MIOpen as `serve` says (ops `fwd_s2`, `data_t2`, `wgt_s2`)."""
    @staticmethod
    def forward(ctx, x, weight):
        x = _check('x', x)
        if x.ndim != 4: raise ValueError(f'expected (B,C,H,W), got {tuple(x.shape)}')
        return _forward(ctx, _S2, x, _check_weight(weight, x.shape[1], 3))

    @staticmethod
    def backward(ctx, g_y): return _ctx_backward(ctx, g_y)


def conv3x3_s2(x, weight):
    """`F.conv2d(x, weight (CO,C,3,3), stride=2, padding=1)`, bias-free: `conv1` of the first BasicBlock of layer2 / layer3 / layer4 of the ResNet encoders
    (the timm blocks built at src/networks/depth.py:95-98, src/networks/pose.py:39-41).  x (B,C,H,W) fp32 -> (B,CO,(H-1)//2+1,(W-1)//2+1) fp32.  C % 16 == 0
    with CO % 32 == 0: forward, data gradient and weight gradient on the split-bf16 MFMA kernels (`smd_conv3x3s2_mfma_*`, `smd_conv3x3s2d_mfma_bwd_data`, the
    zero padding done inside them) or MIOpen, per operator and shape (`conv_routing.serve`, ops `fwd_s2` / `data_t2` / `wgt_s2`; `set_conv_route('mfma')`
    pins the kernels); any other channel count goes to MIOpen."""
    return _Conv3x3s2.apply(x, weight)
