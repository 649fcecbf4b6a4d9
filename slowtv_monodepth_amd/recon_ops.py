"""The loss path as `torch.autograd.Function`s: disparity -> depth, the fused image reconstruction (fed by a depth stack, by the disparity pyramid, or as one
node with the smoothness term), the fused smoothness term, and the frame-only preparation they share.  `functional` re-exports the wrappers."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._device import _aligned, _check, _on, _ptr, _ptrs, _stream, _workspace, call
from ._lib import FLAGS, int_array
from .class_ops import crop_resize
from .geom_ops import inv_intrinsics
from .row_skip import row_skip_tuner


def recon_flags(loss_name: str = 'ssim', use_min: bool = False, use_automask: bool = False) -> int:
    if loss_name not in ('ssim', 'l1'): raise NotImplementedError(f"fused image reconstruction supports loss_name 'ssim'|'l1', not {loss_name!r}")
    return (FLAGS['use_min'] if use_min else 0) | (FLAGS['use_automask'] if use_automask else 0) | (FLAGS['loss_l1'] if loss_name == 'l1' else 0)


def _depth_range(min_depth, max_depth):
    """Validate the range `to_scaled` maps the disparity into -> the (min, max) floats the C calls take (0: not given)."""
    if min_depth is not None and min_depth <= 0: raise ValueError(f'Min depth must be greater than 0. ({min_depth})')
    if max_depth and min_depth and max_depth < min_depth: raise ValueError(f'Max depth must be greater than min. ({max_depth} vs. {min_depth})')
    return float(min_depth or 0), float(max_depth or 0)


def _check_disps(disps, b):
    """-> (the disparity pyramid as checked contiguous tensors, their heights, their widths)."""
    disps = [_check(f'disp[{i}]', d) for i, d in enumerate(disps)]
    for d in disps:
        if d.ndim != 4 or d.shape[0] != b or d.shape[1] != 1: raise ValueError(f'disparities must be (b,1,hs,ws), got {tuple(d.shape)}')
    return disps, [d.shape[2] for d in disps], [d.shape[3] for d in disps]


def _default_K_inv(Ks, K_inv):
    """`K_inv`, or where it is None the inverse of `Ks`: torch's where a gradient has to reach `Ks` (`ViewSynth.forward`, src/tools/geometry.py:383), else one launch."""
    if K_inv is not None: return K_inv
    return torch.linalg.inv(Ks) if Ks.requires_grad else inv_intrinsics(Ks)


class _DispToDepth(torch.autograd.Function):
    """K0: per-scale bilinear upsample + `to_scaled`/`to_inv` (src/core/trainer.py:316-321)."""

    @staticmethod
    def forward(ctx, size, mn, mx, want_disp_up, *disps):
        h, w = size
        b = disps[0].shape[0]
        disps, hs, ws = _check_disps(disps, b)
        S = len(disps)
        depth_up = torch.empty((S, b, 1, h, w), device=disps[0].device, dtype=torch.float32)
        disp_up = torch.empty_like(depth_up) if want_disp_up else None
        call('smd_disp_to_depth_fwd', _ptrs(disps), int_array(hs), int_array(ws), S, b, h, w, mn, mx, depth_up.data_ptr(), _ptr(disp_up), _stream())
        ctx.save_for_backward(depth_up)
        ctx.meta = (hs, ws, S, b, h, w, mn, mx)
        if want_disp_up: ctx.mark_non_differentiable(disp_up)
        return depth_up, disp_up

    @staticmethod
    def backward(ctx, g_depth_up, _g_disp_up):
        (depth_up,) = ctx.saved_tensors
        _on(depth_up)
        hs, ws, S, b, h, w, mn, mx = ctx.meta
        g_depth_up = _check('grad(depth_up)', g_depth_up)
        g_disps = [torch.empty((b, 1, hs[s], ws[s]), device=depth_up.device, dtype=torch.float32) for s in range(S)]
        hs_a, ws_a = int_array(hs), int_array(ws)
        wsp, nbytes = _workspace(depth_up.device, _lib.lib.smd_disp_to_depth_workspace_bytes, hs_a, ws_a, S, b, h, w)
        call('smd_disp_to_depth_bwd', hs_a, ws_a, S, b, h, w, mn, mx, depth_up.data_ptr(), g_depth_up.data_ptr(), _ptrs(g_disps), wsp.data_ptr(), nbytes, _stream())
        return (None, None, None, None, *g_disps)


def disp_to_depth(disps, size, min_depth=None, max_depth=None, want_disp_up=False):
    """disps: sequence of (b,1,hs,ws) -> depth_up (S,b,1,h,w) [, disp_up (S,b,1,h,w)] in one launch."""
    mn, mx = _depth_range(min_depth, max_depth)
    return _DispToDepth.apply(tuple(int(x) for x in size), mn, mx, bool(want_disp_up), *disps)


_PREP_FLAGS = FLAGS['use_min'] | FLAGS['use_automask'] | FLAGS['loss_l1']
_FramesKey = namedtuple('_FramesKey', 'imgs_ptr supp_ptr imgs_shape supp_shape flags hs ws')


def _frames_key(imgs, supp_imgs, flags, hs, ws) -> _FramesKey:
    """What a `PreparedFrames` was built for: the frames (by address and shape), the criterion's flags and the disparity pyramid (hs, ws: None without one)."""
    return _FramesKey(imgs.data_ptr(), supp_imgs.data_ptr(), tuple(imgs.shape), tuple(supp_imgs.shape), int(flags) & _PREP_FLAGS,
                      tuple(hs) if hs is not None else None, tuple(ws) if ws is not None else None)


class PreparedFrames:
    """What the loss path needs from the FRAMES alone: the packed texel / target-window buffer of the reconstruction forward
    (`smd_image_recon_prep`), optionally the edge weights of the smoothness term for the same pyramid (`smd_disp_smooth_prep`), the HIP
    event after which they are complete, and what they were built for.  None of it depends on a network output, so the training step
    fills it on a side stream while the networks run (`MonoDepthModule.step`)."""
    def __init__(self, packed, event, key, edge_w=None):
        self.packed, self.event, self.key, self.edge_w = packed, event, key, edge_w

    def edges_for(self, imgs, hs, ws):
        """The edge-weight buffer if it was built for this frame and pyramid, else None."""
        k = self.key
        if self.edge_w is None or k.imgs_ptr != imgs.data_ptr() or k.imgs_shape != tuple(imgs.shape): return None
        return self.edge_w if (k.hs == tuple(hs) and k.ws == tuple(ws)) else None

    def matches(self, imgs, supp_imgs, flags, hs, ws) -> bool:
        return _frames_key(imgs, supp_imgs, flags, hs, ws) == self.key


def image_recon_prep(imgs, supp_imgs, *, flags: int, pyramid=None, stream=None, smooth_edges: bool = False) -> PreparedFrames:
    """Fill the frame-only buffer of the fused reconstruction for (imgs (b,3,h,w), supp_imgs (n,b,3,h,w)).

    :param flags: `recon_flags(...)` of the criterion that will consume it (the identity error of the automask is part of it).
    :param pyramid: [(hs, ws), ...] of the disparity pyramid when the K0-fused forward follows (its row table is built here).
    :param stream: `torch.cuda.Stream` to run on (default: the current one).  The returned object carries the completion event;
        the forward that consumes it waits for that event on ITS stream.
    :param smooth_edges: also compute the edge weights of `SmoothReg(use_edges=True)` for `pyramid` (`disp_smooth_fused(prepared=...)`)."""
    b, _, h, w = imgs.shape
    n = supp_imgs.shape[0]
    imgs_c = _check('imgs', imgs, (b, 3, h, w)); supp_c = _check('supp_imgs', supp_imgs, (n, b, 3, h, w))
    dev = imgs.device
    cur = torch.cuda.current_stream(dev)
    st = stream if stream is not None else cur
    hs = [int(p[0]) for p in pyramid] if pyramid else None
    ws = [int(p[1]) for p in pyramid] if pyramid else None
    if st is not cur: st.wait_stream(cur)          # the frames were produced on the caller's stream
    with torch.cuda.stream(st):
        packed = torch.empty(_lib.lib.smd_packed_supports_bytes(b, n, h, w)//4, device=dev, dtype=torch.float32)    # padded RGB texels of the supports + the target's SSIM window sums
        call('smd_image_recon_prep', imgs_c.data_ptr(), supp_c.data_ptr(), packed.data_ptr(), int_array(hs) if hs else None, int_array(ws) if ws else None,
             len(hs) if hs else 0, b, n, h, w, int(flags) & _PREP_FLAGS, st.cuda_stream)
        edge_w = None
        if smooth_edges and hs:
            hs_a, ws_a = int_array(hs), int_array(ws)
            edge_w, _ = _workspace(dev, _lib.lib.smd_disp_smooth_edge_weight_bytes, hs_a, ws_a, len(hs), b)
            call('smd_disp_smooth_prep', imgs_c.data_ptr(), hs_a, ws_a, len(hs), b, h, w, FLAGS['use_edges'], edge_w.data_ptr(), st.cuda_stream)
        event = torch.cuda.Event()
        event.record(st)
    if st is not cur:
        for t in (imgs_c, supp_c): t.record_stream(st)
        packed.record_stream(cur)
        if edge_w is not None: edge_w.record_stream(cur)
    return PreparedFrames(packed, event, _frames_key(imgs, supp_imgs, flags, hs, ws), edge_w)


def _packed_for(prepared, imgs, supp, flags, hs, ws, b, n, h, w, dev):
    """-> (packed buffer, flags): the prepared one (after waiting for it on the current stream) or a fresh one for an inline prep."""
    if prepared is not None:
        if not prepared.matches(imgs, supp, flags, hs, ws):
            raise ValueError('PreparedFrames were built for other frames, flags or another disparity pyramid')
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(prepared.event)
        prepared.packed.record_stream(cur)      # allocated on the stream that filled it, used (and later freed) on this one
        return prepared.packed, int(flags) | FLAGS['packed_ready']
    return torch.empty(_lib.lib.smd_packed_supports_bytes(b, n, h, w)//4, device=dev, dtype=torch.float32), int(flags)


def _edge_weights(prepared, img, hs, ws, hs_a, ws_a, S, b, dev, wait: bool):
    """-> (edge weights of the smoothness term, FLAGS['edges_ready'] or 0).  They depend on the frame alone: `prepared`'s when it carries them for this frame and pyramid
    (`wait`: its event has not been waited for on this stream yet), otherwise a fresh buffer that the forward call fills first.  The backward reads them instead of the image."""
    ew = prepared.edges_for(img, hs, ws) if prepared is not None else None
    if ew is None: return _workspace(dev, _lib.lib.smd_disp_smooth_edge_weight_bytes, hs_a, ws_a, S, b)[0], 0
    cur = torch.cuda.current_stream(dev)
    if wait: cur.wait_event(prepared.event)
    ew.record_stream(cur)
    return ew, FLAGS['edges_ready']


def supports_per_pass() -> int:
    """Supports the fused reconstruction kernels take in one pass (more: passes carrying the running minimum; the single-node loss path: unsupported)."""
    return int(_lib.lib.smd_image_recon_supports_per_pass())


def _stale_table(ctx) -> int:
    """FLAGS['bwd_no_live'] when a launch-shape knob changed since the forward that filled the liveness table of this node's packed buffer: the backward
    re-derives the forward's strip partition from the knobs in force when it runs, and a table read with another partition calls live waves dead."""
    return FLAGS['bwd_no_live'] if getattr(ctx, 'knob_epoch', _lib.knob_epoch) != _lib.knob_epoch else 0


def _recon_outputs(dev, S, b, n, h, w, want_err, want_warp):
    """-> (err|None, sel, loss, warp0|None, the outputs to mark non-differentiable) of a reconstruction forward.  (With `want_warp` that is warp0 alone, as it
    has been: `err` then carries a grad_fn whose gradient the backward ignores; `sel` is uint8 either way.)"""
    err = torch.empty((S, b, 1, h, w), device=dev, dtype=torch.float32) if (want_err or n > supports_per_pass()) else None
    sel = torch.empty((S, b, 1, h, w), device=dev, dtype=torch.uint8)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    warp0 = torch.empty((n, b, 3, h, w), device=dev, dtype=torch.float32) if want_warp else None
    return err, sel, loss, warp0, ((warp0,) if want_warp else (sel,) if err is None else (err, sel))


def _recon_ctx(ctx, meta, need_k, nondiff, materialize: bool = True) -> None:
    """What every reconstruction forward leaves for its backward, next to the saved tensors (`need_k`: the intrinsics want a gradient; `knob_epoch`: see `_stale_table`)."""
    ctx.meta, ctx.need_k, ctx.knob_epoch = meta, bool(need_k), _lib.knob_epoch
    if not materialize: ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(*nondiff)


def _pose_k_grads(ctx, n, b, dev):
    """-> (g_T, g_K|None, g_Ki|None, FLAGS['need_k_grad'] or 0) of a reconstruction backward."""
    g_T = torch.empty((n, b, 4, 4), device=dev, dtype=torch.float32)
    g_K, g_Ki = (torch.empty((b, 4, 4), device=dev, dtype=torch.float32), torch.empty((b, 4, 4), device=dev, dtype=torch.float32)) if ctx.need_k else (None, None)
    return g_T, g_K, g_Ki, (FLAGS['need_k_grad'] if ctx.need_k else 0)


def _recon_bwd_call(ctx, dev, name, *args, flags: int) -> None:
    """`call(name, *args, flags, stream)` of a reconstruction backward: the flags completed by the row loop the device's tuner asks for and by `_stale_table`,
    the tuner's timing events around the call (no end event if it raises)."""
    tuner = row_skip_tuner(dev); tflag, token = tuner.begin(dev)
    call(name, *args, flags | tflag | _stale_table(ctx), _stream())
    tuner.end(token)


class _ImageRecon(torch.autograd.Function):
    """Fused `handlers.image_recon` (src/core/handlers.py:14-67)."""

    @staticmethod
    def forward(ctx, depth, tgt, supp, T, K, K_inv, noise, seed, flags, want_warp, want_err, prepared):
        S, b, h, w = depth.shape  # always 4-D here: `image_recon_fused` squeezes the channel dim as an autograd view
        n = supp.shape[0]
        tgt_in, supp_in = tgt, supp
        depth = _check('depth', depth, (S, b, h, w)); tgt = _check('imgs', tgt, (b, 3, h, w)); supp = _check('supp_imgs', supp, (n, b, 3, h, w))
        T = _check('Ts', T, (n, b, 4, 4)); K = _check('Ks', K, (b, 4, 4)); K_inv = _check('K_inv', K_inv, (b, 4, 4))
        if noise is not None: noise = _check('noise', noise.reshape(S, b, h, w), (S, b, h, w))
        dev = depth.device
        err, sel, loss, warp0, nondiff = _recon_outputs(dev, S, b, n, h, w, want_err, want_warp)
        ws, nbytes = _workspace(dev, _lib.lib.smd_image_recon_workspace_bytes, b, n, S, h, w)
        supp_pk, cflags = _packed_for(prepared, tgt_in, supp_in, flags, None, None, b, n, h, w, dev)
        call('smd_image_recon_fwd', depth.data_ptr(), tgt.data_ptr(), supp.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(), _ptr(noise), int(seed) & (2**64 - 1),
             supp_pk.data_ptr(), _ptr(err), sel.data_ptr(), loss.data_ptr(), _ptr(warp0), ws.data_ptr(), nbytes, b, n, S, h, w, cflags, _stream())
        ctx.save_for_backward(depth, tgt, supp_pk, T, K, K_inv, sel)
        _recon_ctx(ctx, (b, n, S, h, w, int(flags)), ctx.needs_input_grad[4] or ctx.needs_input_grad[5], nondiff)
        return loss, err, sel, warp0

    @staticmethod
    def backward(ctx, g_loss, *_):
        depth, tgt, supp_pk, T, K, K_inv, sel = ctx.saved_tensors
        b, n, S, h, w, flags = ctx.meta
        dev = _on(depth)
        g_loss = _aligned(g_loss.to(torch.float32))
        g_depth = torch.empty((S, b, h, w), device=dev, dtype=torch.float32)
        g_T, g_K, g_Ki, kflag = _pose_k_grads(ctx, n, b, dev)
        ws, nbytes = _workspace(dev, _lib.lib.smd_image_recon_workspace_bytes, b, n, S, h, w)
        _recon_bwd_call(ctx, dev, 'smd_image_recon_bwd', depth.data_ptr(), tgt.data_ptr(), supp_pk.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(),
                        sel.data_ptr(), g_loss.data_ptr(), g_depth.data_ptr(), g_T.data_ptr(), _ptr(g_K), _ptr(g_Ki), ws.data_ptr(), nbytes, b, n, S, h, w, flags=flags | kflag)
        return g_depth, None, None, g_T, (g_K if ctx.needs_input_grad[4] else None), (g_Ki if ctx.needs_input_grad[5] else None), None, None, None, None, None, None


def image_recon_fused(depth, imgs, supp_imgs, Ts, Ks, K_inv=None, *, flags: int, noise=None, seed: int = 0, want_warp: bool = False,
                      want_err: bool = True, prepared: PreparedFrames | None = None):
    """depth (S,b,1,h,w)|(S,b,h,w); returns (loss, err (S,b,1,h,w)|None, sel uint8 (S,b,1,h,w), warp0 (n,b,3,h,w)|None).

    `want_err=False` (the handlers' choice: nothing on the training path reads the error map) saves its store in the kernel.

    `K_inv=None` inverts `Ks` with torch (differentiable), as `ViewSynth.forward` does (src/tools/geometry.py:383).
    `prepared`: the frame-only buffer from `image_recon_prep(imgs, supp_imgs, flags=flags)` (built without `pyramid`)."""
    K_inv = _default_K_inv(Ks, K_inv)
    was5 = depth.ndim == 5
    d4 = depth.squeeze(2) if was5 else depth
    return _ImageRecon.apply(d4, imgs, supp_imgs, Ts, Ks, K_inv, noise, seed, flags, want_warp, want_err, prepared)


class _ImageReconDisp(torch.autograd.Function):
    """K0 fused into `handlers.image_recon`: from the network's multi-scale sigmoid disparity straight to
    the loss — `forward_postprocess`' up-sampling + `to_scaled` / `to_inv` (src/core/trainer.py:316-321) happens inside the fused
    kernel, which also writes `depth_up` for the backward and for `fwd['depth_up']`."""

    @staticmethod
    def forward(ctx, tgt, supp, T, K, K_inv, noise, seed, flags, want_warp, want_err, mn, mx, prepared, *disps):
        b, _, h, w = tgt.shape
        n, S = supp.shape[0], len(disps)
        tgt_in, supp_in = tgt, supp
        tgt = _check('imgs', tgt, (b, 3, h, w)); supp = _check('supp_imgs', supp, (n, b, 3, h, w)); T = _check('Ts', T, (n, b, 4, 4))
        K = _check('Ks', K, (b, 4, 4)); K_inv = _check('K_inv', K_inv, (b, 4, 4))
        disps, hs, ws = _check_disps(disps, b)
        if noise is not None: noise = _check('noise', noise.reshape(S, b, h, w), (S, b, h, w))
        dev = tgt.device
        depth_up = torch.empty((S, b, 1, h, w), device=dev, dtype=torch.float32)
        err, sel, loss, warp0, nondiff = _recon_outputs(dev, S, b, n, h, w, want_err, want_warp)
        wsp, nbytes = _workspace(dev, _lib.lib.smd_image_recon_workspace_bytes, b, n, S, h, w)
        packed, cflags = _packed_for(prepared, tgt_in, supp_in, flags, hs, ws, b, n, h, w, dev)
        call('smd_image_recon_disp_fwd', _ptrs(disps), int_array(hs), int_array(ws), S, mn, mx, tgt.data_ptr(), supp.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(),
             _ptr(noise), int(seed) & (2**64 - 1), packed.data_ptr(), depth_up.data_ptr(), _ptr(err), sel.data_ptr(), loss.data_ptr(), _ptr(warp0), wsp.data_ptr(), nbytes,
             b, n, h, w, cflags, _stream())
        ctx.save_for_backward(depth_up, packed, T, K, K_inv, sel)
        # `depth_up` is a differentiable output that usually has no other consumer: without materialize=False autograd would hand the backward
        # a materialised zero tensor for it (one more (S,b,h,w) read, and no dead-row skipping on the last support pass)
        _recon_ctx(ctx, (b, n, S, h, w, int(flags), hs, ws, mn, mx), ctx.needs_input_grad[3] or ctx.needs_input_grad[4], nondiff, materialize=False)
        return loss, err, sel, warp0, depth_up

    @staticmethod
    def backward(ctx, g_loss, _ge, _gs, _gw, g_depth_up):
        depth_up, packed, T, K, K_inv, sel = ctx.saved_tensors
        b, n, S, h, w, flags, hs, ws, mn, mx = ctx.meta
        dev = _on(depth_up)
        g_loss = _aligned((g_loss if g_loss is not None else torch.zeros((), device=dev)).to(torch.float32))
        if g_depth_up is not None: g_depth_up = _check('grad(depth_up)', g_depth_up.reshape(S, b, h, w), (S, b, h, w))
        g_disps = [torch.empty((b, 1, hs[s], ws[s]), device=dev, dtype=torch.float32) for s in range(S)]
        g_T, g_K, g_Ki, kflag = _pose_k_grads(ctx, n, b, dev)
        hs_a, ws_a = int_array(hs), int_array(ws)
        wsp, nbytes = _workspace(dev, _lib.lib.smd_image_recon_disp_workspace_bytes, hs_a, ws_a, S, b, n, h, w)
        _recon_bwd_call(ctx, dev, 'smd_image_recon_disp_bwd', hs_a, ws_a, S, mn, mx, depth_up.data_ptr(), packed.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(),
                        sel.data_ptr(), g_loss.data_ptr(), _ptr(g_depth_up), _ptrs(g_disps), g_T.data_ptr(), _ptr(g_K), _ptr(g_Ki), wsp.data_ptr(), nbytes, b, n, h, w,
                        flags=flags | kflag)
        return (None, None, g_T, (g_K if ctx.needs_input_grad[3] else None), (g_Ki if ctx.needs_input_grad[4] else None),
                None, None, None, None, None, None, None, None, *g_disps)


def image_recon_fused_disp(disps, imgs, supp_imgs, Ts, Ks, K_inv=None, *, flags: int, min_depth=None, max_depth=None, noise=None, seed: int = 0,
                           want_warp: bool = False, want_err: bool = True, prepared: PreparedFrames | None = None):
    """disps: sequence of (b,1,hs,ws) sigmoid disparities -> (loss, err|None, sel, warp0|None, depth_up (S,b,1,h,w)).

    The K0-fused form of `disp_to_depth` + `image_recon_fused`: one prep launch (or none with `prepared` =
    `image_recon_prep(imgs, supp_imgs, flags=flags, pyramid=[d.shape[-2:] for d in disps])`) and one fused launch that also reduces the loss."""
    mn, mx = _depth_range(min_depth, max_depth)
    K_inv = _default_K_inv(Ks, K_inv)
    return _ImageReconDisp.apply(imgs, supp_imgs, Ts, Ks, K_inv, noise, seed, flags, want_warp, want_err, mn, mx, prepared, *disps)


class _DispSmooth(torch.autograd.Function):
    """Fused `handlers.disp_smooth` (src/core/handlers.py:262-281) over every scale."""

    @staticmethod
    def forward(ctx, img, flags, keys, want_aux, prepared, *disps):
        b, _, h, w = img.shape
        img_in = img
        img = _check('imgs', img, (b, 3, h, w))
        disps, hs, ws = _check_disps(disps, b)
        S = len(disps)
        dev = img.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        stats = torch.empty((S, b, 2), device=dev, dtype=torch.float32)
        aux = want_aux and keys[0] == 0
        dg, ig = (torch.empty_like(disps[0]), torch.empty_like(disps[0])) if aux else (None, None)
        hs_a, ws_a, keys_a = int_array(hs), int_array(ws), int_array(keys)
        wsp, nbytes = _workspace(dev, _lib.lib.smd_disp_smooth_workspace_bytes, hs_a, ws_a, S, b, floor=256)
        ew, cflags = None, int(flags)
        if cflags & FLAGS['use_edges']:     # (prepared weights are first-order ones: not for the Laplacian form)
            ew, ready = _edge_weights(None if cflags & FLAGS['use_laplacian'] else prepared, img_in, hs, ws, hs_a, ws_a, S, b, dev, wait=True)
            cflags |= ready
        call('smd_disp_smooth_fwd', _ptrs(disps), hs_a, ws_a, keys_a, S, b, img.data_ptr(), h, w, cflags, loss.data_ptr(), stats.data_ptr(), _ptr(dg), _ptr(ig),
             _ptr(ew), wsp.data_ptr(), nbytes, _stream())
        ctx.save_for_backward(img, stats, ew, *disps)
        ctx.meta = (hs, ws, list(keys), S, b, h, w, int(flags))
        if aux: ctx.mark_non_differentiable(dg, ig)
        return loss, dg, ig

    @staticmethod
    def backward(ctx, g_loss, *_):
        img, stats, ew, *disps = ctx.saved_tensors
        _on(img)
        hs, ws, keys, S, b, h, w, flags = ctx.meta
        g_loss = _aligned(g_loss.to(torch.float32))
        g_disps = [torch.empty_like(d) for d in disps]
        call('smd_disp_smooth_bwd', _ptrs(disps), int_array(hs), int_array(ws), int_array(keys), S, b, img.data_ptr(), h, w, flags, stats.data_ptr(), _ptr(ew),
             g_loss.data_ptr(), _ptrs(g_disps), _stream())
        return (None, None, None, None, None, *g_disps)


def disp_smooth_fused(disps: dict, imgs, *, use_edges: bool = False, want_aux: bool = True, use_laplacian: bool = False, prepared: PreparedFrames | None = None):
    """disps {key: (b,1,hs,ws)} -> (loss, disp_grad|None, image_grad|None); aux maps are those of key 0.
    `use_laplacian`: second-order differences, `SmoothReg(use_laplacian=True)` (src/regularizers/smooth.py:33-48).
    `prepared`: `image_recon_prep(imgs, ..., pyramid=..., smooth_edges=True)` — its edge weights are used if they were built for `imgs` and
    this pyramid (silently ignored otherwise)."""
    keys = [int(k) for k in disps.keys()]
    flags = (FLAGS['use_edges'] if use_edges else 0) | (FLAGS['use_laplacian'] if use_laplacian else 0)
    return _DispSmooth.apply(imgs, flags, keys, want_aux, prepared, *disps.values())


class _LossPath(torch.autograd.Function):
    """`forward_loss` of the kbr configuration as ONE autograd node (round 5): `handlers.image_recon` (K0 fused) + `handlers.disp_smooth`
    (first-order, edge-aware) + the weighted sum (src/core/trainer.py:383-392, 436-437, 462-464), and in the backward the chain rule through
    the pose / intrinsics prologue (:250-262) when its leaves are given.  `smd_loss_path_fwd/_bwd`: 1 + 3 launches."""

    @staticmethod
    def forward(ctx, tgt, supp, T, K, K_inv, aa, t, invert, fs, cs, seed, flags, mn, mx, keys, prepared, w_rec, w_sm, *disps):
        b, _, h, w = tgt.shape
        n, S = supp.shape[0], len(disps)
        tgt_in, supp_in = tgt, supp
        tgt = _check('imgs', tgt, (b, 3, h, w)); supp = _check('supp_imgs', supp, (n, b, 3, h, w)); T = _check('Ts', T, (n, b, 4, 4))
        K = _check('Ks', K, (b, 4, 4)); K_inv = _check('K_inv', K_inv, (b, 4, 4))
        disps, hs, ws = _check_disps(disps, b)
        if aa is not None:
            aa = _check('aa', aa, (n*b, 3)); t = _check('t', t, (n*b, 3))
            if invert is not None:
                if invert.dtype != torch.uint8 or tuple(invert.shape) != (n*b,): raise ValueError('invert must be uint8 (n*b,)')
                invert = _aligned(invert)
        if fs is not None: fs = _check('fs', fs, (b, 2)); cs = _check('cs', cs, (b, 2))
        hs_a, ws_a, keys_a = int_array(hs), int_array(ws), int_array(keys)
        dev = tgt.device
        depth_up = torch.empty((S, b, 1, h, w), device=dev, dtype=torch.float32)
        sel = torch.empty((S, b, 1, h, w), device=dev, dtype=torch.uint8)
        loss3 = torch.empty(3, device=dev, dtype=torch.float32)
        stats = torch.empty((S, b, 2), device=dev, dtype=torch.float32)
        wsp, nbytes = _workspace(dev, _lib.lib.smd_loss_path_workspace_bytes, hs_a, ws_a, S, b, n, h, w, floor=256)
        packed, cflags = _packed_for(prepared, tgt_in, supp_in, flags, hs, ws, b, n, h, w, dev)
        ew, ready = _edge_weights(prepared, tgt_in, hs, ws, hs_a, ws_a, S, b, dev, wait=False)     # (the wait for `prepared.event` happened in _packed_for)
        call('smd_loss_path_fwd', _ptrs(disps), hs_a, ws_a, keys_a, S, mn, mx, tgt.data_ptr(), supp.data_ptr(), T.data_ptr(), K.data_ptr(), K_inv.data_ptr(),
             int(seed) & (2**64 - 1), packed.data_ptr(), ew.data_ptr(), depth_up.data_ptr(), sel.data_ptr(), loss3.data_ptr(), stats.data_ptr(), wsp.data_ptr(), nbytes,
             b, n, h, w, cflags | FLAGS['use_edges'] | ready, float(w_rec), float(w_sm), _stream())
        ctx.save_for_backward(depth_up, packed, T, K, K_inv, sel, stats, ew, aa, t, invert, fs, cs, *disps)
        total, l_rec, l_sm = loss3[0], loss3[1], loss3[2]
        _recon_ctx(ctx, (b, n, S, h, w, int(flags), hs, ws, list(keys), mn, mx, float(w_rec), float(w_sm)),
                   fs is not None or ctx.needs_input_grad[3] or ctx.needs_input_grad[4], (l_rec, l_sm, sel), materialize=False)
        return total, l_rec, l_sm, sel, depth_up

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2, _gs, g_depth_up):
        depth_up, packed, T, K, K_inv, sel, stats, ew, aa, t, invert, fs, cs, *disps = ctx.saved_tensors
        b, n, S, h, w, flags, hs, ws, keys, mn, mx, w_rec, w_sm = ctx.meta
        dev = _on(depth_up)
        if g_depth_up is not None: raise NotImplementedError('loss_path_fused: `depth_up` has another differentiable consumer; use image_recon_fused_disp + disp_smooth_fused')
        g_loss = _aligned((g_loss if g_loss is not None else torch.zeros((), device=dev)).to(torch.float32))
        g_disps = [torch.empty((b, 1, hs[s], ws[s]), device=dev, dtype=torch.float32) for s in range(S)]
        g_T, g_K, g_Ki, kflag = _pose_k_grads(ctx, n, b, dev)
        g_aa, g_t = (torch.empty_like(aa), torch.empty_like(t)) if aa is not None else (None, None)
        g_fs, g_cs = (torch.empty_like(fs), torch.empty_like(cs)) if fs is not None else (None, None)
        hs_a, ws_a, keys_a = int_array(hs), int_array(ws), int_array(keys)
        wsp, nbytes = _workspace(dev, _lib.lib.smd_loss_path_workspace_bytes, hs_a, ws_a, S, b, n, h, w, floor=256)
        _recon_bwd_call(ctx, dev, 'smd_loss_path_bwd', _ptrs(disps), hs_a, ws_a, keys_a, S, mn, mx, depth_up.data_ptr(), packed.data_ptr(), T.data_ptr(),
                        K.data_ptr(), K_inv.data_ptr(), sel.data_ptr(), stats.data_ptr(), ew.data_ptr(), g_loss.data_ptr(), w_rec, w_sm,
                        _ptr(aa), _ptr(t), _ptr(invert), _ptr(fs), _ptr(cs), _ptrs(g_disps), g_T.data_ptr(), _ptr(g_K), _ptr(g_Ki), _ptr(g_aa), _ptr(g_t), _ptr(g_fs), _ptr(g_cs),
                        wsp.data_ptr(), nbytes, b, n, h, w, flags=flags | FLAGS['use_edges'] | kflag)
        need = ctx.needs_input_grad
        return (None, None, (g_T if need[2] else None), (g_K if need[3] else None), (g_Ki if need[4] else None), g_aa, g_t, None, g_fs, g_cs,
                None, None, None, None, None, None, None, None, *g_disps)


def loss_path_fused(disps: dict, imgs, supp_imgs, Ts, Ks, K_inv=None, *, pose=None, intrinsics=None, flags: int, min_depth=None, max_depth=None,
                    seed: int = 0, w_recon: float = 1.0, w_smooth: float = 0.001, prepared: PreparedFrames | None = None):
    """`forward_loss` with `img_recon` + `disp_smooth(use_edges=True)` as one operator:
        -> (loss = w_recon*l_recon + w_smooth*l_smooth, l_recon, l_smooth, sel (S,b,1,h,w) uint8, depth_up (S,b,1,h,w)).

    disps {key: (b,1,hs,ws)} sigmoid disparities (key = the `s` of `loss_s / 2**s`); Ts (n,b,4,4), Ks (b,4,4) [, K_inv].
    `pose=(aa, t, invert)`: the (n*b,3) leaves `Ts` was built from with `pose_matrices` — then `Ts` is taken as a value and the backward hands the
    gradients to `aa` and `t` directly (no `pose_matrices` backward launch); likewise `intrinsics=(fs, cs)` for `Ks`, `K_inv` from `intrinsics`.
    Raises `_lib.Unsupported` for what the operator does not serve (see include/smd_hotpath.h); `depth_up` must not have another
    differentiable consumer."""
    mn, mx = _depth_range(min_depth, max_depth)
    aa, t, inv = pose if pose is not None else (None, None, None)
    fs, cs = intrinsics if intrinsics is not None else (None, None)
    if pose is not None: Ts = Ts.detach()
    if intrinsics is not None:
        if K_inv is None: raise ValueError('intrinsics=(fs, cs) goes with the K, K_inv that `functional.intrinsics(fs, cs, size)` returned')
        if pose is None:    # the intrinsics' chain rule rides on the pose chain's guest block (smd_loss_path_bwd): without it the backward would fail, after a forward that succeeded
            raise _lib.Unsupported('intrinsics=(fs, cs) needs pose=(aa, t, invert): pass K, K_inv alone and let autograd carry their gradients')
        Ks, K_inv = Ks.detach(), K_inv.detach()
    K_inv = _default_K_inv(Ks, K_inv)
    keys = [int(k) for k in disps.keys()]
    return _LossPath.apply(imgs, supp_imgs, Ts, Ks, K_inv, aa, t, inv, fs, cs, seed, flags, mn, mx, keys, prepared, w_recon, w_smooth, *disps.values())


class _Blur3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _check('x', x)
        if x.ndim < 2: raise ValueError(f'gaussian_blur3x3 needs (..., h, w), got {tuple(x.shape)}')
        h, w = x.shape[-2:]
        out = torch.empty_like(x)
        call('smd_gaussian_blur3x3', x.data_ptr(), out.data_ptr(), x.numel()//(h*w), h, w, 0, _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        _on(g)
        g = _check('grad', g)
        h, w = g.shape[-2:]
        gx = torch.empty_like(g)
        call('smd_gaussian_blur3x3', g.data_ptr(), gx.data_ptr(), g.numel()//(h*w), h, w, 1, _stream())
        return gx


def gaussian_blur3x3(x):
    """`kornia.filters.gaussian_blur2d(x, kernel_size=(3, 3), sigma=(1, 1))` (src/regularizers/smooth.py:21) on (..., h, w) float32: separable
    3-tap Gaussian, reflect border; differentiable (the backward is the transposed map).  h, w >= 2."""
    return _Blur3.apply(x)


def disp_smooth_blurred(disps: dict, imgs, *, use_edges: bool = False, want_aux: bool = True):
    """`handlers.disp_smooth` with `SmoothReg(use_blur=True)`, first-order form (src/regularizers/smooth.py:21, 71-97; handlers.py:262-281):
    per scale, the mean-normalised disparity and the resized image are blurred before the absolute differences are taken.

    Built from the launches that exist: the image is resized with `crop_resize` (crop = frame) and blurred; the disparity is blurred and then
    shifted by (mean(disp) - mean(blur(disp))) per sample — the fused sweep normalises its input by that input's own mean, only DIFFERENCES of
    the normalised field enter the loss, and with the shift the mean it divides by is mean(disp), so what it evaluates is
    |d blur(disp / mean(disp))| exactly as the reference orders it (the blur is linear).  -> (loss, disp_grad|None, image_grad|None)."""
    keys = [int(k) for k in disps.keys()]
    total, aux = 0., (None, None)
    H, W = imgs.shape[-2:]
    for i, (k, d) in enumerate(zip(keys, disps.values())):
        hs, ws = d.shape[-2:]
        img_s = imgs if (hs, ws) == (H, W) else crop_resize([imgs], (H, W), (hs, ws))[0][0]
        bd = gaussian_blur3x3(d)
        x = bd + (d.mean(dim=(2, 3), keepdim=True) - bd.mean(dim=(2, 3), keepdim=True))
        l, dg, ig = disp_smooth_fused({k: x}, gaussian_blur3x3(img_s), use_edges=use_edges, want_aux=want_aux and k == 0)
        total = total + l
        if k == 0: aux = (dg, ig)      # the reference returns the maps of scale KEY 0 (`ls[0][1]`, src/core/handlers.py:280), wherever it sits in the dict
    return total/len(keys), aux[0], aux[1]
