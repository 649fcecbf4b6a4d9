"""Every public operator in hostile memory (hostile_memory.py): operands in poisoned, guarded blocks, every `torch.empty` / `torch.empty_like` of the
operator modules served from the same arena.  Per case: a friendly run A (plain device tensors, allocator untouched), a hostile run B, then

    guards intact (nothing wrote outside a buffer)  |  B finite (nothing read poison: an unwritten output tile, a stale workspace, a read outside a tensor)
    B within the family's own bound of its fp64 / oracle reference  |  B bit-equal to A (the kernels are bit-reproducible: memory layout must not change a bit)

and the same again with every operand one ELEMENT off 16-byte alignment (`shift = 1`: 4 bytes for fp32, 2 for bf16; what a slice of a flat parameter bucket
looks like).  Every family takes option B of DESIGN.md §2 ("Caller pointers"): the host copies an operand whose base is not 16-byte aligned before the C call
(`_device._aligned`), so the shifted case proves bit-equality through that copy; the blocks the operators allocate themselves stay 16-byte aligned, as the
caching allocator's are and as the ABI requires.

What a hostile run does NOT see.  (1) At shift 1 the host's copy of a misaligned operand is a `clone()`, which the patch does not serve: the kernels then read
their operands from plain allocator memory again, so a read outside an OPERAND is caught by the aligned run only (outputs and workspaces stay in the arena at
both shifts).  (2) `scale_mean` keeps a persistent workspace (`class_ops._mean_ws`, `torch.zeros`, one per device and stream) whose arrival counter the kernel
leaves at zero; it is not served from the arena.  The runner empties that cache before every hostile run, so the run at least starts from a fresh buffer and not
from the friendly run's; a stale read inside it would read zeros, not poison.

No tolerance is introduced here: every bound below is a named constant taken from the family's existing parity test.  The references are composed as those tests
compose them, computed once per case and shared by both shifts.  Pinned: the routed convolutions to the MFMA kernels, the fused backward's row loop
(`SMD_BWD_SKIP=0`, as test_gpu_parity.py pins it)."""
import contextlib
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

import conv_exact as X
from conftest import load_golden, rel_to_max
from hostile_memory import Arena, assert_finite, hostile

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# ---- bounds, each from the existing test named next to it (rel: max |a - b| / max |b| as conftest.rel_to_max; close: torch.testing.assert_close) ----------
rel = lambda bound: ('rel', bound)
close = lambda rtol, atol: ('close', rtol, atol)
EQUAL = ('equal',)
TOL_CONV_F32 = rel(2e-6)             # test_conv3x3_head_kernel / _thin_kernel / _mfma_kernel, test_conv3x3_headn_kernel, test_gpu_encoder_conv.py, test_gpu_stem_conv.py
TOL_BF16_OUT = rel(4e-3)             # test_conv3x3_mfma_bf16_tensors, test_conv3x3_head_bf16_activation: half an ulp of bf16
TOL_BF16_WGRAD = rel(1e-5)           # test_conv3x3_mfma_bf16_tensors: the fp32 weight gradient of the bf16 form
TOL_GLUE_OUT = close(1e-6, 1e-6)     # test_elu_pad_kernel, test_elu_up_cat_pad_kernel: outputs
TOL_GLUE_GX = close(1e-5, 1e-6)      # test_elu_pad_kernel: g_x; test_elu_up_cat_pad_kernel: g_skip
TOL_GLUE_GA = close(1e-5, 1e-5)      # test_elu_up_cat_pad_kernel: g_a
TOL_GLUE_BIAS = rel(1e-5)            # test_decoder_glue_with_bias: everything with a bias
TOL_GLUE_BF16 = rel(3e-2)            # test_decoder_glue_bf16_io
TOL_BN = rel(2e-5)                   # test_batch_norm_act_kernel
TOL_POOL_GX = close(1e-6, 1e-6)      # test_max_pool_kernel (values: exact)
TOL_DWCONV = rel(2e-5)               # test_depthwise_conv7x7_kernel
TOL_LN = rel(3e-5)                   # test_channel_layer_norm_kernel
TOL_LN_BF16_OUT, TOL_LN_BF16_GRAD = rel(1e-2), rel(2e-2)    # test_channel_layer_norm_bf16_io
TOL_UP_OUT, TOL_UP_GRAD = close(0, 1e-6), rel(2e-6)         # test_upsample_stack_matches_interpolate_and_its_adjoint
TOL_MEAN_LOSS, TOL_MEAN_GRAD = close(1e-6, 0), rel(2e-6)    # test_scale_mean_matches_fp64
# test_strip_boundary_shapes_match_oracle: selection flips, the error map off the flips, the loss, the gradients without / with a flip
SWEEP_FLIPS, SWEEP_ERR_ATOL, SWEEP_LOSS, SWEEP_GRAD, SWEEP_GRAD_FLIPPED = 0.01, 3e-4, close(1e-4, 1e-6), 2e-3, 5e-2
TOL_K0_DEPTH, TOL_K0_GRAD, TOL_K0_LOSS = close(2e-5, 1e-5), rel(1e-3), close(2e-5, 1e-7)    # test_k0_and_smoothness_at_non_integer_ratios
TOL_VS_WARP, TOL_VS_DWARP, TOL_VS_GRAD = close(0, 1e-4), close(1e-5, 1e-5), rel(1e-3)       # test_view_synth_operator_matches_reference
TOL_PHOTO_ERR, TOL_PHOTO_GRAD, TOL_PHOTO_GRAD_C = close(1e-5, 2e-6), close(2e-4, 2e-5), rel(2e-4)   # test_photo_error_operator_matches_reference, test_generic_channel_photo_errors
TOL_MASKED_LOSS, TOL_MASKED_GRAD = close(2e-5, 1e-7), rel(1e-3)                              # test_masked_reconstruction_loss
TOL_REGR, TOL_REGR_GRAD = close(2e-6, 1e-7), close(2e-5, 1e-8)                               # test_regression_loss_matches_reference
TOL_POSE_T, TOL_POSE_GAA, TOL_POSE_GT = close(1e-5, 1e-6), close(1e-4, 2e-5), close(1e-5, 1e-6)   # test_inverted_pose_matches_general_inverse
TOL_K, TOL_KINV, TOL_K_GRAD = close(1e-6, 1e-6), close(1e-5, 1e-7), close(1e-4, 1e-5)        # test_intrinsics_match_oracle
TOL_CROP, TOL_CROP_K = close(1e-5, 3e-5), close(1e-6, 1e-6)                                  # test_crop_resize_kernel_matches_reference_resize_and_oracle
TOL_BLUR, TOL_BLUR_GRAD = close(1e-6, 1e-6), close(1e-5, 1e-6)                               # test_blurred_smoothness: the blur launch and its adjoint
TOL_BLURRED_LOSS, TOL_BLURRED_GRAD = close(2e-5, 1e-7), rel(1e-3)                            # test_blurred_smoothness: the regulariser
TOL_SMOOTH_AUX = close(1e-4, 1e-5)                                                           # test_blurred_smoothness, test_laplacian_smoothness: the aux maps `disp_grad` / `image_grad`
TOL_CHAIN_LOSS, TOL_CHAIN_GRAD = close(2e-5, 1e-7), rel(1e-3)     # test_whole_chain_from_network_outputs_matches_reference_gradients (and the single-node test's losses): loss, every network output's gradient
TOL_CHAIN_DEPTH = close(2e-5, 1e-5)                               # test_whole_chain_at_baseline_resolution_matches_reference, test_single_node_loss_path_at_baseline_resolution_matches_reference: depth_up

# name; ops: the public operators it covers; operands(gen) -> {name: CPU tensor}; run(F, ops) -> {name: tensor} (outputs and all gradients);
# ref(ops) -> {name: tensor} (fp64 / oracle / reference fixture); tol: {name: bound, '*': default} or judge(out, ref); loose: outputs that are not bit-stable
Case = namedtuple('Case', 'name ops operands run ref tol loose')
CASES = []


def case(name, ops, operands, run, ref, tol, loose=()):
    CASES.append(Case(name, tuple(ops), operands, run, ref, tol, tuple(loose)))


def _leaf(t): return t.requires_grad_(True)
def _d(t): return t.detach().double().clone().requires_grad_(True)
def _g(t): return None if t is None else t.grad


# ---- decoder glue -----------------------------------------------------------------------------------------------------------------------------------
def _elu_pad(shape, elu, bias, bf=False):
    def operands(gen):
        o = dict(x=torch.randn(*shape, generator=gen), gy=torch.randn(shape[0], shape[1], shape[2] + 2, shape[3] + 2, generator=gen))
        if bias: o['bias'] = torch.randn(shape[1], generator=gen)
        if bf: o['x'], o['gy'] = o['x'].to(BF), o['gy'].to(BF)
        return o

    def run(F, o):
        x, b = _leaf(o['x']), (_leaf(o['bias']) if bias else None)
        out = F.elu_pad(x, b, elu, out_dtype=BF if bf else None); out.backward(o['gy'])
        return dict(out=out, g_x=x.grad, g_bias=_g(b))

    def ref(o):
        x, b = _d(o['x']), (_d(o['bias']) if bias else None)
        pre = x + b[None, :, None, None] if bias else x
        out = TF.pad(TF.elu(pre) if elu else pre, (1, 1, 1, 1), mode='reflect'); out.backward(o['gy'].double())
        return dict(out=out, g_x=x.grad, g_bias=_g(b))
    tol = {'*': TOL_GLUE_BF16} if bf else {'*': TOL_GLUE_BIAS} if bias else dict(out=TOL_GLUE_OUT, g_x=TOL_GLUE_GX)
    case(f'elu_pad{shape}{"_elu" if elu else ""}{"_bias" if bias else ""}{"_bf16" if bf else ""}', ['elu_pad'], operands, run, ref, tol)


for _shape in [(2, 5, 2, 2), (2, 3, 7, 9)]:
    for _elu, _bias in [(True, False), (False, False), (True, True), (False, True)]: _elu_pad(_shape, _elu, _bias)
_elu_pad((2, 3, 7, 9), True, True, bf=True)


def _elu_up_cat_pad(B, Ca, Cs, h, w, bias, bf=False):
    def operands(gen):
        o = dict(a=torch.randn(B, Ca, h, w, generator=gen), gy=torch.randn(B, Ca + Cs, 2*h + 2, 2*w + 2, generator=gen))
        if Cs: o['skip'] = torch.randn(B, Cs, 2*h, 2*w, generator=gen)
        if bias: o['bias'] = torch.randn(Ca, generator=gen)
        if bf: o['a'], o['gy'] = o['a'].to(BF), o['gy'].to(BF)     # (bf16 conv output in, bf16 padded tensor out, fp32 skip: test_decoder_glue_bf16_io)
        return o

    def run(F, o):
        a, s, b = _leaf(o['a']), (_leaf(o['skip']) if Cs else None), (_leaf(o['bias']) if bias else None)
        out = F.elu_up_cat_pad(a, s, bias=b, out_dtype=BF if bf else None); out.backward(o['gy'])
        return dict(out=out, g_a=a.grad, g_skip=_g(s), g_bias=_g(b))

    def ref(o):
        a, s, b = _d(o['a']), (_d(o['skip']) if Cs else None), (_d(o['bias']) if bias else None)
        up = TF.interpolate(TF.elu(a + b[None, :, None, None] if bias else a), scale_factor=2, mode='nearest')
        out = TF.pad(torch.cat((up, s), 1) if Cs else up, (1, 1, 1, 1), mode='reflect'); out.backward(o['gy'].double())
        return dict(out=out, g_a=a.grad, g_skip=_g(s), g_bias=_g(b))
    tol = {'*': TOL_GLUE_BF16} if bf else {'*': TOL_GLUE_BIAS} if bias else dict(out=TOL_GLUE_OUT, g_a=TOL_GLUE_GA, g_skip=TOL_GLUE_GX)
    case(f'elu_up_cat_pad({B},{Ca},{Cs},{h},{w}){"_bias" if bias else ""}{"_bf16" if bf else ""}', ['elu_up_cat_pad'], operands, run, ref, tol)


for _dims in [(2, 4, 3, 1, 2), (2, 5, 2, 6, 9), (2, 3, 0, 1, 1)]:
    for _bias in (False, True): _elu_up_cat_pad(*_dims, _bias)
_elu_up_cat_pad(2, 5, 2, 6, 9, True, bf=True)


# ---- heads --------------------------------------------------------------------------------------------------------------------------------------------
def _head(B, C, h, w, act, bias, n=None, bf=False):
    """n None: `conv3x3_head` (one channel); else `conv3x3_headn`."""
    co = n or 1

    def operands(gen):
        o = dict(xp=torch.randn(B, C, h + 2, w + 2, generator=gen), w=torch.randn(co, C, 3, 3, generator=gen)/(3*C**0.5), gy=torch.randn(B, co, h, w, generator=gen))
        if bias: o['bias'] = torch.randn(co, generator=gen)
        if bf: o['xp'] = o['xp'].to(BF)
        return o

    def run(F, o):
        xp, wt, b = _leaf(o['xp']), _leaf(o['w']), (_leaf(o['bias']) if bias else None)
        y = (F.conv3x3_headn if n else F.conv3x3_head)(xp, wt, b, act); y.backward(o['gy'])
        return dict(y=y, g_xp=xp.grad, g_w=wt.grad, g_bias=_g(b))

    def ref(o):
        xp, wt, b = _d(o['xp']), _d(o['w']), (_d(o['bias']) if bias else None)
        y = TF.conv2d(xp, wt, b)
        if act == 'sigmoid': y = torch.sigmoid(y)
        y.backward(o['gy'].double())
        return dict(y=y, g_xp=xp.grad, g_w=wt.grad, g_bias=_g(b))
    tol = {'*': TOL_CONV_F32, 'g_xp': TOL_BF16_OUT if bf else TOL_CONV_F32}
    nm = f'conv3x3_headn{n}' if n else 'conv3x3_head'
    case(f'{nm}({B},{C},{h},{w})_{act}{"_bias" if bias else ""}{"_bf16" if bf else ""}', ['conv3x3_headn' if n else 'conv3x3_head'], operands, run, ref, tol)


for _dims in [(3, 5, 2, 2), (2, 32, 17, 129)]:
    for _act, _bias in [('sigmoid', True), (None, False), ('sigmoid', False), (None, True)]: _head(*_dims, _act, _bias)
    for _n in (1, 4): _head(*_dims, 'sigmoid', True, n=_n)
_head(2, 32, 17, 129, 'sigmoid', True, bf=True)


def _upsample_stack(b, n, size, sizes):
    def operands(gen):
        o = {f'x{s}': torch.rand(b, n, hs, ws, generator=gen) for s, (hs, ws) in enumerate(sizes)}
        o['g'] = torch.randn(len(sizes), b, n, *size, generator=gen)
        return o

    def run(F, o):
        L = [_leaf(o[f'x{s}']) for s in range(len(sizes))]
        up = F.upsample_stack(L, size); up.backward(o['g'])
        return dict(up=up, **{f'g_x{s}': x.grad for s, x in enumerate(L)})

    def ref(o):
        R = [_d(o[f'x{s}']) for s in range(len(sizes))]
        up = torch.stack([TF.interpolate(r, size=size, mode='bilinear', align_corners=False) for r in R]); up.backward(o['g'].double())
        return dict(up=up, **{f'g_x{s}': x.grad for s, x in enumerate(R)})
    case(f'upsample_stack({b},{n},{size})', ['upsample_stack'], operands, run, ref, {'up': TOL_UP_OUT, '*': TOL_UP_GRAD})


_upsample_stack(3, 1, (25, 38), [(12, 19), (7, 5)])
_upsample_stack(1, 4, (33, 47), [(33, 47), (17, 23), (5, 9), (1, 1)])


def _scale_mean(mode, n):
    shapes = [(2, n, 33, 47), (1, 1, 1, 1), (3, n, 64, 64)]      # sizes off the 4096-element blocks (test_scale_mean_matches_fp64)

    def operands(gen): return {f'x{s}': torch.sigmoid(3*torch.randn(sh, generator=gen)) for s, sh in enumerate(shapes)}

    def run(F, o):
        L = [_leaf(o[f'x{s}']) for s in range(len(shapes))]
        loss = F.scale_mean(L, mode); (2.5*loss).backward()
        return dict(loss=loss, **{f'g_x{s}': x.grad for s, x in enumerate(L)})

    def ref(o):
        R = [_d(o[f'x{s}']) for s in range(len(shapes))]
        if mode == 'bce_ones': loss = torch.stack([TF.binary_cross_entropy(r, torch.ones_like(r)) for r in R]).mean()
        else: loss = torch.stack([r.mean() for r in R]).mean()
        (2.5*loss).backward()
        return dict(loss=loss, **{f'g_x{s}': x.grad for s, x in enumerate(R)})
    case(f'scale_mean_{mode}_n{n}', ['scale_mean'], operands, run, ref, {'loss': TOL_MEAN_LOSS, '*': TOL_MEAN_GRAD})


_scale_mean('bce_ones', 1); _scale_mean('identity', 4)


# ---- convolutions -------------------------------------------------------------------------------------------------------------------------------------
def _conv(name, op, fn, xs, ws, ys, kw, bf=False, knob=None):
    def operands(gen):
        o = dict(x=torch.randn(*xs, generator=gen), w=torch.randn(*ws, generator=gen)/(ws[2]*ws[1]**0.5), gy=torch.randn(*ys, generator=gen))
        if bf: o['x'], o['gy'] = o['x'].to(BF), o['gy'].to(BF)
        return o

    def run(F, o):
        from slowtv_monodepth_amd import _lib
        x, wt = _leaf(o['x']), _leaf(o['w'])
        try:
            if knob: _lib.set_knob(knob, 1)
            y = fn(F, x, wt); y.backward(o['gy'])
        finally:
            if knob: _lib.reset_knobs()
        return dict(y=y, g_x=x.grad, g_w=wt.grad)

    def ref(o):
        x, wt = _d(o['x']), (_d(o['w'].to(BF)) if bf else _d(o['w']))      # (bf16 form: the weights as their bf16 rounding, test_conv3x3_mfma_bf16_tensors)
        y = TF.conv2d(x, wt, **kw); y.backward(o['gy'].double())
        return dict(y=y, g_x=x.grad, g_w=wt.grad)
    tol = dict(y=TOL_BF16_OUT, g_x=TOL_BF16_OUT, g_w=TOL_BF16_WGRAD) if bf else {'*': TOL_CONV_F32}
    case(name, [op], operands, run, ref, tol)


def _padded(dims, op='conv3x3_mfma', **k):
    B, C, CO, h, w = dims
    fn = {'conv3x3_mfma': lambda F, x, wt: F.conv3x3_mfma(x, wt), 'conv3x3_wide': lambda F, x, wt: F.conv3x3_wide(x, wt), 'conv3x3_thin': lambda F, x, wt: F.conv3x3_thin(x, wt)}[op]
    tag = ('_bf16' if k.get('bf') else '') + ('_two_tiles' if k.get('knob') else '')
    _conv(f'{op}{dims}{tag}', op, fn, (B, C, h + 2, w + 2), (CO, C, 3, 3), (B, CO, h, w), {}, **k)


for _dims in [(1, 16, 2, 2), (3, 16, 17, 129), (2, 32, 33, 65)]: _padded((*_dims[:2], 16, *_dims[2:]), 'conv3x3_thin')
for _dims in [(1, 16, 32, 1, 1), (2, 48, 64, 9, 70), (2, 96, 32, 13, 100), (3, 160, 64, 6, 20), (2, 512, 256, 6, 20), (3, 16, 16, 13, 129)]: _padded(_dims)
_padded(X.TWO_TILES, knob='conv_two_tiles')
_padded((2, 32, 16, 9, 33), bf=True)
_padded((2, 48, 64, 9, 70), 'conv3x3_wide')      # routed: pinned to the MFMA kernels by the module's fixture
# conv_exact.SAME and STEM: every shape is a launch shape of its own (tile forms, row bands, the K split: the comments in test_gpu_encoder_conv.py / _stem_conv.py)
for _dims in X.SAME:
    _B, _C, _CO, _h, _w = _dims
    _conv(f'conv3x3_same{_dims}', 'conv3x3_same', lambda F, x, wt: F.conv3x3_same(x, wt), (_B, _C, _h, _w), (_CO, _C, 3, 3), (_B, _CO, _h, _w), dict(padding=1))
for _dims in X.STEM:
    _B, _C, _H, _W = _dims
    _conv(f'conv7x7s2_stem{_dims}', 'conv7x7s2_stem', lambda F, x, wt: F.conv7x7s2_stem(x, wt), (_B, _C, _H, _W), (64, _C, 7, 7), (_B, 64, (_H - 1)//2 + 1, (_W - 1)//2 + 1),
          dict(stride=2, padding=3))


# ---- encoder layers ------------------------------------------------------------------------------------------------------------------------------------
def _batch_norm(shape, relu, res):
    N, C, H, W = shape

    def operands(gen):
        o = dict(x=torch.randn(*shape, generator=gen)*2 + 3*torch.randn(1, C, 1, 1, generator=gen), w=torch.rand(C, generator=gen) + 0.5, b=torch.randn(C, generator=gen),
                 g=torch.randn(*shape, generator=gen), rm=torch.zeros(C), rv=torch.ones(C))
        if res: o['r'] = torch.randn(*shape, generator=gen)
        return o

    def go(o, cast, fn):
        x, w, b, r = cast(o['x']), cast(o['w']), cast(o['b']), (cast(o['r']) if res else None)
        rm, rv = o['rm'].detach().clone().to(x.dtype) if x.dtype == torch.float64 else o['rm'], o['rv'].detach().clone().to(x.dtype) if x.dtype == torch.float64 else o['rv']
        y = fn(x, w, b, rm, rv, r); y.backward(o['g'].to(x.dtype))
        return dict(y=y, g_x=x.grad, g_w=w.grad, g_b=b.grad, g_res=_g(r), running_mean=rm, running_var=rv)

    def run(F, o): return go(o, _leaf, lambda x, w, b, rm, rv, r: F.batch_norm_act(x, w, b, rm, rv, residual=r, momentum=0.1, eps=1e-5, relu=relu))

    def ref(o):
        def f(x, w, b, rm, rv, r):
            y = TF.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
            if res: y = y + r
            return TF.relu(y) if relu else y
        return go(o, _d, f)
    case(f'batch_norm_act{shape}{"_relu" if relu else ""}{"_res" if res else ""}', ['batch_norm_act'], operands, run, ref, {'*': TOL_BN})


for _shape in [(3, 5, 7, 9), (4, 8, 6, 20), (2, 130, 3, 5)]:      # the scalar path, the `f4` path (HW % 4 == 0), more channels than a block
    for _relu, _res in [(False, False), (True, False), (True, True), (False, True)]: _batch_norm(_shape, _relu, _res)


def _simple(name, op, operands, fwd, ref_fwd, tol, grads, gy='g'):
    """One differentiable output `y`; gradients to the operands named in `grads`."""
    def run(F, o):
        L = {k: _leaf(o[k]) for k in grads}
        y = fwd(F, {**o, **L}); y.backward(o[gy])
        return dict(y=y, **{f'g_{k}': v.grad for k, v in L.items()})

    def ref(o):
        R = {k: _d(o[k]) for k in grads}
        y = ref_fwd({**{k: (v.double() if v.is_floating_point() else v) for k, v in o.items()}, **R}); y.backward(o[gy].double())
        return dict(y=y, **{f'g_{k}': v.grad for k, v in R.items()})
    case(name, [op], operands, run, ref, tol)


for _shape in [(2, 3, 1, 1), (3, 4, 9, 7)]:
    _ho, _wo = (_shape[2] - 1)//2 + 1, (_shape[3] - 1)//2 + 1
    _simple(f'max_pool3x3s2{_shape}', 'max_pool3x3s2',
            lambda gen, s=_shape, ho=_ho, wo=_wo: dict(x=torch.relu(torch.randn(*s, generator=gen)), g=torch.randn(s[0], s[1], ho, wo, generator=gen)),   # post-ReLU: exact ties at 0
            lambda F, o: F.max_pool3x3s2(o['x']), lambda o: TF.max_pool2d(o['x'], 3, 2, 1), dict(y=EQUAL, g_x=TOL_POOL_GX), ['x'])
for _shape in [(2, 3, 1, 1), (1, 4, 33, 65), (2, 6, 40, 70)]:
    _simple(f'dwconv7x7{_shape}', 'dwconv7x7',
            lambda gen, s=_shape: dict(x=torch.randn(*s, generator=gen), w=torch.randn(s[1], 1, 7, 7, generator=gen)*0.2, b=torch.randn(s[1], generator=gen), g=torch.randn(*s, generator=gen)),
            lambda F, o: F.dwconv7x7(o['x'], o['w'], o['b']), lambda o: TF.conv2d(o['x'], o['w'], o['b'], padding=3, groups=o['x'].shape[1]), {'*': TOL_DWCONV}, ['x', 'w', 'b'])


def _ln_operands(shape, bf=False):
    N, C, H, W = shape

    def operands(gen):
        o = dict(x=torch.randn(*shape, generator=gen)*2 + 3*torch.randn(N, 1, H, W, generator=gen), w=torch.rand(C, generator=gen) + 0.5, b=torch.randn(C, generator=gen),
                 g=torch.randn(*shape, generator=gen))
        if bf: o['g'] = o['g'].to(BF)
        return o
    return operands


_ln_ref = lambda o: TF.layer_norm(o['x'].permute(0, 2, 3, 1), (o['x'].shape[1],), o['w'], o['b'], 1e-6).permute(0, 3, 1, 2)
for _shape in [(2, 3, 1, 1), (1, 7, 33, 65), (2, 1030, 5, 7)]:
    _simple(f'layer_norm_cf{_shape}', 'layer_norm_cf', _ln_operands(_shape), lambda F, o: F.layer_norm_cf(o['x'], o['w'], o['b'], 1e-6), _ln_ref, {'*': TOL_LN}, ['x', 'w', 'b'])
_simple('layer_norm_cf(2, 48, 9, 11)_bf16', 'layer_norm_cf', _ln_operands((2, 48, 9, 11), bf=True), lambda F, o: F.layer_norm_cf(o['x'], o['w'], o['b'], 1e-6, out_dtype=BF), _ln_ref,
        {'y': TOL_LN_BF16_OUT, '*': TOL_LN_BF16_GRAD}, ['x', 'w', 'b'])


# ---- the fused loss path against the oracle --------------------------------------------------------------------------------------------------------------
def _K(b, h, w): return torch.tensor([[0.58*w, 0, 0.5*w, 0], [0, 1.92*h, 0.5*h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(b, 1, 1)


def _sweep(b, h, w, n, S, mode):
    """`image_recon_fused` at a strip-boundary shape of test_gpu_parity.SWEEP, judged as test_strip_boundary_shapes_match_oracle judges it."""
    use = mode == 'min_automask'

    def operands(gen):
        from oracle import view_synth_oracle as O
        imgs = torch.rand(b, 3, h, w, generator=gen)
        aa, t = 0.02*torch.randn(n*b, 3, generator=gen), 0.2*torch.randn(n*b, 3, generator=gen)
        return dict(imgs=imgs, supp=(imgs[None] + 0.1*torch.randn(n, b, 3, h, w, generator=gen)).clamp(0, 1), depth=1 + 10*torch.rand(S, b, 1, h, w, generator=gen),
                    T=O.T_from_AAt(aa, t).unflatten(0, (n, b)).contiguous(), K=_K(b, h, w), noise=torch.randn(S*b, 1, h, w, generator=gen))

    def run(F, o):
        d, T = _leaf(o['depth']), _leaf(o['T'])
        loss, err, sel, _ = F.image_recon_fused(d, o['imgs'], o['supp'], T, o['K'], flags=F.recon_flags('ssim', use, use), noise=o['noise'])
        loss.backward()
        return dict(loss=loss, err=err, sel=sel, g_depth=d.grad, g_T=T.grad)

    def ref(o):
        from oracle import view_synth_oracle as O
        d, T = o['depth'].clone().requires_grad_(True), o['T'].clone().requires_grad_(True)
        loss, _, full = O.image_recon({s: d[s] for s in range(S)}, o['imgs'], o['supp'], T, o['K'], 'ssim', use, use, noise=o['noise'])
        loss.backward()
        return dict(loss=loss, err=full['err'], sel=full['sel'], g_depth=d.grad, g_T=T.grad)

    def judge(out, r):
        flips = (out['sel'].cpu() != r['sel'].reshape(out['sel'].shape)).flatten()
        assert flips.float().mean().item() <= SWEEP_FLIPS, f'selection differs on {flips.float().mean().item():.2%} of pixels'
        torch.testing.assert_close(out['err'].cpu().flatten()[~flips], r['err'].detach().flatten()[~flips], rtol=0, atol=SWEEP_ERR_ATOL)
        _hold('loss', out['loss'], r['loss'], SWEEP_LOSS)
        tol = SWEEP_GRAD_FLIPPED if flips.any() else SWEEP_GRAD
        assert rel_to_max(out['g_depth'].cpu(), r['g_depth']) < tol and rel_to_max(out['g_T'].cpu()[..., :3, :], r['g_T'][..., :3, :]) < tol
    case(f'image_recon_fused({b},{h},{w},{n},{S})_{mode}', ['image_recon_fused'], operands, run, ref, judge)


for _dims in [(1, 2, 2, 1, 1), (1, 4, 61, 2, 2), (2, 6, 62, 3, 1), (1, 33, 125, 2, 2), (2, 9, 40, 6, 2)]:
    for _mode in ('min_automask', 'mean'): _sweep(*_dims, _mode)


def _k0_smooth(b, h, w, lows):
    """`disp_to_depth` and `disp_smooth_fused` at a pyramid of non-integer ratios (test_k0_and_smoothness_at_non_integer_ratios)."""
    S = len(lows)

    def operands(gen):
        o = dict(imgs=torch.rand(b, 3, h, w, generator=gen), gup=torch.randn(S, b, 1, h, w, generator=gen))
        o.update({f'd{s}': 0.05 + 0.9*torch.rand(b, 1, hs, ws, generator=gen) for s, (hs, ws) in enumerate(lows)})
        return o

    def run(F, o):
        d = {s: _leaf(o[f'd{s}']) for s in range(S)}
        dep, _ = F.disp_to_depth([d[s] for s in d], (h, w), 0.1, 100)
        l, dg, ig = F.disp_smooth_fused(d, o['imgs'], use_edges=True, want_aux=True)
        ((dep*o['gup']).sum()*1e-3 + l).backward()
        return dict(depth_up=dep, loss=l, disp_grad=dg, image_grad=ig, **{f'g_d{s}': v.grad for s, v in d.items()})

    def ref(o):
        from oracle import view_synth_oracle as O
        d = {s: o[f'd{s}'].clone().requires_grad_(True) for s in range(S)}
        _, dep = O.disp_to_depth_up(d, (h, w), 0.1, 100)
        l, aux = O.disp_smooth(d, o['imgs'], True)
        (sum((dep[s]*o['gup'][s]).sum() for s in d)*1e-3 + l).backward()
        return dict(depth_up=torch.stack([dep[s] for s in d]), loss=l, disp_grad=aux['disp_grad'], image_grad=aux['image_grad'], **{f'g_d{s}': v.grad for s, v in d.items()})
    case(f'k0_smooth({b},{h},{w})', ['disp_to_depth', 'disp_smooth_fused'], operands, run, ref,
         {'depth_up': TOL_K0_DEPTH, 'loss': TOL_K0_LOSS, 'disp_grad': TOL_SMOOTH_AUX, 'image_grad': TOL_SMOOTH_AUX, '*': TOL_K0_GRAD})


_k0_smooth(2, 33, 47, [(33, 47), (16, 23), (8, 11)])
_k0_smooth(1, 8, 12, [(8, 12), (4, 6), (2, 3), (1, 1)])


def _loss_path(b, h, w, n, lows, single):
    """The whole loss path from the networks' outputs, mean over the supports and no automask (no routing decision to flip): as ONE node (`loss_path_fused`) or
    as the operators it replaces (`image_recon_prep` ahead, `image_recon_fused_disp` + `disp_smooth_fused`), each behind `pose_matrices` / `intrinsics`, against
    the oracle's `loss_path`, at the bounds the whole-chain and single-node tests hold the same outputs to against the reference's run."""
    S = len(lows)

    def operands(gen):
        imgs = torch.rand(b, 3, h, w, generator=gen)
        o = dict(imgs=imgs, supp=(imgs[None] + 0.15*torch.randn(n, b, 3, h, w, generator=gen)).clamp(0, 1), aa=0.01*torch.randn(n*b, 3, generator=gen),
                 t=0.05*torch.randn(n*b, 3, generator=gen), fs=torch.tensor([0.58, 1.92])[None].repeat(b, 1)*(1 + 0.05*torch.randn(b, 2, generator=gen)),
                 cs=0.5 + 0.03*torch.randn(b, 2, generator=gen))
        o.update({f'd{s}': 0.05 + 0.9*torch.rand(b, 1, hs, ws, generator=gen) for s, (hs, ws) in enumerate(lows)})
        return o

    def run(F, o):
        d = {s: _leaf(o[f'd{s}']) for s in range(S)}
        aa, t, fs, cs = (_leaf(o[k]) for k in ('aa', 't', 'fs', 'cs'))
        flags = F.recon_flags('ssim', False, False)
        Ts = F.pose_matrices(aa, t).unflatten(0, (n, b)); K, K_inv = F.intrinsics(fs, cs, (h, w))
        pr = F.image_recon_prep(o['imgs'], o['supp'], flags=flags, pyramid=lows, smooth_edges=True)
        if single:
            loss, l_rec, l_sm, sel, dep = F.loss_path_fused(d, o['imgs'], o['supp'], Ts, K, K_inv, pose=(aa, t, None), intrinsics=(fs, cs), flags=flags, min_depth=0.1,
                                                            max_depth=100, seed=11, w_recon=1.0, w_smooth=0.001, prepared=pr)
        else:
            l_rec, _, sel, _, dep = F.image_recon_fused_disp(list(d.values()), o['imgs'], o['supp'], Ts, K, K_inv, flags=flags, min_depth=0.1, max_depth=100, seed=11,
                                                             want_err=False, prepared=pr)
            l_sm, _, _ = F.disp_smooth_fused(d, o['imgs'], use_edges=True, want_aux=False, prepared=pr)
            loss = l_rec + 0.001*l_sm
        loss.backward()
        return dict(loss=loss, l_rec=l_rec, l_sm=l_sm, sel=sel, depth_up=dep, g_aa=aa.grad, g_t=t.grad, g_fs=fs.grad, g_cs=cs.grad, **{f'g_d{s}': v.grad for s, v in d.items()})

    def ref(o):
        from oracle import view_synth_oracle as O
        d = {s: o[f'd{s}'].clone().requires_grad_(True) for s in range(S)}
        aa, t, fs, cs = (o[k].clone().requires_grad_(True) for k in ('aa', 't', 'fs', 'cs'))
        Ts = O.T_from_AAt(aa, t).unflatten(0, (n, b)); K = O.resize_K(O.build_K(fs, cs), (h, w))
        loss, out = O.loss_path(d, o['imgs'], o['supp'], Ts, K, min_depth=0.1, max_depth=100, use_min=False, use_automask=False, use_edges=True, w_recon=1.0, w_smooth=0.001)
        loss.backward()
        return dict(loss=loss, l_rec=out['loss_img_recon'], l_sm=out['loss_disp_smooth'], depth_up=torch.stack([out['depth_up'][s] for s in d]), sel=out['full']['sel'], g_aa=aa.grad, g_t=t.grad,
                    g_fs=fs.grad, g_cs=cs.grad, **{f'g_d{s}': v.grad for s, v in d.items()})
    tol = {'loss': TOL_CHAIN_LOSS, 'l_rec': TOL_CHAIN_LOSS, 'l_sm': TOL_CHAIN_LOSS, 'depth_up': TOL_CHAIN_DEPTH, 'sel': EQUAL, '*': TOL_CHAIN_GRAD}
    case(f'loss_path_{"one_node" if single else "two_nodes"}({b},{h},{w},{n})', ['loss_path_fused', 'image_recon_prep', 'pose_matrices', 'intrinsics'] if single else
         ['image_recon_fused_disp', 'image_recon_prep', 'disp_smooth_fused', 'pose_matrices', 'intrinsics'], operands, run, ref, tol)


_loss_path(2, 33, 47, 3, [(33, 47), (16, 23), (8, 11)], True)
_loss_path(2, 33, 47, 3, [(33, 47), (16, 23), (8, 11)], False)


# ---- un-fused operators and the rest ---------------------------------------------------------------------------------------------------------------------
def _view_synth():
    def operands(gen):
        from oracle import view_synth_oracle as O
        g = load_golden('op_view_synth')
        return dict(inp=g['in_input'], depth=g['in_depth'], T=O.T_from_AAt(g['in_aa'], g['in_t']).contiguous(), K=g['in_K'], gw=g['in_gw'], gd=g['in_gd'])

    def run(F, o):
        L = {k: _leaf(o[k]) for k in ('inp', 'depth', 'T', 'K')}
        warp, dwarp, valid = F.view_synth(L['inp'], L['depth'], L['T'], L['K'])
        ((warp*o['gw']).sum() + (dwarp*o['gd']).sum()).backward()
        return dict(warp=warp, dwarp=dwarp, valid=valid.to(torch.uint8), g_input=L['inp'].grad, g_depth=L['depth'].grad, g_T=L['T'].grad[..., :3, :], g_K=L['K'].grad)

    def ref(o):
        from oracle import view_synth_oracle as O
        L = {k: _d(o[k]) for k in ('inp', 'depth', 'T', 'K')}
        warp, dwarp, _ = O.view_synth(L['inp'], L['depth'], L['T'], L['K'])[:3]
        ((warp*o['gw'].double()).sum() + (dwarp*o['gd'].double()).sum()).backward()
        return dict(warp=warp, dwarp=dwarp, g_input=L['inp'].grad, g_depth=L['depth'].grad, g_T=L['T'].grad[..., :3, :], g_K=L['K'].grad)
    # g_input is accumulated with float atomicAdd (csrc/smd_unfused.hip, k_view_synth_bwd): its sum order is not fixed, so between the two runs it is held to
    # its test's bound instead of bit-equality
    case('view_synth_c5', ['view_synth'], operands, run, ref, {'warp': TOL_VS_WARP, 'dwarp': TOL_VS_DWARP, 'valid': None, '*': TOL_VS_GRAD}, loose=['g_input'])


_view_synth()


def _photo(fixture, loss_name, grad_tol):
    def operands(gen):
        g = load_golden(fixture)
        return dict(pred=g['in_pred'], target=g['in_target'], ge=g['in_ge'])
    from oracle import view_synth_oracle as O
    _simple(f'photo_error_{loss_name}_{fixture}', 'photo_error', operands, lambda F, o: F.photo_error(o['pred'], o['target'], loss_name),
            lambda o: O.photo_error(o['pred'], o['target'], loss_name), dict(y=TOL_PHOTO_ERR, g_pred=grad_tol), ['pred'], gy='ge')


_photo('op_photo_error', 'ssim', TOL_PHOTO_GRAD); _photo('op_photo_error', 'l1', TOL_PHOTO_GRAD); _photo('op_photo_ssim_c5', 'ssim', TOL_PHOTO_GRAD_C)


def _masked_recon():
    """`recon_reduce` through the masked reconstruction (mean over the supports, no automask: no decision to flip), against the reference's recorded run."""
    fixture = 'op_recon_mask_uncer_min0_auto0_c3'

    def operands(gen):
        g = load_golden(fixture)
        return dict(pred=g['in_pred'], target=g['in_target'], mask=g['in_mask'])

    def run(F, o):
        pred, mask = _leaf(o['pred']), _leaf(o['mask'])
        n, b = pred.shape[:2]
        ew = F.photo_error(pred.flatten(0, 1), o['target'][None].expand_as(pred).flatten(0, 1)).view(n, b, *pred.shape[-2:])
        loss, err, sel = F.recon_reduce(ew, None, use_min=False, mask=mask, mask_name='uncertainty')
        loss.backward()
        return dict(loss=loss, err=err, sel=sel, g_pred=pred.grad, g_mask=mask.grad)

    def ref(o):
        from oracle import view_synth_oracle as O
        g = load_golden(fixture)
        _, out = O.recon_loss(o['pred'], o['target'], use_min=False, use_automask=False, mask=o['mask'], mask_name='uncertainty')      # the maps: the fixture records none
        return dict(loss=torch.as_tensor(g['out_loss']), err=out['err'], sel=out['sel'], g_pred=g['grad_pred'], g_mask=g['grad_mask'])
    case('recon_reduce_masked_uncertainty', ['recon_reduce', 'photo_error'], operands, run, ref,
         {'loss': TOL_MASKED_LOSS, 'err': close(0, SWEEP_ERR_ATOL), 'sel': EQUAL, '*': TOL_MASKED_GRAD})      # (error map and selection: the sweep test's bounds for them)


_masked_recon()


def _regression(fixture, loss_name, masked):
    def operands(gen):
        g = load_golden(fixture)
        return dict(pred=g['in_pred'], target=g['in_target'], **({'mask': g['in_mask'].bool()} if masked else {}))

    def run(F, o):
        pred = _leaf(o['pred'])
        loss, err = F.regression_loss(pred, o['target'], o.get('mask'), loss_name=loss_name); loss.backward()
        return dict(loss=loss, err=err, g_pred=pred.grad)

    def ref(o):
        g = load_golden(fixture)
        return dict(loss=torch.as_tensor(g['out_loss']), err=g['out_err'], g_pred=g['grad_pred'])
    case(f'regression_{fixture}', ['regression_loss'], operands, run, ref, {'g_pred': TOL_REGR_GRAD, '*': TOL_REGR})


_regression('op_regr_berhu_mask', 'berhu', True); _regression('op_regr_log_l1', 'log_l1', False)


def _pose():
    N = 9

    def operands(gen):
        aa = torch.randn(N, 3, generator=gen)*0.3
        aa[0] = 0.0; aa[1] = aa[1]*1e-4/aa[1].norm()       # the clip branch and the |aa| < eps branch (test_inverted_pose_matches_general_inverse)
        return dict(aa=aa, t=torch.randn(N, 3, generator=gen), inv=torch.tensor([0, 1, 1, 0, 1, 0, 1, 1, 0], dtype=torch.uint8), gT=torch.randn(N, 4, 4, generator=gen))

    def run(F, o):
        aa, t = _leaf(o['aa']), _leaf(o['t'])
        T = F.pose_matrices(aa, t, o['inv']); T.backward(o['gT'])
        return dict(T=T, g_aa=aa.grad, g_t=t.grad)

    def ref(o):
        from oracle import view_synth_oracle as O
        aa, t = o['aa'].clone().requires_grad_(True), o['t'].clone().requires_grad_(True)
        T = O.T_from_AAt(aa, t)
        T = torch.stack([torch.linalg.inv(Ti) if f else Ti for Ti, f in zip(T, o['inv'])]); T.backward(o['gT'])
        return dict(T=T, g_aa=aa.grad, g_t=t.grad)
    case('pose_matrices_inverted', ['pose_matrices'], operands, run, ref, dict(T=TOL_POSE_T, g_aa=TOL_POSE_GAA, g_t=TOL_POSE_GT))


def _intrinsics():
    b, size = 5, (96, 320)

    def operands(gen):
        return dict(fs=torch.rand(b, 2, generator=gen) + 0.5, cs=torch.rand(b, 2, generator=gen)*0.2 + 0.4, gK=torch.randn(b, 4, 4, generator=gen), gKi=torch.randn(b, 4, 4, generator=gen))

    def run(F, o):
        fs, cs = _leaf(o['fs']), _leaf(o['cs'])
        K, Ki = F.intrinsics(fs, cs, size); ((K*o['gK']).sum() + (Ki*o['gKi']).sum()).backward()
        Ks = K.detach().clone(); Ks[:, 0, 1] = 0.7        # caller-supplied K with skew: the adjugate inverse of the 3x3 block
        return dict(K=K, K_inv=Ki, g_fs=fs.grad, g_cs=cs.grad, skew_inv=F.inv_intrinsics(Ks))

    def ref(o):
        from oracle import view_synth_oracle as O
        fs, cs = o['fs'].clone().requires_grad_(True), o['cs'].clone().requires_grad_(True)
        K = O.resize_K(O.build_K(fs, cs), size); Ki = torch.linalg.inv(K); ((K*o['gK']).sum() + (Ki*o['gKi']).sum()).backward()
        Ks = K.detach().clone(); Ks[:, 0, 1] = 0.7
        return dict(K=K, K_inv=Ki, g_fs=fs.grad, g_cs=cs.grad, skew_inv=torch.linalg.inv(Ks))
    case('intrinsics', ['intrinsics', 'inv_intrinsics'], operands, run, ref, dict(K=TOL_K, K_inv=TOL_KINV, skew_inv=TOL_KINV, g_fs=TOL_K_GRAD, g_cs=TOL_K_GRAD))


_pose(); _intrinsics()


def _crop_resize(crop, out):
    def operands(gen):
        return dict(a=torch.rand(2, 3, 37, 61, generator=gen), b=torch.rand(3, 2, 3, 37, 61, generator=gen), c=torch.rand(2, 1, 37, 61, generator=gen), K=torch.rand(2, 4, 4, generator=gen))

    def run(F, o):
        outs, K = F.crop_resize([o['a'], o['b'], o['c']], crop, out, o['K'])
        return dict(a=outs[0], b=outs[1], c=outs[2], K=K)

    def ref(o):
        from oracle import aspect_ratio_oracle as A
        outs, K = A.crop_resize([o['a'], o['b'], o['c']], crop, out, o['K'])
        return dict(a=outs[0], b=outs[1], c=outs[2], K=K)
    case(f'crop_resize{crop}->{out}', ['crop_resize'], operands, run, ref, {'K': TOL_CROP_K, '*': TOL_CROP})


_crop_resize((20, 33), (32, 64)); _crop_resize((21, 32), (32, 32))


def _depth_metrics(name):
    """`depth_metrics` on a case of metrics_cases.py, judged as test_gpu_metrics.py judges it: 4 x the ATen fp32 sequence's own error per number, floor 1e-6."""
    def operands(gen):
        from metrics_cases import make_case
        pred, target, lo, hi = make_case(name)
        assert lo is None and hi is None
        return dict(pred=pred, target=target)

    def run(F, o):
        import test_gpu_metrics as TM
        values, medians, counts = F.depth_metrics(o['pred'], o['target'])
        av, am = TM.aten_sequence(o['pred'], o['target'])
        return dict(values=values, medians=medians, counts=counts, aten_values=av, aten_medians=am)

    def ref(o):
        import test_gpu_metrics as TM
        rv, rm, rc, _ = TM.restate(o['pred'], o['target'])
        return dict(values=rv, medians=rm, counts=rc)

    def judge(out, r):
        import numpy as np
        import test_gpu_metrics as TM
        v, m, av, am = (out[k].double().cpu().numpy() for k in ('values', 'medians', 'aten_values', 'aten_medians'))
        assert out['counts'].cpu().tolist() == r['counts'].tolist()
        assert (out['medians'][:, 1].cpu().numpy() == r['medians'][:, 1].astype(np.float32)).all()
        TM.check_against_aten(f'hostile depth_metrics[{name}]', np.concatenate([m[:, :1], v], axis=1), np.concatenate([am[:, :1], av], axis=1),
                              np.concatenate([r['medians'][:, :1], r['values']], axis=1))
    case(f'depth_metrics_{name}', ['depth_metrics'], operands, run, ref, judge, loose=['aten_values', 'aten_medians'])


_depth_metrics('up'); _depth_metrics('multi')      # 481 pixels: not a multiple of 64; 30720: more than one block per sample


def _blur():
    from oracle import view_synth_oracle as O
    for shape in [(2, 3, 2, 2), (3, 2, 33, 70)]:
        _simple(f'gaussian_blur3x3{shape}', 'gaussian_blur3x3', lambda gen, s=shape: dict(x=torch.rand(*s, generator=gen), g=torch.randn(*s, generator=gen)),
                lambda F, o: F.gaussian_blur3x3(o['x']), lambda o: O.gaussian_blur3x3(o['x']), dict(y=TOL_BLUR, g_x=TOL_BLUR_GRAD), ['x'])

    def operands(gen): return dict(img=torch.rand(2, 3, 33, 47, generator=gen), d=0.05 + 0.9*torch.rand(2, 1, 33, 47, generator=gen))

    def run(F, o):
        d = _leaf(o['d'])
        loss, dg, ig = F.disp_smooth_blurred({0: d}, o['img'], use_edges=True, want_aux=True); loss.backward()
        return dict(loss=loss, disp_grad=dg, image_grad=ig, g_d=d.grad)

    def ref(o):
        d = o['d'].clone().requires_grad_(True)
        loss, ld = O.smooth_reg(d, o['img'], True, use_blur=True); loss.backward()
        return dict(loss=loss, disp_grad=ld['disp_grad'], image_grad=ld['image_grad'], g_d=d.grad)
    case('disp_smooth_blurred(2,33,47)', ['disp_smooth_blurred', 'gaussian_blur3x3', 'disp_smooth_fused'], operands, run, ref,
         dict(loss=TOL_BLURRED_LOSS, disp_grad=TOL_SMOOTH_AUX, image_grad=TOL_SMOOTH_AUX, g_d=TOL_BLURRED_GRAD))


_blur()

# Public names of `functional` that no case runs, and why.  Only names without a device allocation or kernel of their own, the `smd_debug_*` / profiling
# helpers and the experiments-only kernel may stand here (test_hostile_memory_host.py holds the table to `functional.__all__`).
NOT_COVERED = {
    'set_conv_route': 'route setter: no allocation, no kernel', 'conv_routes': 'query of the cached routing decisions',
    'PreparedFrames': 'the record `image_recon_prep` returns (its buffers are allocated and filled there: the loss_path cases)',
    'recon_flags': 'flag arithmetic on the host', 'supports_per_pass': 'query of a library constant', 'row_skip_tuner': 'host-side tuner object (pinned here by SMD_BWD_SKIP)',
    'dead_tile_shares': 'host-side statistic on ATen, no kernel', 'dead_wave_shares': 'host-side statistic on ATen, no kernel',
    'lane_shift_selftest': 'the `smd_debug_lane_shift` self-test helper'}


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def F():
    if not torch.cuda.is_available(): pytest.skip('needs a GPU')
    from slowtv_monodepth_amd import functional
    functional.set_conv_route('mfma')
    yield functional
    functional.set_conv_route('auto')


def _hold(name, got, ref, bound):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu().reshape(got.shape)
    if bound[0] == 'equal': assert torch.equal(got, ref), f'{name}: {X.first_difference(got, ref, [f"d{k}" for k in range(got.ndim)])}'
    elif bound[0] == 'rel': assert rel_to_max(got, ref) <= bound[1], f'{name}: {rel_to_max(got, ref):.3e} of the maximum against the reference (bound {bound[1]:g})'
    else: torch.testing.assert_close(got, ref, rtol=bound[1], atol=bound[2], msg=lambda m: f'{name}: {m}')


def _execute(F, c, ops_cpu, arena=None, shift=0):
    """-> {name: tensor} of one run; with an arena: operands guarded (and shifted), allocations served from it (16-byte aligned), guards checked."""
    if arena is None: ops, ctx = {k: v.cuda() for k, v in ops_cpu.items()}, contextlib.nullcontext()
    else: ops, ctx = {k: arena.guarded(v.cuda(), shift) for k, v in ops_cpu.items()}, hostile(arena)
    if arena is not None:
        from slowtv_monodepth_amd import class_ops
        class_ops._mean_ws.clear()          # `scale_mean`'s persistent workspace: a fresh one for the hostile run (module text, point 2)
    n_operands = len(arena.blocks) if arena is not None else 0
    with ctx: out = c.run(F, ops)
    if arena is not None: assert len(arena.blocks) > n_operands, f'{c.name}: the operator allocated nothing from the arena (the patch did not reach its `torch.empty` calls)'
    out = {k: v.detach() for k, v in out.items() if v is not None}
    if arena is not None: arena.check()
    else: torch.cuda.synchronize()
    return out


_shared = {}      # case name -> (operands, the friendly run, the reference): computed once, shared by both shifts, never modified


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted'])
@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_operator_in_hostile_memory(F, monkeypatch, c, shift):
    monkeypatch.setenv('SMD_BWD_SKIP', '0')          # one row loop of the fused backward for every run (the tuner would time its two loops on different calls)
    if c.name not in _shared:
        ops_cpu = c.operands(torch.Generator().manual_seed(len(c.name)*7919 + 17))
        _shared[c.name] = (ops_cpu, _execute(F, c, ops_cpu), c.ref({k: v.clone() for k, v in ops_cpu.items()}))
    ops_cpu, A, ref = _shared[c.name]
    B = _execute(F, c, ops_cpu, Arena(), shift)
    assert set(A) == set(B)
    for k, v in B.items(): assert_finite(v, f'{c.name}: {k}')
    if callable(c.tol): c.tol(B, ref)
    else:
        for k, v in B.items():
            bound = c.tol.get(k, c.tol.get('*'))
            if bound is not None: _hold(f'{c.name}: {k}', v, ref[k], bound)
    for k, v in B.items():
        if k not in c.loose: assert torch.equal(A[k], v), f'{c.name}: {k} differs between the friendly and the hostile run: {X.first_difference(v, A[k], [f"d{i}" for i in range(v.ndim)])}'
        elif not callable(c.tol): _hold(f'{c.name}: {k} (hostile against friendly run)', v, A[k], c.tol.get(k, c.tol.get('*')))
