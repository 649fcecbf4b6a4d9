"""`torch.autograd.Function`s around the C ABI (`include/smd_hotpath.h`): the one surface the rest of the package, the tests and the benchmark call.

PyTorch's role here is plumbing only: it owns the device buffers, provides the current HIP stream and carries the hand-written backward kernels in its autograd graph.
Every function validates its inputs on the host and raises the exception types the reference raises (`ValueError`) before any launch; there is no fallback path —
CPU tensors are rejected.  The operators live in one module per family, and every name here IS the object of its home module: `recon_ops` (the loss path), `row_skip`
(the fused backward's row-loop tuner and its diagnostics), `class_ops` (the un-fused class-level operators), `net_ops` (the network glue), `geom_ops` (pose and
intrinsics), `conv_ops` / `conv_routing` (the routed MFMA convolutions, the stem and the stride-2 layers included: one operator skeleton, one rule table), `metric_ops` (the validation depth metrics), `attention_ops` (the CADepth decoder's attention blocks), `fusion_ops` (the DiffNet decoder's glue), `subpixel` (the SuperDepth decoder's sub-pixel convolution), `blend` (the flip-and-blend post-process of the inference path); `_device` holds what they share."""
from ._device import _stream, call
from .attention_ops import channel_attention, se_gate
from .blend import flip_blend, flip_blend_pyramid
from .ddv_ops import ddv_head
from .fusion_ops import relu_pad, up_cat_gate_pad
from .class_ops import _ScaleMean, crop_resize, lane_shift_selftest, photo_error, recon_reduce, regression_loss, scale_mean, upsample_stack, view_synth
from .conv_ops import conv3x3_mfma, conv3x3_s2, conv3x3_same, conv3x3_thin, conv3x3_wide, conv7x7s2_stem
from .conv_routing import _conv_route, conv_routes, set_conv_route
from .geom_ops import intrinsics, inv_intrinsics, pose_matrices
from .metric_ops import depth_metrics
from .net_ops import batch_norm_act, conv3x3_head, conv3x3_headn, dwconv7x7, elu_pad, elu_up_cat_pad, layer_norm_cf, max_pool3x3s2
from .recon_ops import (PreparedFrames, disp_smooth_blurred, disp_smooth_fused, disp_to_depth, gaussian_blur3x3, image_recon_fused, image_recon_fused_disp,
                        image_recon_prep, loss_path_fused, recon_flags, supports_per_pass)
from .row_skip import _RowSkipTuner, dead_tile_shares, dead_wave_shares, row_skip_tuner
from .subpixel import subpixel_conv

__all__ = ['conv3x3_headn', 'upsample_stack', 'scale_mean', 'conv3x3_mfma', 'conv3x3_wide', 'conv3x3_same', 'set_conv_route', 'conv_routes', 'loss_path_fused', 'crop_resize', 'disp_to_depth', 'image_recon_prep', 'PreparedFrames', 'image_recon_fused', 'image_recon_fused_disp', 'disp_smooth_fused', 'view_synth', 'photo_error', 'recon_reduce',
           'lane_shift_selftest', 'recon_flags', 'regression_loss', 'elu_pad', 'elu_up_cat_pad', 'batch_norm_act', 'max_pool3x3s2', 'dwconv7x7', 'layer_norm_cf', 'pose_matrices', 'intrinsics', 'inv_intrinsics',
           'conv3x3_head', 'conv3x3_thin', 'conv7x7s2_stem', 'gaussian_blur3x3', 'disp_smooth_blurred', 'supports_per_pass', 'row_skip_tuner', 'dead_tile_shares', 'dead_wave_shares', 'depth_metrics']
