/* smd_hotpath.h — C ABI of the MI355X (gfx950) view-synthesis loss hot path.
 *
 * This is the drop-in boundary for the ONE path this repository accelerates: the self-supervised
 * view-synthesis loss of jspenmar/slowtv_monodepth.  The reference has no FFI of its own (it is pure
 * Python on ATen), so each entry point below names the reference Python interface it replaces; the
 * ctypes binding a maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All pointers are DEVICE pointers to contiguous fp32 (or uint8 where stated) arrays in the
 *     reference's own layouts (NCHW images, row-major 4x4 matrices).  Inputs are const; the library
 *     never allocates, frees or retains a pointer; the caller (PyTorch) owns every buffer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Nothing synchronises.
 *   - Alignment: every pointer handed in (operands, outputs, workspaces) is 16-BYTE ALIGNED.  The kernels go through naturally aligned vector
 *     types (16-byte float4 rows, float2 pairs, dwords over bf16 rows); what they do at an element-aligned base is undefined.  Exceptions, read and
 *     written one element at a time: the per-channel vectors of smd_bn_* (running statistics, saved mean / inverse deviation: rows of a (2,C) array)
 *     and the per-pixel statistics rows of smd_layernorm_cf_* need only their element's alignment.  An allocator's blocks satisfy this; a contiguous
 *     view at a storage offset may not, and the Python layer copies such an operand before the call (`_device._aligned`).
 *   - Return value: 0 on success, negative on error (SMD_E_*); smd_last_error() returns the message
 *     for the calling thread.
 *   - Symbols: b batch, n support frames, S scales, (h, w) image size.  Every (S,b,...) tensor is
 *     scale-major, matching the `torch.stack(list(depths.values()))` of src/core/handlers.py:48.
 */
#ifndef SMD_HOTPATH_H
#define SMD_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMD_ABI_VERSION 8

#define SMD_OK 0
#define SMD_E_INVALID (-1)     /* bad argument (null pointer, size out of range, unsupported flag combination) */
#define SMD_E_LAUNCH (-2)      /* hipLaunch / hipGetLastError failure */
#define SMD_E_WORKSPACE (-3)   /* workspace too small: call the matching *_workspace_bytes() */
#define SMD_E_UNSUPPORTED (-4) /* the request exists, but not in this build / not for these arguments (the caller takes the general path) */

/* flags for smd_image_recon_* / smd_recon_reduce_* */
#define SMD_USE_MIN 0x1        /* ReconstructionLoss(use_min=True): min over supports, else mean (reconstruction.py:43-44) */
#define SMD_USE_AUTOMASK 0x2   /* ReconstructionLoss(use_automask=True) (reconstruction.py:59-77) */
#define SMD_LOSS_L1 0x4        /* loss_name='l1' (DenseL1Error) instead of 'ssim' (PhotoError 0.85/0.15) */
#define SMD_NEED_K_GRAD 0x8    /* backward also emits dL/dK and dL/dK_inv (learned intrinsics) */
#define SMD_USE_EDGES 0x10     /* SmoothReg(use_edges=True) (smooth.py:91-94) */
#define SMD_LOSS_L2 0x20       /* DenseL2Error (photometric.py:17-20; loss_name='l2', un-fused operators only) */
#define SMD_MASK_EXPLAINABILITY 0x80   /* smd_recon_reduce_*: ReconstructionLoss(mask_name='explainability'): err * mask (reconstruction.py:55) */
#define SMD_MASK_UNCERTAINTY 0x100     /* smd_recon_reduce_*: mask_name='uncertainty': err * exp(-mask) + mask (reconstruction.py:56) */
#define SMD_BWD_SKIP_DEAD_ROWS 0x400   /* smd_image_recon*_bwd: the liveness-gated row loop — a wave scans the `sel` rows of its strip first and then re-synthesises,
                                        * scores and back-propagates only the rows a pixel of its columns routes gradient through.  Same result bit for bit; all-masked
                                        * input: 52 instead of 117 us at 12x192x640; pays from ~75 % dead (row, strip) units on, costs 12-24 % where every row is live
                                        * (profiles/r04_skip_regimes.txt).  Default: off.  (The knob `bwd_skip`, smd_set_knob, overrides.) */
#define SMD_BWD_NO_LIVE 0x1000         /* smd_image_recon*_bwd, smd_loss_path_bwd: do not consult the forward's liveness table (the caller knows that a launch-shape knob
                                        * changed between the forward that filled it and this call: the table's strip heights would be read with another partition) */
#define SMD_USE_LAPLACIAN 0x200        /* smd_disp_smooth_*: SmoothReg(use_laplacian=True): second-order differences (smooth.py:33-48) */
#define SMD_EDGES_READY 0x800  /* smd_disp_smooth_fwd: `edge_weights` was already filled by smd_disp_smooth_prep() for this frame and pyramid */
#define SMD_PACKED_READY 0x40  /* smd_image_recon_*_fwd: `supp_packed` was already filled by smd_image_recon_prep() for these frames */
/* RegressionLoss (src/losses/regression.py:40-75) */
#define SMD_REGR_L1 0x0
#define SMD_REGR_LOG_L1 0x1
#define SMD_REGR_BERHU 0x2
#define SMD_REGR_INVERT 0x4    /* RegressionLoss(invert=True): both inputs through to_inv first (:70) */
#define SMD_REGR_AUTOMASK 0x8  /* smd_hints_regr_*: RegressionLoss(use_automask=True): the Depth-Hints automask of src/core/handlers.py:236-256 from `err` */

#define SMD_MAX_SCALES 8
#define SMD_MAX_SUPPORTS 8
#define SMD_SEL_MASKED 255     /* value of `sel` where automasking removed the pixel */

const char* smd_last_error(void);
int smd_abi_version(void);

/* Launch-shape knobs.  Process-wide overrides of the built-in heuristics that choose between partitions / code paths which MUST give the
 * same results: rows per strip, the tapered partition, shared LDS ring vs. per-wave loads in the forward, the backward's two row loops,
 * guest work vs. launches of their own.  They exist so that the parity tests can pin both sides of each such choice and compare; the
 * library never reads the environment.  Names: fwd_rh bwd_rh fwd_taper_b bwd_taper_b fwd_taper_rh bwd_taper_rh fwd_ni fwd_share bwd_skip
 * bwd_wps bwd_guest_finalize bwd_direct_level loss_path_guests bwd_live bwd_scales_block conv_two_tiles metrics_store_pred.
 * smd_set_knob: 0, SMD_E_INVALID for a name that is not in this list. */
int smd_set_knob(const char* name, int value);
void smd_reset_knobs(void);

/* ------------------------------------------------------------------------------------------------
 * K0 — upsample + disparity->depth.  Replaces, per scale, `ops.interpolate_like(disp, imgs, 'bilinear')`
 * followed by `to_scaled(.., min, max)[1]` or `to_inv` (src/core/trainer.py:316-321, src/tools/ops.py:311-314,
 * src/tools/geometry.py:62-90).
 *   disp[s]        : (b,1,hs[s],ws[s])  sigmoid disparity of scale s (host array of S device pointers)
 *   depth_up       : (S,b,h,w) out     depth
 *   disp_up        : (S,b,h,w) out or NULL — the upsampled (un-scaled) disparity (`fwd['disp_up']`)
 *   min_depth/max_depth <= 0 mean "not set" (both unset -> to_inv of the raw disparity).
 * Backward: (depth_up, g_depth_up) (S,b,h,w) -> g_disp[s] (b,1,hs,ws), overwritten.  Needs only the forward's
 * OUTPUT (d depth/d d = -depth^2 on the pass-through branch), not the low-resolution disparity. */
int smd_disp_to_depth_fwd(const float* const* disp, const int* hs, const int* ws, int S, int b, int h, int w,
                          float min_depth, float max_depth, float* depth_up, float* disp_up, void* stream);
size_t smd_disp_to_depth_workspace_bytes(const int* hs, const int* ws, int S, int b, int h, int w);
int smd_disp_to_depth_bwd(const int* hs, const int* ws, int S, int b, int h, int w, float min_depth, float max_depth,
                          const float* depth_up, const float* g_depth_up, float* const* g_disp,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused image reconstruction.  Replaces `handlers.image_recon(crit, synth, depths, None, imgs, supp_imgs, Ts, Ks)`
 * (src/core/handlers.py:14-67) = ViewSynth.forward (src/tools/geometry.py:366-391) + ReconstructionLoss.forward
 * (src/losses/reconstruction.py:98-126) + PhotoError (src/losses/photometric.py:54-88), without materialising
 * the (n,S*b,...) expansions, point clouds, grids or warped images.
 *   depth   (S,b,h,w)    tgt (b,3,h,w)    supp (n,b,3,h,w)    T (n,b,4,4)    K, K_inv (b,4,4)
 *   noise   (S,b,h,w) or NULL: the `randn_like` draw of reconstruction.py:72; NULL -> counter-based
 *           in-kernel Gaussian keyed by `seed` (statistically equivalent tie-break, different stream)
 *   supp_packed out, smd_packed_supports_bytes() bytes (< 4 GB): what every scale and support shares, produced once per
 *           sample by the forward's prep kernel and kept by the caller for the backward — the supports as padded 12-byte
 *           RGB texels (n,b,h+1,w+1,3), the target as RGB texels (b,h,w,3), and per target pixel the SSIM window sums of the
 *           target and the identity error of the automask (2 x (b,h,w,4)); then a small tail of launch scratch (the K0
 *           row table and the arrival counters of the in-launch reductions; the backward resets its counters, which is
 *           why it takes the buffer non-const).  It depends on the frames only: smd_image_recon_prep() can fill it ahead of
 *           time (e.g. on a side stream while the networks run) and the forward is then called with SMD_PACKED_READY.
 *   err     (S,b,h,w) out or NULL (allowed when n <= 4): per-pixel error after min/mean-reprojection and automasking; the
 *           training path does not need it (the loss is reduced in the kernel) and saves its 4 bytes per pixel and scale
 *   sel     (S,b,h,w) out uint8: winning support index, or SMD_SEL_MASKED where the static error won
 *   loss    (1) out: mean of err  (= `loss_img_recon`)
 *   warp0   (n,b,3,h,w) out or NULL: warped supports of scale 0 (`loss_dict['supp_imgs_warp']`)
 *   workspace: smd_image_recon_workspace_bytes() bytes of scratch (fwd and bwd may share it).
 * Backward (loss is the only differentiable output):
 *   g_loss  (1) device scalar dL/dloss
 *   g_depth (S,b,h,w) out;  g_T (n,b,4,4) out (row 3 zero);  g_K, g_Kinv (b,4,4) out or NULL
 *           (required iff SMD_NEED_K_GRAD; only the 3x3 / 2x3 blocks the path reads are non-zero). */
size_t smd_image_recon_workspace_bytes(int b, int n, int S, int h, int w);
size_t smd_packed_supports_bytes(int b, int n, int h, int w);
/* The frame-only half of the forward (texel repack, target window sums, identity error; reference: the un-warped `source`
 * branch of src/losses/reconstruction.py:70-71 and the per-scale re-reads of handlers.py:45-56).  `flags` must carry the same
 * SMD_USE_MIN / SMD_USE_AUTOMASK / SMD_LOSS_L1 bits as the forward that follows.  hs, ws (S entries) describe the disparity
 * pyramid of the K0-fused forward (its row table is built here); NULL / S = 0 for the depth-input forward. */
int smd_image_recon_prep(const float* tgt, const float* supp, float* supp_packed, const int* hs, const int* ws, int S,
                         int b, int n, int h, int w, int flags, void* stream);
/* Supports one forward launch holds in registers (4 unless the knob fwd_ni overrides it): `err` may be NULL only when n <= this. */
int smd_image_recon_supports_per_pass(void);
int smd_image_recon_fwd(const float* depth, const float* tgt, const float* supp, const float* T, const float* K,
                        const float* K_inv, const float* noise, uint64_t seed, float* supp_packed, float* err, uint8_t* sel, float* loss,
                        float* warp0, void* workspace, size_t workspace_bytes,
                        int b, int n, int S, int h, int w, int flags, void* stream);
int smd_image_recon_bwd(const float* depth, const float* tgt, float* supp_packed, const float* T, const float* K,
                        const float* K_inv, const uint8_t* sel, const float* g_loss,
                        float* g_depth, float* g_T, float* g_K, float* g_Kinv, void* workspace, size_t workspace_bytes,
                        int b, int n, int S, int h, int w, int flags, void* stream);

/* K0 fused into the reconstruction: the same operator fed with the network's multi-scale sigmoid
 * disparity instead of the up-sampled depth.  Replaces, in one launch sequence, `forward_postprocess`' per-scale
 * `ops.interpolate_like` + `to_scaled` / `to_inv` (src/core/trainer.py:316-321) AND `handlers.image_recon`
 * (src/core/handlers.py:14-67): the fused kernel up-samples the disparity of the rows it is about to warp, converts it to
 * depth and writes `depth_up` (S,b,h,w) once (the backward and `fwd['depth_up']` read it); no K0 launch is needed.
 *   disp[s] (b,1,hs[s],ws[s]) host array of S device pointers;  min_depth / max_depth <= 0 mean "not set" (to_inv).
 * Backward: recomputes nothing of K0 — it reads depth_up, adds `g_depth_up_in` (S,b,h,w; the gradient reaching depth_up from
 * other consumers, or NULL), applies d depth / d disparity inside the fused backward and sends the result through the
 * bilinear adjoint -> g_disp[s] (b,1,hs,ws), overwritten.  Workspace: smd_image_recon_disp_workspace_bytes(). */
size_t smd_image_recon_disp_workspace_bytes(const int* hs, const int* ws, int S, int b, int n, int h, int w);
int smd_image_recon_disp_fwd(const float* const* disp, const int* hs, const int* ws, int S, float min_depth, float max_depth,
                             const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                             const float* noise, uint64_t seed, float* supp_packed, float* depth_up, float* err, uint8_t* sel, float* loss,
                             float* warp0, void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream);
int smd_image_recon_disp_bwd(const int* hs, const int* ws, int S, float min_depth, float max_depth, const float* depth_up,
                             float* supp_packed, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                             const float* g_loss, const float* g_depth_up_in, float* const* g_disp, float* g_T, float* g_K, float* g_Kinv,
                             void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream);

/* The whole `forward_loss` of the kbr configuration as ONE operator (round 5): `handlers.image_recon` on the K0-fused path +
 * `handlers.disp_smooth` with `SmoothReg(use_edges=True)` + the weighted sum `sum_k w_k l_k` (src/core/trainer.py:383-392, 436-437,
 * 462-464) — and, in the backward, the chain rule through `T_from_AAt` (+ `T.inverse()`) and `build_K` / `resize_K` down to the pose
 * network's outputs (src/core/trainer.py:250-262).  Five launches for forward + backward where the separate operators need eleven:
 *   forward:  the K0-fused reconstruction launch, with the smoothness sweep as guest blocks behind its own and the weighted sum formed
 *             in-launch by whichever of the two final reducers arrives second -> loss3 = {total, l_recon, l_smooth};
 *   backward: the fused reconstruction backward; the K0 adjoint's first launch, carrying as guests the pose epilogue — continued in the
 *             same wave to g_aa, g_t (and g_fs, g_cs) — and the smoothness adjoint, which WRITES its share into g_disp[s] (adds, for a
 *             level of the image's own size that the reconstruction backward already wrote); the K0 adjoint's second launch ADDS.
 * flags: SMD_USE_MIN | SMD_USE_AUTOMASK | SMD_USE_EDGES (required) | SMD_PACKED_READY | SMD_EDGES_READY | SMD_NEED_K_GRAD |
 *        SMD_BWD_SKIP_DEAD_ROWS.  In-kernel tie-break noise (`seed`), no error map, no warped images: the trainer's hot call.
 * Returns SMD_E_UNSUPPORTED (nothing launched) for what it does not serve — loss_name 'l1', more than four supports, a smoothness term
 * other than first-order edge-aware, fewer than two pyramid levels, a level taller than the image: the caller then uses the operators above.
 *   scale_keys[s]: the `s` of `loss_s / 2**s` (src/core/handlers.py:279);  stats (S,b,2): per-image (mean, E) kept for the backward;
 *   edge_weights: smd_disp_smooth_edge_weight_bytes() (filled here unless SMD_EDGES_READY);  w_recon / w_smooth: the frozen loss weights;
 *   g_loss: device scalar dL/d total.  aa, t, invert (n*b rows, as given to smd_pose_fwd) with g_aa, g_t, and fs, cs with g_fs, g_cs
 *   (needs SMD_NEED_K_GRAD), are optional (all NULL: stop at g_T / g_K / g_Kinv, which are always written).
 * Same values as the separate operators: l_recon, l_smooth, sel, depth_up and every gradient bit for bit (tests/test_gpu_parity.py). */
size_t smd_loss_path_workspace_bytes(const int* hs, const int* ws, int S, int b, int n, int h, int w);
int smd_loss_path_fwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, float min_depth, float max_depth,
                      const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv, uint64_t seed,
                      float* supp_packed, float* edge_weights, float* depth_up, uint8_t* sel, float* loss3, float* stats,
                      void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, float w_recon, float w_smooth, void* stream);
int smd_loss_path_bwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, float min_depth, float max_depth,
                      const float* depth_up, float* supp_packed, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                      const float* stats, const float* edge_weights, const float* g_loss, float w_recon, float w_smooth,
                      const float* aa, const float* t, const uint8_t* invert, const float* fs, const float* cs,
                      float* const* g_disp, float* g_T, float* g_K, float* g_Kinv, float* g_aa, float* g_t, float* g_fs, float* g_cs,
                      void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-aware disparity smoothness over all scales.  Replaces `handlers.disp_smooth(crit, disps, imgs)`
 * (src/core/handlers.py:262-281) = per scale SmoothReg.forward (src/regularizers/smooth.py:71-97) on the
 * bilinearly resized image, then mean_s(loss_s / 2^s).  SMD_USE_LAPLACIAN selects the second-order form (smooth.py:33-48);
 * use_blur: the host side blurs the disparity and the resized image with smd_gaussian_blur3x3 and calls this path on the results (first-order form).
 *   disp[s] (b,1,hs,ws)   img (b,3,h,w)   scale_keys[s]: the dictionary key of scale s (loss_s is divided by 2^key;
 *   NULL -> key = s)
 *   loss (1) out;  stats (S,b,2) out: per (scale, sample) {mean disparity, un-normalised edge sum E} kept for backward
 *   disp_grad, image_grad: (b,1,hs[0],ws[0]) out or NULL (aux maps of the first scale, smooth.py:86,89)
 *   edge_weights: required with SMD_USE_EDGES, else NULL; smd_disp_smooth_edge_weight_bytes() bytes holding
 *   {exp(-mean_c |dI/dx|), exp(-mean_c |dI/dy|)} per pixel of every scale (and a few launch counters behind them).  They depend on the frames
 *   alone: smd_disp_smooth_prep() fills the buffer ahead of time (e.g. on a side stream while the networks run, next to
 *   smd_image_recon_prep) and the forward is then called with SMD_EDGES_READY; without that flag the forward fills it first itself.
 *   Handing the same buffer to the backward spares it every image access.
 * Backward: g_disp[s] (b,1,hs,ws) out. */
/* SmoothReg(use_blur=True) (smooth.py:21): `kornia.filters.gaussian_blur2d(x, kernel_size=(3, 3), sigma=(1, 1))` on `planes` planes of h x w
 * floats — separable 3-tap Gaussian (0.27406862, 0.45186276, 0.27406862), reflect border (kornia 0.6.10 filter2d_separable; restated from its
 * published source, parity unpinned: the library is absent from the build image).  adjoint != 0: the transpose of that linear map (backward).
 * x != out; h, w >= 2. */
int smd_gaussian_blur3x3(const float* x, float* out, int planes, int h, int w, int adjoint, void* stream);
size_t smd_disp_smooth_workspace_bytes(const int* hs, const int* ws, int S, int b);
size_t smd_disp_smooth_edge_weight_bytes(const int* hs, const int* ws, int S, int b);
int smd_disp_smooth_prep(const float* img, const int* hs, const int* ws, int S, int b, int h, int w, int flags, float* edge_weights, void* stream);
int smd_disp_smooth_fwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, int b,
                        const float* img, int h, int w, int flags, float* loss, float* stats, float* disp_grad, float* image_grad,
                        float* edge_weights, void* workspace, size_t workspace_bytes, void* stream);
int smd_disp_smooth_bwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, int b,
                        const float* img, int h, int w, int flags, const float* stats, const float* edge_weights,
                        const float* g_loss, float* const* g_disp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Un-fused operators (class-level drop-ins for callers that hold the intermediate tensors).
 *
 * smd_view_synth_*: `ViewSynth.forward(input, depth, T, K, K_inv)` (src/tools/geometry.py:366-391) for any
 * channel count C.  B is the already-expanded batch.  warp (B,C,h,w); depth_warp (B,1,h,w) or NULL;
 * mask_valid (B,1,h,w) uint8 or NULL.  Backward takes g_warp (and optional g_depth_warp) and emits
 * g_input (B,C,h,w) or NULL, g_depth (B,1,h,w), g_T (B,4,4), g_K / g_Kinv (B,4,4) or NULL. */
size_t smd_view_synth_workspace_bytes(int B, int h, int w);
int smd_view_synth_fwd(const float* input, const float* depth, const float* T, const float* K, const float* K_inv,
                       float* warp, float* depth_warp, uint8_t* mask_valid, int B, int C, int h, int w, void* stream);
int smd_view_synth_bwd(const float* input, const float* depth, const float* T, const float* K, const float* K_inv,
                       const float* g_warp, const float* g_depth_warp,
                       float* g_input, float* g_depth, float* g_T, float* g_K, float* g_Kinv,
                       void* workspace, size_t workspace_bytes, int B, int C, int h, int w, void* stream);

/* smd_photo_error_*: `PhotoError(weight_ssim)(pred, target)`, `DenseL1Error` with SMD_LOSS_L1, `DenseL2Error` with SMD_LOSS_L2
 * (src/losses/photometric.py:11-20, 54-88) for any channel count C (images: 3; `feat_recon` features: 64..256).
 * weight_ssim in [0, 1] (photometric.py:65-73; `ReconstructionLoss` builds 0.85; 0 = L1 only, 1 = SSIM only); ignored by L1 / L2.
 * pred, target (N,C,h,w) -> err (N,1,h,w).  Backward: g_err (N,1,h,w) -> g_pred (N,C,h,w). */
size_t smd_photo_error_workspace_bytes(int N, int C, int h, int w);
int smd_photo_error_fwd(const float* pred, const float* target, float* err, int N, int C, int h, int w, int flags, float weight_ssim, void* stream);
int smd_photo_error_bwd(const float* pred, const float* target, const float* g_err, float* g_pred,
                        void* workspace, size_t workspace_bytes, int N, int C, int h, int w, int flags, float weight_ssim, void* stream);

/* smd_regression_*: `RegressionLoss.forward(pred, target, mask)` (src/losses/regression.py:69-75) used by the
 * `stereo_const` and `depth_regr` handlers (src/core/handlers.py:152-259).  pred, target: N floats; mask: N uint8 or
 * NULL (all ones); flags: SMD_REGR_{L1,LOG_L1,BERHU} | SMD_REGR_INVERT.  -> loss (1), err (N, `err_regr`) or NULL,
 * stats (8 floats, handed back to the backward).  Backward: g_loss (1) -> g_pred and/or g_target (N). */
size_t smd_regression_workspace_bytes(size_t N);
int smd_regression_fwd(const float* pred, const float* target, const uint8_t* mask, size_t N, int flags, float* loss, float* err,
                       float* stats, void* workspace, size_t workspace_bytes, void* stream);
int smd_regression_bwd(const float* pred, const float* target, const uint8_t* mask, size_t N, int flags, float* stats,
                       const float* g_loss, float* g_pred, float* g_target, void* workspace, size_t workspace_bytes, void* stream);

/* smd_depth_metrics: the training-time validation metrics of `MonoDepthModule.compute_metrics` (src/core/trainer.py:531-552, src/utils/metrics.py)
 * in one call.  pred (b,1,h,w) depth, target (b,1,H,W) (any size relation): p0 = clamp(bilinear(pred -> (H,W), align_corners=False), min, max);
 * valid = min < target < max (NaN: invalid); both per-sample LOWER medians (rank (n-1)/2, torch.nanmedian) over the valid pixels by an exact radix
 * select; p = clamp(p0 * med_t/med_p, min, max).
 * -> values (b,5): MAE, RMSE, LogSI (x100), AbsRel (x100), Acc (x100; count(q < 1.25) over the SUM of q = max(t/p, p/t), as the reference's DeltaAcc),
 *    NaN for a sample without a valid pixel; medians (b,2): med_p, med_t; counts (b) int32: valid pixels.
 * Deterministic (integer atomics and fixed-order fp64 sums only); no synchronisation, no copy to the host; the workspace may be reused dirty. */
size_t smd_depth_metrics_workspace_bytes(int b, int H, int W);
int smd_depth_metrics(const float* pred, const float* target, int b, int h, int w, int H, int W, float min_depth, float max_depth,
                      float* values, float* medians, int* counts, void* workspace, size_t workspace_bytes, void* stream);

/* smd_recon_reduce_*: the reduction half of `ReconstructionLoss.forward` on per-support error maps
 * (reconstruction.py:43-57, 59-77, 125).  err_warp (n,B,h,w); err_static (n,B,h,w) (required with SMD_USE_AUTOMASK);
 * mask (B,n,h,w) or NULL: the predictive weighting mask of `apply_mask` (reconstruction.py:46-57), reference layout, applied to the
 * warped AND the static errors before the reductions, with SMD_MASK_EXPLAINABILITY (err * mask) or SMD_MASK_UNCERTAINTY
 * (err * exp(-mask) + mask); noise (B,h,w) or NULL (in-kernel tie-break noise keyed by `seed`).
 * -> err (B,h,w), sel (B,h,w) uint8, loss (1).  Backward -> g_err_warp (n,B,h,w) and, with a mask, g_mask (B,n,h,w)
 * (then err_warp / err_static / mask are read again; all three may be NULL without a mask). */
size_t smd_recon_reduce_workspace_bytes(int B, int h, int w);
int smd_recon_reduce_fwd(const float* err_warp, const float* err_static, const float* mask, const float* noise, uint64_t seed,
                         float* err, uint8_t* sel, float* loss, void* workspace, size_t workspace_bytes,
                         int n, int B, int h, int w, int flags, void* stream);
int smd_recon_reduce_bwd(const uint8_t* sel, const float* g_loss, float* g_err_warp, const float* err_warp, const float* err_static,
                         const float* mask, float* g_mask, int n, int B, int h, int w, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Monodepth decoder glue: everything between two 3x3 convolutions of
 * `MonodepthDecoder.forward` (src/networks/decoders/monodepth.py:71-89; conv_block / conv3x3 with reflection padding,
 * src/networks/decoders/utils.py:44-54) as one gather that writes the next convolution's padded input.
 *
 * smd_elu_pad_*:        out (B,C,h+2,w+2) = reflect_pad1(apply_elu ? elu(x + bias) : x + bias),  x (B,C,h,w) the raw
 *                       (bias-free) conv output, bias (C) or NULL.
 * smd_elu_up_cat_pad_*: out (B,Ca+Cs,2h+2,2w+2) = reflect_pad1(cat(nearest_x2(elu(a + bias)), skip)),  a (B,Ca,h,w),
 *                       bias (Ca) or NULL, skip (B,Cs,2h,2w) or NULL with Cs = 0.
 * Backward: g_out -> g_x / (g_a, g_skip) and g_bias (C) or NULL (needs the workspace); g_a or g_skip may be NULL.
 * dtypes: bit 0 (SMD_GLUE_A_BF16) x / a and their gradients are bfloat16, bit 1 (SMD_GLUE_SKIP_BF16) skip and its gradient,
 * bit 2 (SMD_GLUE_OUT_BF16) out and its gradient — for decoders running under bf16 autocast; bias, g_bias and the arithmetic are fp32. */
#define SMD_GLUE_A_BF16 1
#define SMD_GLUE_SKIP_BF16 2
#define SMD_GLUE_OUT_BF16 4
size_t smd_decoder_glue_workspace_bytes(int B, int C, int h, int w);
int smd_elu_pad_fwd(const void* x, const float* bias, void* out, int B, int C, int h, int w, int apply_elu, int dtypes, void* stream);
int smd_elu_pad_bwd(const void* x, const float* bias, const void* g_out, void* g_x, float* g_bias,
                    void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int apply_elu, int dtypes, void* stream);
int smd_elu_up_cat_pad_fwd(const void* a, const float* bias, const void* skip, void* out, int B, int Ca, int Cs, int h, int w, int dtypes,
                           void* stream);
int smd_elu_up_cat_pad_bwd(const void* a, const float* bias, const void* g_out, void* g_a, void* g_skip, float* g_bias,
                           void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int dtypes, void* stream);

/* Output head of the Monodepth decoder (ABI 7, round 5; reference: src/networks/decoders/monodepth.py:52, 86-87 — `self.act(self.out[i](x))` with
 * `conv3x3(num_ch_dec[i], 1)`, decoders/utils.py:44-46): y (B,1,h,w) = act(conv3x3(xp; weight (1,C,3,3)) + bias (1) or NULL), where xp (B,C,h+2,w+2)
 * is the reflection-padded activation smd_elu_pad_fwd leaves; act 0: identity, 1: sigmoid.  A one-output-channel convolution is a stencil: three
 * streaming kernels, fp32, deterministic.  Backward: g_y and the saved y -> g_xp (B,C,h+2,w+2) (or NULL), g_weight (1,C,3,3) with g_bias (1) (g_weight
 * NULL: neither; g_bias may be NULL alone); the weight gradient needs the workspace.
 * act | SMD_HEAD_X_BF16 (ABI 8): xp and g_xp are bfloat16 (the decoder under bf16 autocast: `cfg/kbr/default.yaml` trains in bf16-mixed — the glue kernels
 * then leave a bf16 activation; these kernels are HBM-bound, so half the bytes); weights, bias, y, g_y and every sum stay fp32. */
#define SMD_HEAD_X_BF16 2
size_t smd_conv3x3_head_workspace_bytes(int B, int C, int h, int w);
int smd_conv3x3_head_fwd(const void* xp, const float* weight, const float* bias, float* y, int B, int C, int h, int w, int act, void* stream);
int smd_conv3x3_head_bwd(const void* xp, const float* weight, const float* y, const float* g_y, void* g_xp, float* g_weight, float* g_bias,
                         void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int act, void* stream);

/* Output heads with a few output channels: the predictive-mask decoder (additive to ABI 8; reference: src/networks/depth.py:12, 108-114 —
 * `MonodepthDecoder(out_ch=num_ch_mask, out_act=MASKS[mask_name])`, MASKS = {'explainability': 'sigmoid', 'uncertainty': 'relu'}; the heads themselves
 * src/networks/decoders/monodepth.py:52, 86-87 — `self.act(self.out[i](x))` with `conv3x3(num_ch_dec[i], out_ch)`):
 * y (B,n,h,w) = act(conv3x3(xp; weight (n,C,3,3)) + bias (n) or NULL), 1 <= n <= 4, xp (B,C,h+2,w+2) the reflection-padded activation smd_elu_pad_fwd
 * leaves.  The padded activation is read once for all n channels (n accumulators per output row).  act: SMD_HEADN_NONE / _SIGMOID / _RELU, ored with
 * SMD_HEADN_X_BF16 when xp and g_xp are bfloat16 (the decoder under bf16 autocast); weights, bias, y, g_y and every sum stay fp32.
 * Backward, from g_y and the saved y (gp = g_y * act'(y); relu: y > 0): _bwd_data -> g_xp (B,C,h+2,w+2), summed over the n channels per padded position;
 * _bwd_wgt -> g_weight (n,C,3,3) and g_bias (n) or NULL, per-block partial sums in the workspace and a fixed-order fp64 final sum.  Deterministic. */
#define SMD_HEADN_NONE 0
#define SMD_HEADN_SIGMOID 1
#define SMD_HEADN_RELU 2
#define SMD_HEADN_X_BF16 4
size_t smd_conv3x3_headn_workspace_bytes(int B, int C, int n, int h, int w);
int smd_conv3x3_headn_fwd(const void* xp, const float* weight, const float* bias, float* y, int B, int C, int n, int h, int w, int act, void* stream);
int smd_conv3x3_headn_bwd_data(const float* weight, const float* y, const float* g_y, void* g_xp, int B, int C, int n, int h, int w, int act, void* stream);
int smd_conv3x3_headn_bwd_wgt(const void* xp, const float* y, const float* g_y, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                              int B, int C, int n, int h, int w, int act, void* stream);

/* Multi-scale, multi-channel bilinear up-sampling (additive to ABI 8).  Replaces, per scale, `ops.interpolate_like(mask, imgs, mode='bilinear')`
 * (src/core/trainer.py:323-324, src/tools/ops.py:311-314; F.interpolate with align_corners=False) and the `torch.stack` of src/core/handlers.py:47:
 *   x[s] (b,n,hs[s],ws[s]) (host array of S device pointers)  ->  out (S,b,n,h,w), one launch.
 * Backward: g_out (S,b,n,h,w) -> g_x[s] (b,n,hs,ws), overwritten: the exact adjoint, a gather per source pixel (no atomics), one launch.
 * b*n <= 65535.  (K0 above is the one-channel form that also converts to depth.) */
int smd_upsample_stack_fwd(const float* const* x, const int* hs, const int* ws, int S, int b, int n, int h, int w, float* out, void* stream);
int smd_upsample_stack_bwd(const int* hs, const int* ws, int S, int b, int n, int h, int w, const float* g_out, float* const* g_x, void* stream);

/* Mean over scales of per-scale means (additive to ABI 8): loss = mean_s( mean(f(x[s])) ) for S tensors of numel[s] elements each, one launch.  Replaces
 * `handlers.disp_mask` / `handlers.disp_occ` (src/core/handlers.py:314-347) around `MaskReg` (src/regularizers/mask.py:29 —
 * `F.binary_cross_entropy(x, ones_like(x))`, i.e. f(x) = -max(log x, -100) with ATen's clamp) and `OccReg` (src/regularizers/occlusion.py:39 — f(x) = sign * x).
 * mode: SMD_MEAN_BCE_ONES, SMD_MEAN_IDENTITY, SMD_MEAN_NEGATE.  Per-block partial sums in fp32; the block that arrives last adds them in fp64 in block order.
 * workspace: smd_scale_mean_workspace_bytes() bytes whose first 4 bytes, the arrival counter, must be ZERO on entry; the forward leaves them zero, so a
 * buffer cleared once can be kept and reused by calls that are ordered on one stream.
 * Backward: g_x[s] = g_loss[0] * f'(x[s]) / (S * numel[s]), one launch; for SMD_MEAN_BCE_ONES f'(x) = (x - 1) / max((1 - x) x, 1e-12), ATen's
 * binary_cross_entropy_backward (x may be NULL for the two linear modes). */
#define SMD_MEAN_BCE_ONES 0
#define SMD_MEAN_IDENTITY 1
#define SMD_MEAN_NEGATE 2
size_t smd_scale_mean_workspace_bytes(const long long* numel, int S);
int smd_scale_mean_fwd(const float* const* x, const long long* numel, int S, int mode, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int smd_scale_mean_bwd(const float* const* x, const long long* numel, int S, int mode, const float* g_loss, float* const* g_x, void* stream);

/* The decoder's thin up-convolutions (ABI 7, round 5; reference: src/networks/decoders/monodepth.py:45-50, 80-84 — `ConvELU(cin, 16)`; the bias and the ELU
 * are the next glue kernel's): y (B,16,h,w) = conv3x3(xp (B,C,h+2,w+2); weight (16,C,3,3)), bias-free, C = 16 or 32 (anything else: SMD_E_UNSUPPORTED),
 * on the matrix cores in fp32 (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation; the order of the sum differs from ATen's).
 * Backward: g_y (B,16,h,w) -> g_xp (B,C,h+2,w+2) (or NULL) and g_weight (16,C,3,3) (or NULL; needs xp and the workspace); deterministic. */
size_t smd_conv3x3_thin_workspace_bytes(int B, int C, int h, int w);
int smd_conv3x3_thin_fwd(const float* xp, const float* weight, float* y, int B, int C, int h, int w, void* stream);
int smd_conv3x3_thin_bwd(const float* xp, const float* weight, const float* g_y, float* g_xp, float* g_weight, void* workspace, size_t workspace_bytes,
                         int B, int C, int h, int w, void* stream);

/* The decoder's wide up-convolutions (ABI 8, round 6; reference: src/networks/decoders/monodepth.py:40-50, 71-84 — `ConvELU(cin, cout)`, decoders/utils.py:44-54;
 * the bias and the ELU are the next glue kernel's): y (B,CO,h,w) = conv3x3(xp (B,C,h+2,w+2); weight (CO,C,3,3)), bias-free, fp32 in and out, computed on the
 * bf16 matrix cores with every fp32 operand split exactly into `pieces` bf16 pieces (3: six bf16 products per fp32 product, what is dropped is below
 * 2^-25 of the product — fp32-class results at 6/16 of the f32 MFMA's time; 2: three products, 16 significant bits, an experiment setting, never the
 * library's choice).  smd_conv3x3_mfma_pack writes the weights' pieces in the operand order of the forward (wp_fwd) and of the data gradient (wp_bwd), each
 * smd_conv3x3_mfma_packed_bytes(C, CO, pieces) bytes (either may be NULL; the size counts C up to a multiple of 32: the data-gradient image is whole tiles of
 * 32 input channels); the backward reads what the forward's pack left.  For the stride-2 data gradient (smd_conv3x3s2d_mfma_bwd_data below) the pack also
 * writes wp_bwd where C % 16 == 0 with CO % 32 == 0 and pieces == 3; the rows past C of its last tile are not written and not used.
 * pieces = 1 (ABI 8): the tensors xp, y, g_y, g_xp are BFLOAT16 (the decoder under bf16 autocast, `cfg/kbr/default.yaml`): one bf16 product per product, the
 * weights enter as their bf16 rounding (what autocast hands a bf16 convolution), accumulation and the weight gradient stay fp32.
 * Served: pieces in {1, 2, 3}; forward C % 16 == 0 and CO % 32 == 0; data gradient CO % 16 == 0 and C % 32 == 0; weight gradient CO % 32 == 0 (any C); and the
 * thin last stage, CO == 16 with C == 16 or 32 (`ConvELU(cin, 16)`, monodepth.py:45-50: all three operators, on the 16 x 16 x 32 form of the instruction);
 * anything else SMD_E_UNSUPPORTED, nothing launched.  g_xp (B,C,h+2,w+2) is the gradient of the PADDED input.  Every call takes a workspace of
 * smd_conv3x3_mfma_workspace_bytes (the coarse decoder levels — few pixels, thousands of K — split K over blocks and add the splits' outputs in split
 * order; the weight gradient leaves per-block sums that a fixed-order fp64 second stage adds — in slices, whose fp64 sums sit behind the per-block sums in the
 * same workspace).  Sizes: one sample's xp and one sample's g_y under 2 GiB each, B x ceil(C / 32) x ceil(CO / 32) < 65536 (else SMD_E_INVALID).  Deterministic. */
size_t smd_conv3x3_mfma_packed_bytes(int C, int CO, int pieces);
size_t smd_conv3x3_mfma_workspace_bytes(int B, int C, int CO, int h, int w);
int smd_conv3x3_mfma_pack(const float* weight, void* wp_fwd, void* wp_bwd, int C, int CO, int pieces, void* stream);
int smd_conv3x3_mfma_fwd(const void* xp, const void* wp_fwd, void* y, void* workspace, size_t workspace_bytes,
                         int B, int C, int CO, int h, int w, int pieces, void* stream);
int smd_conv3x3_mfma_bwd_data(const void* g_y, const void* wp_bwd, void* g_xp, void* workspace, size_t workspace_bytes,
                              int B, int C, int CO, int h, int w, int pieces, void* stream);
int smd_conv3x3_mfma_bwd_weight(const void* xp, const void* g_y, float* g_weight, void* workspace, size_t workspace_bytes,
                                int B, int C, int CO, int h, int w, int pieces, void* stream);

/* The ResNet encoders' 3x3 stride-1 convolutions (ABI 8; reference: the timm BasicBlock / Bottleneck built at src/networks/depth.py:95-98,
 * src/networks/pose.py:39-41 — `nn.Conv2d(c, co, 3, 1, padding=1, bias=False)`): y (B,CO,h,w) = conv2d(x (B,C,h,w), weight (CO,C,3,3), padding = 1) with
 * ZERO padding done inside the kernels (no padded copy of any tensor), on the same split-bf16 matrix-core kernels and the same operand images as
 * smd_conv3x3_mfma_* above (pack with smd_conv3x3_mfma_pack, smd_conv3x3_mfma_packed_bytes(C, CO, pieces) bytes each).  fp32 tensors only: pieces 3 (or the
 * experiment's 2); pieces 1 is SMD_E_UNSUPPORTED.  Backward: g_y (B,CO,h,w) -> g_x (B,C,h,w), the gradient of the UNPADDED input; g_weight (CO,C,3,3) from x
 * and g_y.  Served: forward C % 16 == 0 and CO % 32 == 0; data gradient CO % 16 == 0 and C % 32 == 0; weight gradient CO % 32 == 0 (any C); anything else
 * SMD_E_UNSUPPORTED, nothing launched.  Every call takes a workspace of smd_conv3x3z_mfma_workspace_bytes (0: sizes not served; the limits are those of
 * smd_conv3x3_mfma_*).  Deterministic. */
size_t smd_conv3x3z_mfma_workspace_bytes(int B, int C, int CO, int h, int w);
int smd_conv3x3z_mfma_fwd(const float* x, const void* wp_fwd, float* y, void* workspace, size_t workspace_bytes,
                          int B, int C, int CO, int h, int w, int pieces, void* stream);
int smd_conv3x3z_mfma_bwd_data(const float* g_y, const void* wp_bwd, float* g_x, void* workspace, size_t workspace_bytes,
                               int B, int C, int CO, int h, int w, int pieces, void* stream);
int smd_conv3x3z_mfma_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes,
                                 int B, int C, int CO, int h, int w, int pieces, void* stream);

/* The ResNet stem (ABI 8; reference: timm's `conv1 = nn.Conv2d(in_chans, 64, 7, stride=2, padding=3, bias=False)` of the encoders built at
 * src/networks/depth.py:95-98, src/networks/pose.py:39-41): y (B,64,Ho,Wo) = conv2d(x (B,C,H,W), weight (64,C,7,7), stride 2, padding 3), Ho = (H - 1)/2 + 1,
 * Wo = (W - 1)/2 + 1, fp32 NCHW in and out, zero padding inside the kernels, on the split-bf16 matrix-core form of smd_conv3x3_mfma_* (three pieces, six
 * products: fp32-class results).  smd_conv7x7s2_pack writes the forward's weight fragments (smd_conv7x7s2_packed_bytes(C, CO) bytes; part of every forward);
 * smd_conv7x7s2_bwd_weight leaves g_weight (64,C,7,7) from x and g_y through per-block sums and a fixed-order fp64 second stage in a workspace of
 * smd_conv7x7s2_workspace_bytes.  No data gradient (the input is the image).  Served: CO == 64 with C == 3 or 6, any B, H, W >= 1 within one sample's x and
 * y under 2 G elements; both queries return 0 for anything else and the calls SMD_E_UNSUPPORTED / SMD_E_INVALID, nothing launched.  Deterministic. */
size_t smd_conv7x7s2_packed_bytes(int C, int CO);
size_t smd_conv7x7s2_workspace_bytes(int B, int C, int CO, int H, int W);
int smd_conv7x7s2_pack(const float* weight, void* wp, int C, int CO, void* stream);
int smd_conv7x7s2_fwd(const float* x, const void* wp, float* y, int B, int C, int CO, int H, int W, void* stream);
int smd_conv7x7s2_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes,
                             int B, int C, int CO, int H, int W, void* stream);

/* The ResNet encoders' 3x3 stride-2 transition convolutions (ABI 8; reference: `conv1 = nn.Conv2d(c, co, 3, 2, padding=1, bias=False)` of the first BasicBlock
 * of layer2 / layer3 / layer4 of the timm ResNets built at src/networks/depth.py:95-98, src/networks/pose.py:39-41): y (B,CO,Ho,Wo) = conv2d(x (B,C,H,W),
 * weight (CO,C,3,3), stride 2, padding 1), Ho = (H - 1)/2 + 1, Wo = (W - 1)/2 + 1 (odd H, W are legal), fp32 NCHW in and out, ZERO padding done inside the
 * kernels, on the split-bf16 matrix-core form of smd_conv3x3_mfma_* (three pieces, six products: fp32-class results).  The forward reads the forward operand
 * image of smd_conv3x3_mfma_pack(weight, wp_fwd, NULL, C, CO, 3, stream) (smd_conv3x3_mfma_packed_bytes(C, CO, 3) bytes: no pack of its own; part of
 * every forward).  smd_conv3x3s2_mfma_bwd_weight leaves g_weight (CO,C,3,3) from x and g_y (B,CO,Ho,Wo) through per-block sums and the fixed-order fp64
 * second stage (no atomic add, no zeroing pass).  The data gradient: smd_conv3x3s2d_* below.  Both calls take a workspace of smd_conv3x3s2_mfma_workspace_bytes (the coarse levels'
 * forward splits K over blocks and adds the splits' outputs in split order).  Served: C % 16 == 0 and CO % 32 == 0, any B, H, W >= 1 with one sample's x and
 * one sample's y under 2 GiB each and B x ceil(C / 64) x ceil(CO / 64) < 65536; the query returns 0 for anything else and the calls SMD_E_UNSUPPORTED,
 * nothing launched.  Deterministic. */
size_t smd_conv3x3s2_mfma_workspace_bytes(int B, int C, int CO, int H, int W);
int smd_conv3x3s2_mfma_fwd(const float* x, const void* wp_fwd, float* y, void* workspace, size_t workspace_bytes,
                           int B, int C, int CO, int H, int W, void* stream);
int smd_conv3x3s2_mfma_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes,
                                  int B, int C, int CO, int H, int W, void* stream);

/* The data gradient of the same convolutions (ABI 8): g_x (B,C,H,W) from g_y (B,CO,Ho,Wo), the forward's padding and output size, any H, W >= 1.  By the
 * parity of the input pixel it is four stride-1 convolutions over g_y with 1, 2, 2 and 4 taps (nine per 2 x 2 input cell, no zero insertion), on the same
 * split-bf16 form.  wp_bwd is the data-gradient operand image of smd_conv3x3_mfma_pack(weight, wp_fwd or NULL, wp_bwd, C, CO, 3, stream)
 * (smd_conv3x3_mfma_packed_bytes(C, CO, 3) bytes: no pack of its own).  The coarse levels split K over blocks and add the splits' partial gradients in split
 * order, in a workspace of smd_conv3x3s2d_mfma_workspace_bytes (no atomic add, no zeroing pass).  Served, argument checks and error codes: as
 * smd_conv3x3s2_mfma_* above; the query returns 0 for anything else.  Deterministic. */
size_t smd_conv3x3s2d_mfma_workspace_bytes(int B, int C, int CO, int H, int W);
int smd_conv3x3s2d_mfma_bwd_data(const float* g_y, const void* wp_bwd, float* g_x, void* workspace, size_t workspace_bytes,
                                 int B, int C, int CO, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Producer side of the path: training-mode BatchNorm2d of the ResNet encoders fused with the residual add and ReLU
 * that follow it (timm resnet blocks built at src/networks/depth.py:95-98, src/networks/pose.py:39-41;
 * `F.batch_norm(training=True, momentum, eps)` semantics: biased variance for normalisation, unbiased for the running
 * estimate).  x, y, residual (N,C,H,W) with HW = H*W; gamma, beta, running_*, save_* (C).
 *   y = [relu]( (x - mean)/sqrt(var + eps) * gamma + beta [+ residual] )
 * Backward: g_y -> g_x, g_gamma, g_beta and, when g_residual != NULL, the gradient of the residual branch
 * (g_y masked by y > 0 when relu). */
size_t smd_bn_workspace_bytes(int N, int C, int HW);
int smd_bn_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* running_mean, float* running_var,
               float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd,
               void* workspace, size_t workspace_bytes, int N, int C, int HW, void* stream);
int smd_bn_bwd(const float* x, const float* y, const float* g_y, const float* gamma, const float* save_mean, const float* save_invstd,
               int relu, float* g_x, float* g_residual, float* g_gamma, float* g_beta,
               void* workspace, size_t workspace_bytes, int N, int C, int HW, void* stream);

/* smd_maxpool3x3s2_*: `nn.MaxPool2d(3, 2, 1)` of the ResNet stem.  x (N,C,H,W) -> y (N,C,Ho,Wo), Ho = (H-1)/2+1, and
 * idx (N,C,Ho,Wo) uint8 = winning window position dh*3+dw (first maximum in scan order, as ATen).  Backward gathers. */
int smd_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int C, int H, int W, void* stream);
int smd_maxpool3x3s2_bwd(const float* g_y, const uint8_t* idx, float* g_x, int N, int C, int H, int W, void* stream);

/* smd_dwconv7x7_*: the depthwise 7x7 convolution (stride 1, padding 3, groups = C) of the ConvNeXt blocks
 * (timm convnext_* encoders of BASELINE configs 2-4, built at src/networks/depth.py:95-98).
 * x, y (N,C,H,W); weight (C,1,7,7); bias (C) or NULL.  flip = 0: forward.  flip = 1: data gradient (call with x = g_y,
 * bias = NULL; weights are read mirrored).  wrw: g_weight (C,1,7,7) and g_bias (C) or NULL from x and g_y. */
size_t smd_dwconv7x7_workspace_bytes(int C, int H, int W);
int smd_dwconv7x7_fwd(const float* x, const float* weight, const float* bias, float* y, int N, int C, int H, int W, int flip, void* stream);
int smd_dwconv7x7_wrw(const float* x, const float* g_y, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, void* stream);

/* smd_layernorm_cf_*: LayerNorm over the channel dimension of an NCHW tensor, i.e. timm's `LayerNorm2d` and the block norm
 * of ConvNeXt evaluated without the NCHW <-> NHWC permutes (`F.layer_norm(x.permute(0,2,3,1), (C,), gamma, beta, eps)`).
 * x, y (N,C,H,W) with HW = H*W; gamma, beta (C); mean, rstd (N*HW) kept for the backward.  y may be written as bfloat16
 * (y_is_bf16 != 0) and g_y read as bfloat16 (g_y_is_bf16 != 0) when the consumer is a bf16 convolution under autocast;
 * the arithmetic is fp32 either way.  Backward: g_y -> g_x, g_gamma, g_beta (fp32). */
size_t smd_layernorm_cf_workspace_bytes(int N, int C, int HW);
int smd_layernorm_cf_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_is_bf16, float* mean, float* rstd,
                         int N, int C, int HW, float eps, void* stream);
int smd_layernorm_cf_bwd(const float* x, const void* g_y, int g_y_is_bf16, const float* gamma, const float* mean, const float* rstd,
                         float* g_x, float* g_gamma, float* g_beta, void* workspace, size_t workspace_bytes, int N, int C, int HW, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The attention blocks of the CADepth decoder (src/networks/decoders/cadepth.py; csrc/smd_attention.hip).  fp32, deterministic.
 *
 * Structure perception (cadepth.py:14-27: `att = q @ k; att = att.max(-1, keepdim=True)[0] - att; out = x + (att.softmax(-1) @ v).view(...)`):
 * x, out (B,C,h,w) with n = h*w, any C >= 1 and n >= 1.  out = x + softmax(-(V V^T)) V with V = x.view(B,C,n), evaluated as
 * exp(rowmin - A) / sum on the f32 matrix cores.  stats (2,B,C) receives (rowmin, 1 / sum) per row: all the backward needs besides x.
 * Backward: g (B,C,h,w) -> g_x.  Both calls take a workspace of the channel-attention workspace query (backward = 0: one, != 0: two
 * (B,C,C) matrices; 0 for sizes that are not served): B and ceil(n / 64) below 65536, B*C*max(C, n) below 2^40. */
size_t smd_channel_attention_workspace_bytes(int B, int C, int n, int backward);
int smd_channel_attention_fwd(const float* x, float* out, float* stats, void* workspace, size_t workspace_bytes, int B, int C, int n, void* stream);
int smd_channel_attention_bwd(const float* x, const float* stats, const float* g, float* g_x, void* workspace, size_t workspace_bytes,
                              int B, int C, int n, void* stream);

/* The squeeze-excite gate of detail emphasis (cadepth.py:35-41, 45: `x + x*self.att(x)` with att = AdaptiveAvgPool2d(1), Conv2d(ch, ch, 1), ReLU,
 * Conv2d(ch, ch, 1), Sigmoid).  x, y (B,C,h,w) with HW = h*w; w1, w2 (C,C) row-major (the 1x1 convolutions' weights), b1, b2 (C).
 *   y = x (1 + a),  a = sigmoid(w2 relu(w1 mean_hw(x) + b1) + b2)
 * save (3,B,C) receives (a, mean, relu(w1 mean + b1)) for the backward.  Backward: g_y -> g_x (or NULL) and g_w1, g_b1, g_w2, g_b2 (all four or all
 * NULL); every sum in a fixed order.  One workspace size serves both directions (0 for sizes that are not served: a plane of 2^31 elements or more,
 * 2^31 blocks or more). */
size_t smd_se_gate_workspace_bytes(int B, int C, int HW);
int smd_se_gate_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* save,
                    void* workspace, size_t workspace_bytes, int B, int C, int HW, void* stream);
int smd_se_gate_bwd(const float* x, const float* g_y, const float* w1, const float* w2, const float* save, float* g_x, float* g_w1, float* g_b1,
                    float* g_w2, float* g_b2, void* workspace, size_t workspace_bytes, int B, int C, int HW, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The DDVNet decoder's output head (additive to ABI 8): `conv3x3(C -> 128 G)` on an already reflection-padded xp (B, C, h + 2, w + 2), softmax over
 * each group's 128 bins and the expectation over the bin values k/128 (src/networks/decoders/ddvnet.py:110, 116-124, 147-150), G = out_ch in 1..4,
 * C a multiple of 16.  wp_fwd: the forward image smd_conv3x3_mfma_pack writes for (C, 128 G, pieces = 3); bias (128 G).  The logits are never written:
 * disp (B, G, h, w), stats (B, G, 2, h, w) = per pixel the row maximum and the reciprocal of the sum of the shifted exponentials.
 * smd_ddv_head_bwd_logits recomputes the logits and writes g_logits (B, 128 G, h, w) = p_k (k/128 - disp) g_disp — what the convolution's data and weight
 * gradients (smd_conv3x3_mfma_bwd_* or any other) take as dL/dy — and, where g_bias is not NULL, the bias gradient (128 G), summed in a fixed order.
 * smd_ddv_head_workspace_bytes: the backward's workspace; 0 for sizes the kernels do not take. */
size_t smd_ddv_head_workspace_bytes(int B, int C, int G, int h, int w);
int smd_ddv_head_fwd(const float* xp, const void* wp_fwd, const float* bias, float* disp, float* stats, int B, int C, int G, int h, int w, void* stream);
int smd_ddv_head_bwd_logits(const float* xp, const void* wp_fwd, const float* bias, const float* disp, const float* stats, const float* g_disp,
                            float* g_logits, float* g_bias, void* workspace, size_t workspace_bytes, int B, int C, int G, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The DiffNet decoder's attention stage in front of its convolution (additive to ABI 8; reference: src/networks/decoders/diffnet.py:44-47 —
 * ChannelAttention.forward: `x * sigmoid(fc(avg_pool(x)))` with two bias-free Linear layers — and :70-74 — AttentionBlock.forward: `cat(interpolate(x, 2),
 * x_skip)` in front of it; the reflection padding is that of the block's conv3x3, decoders/utils.py:44-46; the ReLU on `a` is the previous block's,
 * diffnet.py:67).  All tensors fp32.
 *   src  = cat(nearest_x2(act(a + bias_a)), skip)      a (B,Ca,h,w) a raw (bias-free) convolution output or an encoder feature, bias_a (Ca) or NULL,
 *                                                      act SMD_UCG_NONE / SMD_UCG_RELU, skip (B,Cs,2h,2w) with Cs >= 1; src is never written
 *   mean = mean_hw(src)                                (for the a half: the mean over h x w of act(a + bias_a))
 *   hid  = relu(w1 mean),  gate = sigmoid(w2 hid)      w1 (R,C), w2 (C,R) row-major, C = Ca + Cs, any R >= 1
 *   out (B,C,2h+2,2w+2) = reflect_pad1(gate o src)
 * gate (B,C), mean (B,C) and hid (B,R) are written for the backward, which recomputes act(a + bias_a): g_out -> g_a, g_skip, g_bias_a (Ca), g_w1 with g_w2
 * (both or neither); any of them may be NULL.  Every sum runs in a fixed order (no atomics): two runs on the same inputs are bit-equal.  One workspace
 * size serves both directions; it is 0 for sizes that are not served (a non-positive size, 2^31 blocks or more, a padded plane of 2^30 elements or more). */
#define SMD_UCG_NONE 0
#define SMD_UCG_RELU 1
size_t smd_up_cat_gate_pad_workspace_bytes(int B, int Ca, int Cs, int h, int w, int R);
int smd_up_cat_gate_pad_fwd(const float* a, const float* bias_a, const float* skip, const float* w1, const float* w2, float* out, float* gate, float* mean,
                            float* hid, void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int R, int act, void* stream);
int smd_up_cat_gate_pad_bwd(const float* a, const float* bias_a, const float* skip, const float* w1, const float* w2, const float* gate, const float* mean,
                            const float* hid, const float* g_out, float* g_a, float* g_skip, float* g_bias_a, float* g_w1, float* g_w2,
                            void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int R, int act, void* stream);
/* The ReLU form of smd_elu_pad_* (the same kernels with another activation): out (B,C,h+2,w+2) = reflect_pad1(relu(x + bias)), the padded activation of a
 * DiffNet attention stage (diffnet.py:64-68: conv3x3 + ReLU) that its output head and a following up-sample block read.  fp32; bias (C) or NULL.
 * Backward: g_out -> g_x and g_bias (C) or NULL (needs smd_decoder_glue_workspace_bytes(B, C, h, w)). */
int smd_relu_pad_fwd(const float* x, const float* bias, float* out, int B, int C, int h, int w, void* stream);
int smd_relu_pad_bwd(const float* x, const float* bias, const float* g_out, float* g_x, float* g_bias, void* workspace, size_t workspace_bytes,
                     int B, int C, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The SuperDepth decoder's sub-pixel convolution with what stands around it (additive to ABI 8; reference: src/networks/decoders/superdepth.py:13-26 —
 * SubPixelConv: `Conv2d(ch_in, ch_in r^2, 3, groups=ch_in, padding=1)` then `PixelShuffle(r)` — between the ELU of the `conv_block` in front of it
 * (decoders/utils.py:49-54) and, in a stage, superdepth.py:70-74 and :105-113: `ReLU`, `torch.cat` with the skip feature and the reflection padding of the
 * next conv3x3 (decoders/utils.py:44-46); in a head, superdepth.py:93-97: the output activation).  All tensors fp32, r in {2, 4, 8}.
 *   u = pre_act(x + pre_bias[c])                       x (B,C,h,w) a raw (bias-free) convolution output, pre_bias (C) or NULL, pre_act SMD_SP_PRE_NONE / _ELU
 *   v[b,c,r y+dy,r x+dx] = bias[o] + sum_ij weight[o,0,i,j] u[b,c,y+i-1,x+j-1]      o = c r^2 + dy r + dx, u = 0 outside the plane;
 *                                                      weight (C r^2,1,3,3), bias (C r^2): the layout of the reference's Conv2d
 *   z = act(v)                                         act SMD_SP_NONE / _RELU / _SIGMOID
 *   out = z (B,C,r h,r w)                              pad = 0 (then Cs = 0 and skip is ignored)
 *       | reflect_pad1(cat(z, skip)) (B,C+Cs,r h+2,r w+2)   pad = 1; skip (B,Cs,r h,r w), or NULL with Cs = 0
 * Neither u nor v nor the un-shuffled C r^2-channel tensor is written.  Backward: g_out (out's shape) and out itself (for the derivative of act; NULL is
 * accepted with SMD_SP_NONE) -> g_x, g_pre_bias (C), g_weight, g_bias, g_skip; any of them may be NULL.  The pad adjoint is folded in on the fly, u is
 * recomputed; a ReLU output of exactly 0 passes no gradient.  Every sum runs in a fixed order (no atomics): two runs on the same inputs are bit-equal.
 * smd_subpixel_workspace_bytes: the backward's workspace (per-block sums of the two bias gradients and of the C r^2 9 weight-gradient sums, added in a
 * second stage); 0 for sizes that are not served (a non-positive size, another r, skip channels without pad, a padded plane of 2^30 elements or more,
 * 2^31 blocks or more).  The forward needs none. */
#define SMD_SP_PRE_NONE 0
#define SMD_SP_PRE_ELU 1
#define SMD_SP_NONE 0
#define SMD_SP_RELU 1
#define SMD_SP_SIGMOID 2
size_t smd_subpixel_workspace_bytes(int B, int C, int Cs, int h, int w, int r, int pad);
int smd_subpixel_fwd(const float* x, const float* pre_bias, const float* weight, const float* bias, const float* skip, float* out,
                     int B, int C, int Cs, int h, int w, int r, int pre_act, int act, int pad, void* stream);
int smd_subpixel_bwd(const float* x, const float* pre_bias, const float* weight, const float* out, const float* g_out, float* g_x, float* g_pre_bias,
                     float* g_weight, float* g_bias, float* g_skip, void* workspace, size_t workspace_bytes,
                     int B, int C, int Cs, int h, int w, int r, int pre_act, int act, int pad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Monodepth's flip-and-blend post-process (smd_blend.hip) — replaces `blend_stereo` (src/tools/geometry.py:94-129), the `flip` in front of it
 * (src/core/predictors.py:83, src/networks/depth.py:148-156) and the disparity half of `to_scaled` behind it (src/tools/geometry.py:63-76), for every level
 * of a pyramid in ONE launch:
 *   m_l = ramp (ws[s],) = clamp(20 (linspace(0,1,w) - 0.05), 0, 1), built by the caller so that its bits are torch's; m_r[j] = m_l[w-1-j]; m_mu = (1 - m_l) - m_r
 *   out = (m_r l + m_l r) + m_mu ((l + r)/2)           every product and sum rounded on its own, in ATen's order
 *   out = scale out + offset                            with SMD_BLEND_SCALE: scale = 1/min - 1/max and offset = 1/max (0 without a maximum), each formed
 *                                                       in double by the caller and rounded once to fp32, as ATen applies the reference's Python scalars
 * l[s], r[s], out[s]: (planes, hs[s], ws[s]) fp32, contiguous; hs[s], ws[s] >= 1, S <= SMD_MAX_SCALES.  With SMD_BLEND_MIRROR r[s] is the prediction for the
 * mirrored image as the network wrote it and column j reads r[s][.., w-1-j]: no flipped copy exists.  Without it r[s] is already flipped back.
 * Backward (src/tools/geometry.py:121-126 differentiated): g_l[j] = k g[j] m_r[j] + (k g[j] m_mu[j])/2 and g_r[j'] = k g[j] m_l[j] + (k g[j] m_mu[j])/2 at
 * j' = w-1-j with SMD_BLEND_MIRROR, else j; k = scale with SMD_BLEND_SCALE, else 1.  g_l, g_r: either array, or any entry, may be NULL (not both for every
 * level).  Every output element is written once by one thread: no atomics, two runs are bit-equal.  No workspace.
 * Pointers need only be 4-byte aligned: a four-column group moves as one 16-byte vector where every address it touches allows it, element by element
 * elsewhere (so a width that is no multiple of 4 under SMD_BLEND_MIRROR, or rows that start off a 16-byte boundary, take the element path). */
#define SMD_BLEND_MIRROR 0x1
#define SMD_BLEND_SCALE 0x2
int smd_flip_blend_fwd(const float* const* l, const float* const* r, const float* const* ramp, float* const* out, const int* hs, const int* ws,
                       int S, int planes, int flags, float scale, float offset, void* stream);
int smd_flip_blend_bwd(const float* const* g_out, const float* const* ramp, float* const* g_l, float* const* g_r, const int* hs, const int* ws,
                       int S, int planes, int flags, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FeatDepth's feature regularisers (smd_featreg.hip) — replace `FeatPeakReg` and `FeatSmoothReg` (src/regularizers/smooth.py:100-176, on compute_grad and
 * compute_laplacian, :12-48) and the per-scale loop around them (src/core/handlers.py:304-305) for every level of a feature pyramid in ONE launch:
 *   dx[i][j] = |x[i][j] - x[i][j+1]|, dy[i][j] = |x[i][j] - x[i+1][j]|, each with a ZERO last column / row; the second-order differences dxx, dyx (along j)
 *   and dxy, dyy (along i) are the same differences of those padded maps, so dxx[..][w-2] = |dx[..][w-2] - 0| and their last column / row is 0 again
 *   peaky_s  = -(mean(wx dx) + mean(wy dy))                         smooth_s = mean(wxx dxx) + mean(wyy dyy) + mean(wxy dxy) + mean(wyx dyx)
 *   w* = exp(-(mean over the 3 channels of the same difference of img)) with SMD_FEATREG_PEAKY_EDGES / SMD_FEATREG_SMOOTH_EDGES, else 1
 *   *out_peaky = mean_s(peaky_s / 2^s), *out_smooth = mean_s(smooth_s / 2^s)        (S = 1: the regulariser itself)
 * feat[s]: (B, Cs[s], hs[s], ws[s]) fp32, img[s]: (B, 3, hs[s], ws[s]) fp32 (the image already resized to the level), contiguous; every size >= 1,
 * S <= SMD_MAX_SCALES.  SMD_FEATREG_PEAKY / SMD_FEATREG_SMOOTH select what is computed (at least one); an output that is not selected is written as 0.
 * Forward: one sweep that writes two fp64 sums per block to the workspace, then a one-block second stage in a fixed order: no atomics, no full-size
 * intermediates, two runs are bit-equal.  smd_feat_regs_workspace_bytes: 0 for sizes that are not served (a level of 2^31 elements or more).
 * Backward: g_peaky, g_smooth are DEVICE scalars; either may be NULL (not both), and the gradient written is then exactly the other loss's.  g_feat[s] is
 * written once per element as a gather (sign(0) = 0, the padded zeros are constants); every level passed needs its g_feat.  No workspace.
 * Pointers need only be 4-byte aligned: a level whose rows are 16-byte aligned moves in 16-byte vectors, any other element by element. */
#define SMD_FEATREG_PEAKY_EDGES 0x1
#define SMD_FEATREG_SMOOTH_EDGES 0x2
#define SMD_FEATREG_PEAKY 0x4
#define SMD_FEATREG_SMOOTH 0x8
size_t smd_feat_regs_workspace_bytes(const int* Cs, const int* hs, const int* ws, int S, int B);
int smd_feat_regs_fwd(const float* const* feat, const float* const* img, const int* Cs, const int* hs, const int* ws, int S, int B, int flags,
                      float* out_peaky, float* out_smooth, void* workspace, size_t workspace_bytes, void* stream);
int smd_feat_regs_bwd(const float* const* feat, const float* const* img, const float* g_peaky, const float* g_smooth, float* const* g_feat,
                      const int* Cs, const int* hs, const int* ws, int S, int B, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth-Hints proxy-depth regression over every scale (smd_hints.hip) — replaces `handlers.depth_regr` (src/core/handlers.py:201-259) once the photometric
 * errors are known, without the (S*b, ...) expansions of the depths, the hints and the mask:
 *   m[s][i] = hints[i] > 0 && (no SMD_REGR_AUTOMASK || err[1+s][i] > err[0][i])      e[s][i] = m ? crit(depth[s][i], hints[i]) : 0      loss = sum(e) / sum(m)
 * depth (S,b,h,w), hints (b,h,w) (0 = no hint), err (S+1,b,h,w) with SMD_REGR_AUTOMASK, else NULL: err[0] the photometric error of the supports warped by
 * the hints, err[1+s] by depth[s] (`compute_photo`, src/losses/reconstruction.py:79-96; smd_image_recon_fwd's `err` over the stack [hints, depth_0 ..]).
 * flags: SMD_REGR_{L1,LOG_L1,BERHU} | SMD_REGR_INVERT | SMD_REGR_AUTOMASK; crit, `to_inv` and berHu's threshold 0.2 * max|diff| over ALL S*b*h*w elements
 * (masked or not) are smd_regression_*'s, element by element.  sum(m) = 0 gives NaN, as the reference does.  S <= SMD_MAX_SCALES, b*h*w < 2^31.
 * Outputs: loss (1); mask0 (b,h,w) uint8 0/1, the mask of scale 0 (`mask_regr`); bits ((b*h*w + 3)/4 32-bit words: bit 4 s + k of word g is m[s][4 g + k]), the
 * whole mask for the backward; stats (8 floats) for the backward.  The hints are read once per pixel for all scales.  fp64 block sums in the workspace and
 * a one-block second stage in a fixed order: no atomics, two runs are bit-equal; berHu takes a second sweep once the maximum is known.
 * Backward: ONE sweep, g_depth (S,b,h,w) from `bits` and `stats` (it does not read err); g_loss is a DEVICE scalar.  No workspace.
 * Pointers need only their element's alignment (the workspace: 8 bytes): with b*h*w % 4 == 0 and 16-byte aligned bases four pixels move as one 16-byte
 * vector, otherwise element by element. */
size_t smd_hints_regr_workspace_bytes(int S, int b, int h, int w);
int smd_hints_regr_fwd(const float* depth, const float* hints, const float* err, int S, int b, int h, int w, int flags, float* loss, uint8_t* mask0,
                       uint32_t* bits, float* stats, void* workspace, size_t workspace_bytes, void* stream);
int smd_hints_regr_bwd(const float* depth, const float* hints, const uint32_t* bits, const float* stats, const float* g_loss, float* g_depth,
                       int S, int b, int h, int w, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature-metric reconstruction loss from the LOW-resolution features (smd_featrecon.hip) — replaces `handlers.feat_recon` (src/core/handlers.py:70-119):
 * the bilinear up-sampling (align_corners=False) of the target features (b,C,hf,wf) and the support features (n,b,C,hf,wf) to the depth map (b,1,H,W), the
 * warp of the up-sampled supports by depth, T (n,b,4,4), K and K_inv (b,4,4) (`ViewSynth`, as smd_view_synth_fwd), the dense error over the channels and
 * `ReconstructionLoss`'s reduction over the supports, per pixel, without any tensor of size (C,H,W):
 *   flags: SMD_LOSS_L1 (sum_c |d| / C) or SMD_LOSS_L2 (sqrt(max(sum_c d^2, eps))) | SMD_USE_MIN (else the mean) | SMD_USE_AUTOMASK (the static error against the
 *   un-warped up-sampled support, + eps * noise: `noise` (b,1,H,W), or NULL: smd_recon_reduce_fwd's generator under `seed`, equal seeds draw equal noise).
 * Outputs: loss (1) = the mean of the reduced error; sel (b,H,W) uint8: the winning support (0 for the mean), SMD_SEL_MASKED where the automask removed the
 * pixel; warp (n,b,C,H,W) or NULL: the warped supports for the image logger, the only full-resolution C-channel tensor the call can write.
 * Sizes served: 2 <= H, W <= 2048, 1 <= hf <= H, 1 <= wf <= W (any ratio), C >= 1, n <= SMD_MAX_SUPPORTS, b*H*W < 2^31, n*b*C*hf*wf*4 bytes < 2^32;
 * smd_feat_recon_workspace_bytes returns 0 for anything else.  One fp64 sum per block of 64 x 4 pixels in the workspace, added by a one-block second stage in
 * a fixed order: no atomics, two runs are bit-equal.
 * Backward: ONE sweep from `sel`: the selected support's samples (every support's for the mean) are recomputed, g_depth (b,H,W) and g_T (n,b,4,4) through the
 * per-block pose sums in the workspace and the fp64 finalize of smd_view_synth_bwd.  Either may be NULL (not both): the launch then never forms its terms, and
 * the other's bits do not change.  The l2 gradient is 0 where clamp(min=eps) is active.  No gradient to the features, K or K_inv.  g_loss is a DEVICE scalar.
 * Pointers need only their element's alignment (the workspace: 8 bytes). */
size_t smd_feat_recon_workspace_bytes(int b, int n, int C, int H, int W, int hf, int wf);
int smd_feat_recon_fwd(const float* depth, const float* feat, const float* supp_feat, const float* T, const float* K, const float* K_inv, const float* noise,
                       uint64_t seed, float* loss, uint8_t* sel, float* warp, void* workspace, size_t workspace_bytes, int b, int n, int C, int H, int W,
                       int hf, int wf, int flags, void* stream);
int smd_feat_recon_bwd(const float* depth, const float* feat, const float* supp_feat, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                       const float* g_loss, float* g_depth, float* g_T, void* workspace, size_t workspace_bytes, int b, int n, int C, int H, int W, int hf, int wf,
                       int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image reconstruction loss with a predictive weighting mask (smd_maskrecon.hip) — replaces, for a criterion built with `mask_name`, `handlers.image_recon`
 * (src/core/handlers.py:14-67) on the un-fused operators: the warp of every support at every scale (`ViewSynth.forward`, src/tools/geometry.py:366-391), the
 * photometric error of the warps and of the un-warped supports (`PhotoError`, src/losses/photometric.py:54-88), `ReconstructionLoss.apply_mask` on the
 * per-support errors (src/losses/reconstruction.py:46-57) and the reduction, automask and mean (src/losses/reconstruction.py:59-77, 79-96, 125), per tile of
 * 32 x 8 pixels with its reflection halo in LDS, without the (n,S,b,3,h,w) warps and the two (n,S,b,h,w) error stacks.
 *   depth (S,b,h,w) the up-sampled depth stack; mask (S,b,n,h,w) the up-sampled mask stack, one channel per support; tgt (b,3,h,w); supp (n,b,3,h,w);
 *   T (n,b,4,4); K, K_inv (b,4,4); noise (S,b,h,w) or NULL: smd_recon_reduce_fwd's generator under `seed` (equal seeds draw equal noise).
 *   flags: SMD_USE_MIN | SMD_USE_AUTOMASK | SMD_LOSS_L1 (else 0.85 SSIM + 0.15 L1) and exactly one of SMD_MASK_EXPLAINABILITY (err * mask) /
 *   SMD_MASK_UNCERTAINTY (err * exp(-mask) + mask).
 * Every statement is the un-fused operators' (smd_view_synth_fwd, smd_photo_error_fwd, smd_recon_reduce_fwd) in their order: `sel` and `warp0` are theirs bit
 * for bit.  PhotoError pads the WARPED image by reflection: the halo at an image border is the warp of the mirrored pixel.
 * Outputs: loss (1) = the mean of the reduced error; sel (S,b,h,w) uint8: the winning support (0 for the mean), SMD_SEL_MASKED where the static error won;
 * stat (S,b,h,w) uint8: the support whose masked static error is the smallest — written, read by the backward and required only with SMD_USE_MIN and
 * SMD_USE_AUTOMASK together (else it may be NULL); warp0 (n,b,3,h,w) or NULL: the warps of scale 0 for the image logger.
 * Sizes served: 2 <= h, w <= 2048, 1 <= n <= SMD_MAX_SUPPORTS, 1 <= S <= SMD_MAX_SCALES, S*b <= 65535, S*b*h*w < 2^31; smd_mask_recon_workspace_bytes returns 0
 * and the calls SMD_E_UNSUPPORTED (nothing launched) for anything else, other flags included.  One fp64 sum per block in the workspace, added by a one-block
 * second stage in a fixed order: no atomics, two runs are bit-equal.
 * Backward: ONE sweep that reads the decisions (`sel`, `stat`) and never re-decides: g_mask (S,b,n,h,w), every element written, the static branch included (it
 * feeds the mask of the static winner, or of every support for the mean, as smd_recon_reduce_bwd does); g_depth (S,b,h,w) through the error's adjoint (the
 * nine windows that contain a pixel, with the reflection fold) and the bilinear weights' derivatives; g_T (n,b,4,4) through per-block pose sums in the
 * workspace and the fp64 finalize of smd_view_synth_bwd.  Any of the three may be NULL (not all): the launch then never forms its terms, and the others' bits
 * do not change.  No gradient to the images, K or K_inv.  g_loss is a DEVICE scalar.  Pointers need only their element's alignment (the workspace: 8 bytes). */
size_t smd_mask_recon_workspace_bytes(int S, int b, int n, int h, int w);
int smd_mask_recon_fwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                       const float* noise, uint64_t seed, float* loss, uint8_t* sel, uint8_t* stat, float* warp0, void* workspace, size_t workspace_bytes,
                       int S, int b, int n, int h, int w, int flags, void* stream);
int smd_mask_recon_bwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                       const uint8_t* sel, const uint8_t* stat, const float* g_loss, float* g_depth, float* g_mask, float* g_T, void* workspace,
                       size_t workspace_bytes, int S, int b, int n, int h, int w, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Offline evaluation (smd_eval.hip) — replaces the per-item body of `MonoDepthEvaluator.__call__` (src/core/evaluator.py:65-94) for a batch of b items.
 *
 * smd_eval_metrics: `upsample` + `to_inv` (evaluator.py:70, 169-173; src/tools/geometry.py:86-90), `get_mask` and the mask (evaluator.py:73-78, 175-181),
 * `align` (evaluator.py:200-234), `scale` (evaluator.py:236-243), `metrics_eigen` (src/core/metrics.py:39-59) and `metrics_benchmark` (metrics.py:80-105).
 *   disp (b,1,h,w) scaleless disparity; target (b,1,H,W); mask (b,1,H,W) uint8 or NULL (all ones).  The disparity is resized to (H,W) with ATen's
 *   align_corners=False bilinear taps, or with SMD_EVAL_NEAREST source index floor(dst*in/out) (equality with cv2.resize is not claimed), and inverted:
 *   pred = (d > 0)/max(d, eps).  A pixel is valid where target > min_depth, target < max_depth (only with max_depth > 0: 0 means "no maximum"),
 *   crop_y0 <= y < crop_y1, crop_x0 <= x < crop_x1, mask != 0 and pred > 0.
 *   align_mode: SMD_EVAL_ALIGN_FACTOR (scale = factor, shift = 0), SMD_EVAL_ALIGN_MEDIAN (scale = np.median(target)/np.median(pred) over the valid pixels in
 *   float32, both middle values of an even count selected exactly), SMD_EVAL_ALIGN_LSQR (scale and shift of the least-squares fit in disparity space from
 *   fp64 sums; a determinant <= 0 gives (0, 0)).  p = clip(scale*pred + shift, min_depth, max_depth), through to_inv on both sides for LSQR, in float32.
 *   groups: SMD_EVAL_EIGEN | SMD_EVAL_BENCHMARK (at least one).
 * -> values (b,20) fp64: Scale, Shift | AbsRel, SqRel, RMSE, LogRMSE, delta<1.05, <1.1, <1.25, <1.25^2, <1.25^3 (x100) | MAE, RMSE, InvMAE, InvRMSE, LogMAE,
 *    LogRMSE, LogSI, AbsRel, SqRel; zeros for a group that was not asked for and for an item that is not scored;
 *    counts (b) int32 valid pixels; status (b) int32: SMD_EVAL_SCORED, SMD_EVAL_EMPTY_MASK, SMD_EVAL_ZERO_PRED (the valid predictions sum to 0);
 *    medians (b,2) fp32: np.median(pred), np.median(target) (MEDIAN on scored items, else 0);
 *    optional (NULL: not written): depth (b,1,H,W) the aligned prediction at the valid pixels of scored items and 0 elsewhere; valid (b,1,H,W) uint8;
 *    resized (b,1,H,W) the resized disparity.
 * Integer atomics and fixed-order fp64 sums only: two calls give the same bits.  No synchronisation, no copy to the host; the workspace may be reused dirty.
 * Pointers need only their element's alignment (the workspace: 8 bytes).  smd_eval_metrics_workspace_bytes returns 0 for sizes that are not served
 * (b > 65535, H*W or h*w >= 2^31).
 *
 * smd_eval_pointcloud: `metrics_pointcloud` up to its last scalar formulas (metrics.py:111-165; `BackprojectDepth.forward`, geometry.py:304-316).
 *   depth, target (b,1,H,W); mask (b,1,H,W) uint8; prefix (b,H*W) int32: the INCLUSIVE prefix sum of (mask != 0) per item in row-major order;
 *   K_inv (b,4,4).  Both clouds are K_inv[:3,:3] (x, y, 1) * depth at the masked pixels, compacted in row-major order; every second point of each
 *   (`[::2]`, metrics.py:128, 131) looks up its exact nearest neighbour in the other cloud by tiled brute force on the coordinate differences.
 * -> nn (b,2,ceil(H*W/2)) fp32: the distances of the prediction's queries and of the target's (0 past the item's query count ceil(n/2));
 *    stats (b,2,4) fp64: per direction the sum of the distances and the counts of distances < 0.05, < 0.1, < 0.2; counts (b) int32: n.
 * The minimum is order-independent and the sums are added in a fixed order: two calls give the same bits.  Served: b*min(32, ceil(H*W/2048)) <= 65535. */
#define SMD_EVAL_ALIGN_FACTOR 0
#define SMD_EVAL_ALIGN_MEDIAN 1
#define SMD_EVAL_ALIGN_LSQR 2
#define SMD_EVAL_EIGEN 0x1
#define SMD_EVAL_BENCHMARK 0x2
#define SMD_EVAL_NEAREST 0x4
#define SMD_EVAL_SCORED 0
#define SMD_EVAL_EMPTY_MASK 1
#define SMD_EVAL_ZERO_PRED 2
size_t smd_eval_metrics_workspace_bytes(int b, int H, int W);
int smd_eval_metrics(const float* disp, const float* target, const uint8_t* mask, int b, int h, int w, int H, int W, int crop_y0, int crop_y1, int crop_x0,
                     int crop_x1, float min_depth, float max_depth, int align_mode, float factor, int flags, double* values, int* counts, int* status,
                     float* medians, float* depth, uint8_t* valid, float* resized, void* workspace, size_t workspace_bytes, void* stream);
size_t smd_eval_pointcloud_workspace_bytes(int b, int H, int W);
int smd_eval_pointcloud(const float* depth, const float* target, const uint8_t* mask, const int* prefix, const float* K_inv, int b, int H, int W,
                        float* nn, double* stats, int* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image logging (smd_viz.hip) — what the reference's HeavyLogger (src/core/heavy_logger.py:90-210) computes per image: `rgb_from_disp` and `rgb_from_feat`
 * (src/tools/viz.py:20-74) and torchvision's `make_grid` (heavy_logger.py:35-42).  fp32 in and out; ABI 8 (symbols were added, none changed).
 *
 * smd_viz_disp: disp (b,1,h,w) -> rgb (b,3,h,w).  invert: `to_inv` first (src/tools/geometry.py:86-90; a NaN stays one).  select != 0: per item
 *   vmax = np.percentile(d[d > 0], 95) as numpy evaluates it for a float32 array — the virtual index (n - 1)*float32(0.95) in float32, the two order
 *   statistics around it selected exactly by a radix select over the bit patterns, numpy's `_lerp` between them with its `t >= 0.5` form — written to
 *   vmax (b), and den (b) = (vmax - vmin) + 1e-5 in float32; an item without a positive value gets vmax = 0 (viz.py:13-16) and den = den0.  select == 0:
 *   vmax and den are read (the caller's `vmax`).  Then `apply_cmap` (src/utils/misc.py:54-60) with matplotlib's `Colormap.__call__`, in float32 with IEEE
 *   division: clip(vmin, vmax), (x - vmin)/den, * N, `== N -> N - 1`, truncation, lut (N,3) lookup, N <= 1024; below 0 takes entry 0, N and above entry
 *   N - 1, a NaN (0, 0, 0).  Integer atomics on the histograms only, which the call zeroes: two calls give the same bits.
 *
 * smd_viz_feat_moments: feat (b,C,h,w) -> mean (C) fp64 and cov (C,C) fp64 = the sums over all b*h*w samples of the products of the centred channels
 *   (NOT divided by n - 1), through per-block fp32 tiles (32 x 32 channel pairs x a chunk of samples; `v_mfma_f32_32x32x2_f32` for C >= 64) added in fp64 in
 *   a fixed order.  The caller decomposes cov (the exact covariance route: sklearn's `covariance_eigh`; its randomized solver is not restated).
 * smd_viz_feat_project: rgb (b,3,h,w) = (feat - mean) V with V (C,3), then `proj -= proj.min(0); proj /= proj.max(0)` (viz.py:69-70; the maximum of the
 *   shifted values; 0/0 gives NaN as it does there).  Served: 3 <= C <= 1024, 3 <= b*h*w < 2^31 (else the query returns 0 and the calls SMD_E_INVALID).
 *
 * smd_make_grid: x (b,c,h,w), c = 1 or 3, float32 or (is_u8) uint8 / bool bytes -> grid (3,Hg,Wg) of the first n = min(b, n_imgs) images, `nrow` per row:
 *   xmaps = min(nrow, n), ymaps = ceil(n/xmaps), Hg = (h + padding) ymaps + padding, Wg = (w + padding) xmaps + padding, image k at row
 *   (k / xmaps)(h + padding) + padding and column (k % xmaps)(w + padding) + padding, pad_value elsewhere; n == 1 gives the image itself, (3,h,w).  One
 *   channel is repeated three times.  normalize: lo, hi = the extrema of the n images, then clamp(lo, hi) and (x - lo)/max(hi - lo, 1e-5) (scale_each=False).
 * Pointers need only their element's alignment (fp64 arrays and the feature workspace: 8 bytes). */
size_t smd_viz_disp_workspace_bytes(int b, int h, int w);
int smd_viz_disp(const float* disp, int b, int h, int w, int invert, int select, float vmin, float den0, const float* lut, int N, float* rgb, float* vmax,
                 float* den, void* workspace, size_t workspace_bytes, void* stream);
size_t smd_viz_feat_workspace_bytes(int b, int C, int h, int w);
int smd_viz_feat_moments(const float* feat, int b, int C, int h, int w, double* mean, double* cov, void* workspace, size_t workspace_bytes, void* stream);
int smd_viz_feat_project(const float* feat, const double* mean, const float* V, int b, int C, int h, int w, float* rgb, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t smd_make_grid_workspace_bytes(void);
int smd_make_grid(const void* x, int is_u8, int b, int c, int h, int w, int n_imgs, int nrow, int padding, float pad_value, int normalize, float* grid,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose / intrinsics prologue — one launch each instead of ~45 eager ATen launches.
 *
 * smd_pose_*: `T_from_AAt(aa, t)` (src/tools/geometry.py:181-209), followed by `T.inverse()` where invert[i] != 0
 * (src/core/trainer.py:253: supports behind the target when `always_fwd_pose`).  aa, t (N,3) -> T (N,4,4).
 * Backward: g_T (N,4,4) -> g_aa, g_t (N,3).
 *
 * smd_intrinsics_*: with fs != NULL: `resize_K(PoseNet.build_K(fs, cs), (h, w))` (src/networks/pose.py:60-73,
 * src/tools/geometry.py:249-263) -> K (b,4,4) and its inverse K_inv (the `K.inverse()` of geometry.py:383).
 * With fs == NULL: K_inv of the caller's K_in (b,4,4) (3x3 block, rest identity).  Backward (learned K only):
 * g_K, g_Kinv (b,4,4) -> g_fs, g_cs (b,2). */
int smd_pose_fwd(const float* aa, const float* t, const uint8_t* invert, int N, float* T, void* stream);
int smd_pose_bwd(const float* aa, const float* t, const uint8_t* invert, int N, const float* g_T, float* g_aa, float* g_t, void* stream);
int smd_intrinsics_fwd(const float* fs, const float* cs, const float* K_in, int b, int h, int w, float* K, float* K_inv, void* stream);
int smd_intrinsics_bwd(const float* fs, const float* cs, int b, int h, int w, const float* g_K, const float* g_Kinv,
                       float* g_fs, float* g_cs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GPU-side aspect-ratio augmentation.  Replaces `crop_aug` + `resize_aug` of
 * src/core/aspect_ratio.py:67-151 for the image tensors of a batch and `centre_crop_K` + `resize_K`
 * (src/tools/geometry.py:233-263) for its intrinsics, in one launch: every plane of every segment (a tensor viewed as
 * (planes[k], H, W): x.imgs, y.imgs, x.supp_imgs, y.supp_imgs, depth ...) is centre-cropped to (crop_h, crop_w) as kornia's
 * `center_crop(size, mode='bilinear', align_corners=False)` does it (aspect_ratio.py:78) — the integer window starting at
 * int(H/2 - crop_h/2), bilinearly RE-SAMPLED at x(i) = ((i + 0.5)(w - 1)/w + x0) W/(W - 1) - 0.5 with zero padding: kornia's
 * (n - 1)-normalised warp under align_corners=False grids — and the crop resized to (out_h, out_w) with
 * `F.interpolate(mode='bilinear', align_corners=False)` semantics; dst[k] is (planes[k], out_h, out_w).  crop == input size:
 * resize only, no resampling of the frame (the augmentation's not-applied branch); out == crop size: crop only.  H, W >= 2.  K_in / K_out (nK,4,4) or both NULL.  The shapes are sampled on the host
 * (`slowtv_monodepth_amd.aspect_ratio`, same random streams as the reference). */
int smd_crop_resize(const float* const* src, float* const* dst, const int* planes, int nseg, int H, int W, int crop_h, int crop_w,
                    int out_h, int out_w, const float* K_in, float* K_out, int nK, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel timing hooks for bench.py: while enabled, every call of the named entry point records a HIP event pair on the
 * caller's stream, either around its DOMINANT kernel (the fused strip kernel k_recon_main / k_recon_bwd) or around ALL
 * of its launches (forward: per-sample prep, unless SMD_PACKED_READY, + main; backward: the fused adjoint [+ the K0 adjoint is
 * outside]; the scalar / pose reductions run inside those launches since ABI 4), or around the prep launches wherever they run.
 * smd_profile_collect() waits for the recorded events and returns their durations in ms.  Not thread-safe; one device. */
#define SMD_PROF_RECON_FWD 0       /* smd_image_recon_fwd, dominant kernel */
#define SMD_PROF_RECON_BWD 1       /* smd_image_recon_bwd, dominant kernel */
#define SMD_PROF_RECON_FWD_ALL 2   /* smd_image_recon_fwd, every launch */
#define SMD_PROF_RECON_BWD_ALL 3   /* smd_image_recon_bwd, every launch */
#define SMD_PROF_RECON_PREP 4      /* k_recon_prep launches (inside the forward entry point or smd_image_recon_prep) */
/* The template instantiation the process's last fused forward (which = SMD_PROF_RECON_FWD) / backward (SMD_PROF_RECON_BWD) launch
 * picked, spelled as rocprofv3 prints kernel names ("smd::k_recon_main<2, true, true, false, true, 1, true>"); "" before the first launch. */
const char* smd_last_kernel_variant(int which);
int smd_profile_enable(int which, int capacity);
int smd_profile_collect(int which, float* ms_out, int max_out, int* n_out);

/* Measurement aid: STREAM-style sweep over nbytes (multiple of 16): mode 0 copies src -> dst (read + write), mode 1 only
 * reads src; add 2 (modes 2, 3) for the variant with eight instead of four 16-byte loads in flight per lane and plain instead of
 * non-temporal accesses, add 4 (modes 4, 5) for the variant in which every block walks one contiguous chunk 32 KB at a time
 * (non-temporal).  bench.py times all of them and quotes the best as the measured HBM ceiling of the box beside the
 * datasheet peak. */
int smd_debug_stream_copy(const void* src, void* dst, size_t nbytes, int mode, void* stream);

/* Debug/self-test: out[l] = {value held by lane l-1, value held by lane l+1} for in[l] = l (64 lanes).
 * Used by the GPU tests to pin the cross-lane primitive the stencil kernels rely on. */
int smd_debug_lane_shift(float* out_left, float* out_right, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMD_HOTPATH_H */
