// smd_unfused.hip — class-level (un-fused) operators: ViewSynth, PhotoError, and the reduction half of ReconstructionLoss.
//
// These are the drop-ins for callers that hold the intermediate tensors themselves (the reference's `ViewSynth.forward`,
// `PhotoError.forward`, `ReconstructionLoss.forward` on already-warped images).  They share the device
// helpers of the fused kernels but are plain one-thread-per-pixel kernels: the fused path in smd_recon_*.hip is the hot
// one, this file is about API completeness and exact semantics (any channel count, depth_warp / mask_valid outputs,
// gradients to the warped INPUT as feature reconstruction needs them).
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_photo_dev.h"

namespace smd {

constexpr int kUfBlock = 256;

// (the per-element statements of every kernel here: smd_photo_dev.h, shared with smd_maskrecon.hip and smd_featrecon.hip)

// ---------------------------------------------------------------------------------------------
// ViewSynth.forward (src/tools/geometry.py:366-391)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kUfBlock) void k_view_synth_fwd(const float* __restrict__ input, const float* __restrict__ depth,
                                                             const float* __restrict__ T, const float* __restrict__ K,
                                                             const float* __restrict__ Kinv, float* __restrict__ warp,
                                                             float* __restrict__ depth_warp, uint8_t* __restrict__ mask_valid,
                                                             int C, int h, int w, float wscale, float hscale) {
  const int bi = blockIdx.y;
  const int pix = blockIdx.x*kUfBlock + threadIdx.x;
  if (pix >= h*w) return;
  Cam cm;
  make_cam(cm, T + (size_t)bi*16, K + (size_t)bi*16, Kinv + (size_t)bi*16);
  const int v = pix/w, u = pix - v*w;
  const size_t hw = (size_t)h*w;
  const PixGeom g = pix_geom(cm, depth[(size_t)bi*hw + pix], (float)u, (float)v, wscale, hscale);
  const Taps tp = make_taps(g.sx, g.sy, h, w, w);
  const float* in_b = input + (size_t)bi*C*hw;
  for (int c = 0; c < C; ++c) warp[((size_t)bi*C + c)*hw + pix] = bilerp(in_b + (size_t)c*hw, tp, w);
  if (depth_warp) depth_warp[(size_t)bi*hw + pix] = fmaxf(g.yz, kEps32);                      // geometry.py:340
  if (mask_valid) {
    const float gx = (g.nx*g.rz/(float)(w - 1) - 0.5f)*2.f, gy = (g.ny*g.rz/(float)(h - 1) - 0.5f)*2.f;   // :347-349
    mask_valid[(size_t)bi*hw + pix] = (fabsf(gx) < 1.f && fabsf(gy) < 1.f) ? 1 : 0;                        // :388
  }
}

hipError_t launch_view_synth_fwd(const float* input, const float* depth, const float* T, const float* K, const float* Kinv,
                                 float* warp, float* depth_warp, uint8_t* mask_valid, int B, int C, int h, int w, hipStream_t st) {
  const float wscale = synth_scale(w), hscale = synth_scale(h);
  hipLaunchKernelGGL(k_view_synth_fwd, dim3(ceil_div(h*w, kUfBlock), B), dim3(kUfBlock), 0, st, input, depth, T, K, Kinv, warp, depth_warp,
                     mask_valid, C, h, w, wscale, hscale);
  return hipGetLastError();
}

// Backward: dL/d(input) by scattering the four tap weights (atomics), dL/d depth per pixel, and the twelve pose sums
// per block that k_pose_finalize (smd_recon_bwd.hip) turns into dL/dT, dL/dK, dL/dKinv.
__global__ __launch_bounds__(kUfBlock) void k_view_synth_bwd(const float* __restrict__ input, const float* __restrict__ depth,
                                                             const float* __restrict__ T, const float* __restrict__ K,
                                                             const float* __restrict__ Kinv, const float* __restrict__ g_warp,
                                                             const float* __restrict__ g_depth_warp, float* __restrict__ g_input,
                                                             float* __restrict__ g_depth, float* __restrict__ pose_partial,
                                                             int C, int h, int w, float wscale, float hscale) {
  __shared__ float red[kUfBlock/64][kPoseSums];
  const int bi = blockIdx.y;
  const int pix = blockIdx.x*kUfBlock + threadIdx.x;
  const bool live = pix < h*w;
  Cam cm;
  make_cam(cm, T + (size_t)bi*16, K + (size_t)bi*16, Kinv + (size_t)bi*16);
  float ps[kPoseSums] = {};
  if (live) {
    const int v = pix/w, u = pix - v*w;
    const size_t hw = (size_t)h*w;
    const float D = depth[(size_t)bi*hw + pix];
    const float uf = (float)u, vf = (float)v;
    const PixGeom g = pix_geom(cm, D, uf, vf, wscale, hscale);
    const Taps tp = make_taps(g.sx, g.sy, h, w, w);
    const float* in_b = input + (size_t)bi*C*hw;
    float gsx = 0.f, gsy = 0.f;
    for (int c = 0; c < C; ++c) {
      float ddx, ddy;
      (void)bilerp(in_b + (size_t)c*hw, tp, w, ddx, ddy);
      const float go = g_warp[((size_t)bi*C + c)*hw + pix];
      gsx = fmaf(go, ddx, gsx); gsy = fmaf(go, ddy, gsy);
      if (g_input) {
        float* gi = g_input + ((size_t)bi*C + c)*hw + tp.off;
        atomicAdd(gi, go*(1.f - tp.fx)*(1.f - tp.fy)); atomicAdd(gi + 1, go*tp.fx*(1.f - tp.fy));
        atomicAdd(gi + w, go*(1.f - tp.fx)*tp.fy); atomicAdd(gi + w + 1, go*tp.fx*tp.fy);
      }
    }
    float gnx, gny, gz;
    synth_adj(g, tp, gsx, gsy, wscale, hscale, gnx, gny, gz);
    if (g_depth_warp && g.yz >= kEps32) gz += g_depth_warp[(size_t)bi*hw + pix];               // depth_warp = clamp(Yz, eps)
    g_depth[(size_t)bi*hw + pix] = synth_adj_depth(g, gnx, gny, gz);
    pose_sums(ps, gnx, gny, gz, D, uf, vf);
  }
  store_pose_sums<kUfBlock/64>(ps, &red[0][0], pose_partial + ((size_t)bi*gridDim.x + blockIdx.x)*kPoseSums);
}

hipError_t launch_view_synth_bwd(const float* input, const float* depth, const float* T, const float* K, const float* Kinv,
                                 const float* g_warp, const float* g_depth_warp, float* g_input, float* g_depth,
                                 float* g_T, float* g_K, float* g_Kinv, float* ws, int B, int C, int h, int w, hipStream_t st) {
  const float wscale = synth_scale(w), hscale = synth_scale(h);
  const int nblk = ceil_div(h*w, kUfBlock);
  if (g_input) { hipError_t e = hipMemsetAsync(g_input, 0, (size_t)B*C*h*w*sizeof(float), st); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(k_view_synth_bwd, dim3(nblk, B), dim3(kUfBlock), 0, st, input, depth, T, K, Kinv, g_warp, g_depth_warp, g_input, g_depth,
                     ws, C, h, w, wscale, hscale);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_pose_finalize(ws, nblk, nblk, T, K, Kinv, g_T, g_K, g_Kinv, B, 1, st);
}

// ---------------------------------------------------------------------------------------------
// PhotoError(0.85) / DenseL1Error / DenseL2Error for any channel count (src/losses/photometric.py:11-20, 54-88)
// ---------------------------------------------------------------------------------------------
enum { kPhotoSsim = 0, kPhotoL1 = 1, kPhotoL2 = 2 };

// Nine-tap (reflection padded) un-normalised window sums of one channel at (v, u).
__device__ __forceinline__ void window_sums(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int v, int u,
                                            float& sx, float& sxx, float& sxy, float& sy, float& syy) {
  window_walk([&](int dv, int du, float& a, float& b) { const int rv = reflect1(v + dv, h)*w, idx = rv + reflect1(u + du, w); a = x[idx]; b = y[idx]; }, sx, sxx, sxy, sy, syy);
}

__global__ __launch_bounds__(kUfBlock) void k_photo_error_fwd(const float* __restrict__ pred, const float* __restrict__ target,
                                                              float* __restrict__ err, int C, int h, int w, int mode, float w_ssim) {
  const int ni = blockIdx.y;
  const int pix = blockIdx.x*kUfBlock + threadIdx.x;
  if (pix >= h*w) return;
  const int v = pix/w, u = pix - v*w;
  const size_t hw = (size_t)h*w;
  float es = 0.f, el = 0.f, e2 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* x = pred + ((size_t)ni*C + c)*hw; const float* y = target + ((size_t)ni*C + c)*hw;
    const float d = x[pix] - y[pix];
    el += fabsf(d); e2 = fmaf(d, d, e2);
    if (mode == kPhotoSsim) {
      float sx, sxx, sxy, sy, syy;
      window_sums(x, y, h, w, v, u, sx, sxx, sxy, sy, syy);
      es += ssim_win_err(sx, sxx, sxy, sy, syy);
    }
  }
  const float rc = 1.f/(float)C;
  // PhotoError(weight_ssim) (src/losses/photometric.py:85-86): weight_ssim * mean_c SSIM + (1 - weight_ssim) * mean_c |.|
  err[(size_t)ni*hw + pix] = mode == kPhotoL2 ? dense_err(el, e2, 0, rc) : (mode == kPhotoL1 ? dense_err(el, e2, 1, rc) : photo_mix(es, el, rc, w_ssim));
}

static inline int photo_mode(int flags) { return (flags & SMD_LOSS_L2) ? kPhotoL2 : ((flags & SMD_LOSS_L1) ? kPhotoL1 : kPhotoSsim); }

hipError_t launch_photo_error_fwd(const float* pred, const float* target, float* err, int N, int C, int h, int w, int flags, float w_ssim, hipStream_t st) {
  int mode = photo_mode(flags);
  if (mode == kPhotoSsim && w_ssim == 0.f) mode = kPhotoL1;      // PhotoError(0): the SSIM term is not evaluated (photometric.py:72)
  hipLaunchKernelGGL(k_photo_error_fwd, dim3(ceil_div(h*w, kUfBlock), N), dim3(kUfBlock), 0, st, pred, target, err, C, h, w, mode, w_ssim);
  return hipGetLastError();
}

// Backward, pass 1: per pixel p the three SSIM partials (w.r.t. the x9 sums) times the upstream gradient -> coef (N,9,h,w).
__global__ __launch_bounds__(kUfBlock) void k_photo_coef(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const float* __restrict__ g_err, float* __restrict__ coef, int C, int h, int w, float w_ssim) {
  const int ni = blockIdx.y;
  const int pix = blockIdx.x*kUfBlock + threadIdx.x;
  if (pix >= h*w) return;
  const int v = pix/w, u = pix - v*w;
  const size_t hw = (size_t)h*w;
  const float g = g_err[(size_t)ni*hw + pix]*(w_ssim/(float)C);
  for (int c = 0; c < C; ++c) {
    const float* x = pred + ((size_t)ni*C + c)*hw; const float* y = target + ((size_t)ni*C + c)*hw;
    float sx, sxx, sxy, sy, syy;
    window_sums(x, y, h, w, v, u, sx, sxx, sxy, sy, syy);
    float* cp = coef + ((size_t)ni*3*C + c*3)*hw + pix;
    ssim_win_coef(sx, sxx, sxy, sy, syy, g, cp[0], cp[hw], cp[2*hw]);
  }
}

// Backward, pass 2: adjoint of (reflection pad + 3x3 sum) applied to the coefficient maps, plus the L1 term.
__global__ __launch_bounds__(kUfBlock) void k_photo_error_bwd(const float* __restrict__ pred, const float* __restrict__ target,
                                                              const float* __restrict__ g_err, const float* __restrict__ coef,
                                                              float* __restrict__ g_pred, int C, int h, int w, int mode, float w_ssim) {
  const int ni = blockIdx.y;
  const int pix = blockIdx.x*kUfBlock + threadIdx.x;
  if (pix >= h*w) return;
  const int v = pix/w, u = pix - v*w;
  const size_t hw = (size_t)h*w;
  const float ge = g_err[(size_t)ni*hw + pix];
  if (mode == kPhotoL2) {   // sqrt(clamp(sum d^2, eps)): zero gradient where the clamp is active
    float e2 = 0.f;
    for (int c = 0; c < C; ++c) { const float d = pred[((size_t)ni*C + c)*hw + pix] - target[((size_t)ni*C + c)*hw + pix]; e2 = fmaf(d, d, e2); }
    const float k = dense_l2_gfac(ge, e2);
    for (int c = 0; c < C; ++c) g_pred[((size_t)ni*C + c)*hw + pix] = k*(pred[((size_t)ni*C + c)*hw + pix] - target[((size_t)ni*C + c)*hw + pix]);
    return;
  }
  const float gl = ge*(mode == kPhotoL1 ? 1.f : (1.f - w_ssim))/(float)C;
  float wv[3], wu[3];
  reflect_weights_adj(v, h, wv[0], wv[2]); wv[1] = 1.f;
  reflect_weights_adj(u, w, wu[0], wu[2]); wu[1] = 1.f;
  for (int c = 0; c < C; ++c) {
    const float x = pred[((size_t)ni*C + c)*hw + pix], y = target[((size_t)ni*C + c)*hw + pix];
    const float d = x - y;
    float gx = gl*sgn(d);
    if (mode == kPhotoSsim) {
      const float* cp = coef + ((size_t)ni*3*C + c*3)*hw;
      float SA = 0.f, SB = 0.f, SC = 0.f;
#pragma unroll
      for (int dv = -1; dv <= 1; ++dv) {
        const int pv = v + dv;
        if (pv < 0 || pv >= h) continue;
#pragma unroll
        for (int du = -1; du <= 1; ++du) {
          const int pu = u + du;
          if (pu < 0 || pu >= w) continue;
          const float wt = wv[dv + 1]*wu[du + 1];
          const int idx = pv*w + pu;
          SA = fmaf(wt, cp[idx], SA); SB = fmaf(wt, cp[hw + idx], SB); SC = fmaf(wt, cp[2*hw + idx], SC);
        }
      }
      gx += fmaf(2.f*x, SB, fmaf(y, SC, SA));
    }
    g_pred[((size_t)ni*C + c)*hw + pix] = gx;
  }
}

hipError_t launch_photo_error_bwd(const float* pred, const float* target, const float* g_err, float* g_pred, float* ws,
                                  int N, int C, int h, int w, int flags, float w_ssim, hipStream_t st) {
  int mode = photo_mode(flags);
  if (mode == kPhotoSsim && w_ssim == 0.f) mode = kPhotoL1;
  dim3 grid(ceil_div(h*w, kUfBlock), N);
  if (mode == kPhotoSsim) hipLaunchKernelGGL(k_photo_coef, grid, dim3(kUfBlock), 0, st, pred, target, g_err, ws, C, h, w, w_ssim);
  hipLaunchKernelGGL(k_photo_error_bwd, grid, dim3(kUfBlock), 0, st, pred, target, g_err, ws, g_pred, C, h, w, mode, w_ssim);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Reduction half of ReconstructionLoss.forward (src/losses/reconstruction.py:43-44, 59-77, 125)
// ---------------------------------------------------------------------------------------------
// Predictive weighting masks of `ReconstructionLoss.apply_mask` (src/losses/reconstruction.py:46-57): mask (B,n,h,w) in the
// reference's layout, one channel per support (`masked_err`, smd_photo_dev.h).

__global__ __launch_bounds__(kUfBlock) void k_recon_reduce_fwd(const float* __restrict__ err_warp, const float* __restrict__ err_static,
                                                               const float* __restrict__ noise, uint32_t seed_lo, uint32_t seed_hi,
                                                               float* __restrict__ err, uint8_t* __restrict__ sel, float* __restrict__ partial,
                                                               int n, unsigned total, int use_min, const float* __restrict__ mask, int mask_mode, unsigned hw) {
  __shared__ float red[kUfBlock/64];
  const unsigned idx = blockIdx.x*kUfBlock + threadIdx.x;
  float e = 0.f;
  if (idx < total) {
    const unsigned bi = idx/hw, pix = idx - bi*hw;
    auto mk = [&](int i) { return mask_mode ? mask[((size_t)bi*n + i)*hw + pix] : 0.f; };
    float best = masked_err(err_warp[idx], mk(0), mask_mode), acc = best;
    int bsel = 0;
    for (int i = 1; i < n; ++i) { const float v = masked_err(err_warp[(size_t)i*total + idx], mk(i), mask_mode); acc += v; if (v < best) { best = v; bsel = i; } }
    e = use_min ? best : acc/(float)n;
    if (!use_min) bsel = 0;
    if (err_static) {
      float sb = masked_err(err_static[idx], mk(0), mask_mode), sa = sb;
      for (int i = 1; i < n; ++i) { const float v = masked_err(err_static[(size_t)i*total + idx], mk(i), mask_mode); sa += v; sb = fminf(sb, v); }
      float est = use_min ? sb : sa/(float)n;
      est = fmaf(kEps32, noise ? noise[idx] : gauss_noise(seed_lo, seed_hi, idx), est);
      if (est < e) { e = est; bsel = SMD_SEL_MASKED; }
    }
    err[idx] = e; sel[idx] = (uint8_t)bsel;
  }
  block_store_sum<Waves::Sequential, kUfBlock/64>(e, red, partial + blockIdx.x);
}

static inline int mask_mode_of(int flags, const float* mask) { return !mask ? 0 : ((flags & SMD_MASK_UNCERTAINTY) ? 2 : ((flags & SMD_MASK_EXPLAINABILITY) ? 1 : 0)); }

hipError_t launch_recon_reduce_fwd(const float* err_warp, const float* err_static, const float* mask, const float* noise, uint64_t seed,
                                   float* err, uint8_t* sel, float* loss, float* ws, int n, int B, int h, int w, int flags, hipStream_t st) {
  const unsigned total = (unsigned)B*h*w;
  const int nblk = ceil_div((int)total, kUfBlock);
  hipLaunchKernelGGL(k_recon_reduce_fwd, dim3(nblk), dim3(kUfBlock), 0, st, err_warp, (flags & SMD_USE_AUTOMASK) ? err_static : nullptr, noise,
                     (uint32_t)seed, (uint32_t)(seed >> 32), err, sel, ws, n, total, (flags & SMD_USE_MIN) ? 1 : 0, mask, mask_mode_of(flags, mask), (unsigned)(h*w));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_sum_partials(ws, nblk, 1.0/(double)total, loss, st);
}

// Backward.  Without a mask: the upstream gradient routed by `sel`.  With a mask the error that reached the loss was
// f(err, m) = err*m | err*exp(-m) + m, so the routed gradient is scaled by df/derr and the mask receives df/dm — also where the
// STATIC error won (sel == masked): the identity error carries no gradient to the images but it does to the mask
// (reconstruction.py:70-71 evaluates `compute_photo(source, target, mask=mask)`); its winning support is re-derived here.
__global__ __launch_bounds__(kUfBlock) void k_recon_reduce_bwd(const uint8_t* __restrict__ sel, const float* __restrict__ g_loss,
                                                               float* __restrict__ g_err_warp, int n, unsigned total, int use_min,
                                                               const float* __restrict__ err_warp, const float* __restrict__ err_static,
                                                               const float* __restrict__ mask, float* __restrict__ g_mask, int mask_mode, unsigned hw) {
  const unsigned idx = blockIdx.x*kUfBlock + threadIdx.x;
  if (idx >= total) return;
  const float g = g_loss[0]/(float)total, gn = g/(float)n;
  const int s = sel[idx];
  const unsigned bi = idx/hw, pix = idx - bi*hw;
  int jstat = -1;                       // static winner (min-reprojection over the masked identity errors), when the automask removed the pixel
  if (mask_mode && s == SMD_SEL_MASKED && use_min && err_static) {
    float sb = 0.f;
    for (int i = 0; i < n; ++i) {
      const float v = masked_err(err_static[(size_t)i*total + idx], mask[((size_t)bi*n + i)*hw + pix], mask_mode);
      if (i == 0 || v < sb) { sb = v; jstat = i; }
    }
  }
  for (int i = 0; i < n; ++i) {
    float v = routed(s, i, g, gn, use_min);
    if (mask_mode) {
      const size_t mi = ((size_t)bi*n + i)*hw + pix;
      const float m = mask[mi];
      const float gs = routed_static(s, i, jstat, g, gn, use_min, err_static != nullptr);      // gradient reaching the masked STATIC error of support i
      const float ew = err_warp[(size_t)i*total + idx], es = err_static ? err_static[(size_t)i*total + idx] : 0.f;
      const float dm = mask_mode == 1 ? m : __expf(-m);      // d masked / d err
      g_mask[mi] = mask_grad(v, gs, ew, es, dm, mask_mode);
      v *= dm;
    }
    g_err_warp[(size_t)i*total + idx] = v;
  }
}

hipError_t launch_recon_reduce_bwd(const uint8_t* sel, const float* g_loss, float* g_err_warp, const float* err_warp, const float* err_static,
                                   const float* mask, float* g_mask, int n, int B, int h, int w, int flags, hipStream_t st) {
  const unsigned total = (unsigned)B*h*w;
  hipLaunchKernelGGL(k_recon_reduce_bwd, dim3(ceil_div((int)total, kUfBlock)), dim3(kUfBlock), 0, st, sel, g_loss, g_err_warp, n, total,
                     (flags & SMD_USE_MIN) ? 1 : 0, err_warp, (flags & SMD_USE_AUTOMASK) ? err_static : nullptr, mask, g_mask, mask_mode_of(flags, mask), (unsigned)(h*w));
  return hipGetLastError();
}

}  // namespace smd
