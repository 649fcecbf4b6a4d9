// smd_photo_dev.h — the per-element statements of the un-fused view-synthesis loss operators (smd_unfused.hip: ViewSynth's projection, PhotoError's error of
// one pixel from its window sums, ReconstructionLoss' predictive weighting mask), written once for that file and for the fused masked reconstruction
// (smd_maskrecon.hip), which has to take the decisions of the un-fused path bit for bit.  They live in a header, ahead of any `fp contract` pragma of the file
// that includes them, so that both files compile the same statements under the same contraction rule.
#pragma once
#include "smd_common.h"

namespace smd {

// ViewSynth.forward (src/tools/geometry.py:366-391): pixel (uf, vf) with depth D -> the sampling coordinate (sx, sy) in the support frame
struct PixGeom { float hx, hy, hz, nx, ny, yz, rz, sx, sy; };

__device__ __forceinline__ PixGeom pix_geom(const Cam& cm, float D, float uf, float vf, float wscale, float hscale) {
  PixGeom g;
  g.hx = fmaf(cm.H[0], uf, fmaf(cm.H[1], vf, cm.H[2]));
  g.hy = fmaf(cm.H[3], uf, fmaf(cm.H[4], vf, cm.H[5]));
  g.hz = fmaf(cm.H[6], uf, fmaf(cm.H[7], vf, cm.H[8]));
  g.nx = fmaf(D, g.hx, cm.a0); g.ny = fmaf(D, g.hy, cm.a1); g.yz = fmaf(D, g.hz, cm.tz);
  g.rz = __builtin_amdgcn_rcpf(fmaxf(g.yz, kZMin));
  g.sx = fmaf(g.nx*g.rz, wscale, -0.5f); g.sy = fmaf(g.ny*g.rz, hscale, -0.5f);
  return g;
}

// ReflectionPad2d(1): the index a 3x3 window reads for position i in [-1, n]
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2*(n - 1) - i : i); }

// One tap of the nine-tap un-normalised window sums of a channel (a: prediction, b: target), in the order the window is walked (rows, then columns)
__device__ __forceinline__ void window_tap(float a, float b, float& sx, float& sxx, float& sxy, float& sy, float& syy) {
  sx += a; sxx = fmaf(a, a, sxx); sxy = fmaf(a, b, sxy); sy += b; syy = fmaf(b, b, syy);
}

// SSIM error of one channel from the un-normalised (x9) window sums (src/losses/photometric.py:40-50), clamped to [0, 1]
__device__ __forceinline__ float ssim_win_err(float sx, float sxx, float sxy, float sy, float syy) {
  constexpr float c1 = 81.f*kC1, c2 = 81.f*kC2;
  const float t = sx*sy, sx2 = sx*sx;
  const float num = fmaf(2.f, t, c1)*fmaf(2.f, fmaf(9.f, sxy, -t), c2);
  // (the target's variance first, C2 after: added to 9 syy, 81 C2 = 0.07 would take the rounding of a number of size 81 sy^2 into a constant window's whole denominator)
  const float den = (sx2 + fmaf(sy, sy, c1))*(fmaf(9.f, sxx, -sx2) + (fmaf(9.f, syy, -sy*sy) + c2));
  return fminf(fmaxf(fmaf(-0.5f, num/den, 0.5f), 0.f), 1.f);
}

// ... and its three partials with respect to (sx, sxx, sxy) times `g`, zero where the clamp is active (k_photo_coef's statements)
__device__ __forceinline__ void ssim_win_coef(float sx, float sxx, float sxy, float sy, float syy, float g, float& ca, float& cb, float& cc) {
  constexpr float c1 = 81.f*kC1, c2 = 81.f*kC2;
  const float t = sx*sy, sx2 = sx*sx;
  const float a1 = fmaf(2.f, t, c1), a2 = fmaf(2.f, fmaf(9.f, sxy, -t), c2);
  const float b1 = sx2 + fmaf(sy, sy, c1), b2 = fmaf(9.f, sxx, -sx2) + (fmaf(9.f, syy, -sy*sy) + c2);      // (as the forward orders it)
  const float rden = 1.f/(b1*b2), val = a1*a2*rden, e = fmaf(-0.5f, val, 0.5f);
  const float prd = ((e >= 0.f && e <= 1.f) ? -0.5f*g : 0.f)*rden;
  ca = prd*(2.f*sy*(a2 - a1) - 2.f*sx*val*(b2 - b1));
  cb = prd*(-9.f*val*b1);
  cc = prd*(18.f*a1);
}

// PhotoError(weight_ssim) (src/losses/photometric.py:85-86): weight_ssim * mean_c SSIM + (1 - weight_ssim) * mean_c |.|  (es, el: the sums over the channels)
__device__ __forceinline__ float photo_mix(float es, float el, float rc, float w_ssim) { return fmaf(w_ssim*rc, es, ((1.f - w_ssim)*rc)*el); }

// Predictive weighting masks of `ReconstructionLoss.apply_mask` (src/losses/reconstruction.py:46-57): mode 1 'explainability': err * mask;
// mode 2 'uncertainty': err * exp(-mask) + mask.
__device__ __forceinline__ float masked_err(float e, float m, int mode) { return mode == 1 ? e*m : (mode == 2 ? fmaf(e, __expf(-m), m) : e); }

}  // namespace smd
