// smd_photo_dev.h — the per-element statements of the view-synthesis loss written statement by statement: the un-fused operators (smd_unfused.hip: ViewSynth,
// PhotoError, the reduction half of ReconstructionLoss), the fused masked reconstruction (smd_maskrecon.hip) and FeatDepth's feature-metric reconstruction
// (smd_featrecon.hip).  The three files have to take each other's decisions bit for bit, so every stage they share is written once, here.
//
// Contraction rule, stated once.  The FORWARD statements (down to masked_err) are compiled under the default (-ffp-contract=fast) in all three files, with fmaf written
// out wherever a fused multiply-add is meant: `sel` equality between the routes rests on that.  Below them `mask_grad`, `synth_adj` and `pose_sums`, which hold a multiply next to an add, carry
// `#pragma clang fp contract(off)` in their bodies: written apart stays apart in every file and instantiation, whatever the including file sets; the others have nothing to contract.
// (smd_unfused.hip's own copies of `gpx*nx + gpy*ny` and `v*ew + gs*es` were one fused multiply-add each; they now round as the fused kernels'.)
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

// The nine-tap walk: fetch(dv, du, a, b) reads prediction and target at the window's offset (dv, du).  Rows first, then columns: the order is part of the sums.
template <class Fetch>
__device__ __forceinline__ void window_walk(Fetch fetch, float& sx, float& sxx, float& sxy, float& sy, float& syy) {
  sx = sxx = sxy = sy = syy = 0.f;
#pragma unroll
  for (int dv = -1; dv <= 1; ++dv)
#pragma unroll
    for (int du = -1; du <= 1; ++du) { float a, b; fetch(dv, du, a, b); window_tap(a, b, sx, sxx, sxy, sy, syy); }
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

__device__ __forceinline__ float sgn(float d) { return (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f); }

// PhotoError(weight_ssim) (src/losses/photometric.py:85-86): weight_ssim * mean_c SSIM + (1 - weight_ssim) * mean_c |.|  (es, el: the sums over the channels)
__device__ __forceinline__ float photo_mix(float es, float el, float rc, float w_ssim) { return fmaf(w_ssim*rc, es, ((1.f - w_ssim)*rc)*el); }

// DenseL1Error / DenseL2Error (src/losses/photometric.py:11-20) from e1 = sum_c |d|, e2 = sum_c d^2: mean_c |d| or sqrt(clamp(e2, eps)); and the factor of d in
// the L2 error's gradient, ge / sqrt(e2), zero where the clamp is active
__device__ __forceinline__ float dense_err(float e1, float e2, int l1, float rc) { return l1 ? e1*rc : sqrtf(fmaxf(e2, kEps32)); }
__device__ __forceinline__ float dense_l2_gfac(float ge, float e2) { return (e2 >= kEps32) ? ge/sqrtf(e2) : 0.f; }

// Predictive weighting masks of `ReconstructionLoss.apply_mask` (src/losses/reconstruction.py:46-57): mode 1 'explainability': err * mask;
// mode 2 'uncertainty': err * exp(-mask) + mask.
__device__ __forceinline__ float masked_err(float e, float m, int mode) { return mode == 1 ? e*m : (mode == 2 ? fmaf(e, __expf(-m), m) : e); }

// ------------------------------------------------------------------------------------------------- the reduction's last step and the backward statements (contraction: top of the file)
// Backward of the reduction over the supports (src/losses/reconstruction.py:59-77; the forward reduction stays in the three kernels: written as functions here it changed
// the branches and moves the compiler laid out in each of them): the gradient that `sel` = s sends to the (masked) warped error of support i (g for the
// minimum, gn = g / n for the mean); and the one that reaches its masked STATIC error where the automask won (jstat: the static winner).
__device__ __forceinline__ float routed(int s, int i, float g, float gn, int use_min) { return use_min ? (s == i ? g : 0.f) : (s != SMD_SEL_MASKED ? gn : 0.f); }
__device__ __forceinline__ float routed_static(int s, int i, int jstat, float g, float gn, int use_min, bool automask) { return (automask && s == SMD_SEL_MASKED) ? (use_min ? (i == jstat ? g : 0.f) : gn) : 0.f; }
// d loss / d mask of one support: v, gs the gradients at its masked warped and static errors ew, es; dm = d masked / d err (the mask | exp(-mask)).  k_recon_reduce_bwd's;
// k_mask_recon_bwd writes the same statement itself (called as a function it lost LDS reads and gained selects in five instantiations, one VGPR in one)
__device__ __forceinline__ float mask_grad(float v, float gs, float ew, float es, float dm, int mode) {
#pragma clang fp contract(off)
  return mode == 1 ? v*ew + gs*es : v*fmaf(-ew, dm, 1.f) + gs*fmaf(-es, dm, 1.f);
}

// ViewSynth.backward at one pixel: (gsx, gsy) = dL/d(sx, sy) -> dL/d(nx, ny, Yz), and from those the pixel's dL/d depth (k_view_synth_bwd adds the gradient of its
// depth_warp output to gz in between) and its twelve pose sums (smd_pose_fin.h turns the blocks' sums into dL/dT, dL/dK, dL/dKinv).
__device__ __forceinline__ void synth_adj(const PixGeom& g, const Taps& tp, float gsx, float gsy, float wscale, float hscale, float& gnx, float& gny, float& gz) {
#pragma clang fp contract(off)
  const float gpx = gsx*tp.mx*wscale, gpy = gsy*tp.my*hscale;
  gnx = gpx*g.rz; gny = gpy*g.rz;
  gz = (g.yz >= kZMin) ? -(gpx*g.nx + gpy*g.ny)*g.rz*g.rz : 0.f;
}
__device__ __forceinline__ float synth_adj_depth(const PixGeom& g, float gnx, float gny, float gz) { return fmaf(gnx, g.hx, fmaf(gny, g.hy, gz*g.hz)); }
__device__ __forceinline__ void pose_sums(float (&ps)[kPoseSums], float gnx, float gny, float gz, float D, float uf, float vf) {
#pragma clang fp contract(off)
  const float dnx = gnx*D, dny = gny*D, dz = gz*D;
  ps[0] = dnx*uf; ps[1] = dnx*vf; ps[2] = dnx; ps[3] = dny*uf; ps[4] = dny*vf; ps[5] = dny;
  ps[6] = dz*uf; ps[7] = dz*vf; ps[8] = dz; ps[9] = gnx; ps[10] = gny; ps[11] = gz;
}

// The pose sums of a block of NW waves -> dst[0..11].  `red`: NW x 12 floats of LDS; the barrier that lets it be written again is the caller's.
template <int NW> __device__ __forceinline__ void store_pose_sums(const float (&ps)[kPoseSums], float* red, float* __restrict__ dst) {
  stage_wave_sums(ps, red);
  // (0.f +: these sums have always started from +0, and a pose sum, unlike an accumulator, can be -0 in every wave)
  if (threadIdx.x < kPoseSums) dst[threadIdx.x] = 0.f + sum_waves<Waves::Sequential, NW>(red, kPoseSums, threadIdx.x);
}

}  // namespace smd
