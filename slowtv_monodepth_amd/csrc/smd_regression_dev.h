// smd_regression_dev.h — the per-element functions of `RegressionLoss` (src/losses/regression.py:11-37, 69-75), shared by smd_regression.hip (the operator on
// a caller's mask) and smd_hints.hip (the Depth-Hints form that builds its mask itself): `to_inv`, the three criteria, berHu's dynamic threshold
// delta = 0.2 * max|p - t| and the adjoint of each.  One spelling, so the two operators agree element by element.
#pragma once
#include "smd_common.h"
#include "../../include/smd_hotpath.h"

namespace smd {

enum { kRegrL1 = 0, kRegrLogL1 = 1, kRegrBerhu = 2 };

static inline int regr_mode(int flags) { return (flags & SMD_REGR_BERHU) ? kRegrBerhu : ((flags & SMD_REGR_LOG_L1) ? kRegrLogL1 : kRegrL1); }

__device__ __forceinline__ float inv_map(float x, bool invert) { return invert ? ((x > 0.f) ? 1.f/fmaxf(x, kEps32) : 0.f) : x; }
// d to_inv(x)/dx: -1/x^2 on the pass-through branch, 0 where x <= 0 or the clamp is active
__device__ __forceinline__ float inv_map_grad(float x, bool invert) { return invert ? ((x >= kEps32) ? -1.f/(x*x) : 0.f) : 1.f; }

// l1 / log_l1 of one element times its mask value m (berHu needs the threshold: `berhu_value`)
__device__ __forceinline__ float regr_value(float m, int mode, float diff) { return m*(mode == kRegrL1 ? diff : logf(1.f + diff)); }

__device__ __forceinline__ float berhu_value(float diff, float delta) {
  return (diff <= delta) ? diff : (diff*diff + delta*delta)/(2.f*delta + kEps32);
}
// m * d berhu/d delta on the quadratic branch (diff > delta), q = 2 delta + eps
__device__ __forceinline__ float berhu_ddelta(float m, float diff, float delta, float q) { return m*(2.f*delta*q - 2.f*(diff*diff + delta*delta))/(q*q); }

// d loss/d (p' - t') of one element, p' and t' the (optionally inverted) operands and d their difference: `ge` the element's share of the incoming gradient
// (0 where masked out), `g_tie` what an element attaining the maximum receives through berHu's threshold; sign(0) = 0
__device__ __forceinline__ float regr_grad_diff(int mode, float ge, float d, float diff, float delta, float q, float mxd, float g_tie) {
  float gd;
  if (mode == kRegrL1) gd = ge;
  else if (mode == kRegrLogL1) gd = ge/(1.f + diff);
  else gd = ((diff <= delta) ? ge : ge*2.f*diff/q) + ((diff == mxd) ? g_tie : 0.f);
  return gd*((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f));
}

}  // namespace smd
