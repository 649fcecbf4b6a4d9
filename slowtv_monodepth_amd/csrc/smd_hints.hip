// smd_hints.hip — the Depth-Hints proxy-depth regression over every scale in one sweep (reference: `handlers.depth_regr`, src/core/handlers.py:201-259, on
// `RegressionLoss.forward`, src/losses/regression.py:69-75), and its adjoint.
//
//   m[s][i] = hints[i] > 0 && (!automask || err[1+s][i] > err[0][i])          e[s][i] = m ? crit(depth[s][i], hints[i]) : 0          loss = sum(e) / sum(m)
//
// err[0] is the photometric error of the supports warped by the hints, err[1+s] by the prediction of scale s (the fused reconstruction forward's error
// stack over [hints, depth_0 .. depth_{S-1}]); crit and berHu's dynamic threshold 0.2 * max|diff| over ALL elements are smd_regression_dev.h's, shared with
// smd_regression.hip.  Nothing of size (S*b, ...) is expanded: a thread owns four consecutive pixels, reads the hints (and err[0]) ONCE and walks the S
// scales with them in registers.
//
// Streaming shape: depth, err and g_depth are S (S+1) slices of P = b*h*w floats.  Where P % 4 == 0 and every base is 16-byte aligned a group of four pixels
// moves as one 16-byte vector per slice; otherwise (a slice then starts at an odd element) every element goes on its own under an explicit bound.
//
// Reduction: three fp64 sums per block (max of diff, sum of m, sum of e), then a one-block second stage that adds the blocks in a fixed order: no atomics,
// two runs are bit-equal.  berHu needs the maximum before it can form an error, so its forward is two sweeps; the second one also sums d e/d delta, so that
// the backward is ONE sweep in every mode.
//
// The mask goes to the backward as one bit per element: the 4 x S bits of a thread's group in one 32-bit word (bit 4 s + k: scale s, pixel 4 g + k), S <= 8.
// The backward reads that word, never `err`.
//
// stats (8 floats, written by the forward, read by the backward): [0] max diff, [1] sum(m), [2] #elements attaining the max (berHu), [3] sum of
// m * d berhu/d delta (berHu).
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_regression_dev.h"

namespace smd {

namespace {

constexpr int kHintsBlock = 256;

// out[k] = p[i0 + k], zeros at and beyond P; `vec`: P % 4 == 0 and p + i0 is 16-byte aligned
__device__ __forceinline__ void load4(const float* __restrict__ p, size_t i0, size_t P, bool vec, float* out) {
  if (vec) {
    const f4 v = *(const f4*)(p + i0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (i0 + k < P) ? p[i0 + k] : 0.f;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// the block's (max of mx, sums of acc[0], acc[1]) -> part[3 blockIdx.x ..]; red: 12 doubles
__device__ __forceinline__ void block_partials(float mx, const double (&acc)[2], double* red, double* __restrict__ part) {
  const float wmx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[8 + (threadIdx.x >> 6)] = (double)wmx;
  stage_wave_sums(acc, red);      // (its barrier covers the maxima too)
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x*3] = fmax(fmax(red[8], red[9]), fmax(red[10], red[11]));
    part[(size_t)blockIdx.x*3 + 1] = sum_waves<Waves::Sequential, 4>(red, 2, 0);
    part[(size_t)blockIdx.x*3 + 2] = sum_waves<Waves::Sequential, 4>(red, 2, 1);
  }
}

// one block: (max, sum, sum) over the blocks' partials in a fixed order -> every thread
__device__ __forceinline__ void total_partials(const double* __restrict__ part, int nblk, double* red, double& mx, double& a, double& b) {
  double m = 0.0, acc[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += kHintsBlock) { m = fmax(m, part[(size_t)i*3]); acc[0] += part[(size_t)i*3 + 1]; acc[1] += part[(size_t)i*3 + 2]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[8 + (threadIdx.x >> 6)] = m;
  stage_wave_sums(acc, red);
  mx = fmax(fmax(red[8], red[9]), fmax(red[10], red[11]));
  a = sum_waves<Waves::Sequential, 4>(red, 2, 0); b = sum_waves<Waves::Sequential, 4>(red, 2, 1);
}

}  // namespace

// Sweep 1 (every mode): the mask (bits, and scale 0 as bytes), max diff, sum(m); for l1 / log_l1 the error sum too.
__global__ __launch_bounds__(kHintsBlock) void k_hints_sweep1(const float* __restrict__ depth, const float* __restrict__ hints, const float* __restrict__ err,
                                                              int S, size_t P, int mode, int invert, int vec, uint8_t* __restrict__ mask0,
                                                              uint32_t* __restrict__ bits, double* __restrict__ part) {
  __shared__ double red[12];
  const size_t g = (size_t)blockIdx.x*kHintsBlock + threadIdx.x, i0 = g*4;
  float mx = 0.f;
  double acc[2] = {0.0, 0.0};
  if (i0 < P) {
    float t[4], e0[4] = {0.f, 0.f, 0.f, 0.f};
    load4(hints, i0, P, vec, t);
    if (err) load4(err, i0, P, vec, e0);
    uint32_t word = 0;
    for (int s = 0; s < S; ++s) {
      float d[4], es[4] = {0.f, 0.f, 0.f, 0.f};
      load4(depth + (size_t)s*P, i0, P, vec, d);
      if (err) load4(err + (size_t)(s + 1)*P, i0, P, vec, es);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i0 + k < P) {
          const float diff = fabsf(inv_map(d[k], invert) - inv_map(t[k], invert));
          const bool m = t[k] > 0.f && (!err || es[k] > e0[k]);
          mx = fmaxf(mx, diff);
          if (m) {
            word |= 1u << (s*4 + k);
            acc[0] += 1.0;
            if (mode != kRegrBerhu) acc[1] += (double)regr_value(1.f, mode, diff);
          }
        }
      }
    }
    bits[g] = word;
    if (vec) {
      *(uint32_t*)(mask0 + i0) = (word & 1u) | ((word & 2u) << 7) | ((word & 4u) << 14) | ((word & 8u) << 21);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (i0 + k < P) mask0[i0 + k] = (uint8_t)((word >> k) & 1u);
    }
  }
  block_partials(mx, acc, red, part);
}

__global__ __launch_bounds__(kHintsBlock) void k_hints_fin1(const double* __restrict__ part, int nblk, int mode, float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double red[12];
  double mx, ms, es;
  total_partials(part, nblk, red, mx, ms, es);
  if (threadIdx.x == 0) {
    stats[0] = (float)mx; stats[1] = (float)ms; stats[2] = 0.f; stats[3] = 0.f;
    if (mode != kRegrBerhu) loss[0] = (float)(es/ms);
  }
}

// Sweep 2 (berHu): the errors with the now-known threshold, from the mask bits: the error sum, the number of elements attaining the maximum and the sum of
// m * d berhu/d delta (the tie counts travel in a partial array of their own, behind the three-slot one).
__global__ __launch_bounds__(kHintsBlock) void k_hints_sweep2(const float* __restrict__ depth, const float* __restrict__ hints, int S, size_t P, int invert, int vec,
                                                              const uint32_t* __restrict__ bits, const float* __restrict__ stats, double* __restrict__ part,
                                                              double* __restrict__ part_ties) {
  __shared__ double red[12];
  const float mxd = stats[0], delta = 0.2f*mxd, q = 2.f*delta + kEps32;
  const size_t g = (size_t)blockIdx.x*kHintsBlock + threadIdx.x, i0 = g*4;
  double acc[2] = {0.0, 0.0}, ties[2] = {0.0, 0.0};
  if (i0 < P) {
    float t[4];
    load4(hints, i0, P, vec, t);
    const uint32_t word = bits[g];
    for (int s = 0; s < S; ++s) {
      float d[4];
      load4(depth + (size_t)s*P, i0, P, vec, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i0 + k < P) {
          const float diff = fabsf(inv_map(d[k], invert) - inv_map(t[k], invert));
          if (diff == mxd) ties[0] += 1.0;
          if ((word >> (s*4 + k)) & 1u) {
            acc[0] += (double)berhu_value(diff, delta);
            if (diff > delta) acc[1] += (double)berhu_ddelta(1.f, diff, delta, q);
          }
        }
      }
    }
  }
  block_partials(0.f, acc, red, part);
  __syncthreads();
  stage_wave_sums(ties, red);
  if (threadIdx.x == 0) part_ties[blockIdx.x] = sum_waves<Waves::Sequential, 4>(red, 2, 0);
}

__global__ __launch_bounds__(kHintsBlock) void k_hints_fin2(const double* __restrict__ part, const double* __restrict__ part_ties, int nblk,
                                                            float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double red[12];
  double mx, es, dd;
  total_partials(part, nblk, red, mx, es, dd);
  __syncthreads();
  double tie[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += kHintsBlock) tie[0] += part_ties[i];
  stage_wave_sums(tie, red);
  if (threadIdx.x == 0) {
    stats[2] = (float)sum_waves<Waves::Sequential, 4>(red, 2, 0); stats[3] = (float)dd;
    loss[0] = (float)(es/(double)stats[1]);
  }
}

// Backward, one sweep: g_depth from the mask bits (the formulas of smd_regression.hip's k_regr_bwd, element by element).
__global__ __launch_bounds__(kHintsBlock) void k_hints_bwd(const float* __restrict__ depth, const float* __restrict__ hints, const uint32_t* __restrict__ bits,
                                                           int S, size_t P, int mode, int invert, int vec, const float* __restrict__ stats,
                                                           const float* __restrict__ g_loss, float* __restrict__ g_depth) {
  const size_t g = (size_t)blockIdx.x*kHintsBlock + threadIdx.x, i0 = g*4;
  if (i0 >= P) return;
  const float gs = g_loss[0]/stats[1];
  const float mxd = stats[0], delta = 0.2f*mxd, q = 2.f*delta + kEps32;
  const float g_tie = (mode == kRegrBerhu) ? 0.2f*gs*stats[3]/stats[2] : 0.f;   // d loss/d delta through the max, split over ties
  float t[4];
  load4(hints, i0, P, vec, t);
  const uint32_t word = bits[g];
  for (int s = 0; s < S; ++s) {
    float d[4], o[4];
    load4(depth + (size_t)s*P, i0, P, vec, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dd = inv_map(d[k], invert) - inv_map(t[k], invert);
      const float ge = gs*(((word >> (s*4 + k)) & 1u) ? 1.f : 0.f);
      o[k] = regr_grad_diff(mode, ge, dd, fabsf(dd), delta, q, mxd, g_tie)*inv_map_grad(d[k], invert);
    }
    float* po = g_depth + (size_t)s*P + i0;
    if (vec) {
      *(f4*)po = f4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (i0 + k < P) po[k] = o[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------- host
// blocks of 256 groups of four pixels; 0: P outside [1, 2^31)
int hints_blocks(size_t P) {
  if (P < 1 || P >= ((size_t)1 << 31)) return 0;
  const size_t groups = (P + 3)/4;
  return (int)((groups + kHintsBlock - 1)/kHintsBlock);
}

hipError_t launch_hints_regr_fwd(const float* depth, const float* hints, const float* err, int S, size_t P, int flags, int vec, float* loss, uint8_t* mask0,
                                 uint32_t* bits, float* stats, double* ws, hipStream_t st) {
  const int mode = regr_mode(flags), inv = (flags & SMD_REGR_INVERT) ? 1 : 0, nblk = hints_blocks(P);
  hipLaunchKernelGGL(k_hints_sweep1, dim3(nblk), dim3(kHintsBlock), 0, st, depth, hints, err, S, P, mode, inv, vec, mask0, bits, ws);
  hipLaunchKernelGGL(k_hints_fin1, dim3(1), dim3(kHintsBlock), 0, st, (const double*)ws, nblk, mode, stats, loss);
  if (mode == kRegrBerhu) {
    double* ties = ws + (size_t)nblk*3;
    hipLaunchKernelGGL(k_hints_sweep2, dim3(nblk), dim3(kHintsBlock), 0, st, depth, hints, S, P, inv, vec, (const uint32_t*)bits, (const float*)stats, ws, ties);
    hipLaunchKernelGGL(k_hints_fin2, dim3(1), dim3(kHintsBlock), 0, st, (const double*)ws, (const double*)ties, nblk, stats, loss);
  }
  return hipGetLastError();
}

hipError_t launch_hints_regr_bwd(const float* depth, const float* hints, const uint32_t* bits, int S, size_t P, int flags, int vec, const float* stats,
                                 const float* g_loss, float* g_depth, hipStream_t st) {
  const int mode = regr_mode(flags), inv = (flags & SMD_REGR_INVERT) ? 1 : 0, nblk = hints_blocks(P);
  hipLaunchKernelGGL(k_hints_bwd, dim3(nblk), dim3(kHintsBlock), 0, st, depth, hints, bits, S, P, mode, inv, vec, stats, g_loss, g_depth);
  return hipGetLastError();
}

}  // namespace smd
