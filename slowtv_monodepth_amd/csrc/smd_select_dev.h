// smd_select_dev.h — one digit of the exact radix select over float bit patterns, shared by smd_eval.hip (np.median's two middle values) and smd_viz.hip
// (np.percentile's two order statistics).  Positive floats order like their bit patterns, and only integer counts are involved: the selection is exact.
#pragma once
#include "smd_common.h"

namespace smd {

constexpr int kSelBlock = 256;                     // one bin per thread
constexpr int kSelWaves = kSelBlock/kWave;

// `to_inv` (src/tools/geometry.py:86-90) on one value: (d > 0)/clamp(d, eps).  A NaN gives 0/NaN = NaN there; here it gives 0 (the evaluator masks it out by
// `pred > 0` either way; smd_viz.hip, where a NaN has a colour of its own, tests for it first).
__device__ __forceinline__ float to_inv1(float d) { return d > 0.f ? 1.f/fmaxf(d, kEps32) : 0.f; }

// Block-wide (kSelBlock threads): the bin of hist[0, 256) that holds the element of rank k (0-based, ascending) and k's rank inside that bin; -> the
// histogram's total.  With k >= total nothing is selected (bin = rank = 0).  sh: kSelWaves + 2 words of LDS.
__device__ __forceinline__ unsigned select_bin256(const unsigned* __restrict__ hist, unsigned k, unsigned* sh, unsigned& bin, unsigned& rank) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid/kWave;
  const unsigned mine = hist[tid];
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) { const unsigned v = __shfl_up(incl, off, kWave); if (lane >= off) incl += v; }
  if (lane == kWave - 1) sh[wv] = incl;
  if (tid == 0) { sh[kSelWaves] = 0; sh[kSelWaves + 1] = 0; }
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kSelWaves; ++q) { if (q < wv) before += sh[q]; total += sh[q]; }
  const unsigned excl = before + incl - mine;
  if (k >= excl && k < excl + mine) { sh[kSelWaves] = (unsigned)tid; sh[kSelWaves + 1] = k - excl; }   // exactly one thread when k < total
  __syncthreads();
  bin = sh[kSelWaves]; rank = sh[kSelWaves + 1];
  __syncthreads();                               // sh is reused by the next call
  return total;
}

}  // namespace smd
