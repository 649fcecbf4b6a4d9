// smd_norm_dev.h — the walk over one channel of an NCHW tensor that the BatchNorm sweeps (smd_norm.hip) and LayerNorm's gamma / beta reduction
// (smd_layernorm.hip) share, written once: the chunk a block owns, the offset of a flat index, the block-strided loop, and 1- or 4-float steps.
#pragma once
#include "smd_common.h"

namespace smd {

constexpr int kBnBlock = 256;            // threads of every block that sweeps a channel

// A step of a sweep: W = 1 or 4 consecutive floats, loaded and stored as one access; code indexes the lanes e = 0..W-1 in order.
template <int W> using fvec = float __attribute__((ext_vector_type(W)));
template <int W> __device__ __forceinline__ fvec<W> ldv(const float* p) { return *(const fvec<W>*)p; }
template <int W> __device__ __forceinline__ void stv(float* p, fvec<W> v) { *(fvec<W>*)p = v; }

// Range of the flattened (n, p) index space of one channel swept by chunk k (a multiple of 4, so that a 4-float step never straddles two chunks).
__device__ __forceinline__ void chunk_range(long long total, int chunks, int k, long long& lo, long long& hi) {
  long long len = (total + chunks - 1)/chunks;
  len = (len + 3) & ~3ll;
  lo = (long long)k*len; hi = lo + len < total ? lo + len : total;
}

// Element offset of flat index i = n*HW + p of channel c.
__device__ __forceinline__ size_t channel_offset(long long i, int C, int HW, int c) {
  const int n = (int)(i/HW), p = (int)(i - (long long)n*HW);
  return ((size_t)n*C + c)*HW + p;
}

// body(off, i) for the steps of [lo, hi) a thread owns: thread t takes i = lo + t*W, then block-strided by kBnBlock*W (VEC: W = 4, HW % 4 == 0 and lo % 4 == 0,
// so a step stays inside one sample and is 16-byte aligned).
template <bool VEC, class F> __device__ __forceinline__ void channel_sweep(long long lo, long long hi, int C, int HW, int c, F body) {
  constexpr int W = VEC ? 4 : 1;
  for (long long i = lo + (long long)threadIdx.x*W; i < hi; i += kBnBlock*W) body(channel_offset(i, C, HW, c), i);
}

}  // namespace smd
