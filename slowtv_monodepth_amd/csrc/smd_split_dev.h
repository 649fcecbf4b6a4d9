// smd_split_dev.h — the exact three-way bf16 split of fp32 operands and the products kept of it, shared by the split-bf16 matrix-core kernels
// (smd_conv_mfma.hip, where the scheme is described, smd_conv_wgrad.hip, smd_conv_stem.hip and smd_ddv.hip).  The stages those kernels share — block order,
// the LDS patch and its stager, the product sequence, the weight gradients' pieces — are smd_conv_mfma_dev.h; this header stays the arithmetic.
#pragma once
#include "smd_common.h"

namespace smd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// the products kept of (a0 + a1 + a2)(b0 + b1 + b2), smallest terms first
__host__ __device__ constexpr int n_products(int P) { return P == 3 ? 6 : P == 2 ? 3 : 1; }
__host__ __device__ constexpr int prod_a(int P, int t) { return P == 3 ? (t == 0 ? 2 : t == 1 ? 1 : t == 2 ? 0 : t == 3 ? 1 : 0) : P == 2 ? (t == 0 ? 1 : 0) : 0; }
__host__ __device__ constexpr int prod_b(int P, int t) { return P == 3 ? (t == 0 ? 0 : t == 1 ? 1 : t == 2 ? 2 : t == 3 ? 0 : t == 4 ? 1 : 0) : P == 2 ? (t == 1 ? 1 : 0) : 0; }

__device__ __forceinline__ unsigned pack_bf16_rne(float a, float b) { const f32x2v v = {a, b}; return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2v)); }   // v_cvt_pk_bf16_f32
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
// two fp32 values -> P dwords of two bf16 each (low half = a's piece, high half = b's)
template <int P> __device__ __forceinline__ void split_pair(float a, float b, unsigned (&p)[P]) {
  p[0] = pack_bf16_rne(a, b);
  if constexpr (P > 1) { a -= bf16_lo(p[0]); b -= bf16_hi(p[0]); p[1] = pack_bf16_rne(a, b); }
  if constexpr (P > 2) { a -= bf16_lo(p[1]); b -= bf16_hi(p[1]); p[2] = pack_bf16_rne(a, b); }
}
__device__ __forceinline__ bf16x8 as_frag(const uint4& u) { return __builtin_bit_cast(bf16x8, u); }

}  // namespace smd
