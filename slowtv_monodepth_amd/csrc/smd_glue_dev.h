// smd_glue_dev.h — the stages the decoder glue kernels (smd_decoder.hip) and the squeeze-excite gate (smd_attention.hip) are assembled from, each written
// once: the activations, the reflection-pad adjoint (alone and under a nearest x2 up-sampling), the chunking of a pooled plane, the matrix-vector pair of a
// two-layer gate, and the gate's backward (one kernel for both gates, defined in smd_decoder.hip).  The block reductions are the library's one family
// (smd_common.h: block_store_sum<Waves::...>); every sum has a fixed order, named where it is called.
#pragma once
#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

constexpr int kDecBlock = 256;
constexpr int kDecPerThread = 4;   // block-strided elements per thread: 4 independent load->store chains, 4x fewer blocks
constexpr int kDecChunk = kDecBlock*kDecPerThread;

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : __expf(x) - 1.f; }
__device__ __forceinline__ float elu1_grad(float x) { return x > 0.f ? 1.f : __expf(x); }
// the activation the pad kernels apply to x + bias: the Monodepth stages' ELU, the DiffNet attention stages' ReLU
enum { kActNone = 0, kActElu = 1, kActRelu = 2 };
__device__ __forceinline__ float glue_act(float x, int act) { return act == kActElu ? elu1(x) : (act == kActRelu ? fmaxf(x, 0.f) : x); }
__device__ __forceinline__ float glue_act_grad(float x, int act) { return act == kActElu ? elu1_grad(x) : (act == kActRelu ? (x > 0.f ? 1.f : 0.f) : 1.f); }
__device__ __forceinline__ int unpad_reflect(int p, int n) { const int r = p - 1; return r < 0 ? -r : (r >= n ? 2*(n - 1) - r : r); }

// ---------------------------------------------------------------------------------------------------------------- the reflection-pad adjoint
// acc += g over the padded cells that read the un-padded position (r, q) of an nr x nq plane (g: the padded plane, rows of W = nq + 2): the cell
// (r + 1, q + 1), plus along each axis the mirrored border cell when the position is the second / second-to-last one.  Rows in order, columns within a row.
template <typename T> __device__ __forceinline__ void pad_adj_add(float& acc, const T* __restrict__ g, int r, int q, int nr, int nq, int W) {
  const int ys[3] = {r + 1, r == 1 ? 0 : -1, r == nr - 2 ? nr + 1 : -1}, xs[3] = {q + 1, q == 1 ? 0 : -1, q == nq - 2 ? nq + 1 : -1};
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (ys[m] < 0) continue;
#pragma unroll
    for (int n = 0; n < 3; ++n) if (xs[n] >= 0) acc += ld_as_float<T>(g, ys[m]*W + xs[n]);
  }
}
// G(r, q): the reflection-pad adjoint at one un-padded position
template <typename T> __device__ __forceinline__ float pad_adj_at(const T* __restrict__ g, int r, int q, int nr, int nq, int W) {
  float acc = ld_as_float<T>(g, (r + 1)*W + q + 1);
  if (r == 1 || r == nr - 2 || q == 1 || q == nq - 2) { acc = 0.f; pad_adj_add(acc, g, r, q, nr, nq, W); }   // rare: mirrored border cells
  return acc;
}
// the sum of G over the 2 x 2 children of the low-resolution pixel (i, j) of an h x w plane.  On the border ONE_ACC runs one accumulator through the
// four children's cells (the Monodepth kernel's order); otherwise each child is summed by itself and the four are paired (the DiffNet kernels' order).
template <bool ONE_ACC, typename T> __device__ __forceinline__ float up_pad_adj_at(const T* __restrict__ g, int i, int j, int h, int w, int W) {
  if (i > 0 && i < h - 1 && j > 0 && j < w - 1) {   // interior: the plain 2x2 block
    const T* gp = g + (2*i + 1)*W + 2*j + 1;
    return (ld_as_float<T>(gp, 0) + ld_as_float<T>(gp, 1)) + (ld_as_float<T>(gp, W) + ld_as_float<T>(gp, W + 1));
  }
  if (ONE_ACC) {
    float acc = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
      for (int dq = 0; dq < 2; ++dq) pad_adj_add(acc, g, 2*i + dr, 2*j + dq, 2*h, 2*w, W);
    return acc;
  }
  return (pad_adj_at(g, 2*i, 2*j, 2*h, 2*w, W) + pad_adj_at(g, 2*i, 2*j + 1, 2*h, 2*w, W)) +
         (pad_adj_at(g, 2*i + 1, 2*j, 2*h, 2*w, W) + pad_adj_at(g, 2*i + 1, 2*j + 1, 2*h, 2*w, W));
}

// ---------------------------------------------------------------------------------------------------------------- the two-layer gate
// sigmoid(W2 relu(W1 mean)): a pooling sweep (several blocks per plane), one block per sample for the two matrix-vector products, an apply sweep.
constexpr int kPoolItems = 4096;           // floats of a plane one block of a pooling sweep handles
constexpr int kPoolMaxChunks = 256;
constexpr int kGateBlock = 1024;           // the per-sample block of the matrix-vector products
constexpr int kGateWaves = kGateBlock/64;

static inline int pool_chunks(int n) {
  const int c = ceil_div(n, kPoolItems);
  return c < 1 ? 1 : (c > kPoolMaxChunks ? kPoolMaxChunks : c);
}
// [lo, hi): chunk k of the `chunks` a plane of n floats is cut into, in multiples of 4 floats
__device__ __forceinline__ void pool_range(int n, int chunks, int k, int& lo, int& hi) {
  int len = ceil_div(n, chunks);
  len = (len + 3) & ~3;
  const long long l = (long long)k*len;
  lo = l < n ? (int)l : n; hi = l + len < n ? (int)(l + len) : n;
}

// where the per-block sums of a sweep live and how many each plane has: the first Ca channels' planes ((b Ca + c) cha + k), then from `na` the other Cs
// channels' ((b Cs + c) chs + k).  A gate over one tensor has Cs = 0.
struct GatePartial { unsigned na; int cha, chs; };
// the sum over plane (b, c): its per-block sums in order, fp64
template <typename T> __device__ __forceinline__ double gate_plane_sum(const T* __restrict__ partial, GatePartial pp, int b, int c, int Ca, int Cs) {
  const bool from_a = c < Ca;
  const T* p = from_a ? partial + ((size_t)b*Ca + c)*pp.cha : partial + pp.na + ((size_t)b*Cs + (c - Ca))*pp.chs;
  const int n = from_a ? pp.cha : pp.chs;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += (double)p[k];
  return s;
}

// store(r, sum_c M[r][c] v[c]) for the rows of a row-major rows x cols matrix, fp64 (v: float | double): one wave per row of a kGateBlock block
template <typename V, class F> __device__ __forceinline__ void matvec_rows(const float* __restrict__ M, const V* v, int rows, int cols, F store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < rows; r += kGateWaves) {
    double s = 0.0;
    for (int c = lane; c < cols; c += 64) s += (double)M[(size_t)r*cols + c]*(double)v[c];
    s = wave_sum_f64(s);
    if (lane == 0) store(r, s);
  }
}
// store(c, sum_r M[r][c] v[r]): the product with the transpose.  Lanes own columns (coalesced rows), the waves split the rows, `red` (waves x 64) sums them.
template <typename V, class F> __device__ __forceinline__ void matvec_cols(const float* __restrict__ M, const V* v, int rows, int cols, double* red, F store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = 0; c0 < cols; c0 += 64) {
    const int c = c0 + lane;
    double s = 0.0;
    if (c < cols) for (int r = wave; r < rows; r += kGateWaves) s += (double)M[(size_t)r*cols + c]*(double)v[r];
    __syncthreads();
    red[wave*64 + lane] = s;
    __syncthreads();
    if (wave == 0 && c < cols) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < kGateWaves; ++w) t += red[w*64 + lane];
      store(c, t);
    }
  }
}

// The backward of a gate = sigmoid(W2 relu(W1 mean [+ b1]) [+ b2]) over C = Ca + Cs channels with R hidden units (smd_decoder.hip).  partial: the per-block
// sums of dL/dgate; gate, mean, dz2, dmean are (B, C), hid and dz1 (B, R); the planes of the first Ca channels have hw elements, the others 4 hw.
struct GateBwd {
  const float *partial, *w1, *w2, *gate, *mean, *hid;
  float *dz2, *dz1, *dmean;
  GatePartial pp;
  int B, Ca, Cs, R, hw;
};
// dz2, dz1, dmean (divided by the plane's elements); with g_w1, the weights' gradients, and with g_b1, the biases' too
void launch_gate_bwd(const GateBwd& g, float* g_w1, float* g_b1, float* g_w2, float* g_b2, hipStream_t st);

}  // namespace smd
