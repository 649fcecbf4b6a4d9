// smd_attention.hip — the two attention blocks of the CADepth decoder (reference: src/networks/decoders/cadepth.py).
//
// Structure perception (cadepth.py:14-27), once per step on the deepest encoder feature x (b, C, h, w), V = x.view(b, C, n):
//   A = V V^T,  P = softmax(rowmax(A) - A) = softmax(-A),  out = x + P V.
// softmax(-A) is evaluated as exp(rowmin(A) - A) / sum: every exponent is <= 0 and the row's largest term is exactly 1, so nothing overflows
// and the sum is >= 1 whatever the scale of x.  Both products run on the matrix cores as `v_mfma_f32_16x16x4_f32` (exact f32 products and
// accumulation: the bound the operator is held to is torch's own f32 error, which split-bf16 operands would not leave room for at C = 2048).
// The C x C matrix never sits in LDS: it is spilled through a workspace (smd_channel_attention_workspace_bytes) — the row pass writes A and
// overwrites it with exp(rowmin - A), the apply pass reads it back as the left operand of the second product.  A running softmax over column
// tiles would keep it out of memory altogether, but its accumulator is 16 x n per row tile and n = h w has no bound here, so the second product
// would have to be tiled over n and the first recomputed per tile; at the sizes this runs at (C <= 2048, n = 120) the matrix is 1-16 MiB per
// sample and stays in the L2 / Infinity Cache between the two passes.  Only the row statistics (rowmin, 1 / sum) are kept for the backward,
// which recomputes P:
//   dP = g V^T,  dE = P o (dP - rowsum(dP o P)),  dA = -dE  (the row maximum is a per-row shift of a softmax: no gradient),
//   dx = g + (dA + dA^T) V + P^T g.
//
// Detail emphasis (cadepth.py:30-46), once per decoder stage: after conv + BN + ReLU the squeeze-excite gate
//   y = x + x sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2) = x (1 + a).
// Forward: per-plane partial sums (many blocks per plane) -> one block per sample finishes the means and does the two matrix-vector products
// -> one apply sweep.  Backward: partial sums of g x -> one block per sample walks back through sigma, W2, ReLU, W1 -> the parameter gradients
// (a fixed-order sum over the samples per element) and the apply sweep dx = g (1 + a) + dmean / (h w).  Every reduction has a fixed order: no
// float atomics, bit-reproducible.  The gate's stages (chunking, matrix-vector products) and its backward are shared with DiffNet's gate: smd_glue_dev.h.
#include <math.h>

#include "smd_glue_dev.h"

namespace smd {

// ---------------------------------------------------------------------------------------------------------------- structure perception
constexpr int kCaBlock = 256;              // four waves
constexpr int kCaWaves = kCaBlock/64;

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// D[i][j] = sum_k X[r0 + i][k] Y[c0 + j][k]: X, Y row-major with rows of n floats and C rows (rows past C read as zeros).
// Lane l = (i = l & 15, q = l >> 4) feeds X[r0 + i][4 s + q] and Y[c0 + i][4 s + q];  D[row 4 q + v][col i] comes back in element v.
__device__ __forceinline__ f4 tile_nt(const float* __restrict__ X, const float* __restrict__ Y, int r0, int c0, int C, int n, int lane) {
  const int i = lane & 15, q = lane >> 4;
  const bool ra = r0 + i < C, rb = c0 + i < C;
  const float* xp = X + (size_t)(ra ? r0 + i : 0)*n;
  const float* yp = Y + (size_t)(rb ? c0 + i : 0)*n;
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int k0 = 0;                                     // wave-uniform: every lane runs every MFMA
  for (; k0 + 8 <= n; k0 += 8) {                  // two independent accumulators cover the instruction's dependent latency
    const int k = k0 + q;
    const float a0 = ra ? xp[k] : 0.f, b0 = rb ? yp[k] : 0.f;
    const float a1 = ra ? xp[k + 4] : 0.f, b1 = rb ? yp[k + 4] : 0.f;
    acc0 = mfma4(a0, b0, acc0); acc1 = mfma4(a1, b1, acc1);
  }
  for (; k0 < n; k0 += 4) {                       // tail: lanes past n feed zeros
    const int kk = k0 + q;
    const float a0 = (ra && kk < n) ? xp[kk] : 0.f, b0 = (rb && kk < n) ? yp[kk] : 0.f;
    acc0 = mfma4(a0, b0, acc0);
  }
  return acc0 + acc1;
}

// fixed-order reduction of a lane's four row values over the 16 columns its lane group holds, then over the block's waves (through `red`)
template <bool MIN> __device__ __forceinline__ void rows_reduce(float (&v)[4], float* red, int lane, int wave) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) { const float o = __shfl_xor(v[r], off, 64); v[r] = MIN ? fminf(v[r], o) : v[r] + o; }
  __syncthreads();                                // `red` may still be read from the previous reduction
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave*16 + 4*(lane >> 4) + r] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = red[4*(lane >> 4) + r];
#pragma unroll
    for (int w = 1; w < kCaWaves; ++w) { const float o = red[w*16 + 4*(lane >> 4) + r]; t = MIN ? fminf(t, o) : t + o; }
    v[r] = t;
  }
}

// Row pass of the forward: a block owns 16 rows of A (grid: row tiles x samples), its waves take the column tiles in turn.
//   E[i][j] <- A[i][j], rowmin;  E[i][j] <- exp(rowmin_i - A[i][j]), sum;  stats = (rowmin, 1 / sum).
__global__ __launch_bounds__(kCaBlock) void k_ca_fwd_rows(const float* __restrict__ V, float* __restrict__ E, float* __restrict__ stats, int B, int C, int n) {
  __shared__ float red[kCaWaves*16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, r0 = blockIdx.x*16;
  const float* Vb = V + (size_t)b*C*n;
  float* Eb = E + (size_t)b*C*C;
  const int tiles = ceil_div(C, 16), col_l = lane & 15, row_l = 4*(lane >> 4);
  float mn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  for (int jt = wave; jt < tiles; jt += kCaWaves) {
    const f4 a = tile_nt(Vb, Vb, r0, jt*16, C, n, lane);
    const int col = jt*16 + col_l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + row_l + r;
      if (row < C && col < C) { Eb[(size_t)row*C + col] = a[r]; mn[r] = fminf(mn[r], a[r]); }
    }
  }
  rows_reduce<true>(mn, red, lane, wave);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int jt = wave; jt < tiles; jt += kCaWaves) {      // the same lanes read back what they wrote
    const int col = jt*16 + col_l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + row_l + r;
      if (row < C && col < C) { const float e = expf(mn[r] - Eb[(size_t)row*C + col]); Eb[(size_t)row*C + col] = e; sum[r] += e; }
    }
  }
  rows_reduce<false>(sum, red, lane, wave);
  if (wave == 0 && col_l == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + row_l + r;
      if (row < C) { stats[(size_t)b*C + row] = mn[r]; stats[((size_t)B + b)*C + row] = 1.f/sum[r]; }
    }
  }
}

// Apply pass of the forward: out[i][k] = x[i][k] + (1 / sum_i) sum_j E[i][j] V[j][k].  A wave owns a 16 x 16 tile of out (grid: row tiles x
// groups of 64 columns x samples).  Lane (i, q) feeds E[r0 + i][4 s + q] and V[4 s + q][c0 + i].
__global__ __launch_bounds__(kCaBlock) void k_ca_fwd_apply(const float* __restrict__ V, const float* __restrict__ E, const float* __restrict__ stats,
                                                          float* __restrict__ out, int B, int C, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.z, r0 = blockIdx.x*16, c0 = (blockIdx.y*kCaWaves + wave)*16;
  if (c0 >= n) return;
  const float* Vb = V + (size_t)b*C*n;
  const float* Eb = E + (size_t)b*C*C;
  const int i = lane & 15, q = lane >> 4;
  const bool ra = r0 + i < C, cb = c0 + i < n;
  const float* ep = Eb + (size_t)(ra ? r0 + i : 0)*C;
  const float* vp = Vb + (cb ? c0 + i : 0);
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int j0 = 0;
  for (; j0 + 8 <= C; j0 += 8) {
    const int j = j0 + q;
    const float a0 = ra ? ep[j] : 0.f, b0 = cb ? vp[(size_t)j*n] : 0.f;
    const float a1 = ra ? ep[j + 4] : 0.f, b1 = cb ? vp[(size_t)(j + 4)*n] : 0.f;
    acc0 = mfma4(a0, b0, acc0); acc1 = mfma4(a1, b1, acc1);
  }
  for (; j0 < C; j0 += 4) {
    const int jj = j0 + q;
    const float a0 = (ra && jj < C) ? ep[jj] : 0.f, b0 = (cb && jj < C) ? vp[(size_t)jj*n] : 0.f;
    acc0 = mfma4(a0, b0, acc0);
  }
  const f4 acc = acc0 + acc1;
  const int col = c0 + i;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4*q + r;
    if (row < C && col < n) out[((size_t)b*C + row)*n + col] = fmaf(acc[r], stats[((size_t)B + b)*C + row], Vb[(size_t)row*n + col]);
  }
}

// Row pass of the backward: recomputes P from the saved row statistics, forms dP = g V^T and the row sums of dP o P, leaves P and
// dE = P o (dP - rowsum) in the workspace.
__global__ __launch_bounds__(kCaBlock) void k_ca_bwd_rows(const float* __restrict__ V, const float* __restrict__ G, const float* __restrict__ stats,
                                                         float* __restrict__ P, float* __restrict__ DE, int B, int C, int n) {
  __shared__ float red[kCaWaves*16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, r0 = blockIdx.x*16;
  const float* Vb = V + (size_t)b*C*n;
  const float* Gb = G + (size_t)b*C*n;
  float* Pb = P + (size_t)b*C*C;
  float* Db = DE + (size_t)b*C*C;
  const int tiles = ceil_div(C, 16), col_l = lane & 15, row_l = 4*(lane >> 4);
  float mn[4], inv[4], rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + row_l + r;
    mn[r] = row < C ? stats[(size_t)b*C + row] : 0.f; inv[r] = row < C ? stats[((size_t)B + b)*C + row] : 0.f;
  }
  for (int jt = wave; jt < tiles; jt += kCaWaves) {
    const f4 a = tile_nt(Vb, Vb, r0, jt*16, C, n, lane);
    const f4 dp = tile_nt(Gb, Vb, r0, jt*16, C, n, lane);
    const int col = jt*16 + col_l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + row_l + r;
      if (row < C && col < C) {
        const float p = expf(mn[r] - a[r])*inv[r];
        Pb[(size_t)row*C + col] = p; Db[(size_t)row*C + col] = dp[r]; rs[r] = fmaf(dp[r], p, rs[r]);
      }
    }
  }
  rows_reduce<false>(rs, red, lane, wave);
  for (int jt = wave; jt < tiles; jt += kCaWaves) {
    const int col = jt*16 + col_l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + row_l + r;
      if (row < C && col < C) { const size_t o = (size_t)row*C + col; Db[o] = Pb[o]*(Db[o] - rs[r]); }
    }
  }
}

// Apply pass of the backward: dx[i][k] = g[i][k] - sum_j (dE[i][j] + dE[j][i]) V[j][k] + sum_j P[j][i] g[j][k].
__global__ __launch_bounds__(kCaBlock) void k_ca_bwd_apply(const float* __restrict__ V, const float* __restrict__ G, const float* __restrict__ P,
                                                          const float* __restrict__ DE, float* __restrict__ g_x, int C, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.z, r0 = blockIdx.x*16, c0 = (blockIdx.y*kCaWaves + wave)*16;
  if (c0 >= n) return;
  const float* Vb = V + (size_t)b*C*n;
  const float* Gb = G + (size_t)b*C*n;
  const float* Pb = P + (size_t)b*C*C;
  const float* Db = DE + (size_t)b*C*C;
  const int i = lane & 15, q = lane >> 4;
  const bool ra = r0 + i < C, cb = c0 + i < n;
  const int ri = ra ? r0 + i : 0, ci = cb ? c0 + i : 0;
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < C; j0 += 4) {
    const int j = j0 + q;
    const bool in = j < C;
    const size_t jr = in ? j : 0;
    const float s = (ra && in) ? -(Db[(size_t)ri*C + jr] + Db[jr*C + ri]) : 0.f;
    const float pt = (ra && in) ? Pb[jr*C + ri] : 0.f;
    const float v = (cb && in) ? Vb[jr*n + ci] : 0.f;
    const float g = (cb && in) ? Gb[jr*n + ci] : 0.f;
    acc0 = mfma4(s, v, acc0); acc1 = mfma4(pt, g, acc1);
  }
  const f4 acc = acc0 + acc1;
  const int col = c0 + i;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4*q + r;
    if (row < C && col < n) { const size_t o = ((size_t)b*C + row)*n + col; g_x[o] = G[o] + acc[r]; }
  }
}

hipError_t launch_channel_attention_fwd(const float* x, float* out, float* stats, float* ws, int B, int C, int n, hipStream_t st) {
  const int tiles = ceil_div(C, 16);
  hipLaunchKernelGGL(k_ca_fwd_rows, dim3(tiles, B), dim3(kCaBlock), 0, st, x, ws, stats, B, C, n);
  hipLaunchKernelGGL(k_ca_fwd_apply, dim3(tiles, ceil_div(n, 16*kCaWaves), B), dim3(kCaBlock), 0, st, x, ws, stats, out, B, C, n);
  return hipGetLastError();
}

hipError_t launch_channel_attention_bwd(const float* x, const float* stats, const float* g, float* g_x, float* ws, int B, int C, int n, hipStream_t st) {
  const int tiles = ceil_div(C, 16);
  float* P = ws;
  float* DE = ws + (size_t)B*C*C;
  hipLaunchKernelGGL(k_ca_bwd_rows, dim3(tiles, B), dim3(kCaBlock), 0, st, x, g, stats, P, DE, B, C, n);
  hipLaunchKernelGGL(k_ca_bwd_apply, dim3(tiles, ceil_div(n, 16*kCaWaves), B), dim3(kCaBlock), 0, st, x, g, P, DE, g_x, C, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- squeeze-excite gate
constexpr int kSeBlock = 256;

int se_chunks(int HW) { return pool_chunks(HW); }   // (the name the workspace sizes of the C ABI know it by)

// partial[plane][k] = sum over chunk k of x (BWD: of g x).  grid.x = planes x chunks.
template <bool BWD, bool VEC>
__global__ __launch_bounds__(kSeBlock) void k_se_pool(const float* __restrict__ x, const float* __restrict__ g, int HW, int chunks, float* __restrict__ partial) {
  __shared__ float red[kSeBlock/64];
  const unsigned plane = blockIdx.x/chunks, k = blockIdx.x - plane*chunks;
  const float* xp = x + (size_t)plane*HW;
  const float* gp = BWD ? g + (size_t)plane*HW : nullptr;
  int lo, hi;
  pool_range(HW, chunks, k, lo, hi);
  float s = 0.f;
  if (VEC) {
    for (int i = lo + (int)threadIdx.x*4; i < hi; i += kSeBlock*4) {
      const f4 v = *(const f4*)(xp + i);
      if (BWD) { const f4 w = *(const f4*)(gp + i); s += (v[0]*w[0] + v[1]*w[1]) + (v[2]*w[2] + v[3]*w[3]); }
      else s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int i = lo + (int)threadIdx.x; i < hi; i += kSeBlock) s += BWD ? xp[i]*gp[i] : xp[i];
  }
  block_store_sum<Waves::Pairwise, kSeBlock/64>(s, red, partial + blockIdx.x);
}

__device__ __forceinline__ float sigmoidf(double z) { return (float)(1.0/(1.0 + exp(-z))); }

// One block per sample: means from the partial sums, hidden = relu(W1 mean + b1), a = sigmoid(W2 hidden + b2).  save = (a, mean, hidden), each (B, C).
__global__ __launch_bounds__(kGateBlock) void k_se_gate_fwd(const float* __restrict__ partial, const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2, float* save, int B, int C, int HW,
                                                             int chunks) {
  const int b = blockIdx.x;
  float* a = save + (size_t)b*C;
  float* mean = save + ((size_t)B + b)*C;
  float* hidden = save + ((size_t)2*B + b)*C;
  for (int c = threadIdx.x; c < C; c += kGateBlock) mean[c] = (float)(gate_plane_sum(partial, GatePartial{0, chunks, 0}, b, c, C, 0)/(double)HW);
  __threadfence_block(); __syncthreads();
  matvec_rows(w1, mean, C, C, [&](int r, double s) { hidden[r] = fmaxf((float)(s + (double)b1[r]), 0.f); });
  __threadfence_block(); __syncthreads();
  matvec_rows(w2, hidden, C, C, [&](int r, double s) { a[r] = sigmoidf(s + (double)b2[r]); });
}

// y = x (1 + a[plane])  (BWD: g_x = g (1 + a[plane]) + dmean[plane]).  grid.x = planes x chunks, the chunks of k_se_pool.
template <bool BWD, bool VEC>
__global__ __launch_bounds__(kSeBlock) void k_se_apply(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ dmean, int HW,
                                                      int chunks, float* __restrict__ y) {
  const unsigned plane = blockIdx.x/chunks, k = blockIdx.x - plane*chunks;
  const float* xp = x + (size_t)plane*HW;
  float* yp = y + (size_t)plane*HW;
  const float sc = 1.f + a[plane], sh = BWD ? dmean[plane] : 0.f;
  int lo, hi;
  pool_range(HW, chunks, k, lo, hi);
  if (VEC) {
    for (int i = lo + (int)threadIdx.x*4; i < hi; i += kSeBlock*4) {
      const f4 v = *(const f4*)(xp + i);
      f4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = fmaf(v[q], sc, sh);
      *(f4*)(yp + i) = o;
    }
  } else {
    for (int i = lo + (int)threadIdx.x; i < hi; i += kSeBlock) yp[i] = fmaf(xp[i], sc, sh);
  }
}

hipError_t launch_se_gate_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* save, float* ws,
                              int B, int C, int HW, hipStream_t st) {
  const int chunks = se_chunks(HW);
  const unsigned blocks = (unsigned)((size_t)B*C*chunks);
  const bool vec = (HW % 4) == 0;
  if (vec) hipLaunchKernelGGL((k_se_pool<false, true>), dim3(blocks), dim3(kSeBlock), 0, st, x, (const float*)nullptr, HW, chunks, ws);
  else hipLaunchKernelGGL((k_se_pool<false, false>), dim3(blocks), dim3(kSeBlock), 0, st, x, (const float*)nullptr, HW, chunks, ws);
  hipLaunchKernelGGL(k_se_gate_fwd, dim3(B), dim3(kGateBlock), 0, st, ws, w1, b1, w2, b2, save, B, C, HW, chunks);
  if (vec) hipLaunchKernelGGL((k_se_apply<false, true>), dim3(blocks), dim3(kSeBlock), 0, st, x, save, (const float*)nullptr, HW, chunks, y);
  else hipLaunchKernelGGL((k_se_apply<false, false>), dim3(blocks), dim3(kSeBlock), 0, st, x, save, (const float*)nullptr, HW, chunks, y);
  return hipGetLastError();
}

hipError_t launch_se_gate_bwd(const float* x, const float* g_y, const float* w1, const float* w2, const float* save, float* g_x, float* g_w1, float* g_b1,
                              float* g_w2, float* g_b2, float* ws, int B, int C, int HW, hipStream_t st) {
  const int chunks = se_chunks(HW);
  const unsigned blocks = (unsigned)((size_t)B*C*chunks);
  const bool vec = (HW % 4) == 0;
  float* partial = ws;
  float* vecs = ws + (((size_t)B*C*chunks + 3) & ~(size_t)3);     // (dz2, dz1, dmean), each (B, C)
  float* dmean = vecs + (size_t)2*B*C;
  const float* mean = save + (size_t)B*C;                         // save = (a, mean, hidden)
  const float* hidden = save + (size_t)2*B*C;
  if (vec) hipLaunchKernelGGL((k_se_pool<true, true>), dim3(blocks), dim3(kSeBlock), 0, st, x, g_y, HW, chunks, partial);
  else hipLaunchKernelGGL((k_se_pool<true, false>), dim3(blocks), dim3(kSeBlock), 0, st, x, g_y, HW, chunks, partial);
  launch_gate_bwd(GateBwd{partial, w1, w2, save, mean, hidden, vecs, vecs + (size_t)B*C, dmean, GatePartial{0, chunks, 0}, B, C, 0, C, HW}, g_w1, g_b1, g_w2, g_b2, st);
  if (g_x) {
    if (vec) hipLaunchKernelGGL((k_se_apply<true, true>), dim3(blocks), dim3(kSeBlock), 0, st, g_y, save, dmean, HW, chunks, g_x);
    else hipLaunchKernelGGL((k_se_apply<true, false>), dim3(blocks), dim3(kSeBlock), 0, st, g_y, save, dmean, HW, chunks, g_x);
  }
  return hipGetLastError();
}

}  // namespace smd
