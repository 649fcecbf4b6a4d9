// smd_norm.hip — training-mode BatchNorm2d fused with the residual add and ReLU that follow it in the ResNet encoders
// (timm `resnet18/34/50`, built at src/networks/depth.py:95-98 and src/networks/pose.py:39-41: conv -> BN -> ReLU and
// conv -> BN -> (+identity) -> ReLU).  The producer side of the loss path: after the loss kernels, BatchNorm and the
// element-wise ops around it were the largest non-convolution item of the step (MIOpen's spatial BN kernels launch one
// workgroup per channel: 64 workgroups on a 256-CU device for the stem).
//
//   forward : stats sweep (per chunk: mean, then squared deviations from it; many blocks per channel) -> apply sweep (each block combines the chunks in fp64, Chan's formula)
//   backward: reduce sweep (sum dz, sum dz*(x-mean))               -> apply sweep (same; block 0 of a channel writes g_gamma, g_beta)
//   layers with N*HW <= 16384 (layer3/4 of the encoders): ONE launch per direction, one block per channel
// where dz = g_y masked by (y > 0) when the ReLU is fused.  NCHW fp32; 4-float steps when HW % 4 == 0.
// Every sweep is `channel_sweep` (smd_norm_dev.h: chunk range, offset of a flat index, block-strided steps of 1 or 4 floats) around a body written once for
// both step widths; every block sum is `block_sum2<Waves::Sequential>` (smd_common.h).
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_norm_dev.h"

namespace smd {

constexpr int kBnItemsPerBlock = 8192;   // floats a block sweeps in the reduction kernels
constexpr int kBnMaxChunks = 128;
constexpr int kBnWaves = kBnBlock/64;

int bn_chunks(int N, int HW) {
  const long long total = (long long)N*HW;
  long long c = (total + kBnItemsPerBlock - 1)/kBnItemsPerBlock;
  return (int)(c < 1 ? 1 : (c > kBnMaxChunks ? kBnMaxChunks : c));
}

// Statistics of a range in two passes, so that they depend on no single element: pass 1 sums the values (their mean `m` only has to be NEAR the mean: it is the
// shift of pass 2), pass 2 sums r = sum(x - m) and q = sum((x - m)^2).  Then mean = m + r/n exactly and M2 = q - r*r/n, where r is a rounding-sized correction.
// A thread keeps its first kBnKeep values in registers between the passes (a chunk of the stats sweep has no more: one read from memory); whatever a
// longer range holds is read again (the upper half of the single-launch path, from L2, and chunks of more than kBnItemsPerBlock floats).
// (The kept part stays a fully unrolled loop of its own, so that `v` lives in registers; it decodes its indices through the sweep's channel_offset.)
constexpr int kBnKeep = kBnItemsPerBlock/kBnBlock;   // 32

template <bool VEC>
__device__ __forceinline__ void range_stats(const float* __restrict__ x, int C, int HW, int c, long long lo, long long hi, float* red, float& m, float& r, float& q) {
  constexpr int W = VEC ? 4 : 1, STEPS = kBnKeep/W;
  const long long stride = (long long)kBnBlock*W, first = lo + (long long)threadIdx.x*W, rest = lo + STEPS*stride;
  float v[kBnKeep];
  float s = 0.f, unused = 0.f;
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    const long long i = first + j*stride;
    fvec<W> t = 0.f;
    if (i < hi) {
      t = ldv<W>(x + channel_offset(i, C, HW, c));
#pragma unroll
      for (int e = 0; e < W; ++e) s += t[e];
    }
#pragma unroll
    for (int e = 0; e < W; ++e) v[j*W + e] = t[e];
  }
  channel_sweep<VEC>(rest, hi, C, HW, c, [&](size_t off, long long) {
    const fvec<W> t = ldv<W>(x + off);
#pragma unroll
    for (int e = 0; e < W; ++e) s += t[e];
  });
  block_sum2<Waves::Sequential, kBnWaves>(s, unused, red);
  m = s/(float)(hi - lo);
  __syncthreads();   // `red` is written again below
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    if (first + j*stride < hi) {
#pragma unroll
      for (int e = 0; e < W; ++e) { const float d = v[j*W + e] - m; a += d; b = fmaf(d, d, b); }
    }
  }
  channel_sweep<VEC>(rest, hi, C, HW, c, [&](size_t off, long long) {
    const fvec<W> t = ldv<W>(x + off);
#pragma unroll
    for (int e = 0; e < W; ++e) { const float d = t[e] - m; a += d; b = fmaf(d, d, b); }
  });
  block_sum2<Waves::Sequential, kBnWaves>(a, b, red);
  r = a; q = b;
}

// Stats sweep of the chunked path: per chunk (m, r/n, M2) with the chunk's mean = m + r/n.
template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_stats(const float* __restrict__ x, int N, int C, int HW, int chunks, float* __restrict__ partial) {
  __shared__ float red[2*kBnWaves];
  const int c = blockIdx.y, k = blockIdx.x;
  long long lo, hi;
  chunk_range((long long)N*HW, chunks, k, lo, hi);
  float m = 0.f, r = 0.f, q = 0.f;
  if (lo < hi) range_stats<VEC>(x, C, HW, c, lo, hi, red, m, r, q);   // (block-uniform)
  if (threadIdx.x == 0) {
    const float rn = lo < hi ? r/(float)(hi - lo) : 0.f;
    float* out = partial + ((size_t)c*chunks + k)*3;
    out[0] = m; out[1] = rn; out[2] = fmaxf(fmaf(-r, rn, q), 0.f);
  }
}

// The two fp64 combines of a channel's chunks by the whole block (every block of the apply sweeps does this for itself: <= 128 chunks, so the separate
// one-thread-per-channel finalize launch is gone and nothing needs an atomic): what a thread adds up, then one block sum.
// Backward: the plain sums of the reduce sweep's pairs.
__device__ __forceinline__ void combine_partials(const float* __restrict__ partial, int c, int chunks, double* red, double& s1, double& s2) {
  s1 = 0.0; s2 = 0.0;
  for (int k = threadIdx.x; k < chunks; k += kBnBlock) { s1 += (double)partial[((size_t)c*chunks + k)*2]; s2 += (double)partial[((size_t)c*chunks + k)*2 + 1]; }
  block_sum2<Waves::Sequential, kBnWaves>(s1, s2, red);
}
// Forward: Chan's combination of the stats sweep's chunks about the mean of chunk 0 (`shift`): s1 = sum n_k (mean_k - shift), s2 = sum M2_k + n_k (mean_k - shift)^2,
// i.e. the shifted sums of the whole channel that `finish_stats` takes.
__device__ __forceinline__ void combine_chunk_stats(const float* __restrict__ partial, int c, int chunks, long long total, double* red, double& shift, double& s1, double& s2) {
  const float* pc = partial + (size_t)c*chunks*3;
  shift = (double)pc[0] + (double)pc[1];
  s1 = 0.0; s2 = 0.0;
  for (int k = threadIdx.x; k < chunks; k += kBnBlock) {
    long long lo, hi;
    chunk_range(total, chunks, k, lo, hi);
    const double n = hi > lo ? (double)(hi - lo) : 0.0, d = ((double)pc[k*3] + (double)pc[k*3 + 1]) - shift;
    s1 += n*d; s2 += (double)pc[k*3 + 2] + n*d*d;
  }
  block_sum2<Waves::Sequential, kBnWaves>(s1, s2, red);
}

struct BnStat { float mean, invstd; };
__device__ __forceinline__ BnStat finish_stats(double s1, double s2, double shift, int N, int HW, float momentum, float eps, int c, bool writer,
                                               float* running_mean, float* running_var, float* save_mean, float* save_invstd) {
  const double M = (double)N*HW, m1 = s1/M, mean = shift + m1;
  double var = s2/M - m1*m1;
  if (var < 0.0) var = 0.0;
  const double invstd = 1.0/sqrt(var + (double)eps);
  if (writer) {
    save_mean[c] = (float)mean; save_invstd[c] = (float)invstd;
    if (running_mean) running_mean[c] = (float)((1.0 - momentum)*(double)running_mean[c] + momentum*mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum)*(double)running_var[c] + momentum*var*(M > 1.0 ? M/(M - 1.0) : 1.0));
  }
  return {(float)mean, (float)invstd};
}

// y = (x - mean)*sc + beta [+ residual] [ReLU].  The mean comes off x BEFORE the scale: folded into the offset (x*sc + (beta - mean*sc)) the two large terms
// cancel after the offset was rounded, which costs |mean|/sigma ulps of y.
template <bool VEC>
__device__ __forceinline__ void apply_range(const float* __restrict__ x, const float* __restrict__ residual, float* __restrict__ y, int C, int HW, int c,
                                            long long lo, long long hi, float mean, float sc, float beta, int relu) {
  constexpr int W = VEC ? 4 : 1;
  channel_sweep<VEC>(lo, hi, C, HW, c, [&](size_t off, long long) {
    fvec<W> o = ldv<W>(x + off);
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = fmaf(o[e] - mean, sc, beta);
    if (residual) o += ldv<W>(residual + off);
    if (relu) {
#pragma unroll
      for (int e = 0; e < W; ++e) o[e] = fmaxf(o[e], 0.f);
    }
    stv<W>(y + off, o);
  });
}

// Apply sweep of the chunked path: grid (chunks, C), the same ranges as the stats sweep.
template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_apply(const float* __restrict__ x, const float* __restrict__ residual, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ partial, int N, int C, int HW, int chunks,
                                                       float momentum, float eps, int relu, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                       float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ y) {
  __shared__ double red[2*kBnWaves];
  const int c = blockIdx.y, k = blockIdx.x;
  double shift, s1, s2;
  combine_chunk_stats(partial, c, chunks, (long long)N*HW, red, shift, s1, s2);
  const BnStat st = finish_stats(s1, s2, shift, N, HW, momentum, eps, c, k == 0 && threadIdx.x == 0, running_mean, running_var, save_mean, save_invstd);
  long long lo, hi;
  chunk_range((long long)N*HW, chunks, k, lo, hi);
  apply_range<VEC>(x, residual, y, C, HW, c, lo, hi, st.mean, gamma[c]*st.invstd, beta[c], relu);
}

// Single-launch path for small channels (N*HW <= kBnSmall): one block per channel does stats, finalize and apply (later reads from L2).
template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_fwd_small(const float* __restrict__ x, const float* __restrict__ residual, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int N, int C, int HW, float momentum, float eps, int relu,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ y) {
  __shared__ float red[2*kBnWaves];
  const int c = blockIdx.x;
  const long long total = (long long)N*HW;
  float m, r, q;
  range_stats<VEC>(x, C, HW, c, 0, total, red, m, r, q);   // (layer3/4 of the encoders hold <= kBnItemsPerBlock values per channel: nothing is read twice for the statistics)
  const BnStat st = finish_stats((double)r, (double)q, (double)m, N, HW, momentum, eps, c, threadIdx.x == 0, running_mean, running_var, save_mean, save_invstd);
  apply_range<VEC>(x, residual, y, C, HW, c, 0, total, st.mean, gamma[c]*st.invstd, beta[c], relu);
}

// dz of a step: g_y where the fused ReLU let y through
template <int W>
__device__ __forceinline__ fvec<W> bwd_dz(const float* __restrict__ y, const float* __restrict__ g_y, size_t off, int relu) {
  const fvec<W> gv = ldv<W>(g_y + off);
  fvec<W> yv = 1.f, dz;
  if (relu) yv = ldv<W>(y + off);
#pragma unroll
  for (int e = 0; e < W; ++e) dz[e] = (yv[e] > 0.f) ? gv[e] : 0.f;
  return dz;
}

template <bool VEC>
__device__ __forceinline__ void bwd_reduce_range(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_y, int C, int HW, int c,
                                                 long long lo, long long hi, float mu, int relu, float& s1, float& s2) {
  constexpr int W = VEC ? 4 : 1;
  channel_sweep<VEC>(lo, hi, C, HW, c, [&](size_t off, long long) {
    const fvec<W> xv = ldv<W>(x + off), dz = bwd_dz<W>(y, g_y, off, relu);
#pragma unroll
    for (int e = 0; e < W; ++e) { s1 += dz[e]; s2 = fmaf(dz[e], xv[e] - mu, s2); }
  });
}

// What both backward paths derive from the channel's sums s1 = sum dz, s2 = sum dz*(x - mean) (fp64: the chunked path's combine; the single launch's fp32 block
// sums widen exactly): g_beta, g_gamma (by `writer`) and the coefficients of g_x = a*(dz - b - (x - mean)*k2).
struct BnBwdCoef { float a, b, k2; };
__device__ __forceinline__ BnBwdCoef bwd_coeffs(double s1, double s2, float gamma, float invstd, double M, int c, bool writer, float* g_gamma, float* g_beta) {
  const double is = (double)invstd;
  if (writer) { g_beta[c] = (float)s1; g_gamma[c] = (float)(s2*is); }
  return {(float)((double)gamma*is), (float)(s1/M), (float)(s2*is*is/M)};
}

template <bool VEC>
__device__ __forceinline__ void bwd_apply_range(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_y, float* __restrict__ g_x,
                                                float* __restrict__ g_res, int C, int HW, int c, long long lo, long long hi, float mu, BnBwdCoef k, int relu) {
  constexpr int W = VEC ? 4 : 1;
  channel_sweep<VEC>(lo, hi, C, HW, c, [&](size_t off, long long) {
    const fvec<W> xv = ldv<W>(x + off), dz = bwd_dz<W>(y, g_y, off, relu);
    fvec<W> dx;
#pragma unroll
    for (int e = 0; e < W; ++e) dx[e] = k.a*(dz[e] - k.b - (xv[e] - mu)*k.k2);
    stv<W>(g_x + off, dx);
    if (g_res) stv<W>(g_res + off, dz);
  });
}

template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_bwd_reduce(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_y,
                                                            const float* __restrict__ mean, int N, int C, int HW, int chunks, int relu,
                                                            float* __restrict__ partial) {
  __shared__ float red[2*kBnWaves];
  const int c = blockIdx.y, k = blockIdx.x;
  long long lo, hi;
  chunk_range((long long)N*HW, chunks, k, lo, hi);
  float s1 = 0.f, s2 = 0.f;
  bwd_reduce_range<VEC>(x, y, g_y, C, HW, c, lo, hi, mean[c], relu, s1, s2);
  block_sum2<Waves::Sequential, kBnWaves>(s1, s2, red);
  if (threadIdx.x == 0) { partial[((size_t)c*chunks + k)*2] = s1; partial[((size_t)c*chunks + k)*2 + 1] = s2; }
}

template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_bwd_apply(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_y,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ partial, int N, int C, int HW, int chunks, int relu,
                                                           float* __restrict__ g_x, float* __restrict__ g_res, float* __restrict__ g_gamma,
                                                           float* __restrict__ g_beta) {
  __shared__ double red[2*kBnWaves];
  const int c = blockIdx.y, k = blockIdx.x;
  double s1, s2;
  combine_partials(partial, c, chunks, red, s1, s2);
  const BnBwdCoef co = bwd_coeffs(s1, s2, gamma[c], invstd[c], (double)N*HW, c, k == 0 && threadIdx.x == 0, g_gamma, g_beta);
  long long lo, hi;
  chunk_range((long long)N*HW, chunks, k, lo, hi);
  bwd_apply_range<VEC>(x, y, g_y, g_x, g_res, C, HW, c, lo, hi, mean[c], co, relu);
}

template <bool VEC>
__global__ __launch_bounds__(kBnBlock) void k_bn_bwd_small(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_y,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           int N, int C, int HW, int relu, float* __restrict__ g_x, float* __restrict__ g_res,
                                                           float* __restrict__ g_gamma, float* __restrict__ g_beta) {
  __shared__ float red[2*kBnWaves];
  const int c = blockIdx.x;
  const long long total = (long long)N*HW;
  float s1 = 0.f, s2 = 0.f;
  bwd_reduce_range<VEC>(x, y, g_y, C, HW, c, 0, total, mean[c], relu, s1, s2);
  block_sum2<Waves::Sequential, kBnWaves>(s1, s2, red);
  const BnBwdCoef co = bwd_coeffs((double)s1, (double)s2, gamma[c], invstd[c], (double)total, c, threadIdx.x == 0, g_gamma, g_beta);
  bwd_apply_range<VEC>(x, y, g_y, g_x, g_res, C, HW, c, 0, total, mean[c], co, relu);
}

constexpr long long kBnSmall = 16384;   // N*HW up to which one block per channel does the whole layer in one launch

hipError_t launch_bn_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, float* ws, int N, int C, int HW,
                         hipStream_t st) {
  const int chunks = bn_chunks(N, HW);
  for_bool((HW % 4) == 0, [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if ((long long)N*HW <= kBnSmall) {
      hipLaunchKernelGGL(k_bn_fwd_small<VEC>, dim3(C), dim3(kBnBlock), 0, st, x, residual, gamma, beta, N, C, HW, momentum, eps, relu, running_mean, running_var,
                         save_mean, save_invstd, y);
      return;
    }
    hipLaunchKernelGGL(k_bn_stats<VEC>, dim3(chunks, C), dim3(kBnBlock), 0, st, x, N, C, HW, chunks, ws);
    hipLaunchKernelGGL(k_bn_apply<VEC>, dim3(chunks, C), dim3(kBnBlock), 0, st, x, residual, gamma, beta, ws, N, C, HW, chunks, momentum, eps, relu,
                       running_mean, running_var, save_mean, save_invstd, y);
  });
  return hipGetLastError();
}

hipError_t launch_bn_bwd(const float* x, const float* y, const float* g_y, const float* gamma, const float* save_mean, const float* save_invstd,
                         int relu, float* g_x, float* g_res, float* g_gamma, float* g_beta, float* ws, int N, int C, int HW, hipStream_t st) {
  const int chunks = bn_chunks(N, HW);
  for_bool((HW % 4) == 0, [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if ((long long)N*HW <= kBnSmall) {
      hipLaunchKernelGGL(k_bn_bwd_small<VEC>, dim3(C), dim3(kBnBlock), 0, st, x, y, g_y, gamma, save_mean, save_invstd, N, C, HW, relu, g_x, g_res, g_gamma, g_beta);
      return;
    }
    hipLaunchKernelGGL(k_bn_bwd_reduce<VEC>, dim3(chunks, C), dim3(kBnBlock), 0, st, x, y, g_y, save_mean, N, C, HW, chunks, relu, ws);
    hipLaunchKernelGGL(k_bn_bwd_apply<VEC>, dim3(chunks, C), dim3(kBnBlock), 0, st, x, y, g_y, gamma, save_mean, save_invstd, ws, N, C, HW, chunks, relu,
                       g_x, g_res, g_gamma, g_beta);
  });
  return hipGetLastError();
}

}  // namespace smd

// ---------------------------------------------------------------------------------------------
// MaxPool2d(kernel 3, stride 2, padding 1) of the ResNet stem.  Forward keeps the winning window position (0..8, first
// maximum in row-major scan order, as ATen's max_pool2d_with_indices) in one byte instead of an int64 flat index; the
// backward is a gather over the <= 4 windows that cover an input pixel, so g_input is written exactly once and never
// zero-filled or scattered into.
// ---------------------------------------------------------------------------------------------
namespace smd {

__global__ __launch_bounds__(256) void k_maxpool_fwd(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ idx, int H, int W, int Ho, int Wo,
                                                     unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;
  const float* xp = x + (size_t)plane*H*W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int o = chunk*1024 + k*256 + threadIdx.x;
    if (o >= Ho*Wo) break;
    const int oh = o/Wo, ow = o - oh*Wo;
    float best = -INFINITY; int bi = -1;   // no tap yet: a window of nothing but -inf selects its first VALID tap (as ATen), never one in the padding
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) {
      const int h = 2*oh - 1 + dh;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        const int w = 2*ow - 1 + dw;
        if (w < 0 || w >= W) continue;
        const float v = xp[h*W + w];
        if (v > best || v != v || bi < 0) { best = v; bi = dh*3 + dw; }
      }
    }
    y[(size_t)plane*Ho*Wo + o] = best; idx[(size_t)plane*Ho*Wo + o] = (uint8_t)bi;
  }
}

// One thread per 2x2 input block (rows 2k, 2k+1; columns 2j, 2j+1): the four windows A=(k,j), B=(k,j+1), C=(k+1,j),
// D=(k+1,j+1) are the only ones that can have selected any of its pixels, each at a fixed window position:
//   (2k,  2j)   <- A@4            (2k,  2j+1) <- A@5, B@3
//   (2k+1,2j)   <- A@7, C@1       (2k+1,2j+1) <- A@8, B@6, C@2, D@0
__global__ __launch_bounds__(256) void k_maxpool_bwd(const float* __restrict__ g_y, const uint8_t* __restrict__ idx, float* __restrict__ g_x, int H, int W,
                                                     int Ho, int Wo, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;
  const float* gp = g_y + (size_t)plane*Ho*Wo; const uint8_t* ip = idx + (size_t)plane*Ho*Wo;
  float* out = g_x + (size_t)plane*H*W;
  const int Hb = (H + 1)/2, Wb = (W + 1)/2;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int q = chunk*1024 + t*256 + threadIdx.x;
    if (q >= Hb*Wb) break;
    const int k = q/Wb, j = q - k*Wb;
    const bool hasB = j + 1 < Wo, hasC = k + 1 < Ho;
    const int ia = k*Wo + j;
    const int sa = ip[ia], sb = hasB ? ip[ia + 1] : 255, sc = hasC ? ip[ia + Wo] : 255, sd = (hasB && hasC) ? ip[ia + Wo + 1] : 255;
    const float ga = gp[ia], gb = hasB ? gp[ia + 1] : 0.f, gc = hasC ? gp[ia + Wo] : 0.f, gd = (hasB && hasC) ? gp[ia + Wo + 1] : 0.f;
    const float o00 = (sa == 4) ? ga : 0.f;
    const float o01 = ((sa == 5) ? ga : 0.f) + ((sb == 3) ? gb : 0.f);
    const float o10 = ((sa == 7) ? ga : 0.f) + ((sc == 1) ? gc : 0.f);
    const float o11 = (((sa == 8) ? ga : 0.f) + ((sb == 6) ? gb : 0.f)) + (((sc == 2) ? gc : 0.f) + ((sd == 0) ? gd : 0.f));
    const int h0 = 2*k, w0 = 2*j;
    out[h0*W + w0] = o00;
    if (w0 + 1 < W) out[h0*W + w0 + 1] = o01;
    if (h0 + 1 < H) { out[(h0 + 1)*W + w0] = o10; if (w0 + 1 < W) out[(h0 + 1)*W + w0 + 1] = o11; }
  }
}

hipError_t launch_maxpool_fwd(const float* x, float* y, uint8_t* idx, size_t planes, int H, int W, hipStream_t st) {
  const int Ho = (H - 1)/2 + 1, Wo = (W - 1)/2 + 1;
  const unsigned chunks = ceil_div(Ho*Wo, 1024);
  hipLaunchKernelGGL(k_maxpool_fwd, dim3((unsigned)(planes*chunks)), dim3(256), 0, st, x, y, idx, H, W, Ho, Wo, chunks);
  return hipGetLastError();
}
hipError_t launch_maxpool_bwd(const float* g_y, const uint8_t* idx, float* g_x, size_t planes, int H, int W, hipStream_t st) {
  const int Ho = (H - 1)/2 + 1, Wo = (W - 1)/2 + 1;
  const unsigned chunks = ceil_div(((H + 1)/2)*((W + 1)/2), 1024);
  hipLaunchKernelGGL(k_maxpool_bwd, dim3((unsigned)(planes*chunks)), dim3(256), 0, st, g_y, idx, g_x, H, W, Ho, Wo, chunks);
  return hipGetLastError();
}

}  // namespace smd
