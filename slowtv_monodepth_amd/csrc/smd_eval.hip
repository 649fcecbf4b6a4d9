// smd_eval.hip — offline depth evaluation (`MonoDepthEvaluator.__call__`, src/core/evaluator.py:50-94) as two operators.
//
// launch_eval_metrics: resize the disparity to the target, invert it as `to_inv` does, mask, align on the masked values (a fixed factor, the ratio of the
// two `np.median`s, or a least-squares scale and shift in disparity space), scale and clip, and reduce the sums of `metrics_eigen` and `metrics_benchmark`.
//   pass 0     resize + to_inv + mask -> the masked prediction (0 where masked out: every valid prediction is > 0), the six alignment sums as per-block
//              fp64 partials, and (median) the histogram of the top byte of the bit patterns
//   pass 1..3  (median only) the radix select restated from smd_metrics.hip with 8-bit digits and FOUR selections per item: ranks (n-1)/2 and n/2 of the
//              prediction and of the target (np.median of an even count is the float32 mean of the two middle values).  Valid values are positive
//              floats, whose bit patterns order like the values; only integer atomics touch the histograms, so the selection is exact.
//   align      one block per item: count, status, (scale, shift) in fp64
//   sums       p = clip(scale*x + shift) in float32 operation by operation as numpy evaluates it, the fifteen sums as per-block fp64 partials, and the
//              aligned depth (0 where masked out) when the caller asks for it
//   finish     one wave per item adds the partials in a fixed order and writes the twenty values
// No float atomics and no host round trip; the same bits on every call.
//
// launch_eval_pointcloud: `metrics_pointcloud` (src/core/metrics.py:111-165): back-project the aligned depth and the target at the masked pixels, compacted
// in row-major order, and find for every second point of each cloud its exact nearest neighbour in the other by tiled brute force.
//   points     pixel -> its rank under the caller's prefix sum of the mask -> both clouds as separate x, y, z arrays
//   nn         a block owns kPcBlock*kPcQ queries (kPcQ per lane, in registers) and one slice of the database, which it streams through LDS one tile
//              at a time; every lane reads the same LDS address (a broadcast), one 16-byte read per coordinate serves 4*kPcQ distance evaluations;
//              d^2 from the DIFFERENCES; the slices' minima meet in an integer atomic minimum over the bit patterns (order-independent)
//   finish     one square root per query, the mean distance and the three threshold counts per direction as fixed-order fp64 sums
#include <algorithm>

#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_select_dev.h"

namespace smd {

constexpr int kEvPerThread = 4;
constexpr int kEvChunk = kEvBlock*kEvPerThread;
constexpr int kEvWaves = kEvBlock/kWave;
constexpr int kEvLevels = 4;                       // 8-bit digits of a 32-bit pattern

__device__ __forceinline__ unsigned* ev_hist(const EvalArgs& a, int level, int bi, int combo) {
  return a.hist + (((size_t)level*a.b + bi)*4 + combo)*kEvBins;
}

// ATen's upsample_bilinear2d taps (align_corners = False); equal sizes return the input bit for bit.
__device__ __forceinline__ float ev_bilinear(const float* __restrict__ plane, int h, int w, int Y, int X, float sh, float sw) {
#pragma clang fp contract(off)
  const float fy = fmaxf(fmaf(sh, (float)Y + 0.5f, -0.5f), 0.f), fx = fmaxf(fmaf(sw, (float)X + 0.5f, -0.5f), 0.f);
  const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  const float hl1 = fy - (float)y0, hl0 = 1.f - hl1, wl1 = fx - (float)x0, wl0 = 1.f - wl1;
  const float v00 = plane[(size_t)y0*w + x0], v01 = plane[(size_t)y0*w + x1], v10 = plane[(size_t)y1*w + x0], v11 = plane[(size_t)y1*w + x1];
  // ATen's GPU kernel writes h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11) and is compiled with contraction on: of two products under a sum the FIRST is
  // fused, the second rounded.  Spelled out here in that form (smd_metrics.hip fuses the other product, as ATen's CPU kernel rounds).
  const float top = fmaf(wl0, v00, wl1*v01), bot = fmaf(wl0, v10, wl1*v11);
  return fmaf(hl0, top, hl1*bot);
}

// ATen's upsample_nearest2d: source index min(floor(dst*scale), in - 1), scale = in/out in float32.
__device__ __forceinline__ float ev_nearest(const float* __restrict__ plane, int h, int w, int Y, int X, float sh, float sw) {
  const int y = min((int)floorf((float)Y*sh), h - 1), x = min((int)floorf((float)X*sw), w - 1);
  return plane[(size_t)y*w + x];
}

// `to_inv` on one value (smd_select_dev.h): a NaN is 0 here and masked out by `pred > 0`.
__device__ __forceinline__ float ev_inv(float d) { return to_inv1(d); }

__device__ __forceinline__ double ev_wave_sum(double v) {
#pragma unroll
  for (int off = kWave/2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// Block-wide sum of NS per-thread fp64 values in a fixed order -> out[0, NS) (written by the first NS threads).  red: [kEvWaves][NS].
template <int NS>
__device__ __forceinline__ void ev_block_sums(const double* s, double* red, double* out) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid/kWave;
#pragma unroll
  for (int q = 0; q < NS; ++q) { const double v = ev_wave_sum(s[q]); if (lane == 0) red[wv*NS + q] = v; }
  __syncthreads();
  if (tid < NS) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < kEvWaves; ++q) v += red[q*NS + tid];
    out[tid] = v;
  }
}

// One digit of the select: smd_select_dev.h (shared with smd_viz.hip).  kEvBins == kEvBlock == kSelBlock: one bin per thread.
static_assert(kEvBlock == kSelBlock && kEvBins == kSelBlock, "select_bin256 takes one bin per thread");
__device__ __forceinline__ unsigned ev_select(const unsigned* __restrict__ hist, unsigned k, unsigned* sh, unsigned& bin, unsigned& rank) {
  return select_bin256(hist, k, sh, bin, rank);
}

// The prefixes that levels [0, upto) selected for the four (array, rank) combinations of item bi: combo 0, 1 = the prediction's ranks (n-1)/2 and n/2,
// combo 2, 3 = the target's.  -> n (0: nothing to select, keys untouched).
__device__ __forceinline__ unsigned ev_prefixes(const EvalArgs& a, int bi, int upto, unsigned* sh, unsigned key[4], unsigned rk[4]) {
  unsigned bin, r;
  const unsigned n = ev_select(ev_hist(a, 0, bi, 0), 0xffffffffu, sh, bin, r);    // (the total alone: nothing has rank 2^32 - 1)
  if (n == 0) return 0;
  rk[0] = rk[2] = (n - 1)/2; rk[1] = rk[3] = n/2;
  key[0] = key[1] = key[2] = key[3] = 0;
  for (int l = 0; l < upto; ++l)
#pragma unroll
    for (int c = 0; c < 4; ++c) { ev_select(ev_hist(a, l, bi, c), rk[c], sh, bin, rk[c]); key[c] = (key[c] << 8) | bin; }
  return n;
}

// LEVEL 0: resize, invert, mask, the alignment sums, and (MEDIAN) the first histogram.  LEVEL 1..3 (median only): the next digit.
template <int LEVEL, bool MEDIAN>
__global__ __launch_bounds__(kEvBlock) void k_eval_pass(const EvalArgs a) {
  __shared__ unsigned hs[MEDIAN ? 4*kEvBins : 1];
  __shared__ unsigned sel[kEvWaves + 2];
  __shared__ double red[kEvWaves*kEvAlignSums];
  const int bi = blockIdx.y, tid = threadIdx.x;
  const int HW = a.H*a.W;
  unsigned key[4] = {0, 0, 0, 0}, rk[4] = {0, 0, 0, 0};
  if (LEVEL >= 1 && ev_prefixes(a, bi, LEVEL, sel, key, rk) == 0) return;
  if (MEDIAN) {
    for (int i = tid; i < 4*kEvBins; i += kEvBlock) hs[i] = 0;
    __syncthreads();
  }
  constexpr int shift = 24 - 8*LEVEL;
  double s[kEvAlignSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  const float* __restrict__ tgt = a.target + (size_t)bi*HW;
  const float* __restrict__ plane = a.disp + (size_t)bi*a.h*a.w;
  const uint8_t* __restrict__ msk = a.mask ? a.mask + (size_t)bi*HW : nullptr;
  float* __restrict__ pm = a.pred + (size_t)bi*HW;
  for (int base = blockIdx.x*kEvChunk; base < HW; base += a.nbps*kEvChunk) {
#pragma unroll
    for (int k = 0; k < kEvPerThread; ++k) {
      const int i = base + k*kEvBlock + tid;
      if (i >= HW) continue;
      float p, t = tgt[i];
      if (LEVEL == 0) {
        const int Y = i/a.W, X = i - Y*a.W;
        const float d = a.nearest ? ev_nearest(plane, a.h, a.w, Y, X, a.sh, a.sw) : ev_bilinear(plane, a.h, a.w, Y, X, a.sh, a.sw);
        if (a.resized) a.resized[(size_t)bi*HW + i] = d;
        p = ev_inv(d);
        bool ok = t > a.lo && (!a.has_hi || t < a.hi) && p > 0.f;                // a NaN target is invalid
        ok = ok && Y >= a.y0 && Y < a.y1 && X >= a.x0 && X < a.x1 && (!msk || msk[i] != 0);
        if (!ok) p = 0.f;
        pm[i] = p;
        if (a.valid) a.valid[(size_t)bi*HW + i] = ok ? 1 : 0;
        if (ok) {
          const double pi = (double)ev_inv(p), ti = (double)ev_inv(t);            // least squares works in disparity space (evaluator.py:81, 208)
          s[0] += 1.0; s[1] += pi; s[2] += pi*pi; s[3] += pi*ti; s[4] += ti; s[5] += (double)p;
        }
      } else p = pm[i];
      if (MEDIAN && p > 0.f) {
        const unsigned kp = __float_as_uint(p), kt = __float_as_uint(t);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const unsigned v = c < 2 ? kp : kt;
          if (LEVEL == 0 || (v >> (shift + 8)) == key[c]) atomicAdd(&hs[c*kEvBins + ((v >> shift) & 0xffu)], 1u);
        }
      }
    }
  }
  if (MEDIAN) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) { const unsigned v = hs[c*kEvBins + tid]; if (v) atomicAdd(&ev_hist(a, LEVEL, bi, c)[tid], v); }
  }
  if (LEVEL == 0) ev_block_sums<kEvAlignSums>(s, red, a.partial0 + ((size_t)bi*a.nbps + blockIdx.x)*kEvAlignSums);
}

// One block per item: the blocks' alignment sums in a fixed order -> count, status, (scale, shift).
__global__ __launch_bounds__(kEvBlock) void k_eval_align(const EvalArgs a) {
  __shared__ unsigned sel[kEvWaves + 2];
  __shared__ double red[kEvWaves*kEvAlignSums];
  __shared__ double tot[kEvAlignSums];
  const int bi = blockIdx.x, tid = threadIdx.x;
  double s[kEvAlignSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < a.nbps; j += kEvBlock)
#pragma unroll
    for (int q = 0; q < kEvAlignSums; ++q) s[q] += a.partial0[((size_t)bi*a.nbps + j)*kEvAlignSums + q];
  ev_block_sums<kEvAlignSums>(s, red, tot);
  __syncthreads();
  unsigned key[4] = {0, 0, 0, 0}, rk[4];
  if (a.mode == SMD_EVAL_ALIGN_MEDIAN) ev_prefixes(a, bi, kEvLevels, sel, key, rk);
  if (tid != 0) return;
  const double n = tot[0];
  double scale = 0.0, shift = 0.0;
  int status = SMD_EVAL_SCORED;
  if (n == 0.0) status = SMD_EVAL_EMPTY_MASK;
  else if (tot[5] == 0.0) status = SMD_EVAL_ZERO_PRED;                           // `pred_mask.sum() == 0` (evaluator.py:78)
  else if (a.mode == SMD_EVAL_ALIGN_MEDIAN) {
#pragma clang fp contract(off)
    // np.median: the mean of the two middle values in float32 — one rounded sum, then an exact halving —, and the ratio in float32
    const float mp = (__uint_as_float(key[0]) + __uint_as_float(key[1]))*0.5f, mt = (__uint_as_float(key[2]) + __uint_as_float(key[3]))*0.5f;
    a.medians[bi*2] = mp; a.medians[bi*2 + 1] = mt;
    scale = (double)(mt/mp);
  } else if (a.mode == SMD_EVAL_ALIGN_LSQR) {
    // [[Spp, Sp], [Sp, n]] x = [Spt, St] (evaluator.py:229-234); det <= 0: (0, 0)
    const double det = tot[2]*n - tot[1]*tot[1];
    if (det > 0.0) { scale = (n*tot[3] - tot[1]*tot[4])/det; shift = (tot[2]*tot[4] - tot[1]*tot[3])/det; }
  } else scale = (double)a.factor;
  if (status != SMD_EVAL_SCORED || a.mode != SMD_EVAL_ALIGN_MEDIAN) a.medians[bi*2] = a.medians[bi*2 + 1] = 0.f;
  a.align[bi*2] = scale; a.align[bi*2 + 1] = shift;
  a.counts[bi] = (int)n; a.status[bi] = status;
}

// `MonoDepthEvaluator.scale` (evaluator.py:236-243) on one value, every operation rounded to float32 as numpy rounds it (the Python floats scale and
// shift are weak scalars: the arithmetic is float32).
__device__ __forceinline__ float ev_scale(float p, float sc, float sf, bool inv, float lo, float hi, bool has_hi) {
#pragma clang fp contract(off)
  if (inv) p = ev_inv(p);
  p = sc*p + sf;
  if (inv) p = ev_inv(p);
  p = fmaxf(p, lo);
  return has_hi ? fminf(p, hi) : p;
}

__global__ __launch_bounds__(kEvBlock) void k_eval_sums(const EvalArgs a) {
  __shared__ double red[kEvWaves*kEvSums];
  const int bi = blockIdx.y, tid = threadIdx.x;
  const int HW = a.H*a.W;
  const bool scored = a.status[bi] == SMD_EVAL_SCORED, inv = a.mode == SMD_EVAL_ALIGN_LSQR;
  const float sc = (float)a.align[bi*2], sf = (float)a.align[bi*2 + 1];
  double s[kEvSums];
#pragma unroll
  for (int q = 0; q < kEvSums; ++q) s[q] = 0.0;
  const float* __restrict__ tgt = a.target + (size_t)bi*HW;
  const float* __restrict__ pm = a.pred + (size_t)bi*HW;
  float* __restrict__ dout = a.depth ? a.depth + (size_t)bi*HW : nullptr;
  for (int base = blockIdx.x*kEvChunk; base < HW; base += a.nbps*kEvChunk) {
#pragma unroll
    for (int k = 0; k < kEvPerThread; ++k) {
      const int i = base + k*kEvBlock + tid;
      if (i >= HW) continue;
      const float p0 = pm[i];
      const bool ok = scored && p0 > 0.f;
      const float p = ok ? ev_scale(p0, sc, sf, inv, a.lo, a.hi, a.has_hi) : 0.f;
      if (dout) dout[i] = p;
      if (!ok) continue;
      const float t = tgt[i];
      const double pd = (double)p, td = (double)t, err = fabs(pd - td), e2 = err*err, l = log(pd) - log(td);
      s[0] += err; s[1] += e2; s[2] += err/td; s[3] += e2/td; s[4] += e2/(td*td); s[5] += l; s[6] += l*l; s[7] += fabs(l);
      if (a.groups & SMD_EVAL_BENCHMARK) { const double iv = 1000.0*fabs(1.0/pd - 1.0/td); s[8] += iv; s[9] += iv*iv; }
      if (a.groups & SMD_EVAL_EIGEN) {
        // the threshold test is float32 against float32 constants, as numpy's `thresh < 1.05` on a float32 array is
        const float q = fmaxf(t/p, p/t);
        s[10] += q < 1.05f ? 1.0 : 0.0; s[11] += q < 1.1f ? 1.0 : 0.0; s[12] += q < 1.25f ? 1.0 : 0.0; s[13] += q < 1.5625f ? 1.0 : 0.0;
        s[14] += q < 1.953125f ? 1.0 : 0.0;
      }
    }
  }
  ev_block_sums<kEvSums>(s, red, a.partial1 + ((size_t)bi*a.nbps + blockIdx.x)*kEvSums);
}

// One wave per item -> values (b,20): Scale, Shift | AbsRel, SqRel, RMSE, LogRMSE, five deltas (metrics.py:39-59) | MAE, RMSE, InvMAE, InvRMSE, LogMAE,
// LogRMSE, LogSI, AbsRel, SqRel (metrics.py:80-105).  An item that is not scored gets zeros.
__global__ __launch_bounds__(kWave) void k_eval_finish(const EvalArgs a) {
  const int bi = blockIdx.x, lane = threadIdx.x;
  double s[kEvSums];
#pragma unroll
  for (int q = 0; q < kEvSums; ++q) {
    double v = 0.0;
    for (int j = lane; j < a.nbps; j += kWave) v += a.partial1[((size_t)bi*a.nbps + j)*kEvSums + q];
    s[q] = ev_wave_sum(v);
  }
  if (lane != 0) return;
  double* out = a.values + (size_t)bi*kEvValues;
  for (int q = 0; q < kEvValues; ++q) out[q] = 0.0;
  if (a.status[bi] != SMD_EVAL_SCORED) return;
  const double inv = 1.0/(double)a.counts[bi];
  out[0] = a.align[bi*2]; out[1] = a.align[bi*2 + 1];
  if (a.groups & SMD_EVAL_EIGEN) {
    out[2] = s[2]*inv; out[3] = s[3]*inv; out[4] = sqrt(s[1]*inv); out[5] = sqrt(s[6]*inv);
    for (int q = 0; q < 5; ++q) out[6 + q] = 100.0*(s[10 + q]*inv);
  }
  if (a.groups & SMD_EVAL_BENCHMARK) {
    const double ml = 100.0*s[5]*inv, ml2 = 1e4*s[6]*inv;
    out[11] = s[0]*inv; out[12] = sqrt(s[1]*inv); out[13] = s[8]*inv; out[14] = sqrt(s[9]*inv); out[15] = 100.0*s[7]*inv; out[16] = sqrt(ml2);
    out[17] = sqrt(ml2 - ml*ml);                   // not clamped under the root: the reference's is not either
    out[18] = 100.0*s[2]*inv; out[19] = 100.0*s[4]*inv;
  }
}

int eval_blocks_per_item(int b, int H, int W) {
  const long HW = (long)H*W;
  const long want = (HW + 4095)/4096, cap = std::max(1L, 1024L/b);   // >= 4096 pixels per block (the LDS histograms are zeroed and merged per block)
  return (int)std::max(1L, std::min(want, cap));
}
size_t eval_hist_bytes(int b) { return (size_t)kEvLevels*b*4*kEvBins*sizeof(unsigned); }

hipError_t launch_eval_metrics(EvalArgs a, hipStream_t st) {
  a.nbps = eval_blocks_per_item(a.b, a.H, a.W);
  a.sh = (float)a.h/(float)a.H; a.sw = (float)a.w/(float)a.W;
  const dim3 grid(a.nbps, a.b), blk(kEvBlock);
  if (a.mode == SMD_EVAL_ALIGN_MEDIAN) {
    hipError_t e = hipMemsetAsync(a.hist, 0, eval_hist_bytes(a.b), st);   // a reused workspace is safe: the call zeroes what it accumulates into
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_eval_pass<0, true>), grid, blk, 0, st, a);
    hipLaunchKernelGGL((k_eval_pass<1, true>), grid, blk, 0, st, a);
    hipLaunchKernelGGL((k_eval_pass<2, true>), grid, blk, 0, st, a);
    hipLaunchKernelGGL((k_eval_pass<3, true>), grid, blk, 0, st, a);
  } else hipLaunchKernelGGL((k_eval_pass<0, false>), grid, blk, 0, st, a);
  hipLaunchKernelGGL(k_eval_align, dim3(a.b), blk, 0, st, a);
  hipLaunchKernelGGL(k_eval_sums, grid, blk, 0, st, a);
  hipLaunchKernelGGL(k_eval_finish, dim3(a.b), dim3(kWave), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Point clouds.  pts: [b][cloud: 0 prediction, 1 target][x | y | z][cap]; best: [b][direction][nqcap] bit patterns of the smallest d^2 so far.

// `BackprojectDepth.forward` (src/tools/geometry.py:304-316): K_inv[:3,:3] @ (x, y, 1), then times the depth.  The row product is accumulated in the order
// k0*x, + k1*y, + k2*1; for intrinsics without skew (one of the first two terms is an exact zero) this is what any matrix product gives, fused or not.
__global__ __launch_bounds__(kPcBlock) void k_pc_points(const PcArgs a) {
  const int bi = blockIdx.y, i = blockIdx.x*kPcBlock + threadIdx.x;
  if (i >= a.cap) return;
  const size_t px = (size_t)bi*a.cap + i;
  if (a.mask[px] == 0) return;
  const int r = a.cs[px] - 1;
  if (r < 0 || r >= a.cap) return;                 // (a prefix sum that is not the mask's: refuse the pixel, never write outside)
  const int Y = i/a.W, X = i - Y*a.W;
  const float* __restrict__ k = a.Kinv + (size_t)bi*16;
  const float x = (float)X, y = (float)Y, dp = a.depth[px], dt = a.target[px];
  float* __restrict__ P = a.pts + (size_t)bi*6*a.cap;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float ray = fmaf(k[c*4 + 2], 1.f, fmaf(k[c*4 + 1], y, k[c*4]*x));
    P[(size_t)c*a.cap + r] = ray*dp;
    P[(size_t)(3 + c)*a.cap + r] = ray*dt;
  }
}

__device__ __forceinline__ int pc_count(const PcArgs& a, int bi) { return max(0, min(a.cs[(size_t)bi*a.cap + a.cap - 1], a.cap)); }

// grid: (query tiles, b*nsplit, direction).  Direction 0: every second prediction point against the target cloud; 1: the other way round.
__global__ __launch_bounds__(kPcBlock) void k_pc_nn(const PcArgs a) {
  __shared__ __attribute__((aligned(16))) float sx[kPcTile], sy[kPcTile], sz[kPcTile];
  const int tid = threadIdx.x, dir = blockIdx.z, bi = blockIdx.y/a.nsplit, split = blockIdx.y - bi*a.nsplit;
  const int n = pc_count(a, bi), nq = (n + 1)/2;
  const int q0 = blockIdx.x*(kPcBlock*kPcQ);
  if (q0 >= nq) return;                            // (uniform over the block: no barrier is skipped by part of it)
  const int len = (n + a.nsplit - 1)/a.nsplit, d0 = split*len, d1 = min(n, d0 + len);
  if (d0 >= d1) return;
  const float* __restrict__ Q = a.pts + ((size_t)bi*2 + dir)*3*a.cap;
  const float* __restrict__ D = a.pts + ((size_t)bi*2 + (1 - dir))*3*a.cap;
  float qx[kPcQ], qy[kPcQ], qz[kPcQ], best[kPcQ];
#pragma unroll
  for (int k = 0; k < kPcQ; ++k) {
    const int j = q0 + k*kPcBlock + tid, src = j < nq ? 2*j : 0;                  // (2j <= n - 1 for j < nq; slot 0 exists: n >= 1 here)
    qx[k] = Q[src]; qy[k] = Q[(size_t)a.cap + src]; qz[k] = Q[(size_t)2*a.cap + src];
    best[k] = __builtin_inff();
  }
  for (int t0 = d0; t0 < d1; t0 += kPcTile) {
    __syncthreads();
    const int cnt = min(kPcTile, d1 - t0), src = t0 + (tid < cnt ? tid : 0);      // the tail of the last tile repeats its first point: the minimum is unchanged
    sx[tid] = D[src]; sy[tid] = D[(size_t)a.cap + src]; sz[tid] = D[(size_t)2*a.cap + src];
    __syncthreads();
    const int cnt4 = (cnt + 3) & ~3;
    for (int j = 0; j < cnt4; j += 4) {
      const f4 X = *(const f4*)&sx[j], Y = *(const f4*)&sy[j], Z = *(const f4*)&sz[j];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < kPcQ; ++k) {
          const float dx = qx[k] - X[u], dy = qy[k] - Y[u], dz = qz[k] - Z[u];
          best[k] = fminf(best[k], fmaf(dz, dz, fmaf(dy, dy, dx*dx)));
        }
    }
  }
  unsigned* __restrict__ out = a.best + ((size_t)bi*2 + dir)*a.nqcap;
#pragma unroll
  for (int k = 0; k < kPcQ; ++k) {
    const int j = q0 + k*kPcBlock + tid;
    if (j < nq) atomicMin(&out[j], __float_as_uint(best[k]));                     // d^2 >= 0: the bit patterns order like the values
  }
}

// grid: (direction, b): nn (b,2,nqcap) = the distances (0 past the item's query count), stats (b,2,4) = sum of distances, counts below 0.05 / 0.1 / 0.2.
__global__ __launch_bounds__(kPcBlock) void k_pc_finish(const PcArgs a) {
  __shared__ double red[(kPcBlock/kWave)*4];
  const int tid = threadIdx.x, dir = blockIdx.x, bi = blockIdx.y;
  const int n = pc_count(a, bi), nq = (n + 1)/2;
  const unsigned* __restrict__ in = a.best + ((size_t)bi*2 + dir)*a.nqcap;
  float* __restrict__ nn = a.nn + ((size_t)bi*2 + dir)*a.nqcap;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < a.nqcap; j += kPcBlock) {
    float d = 0.f;
    if (j < nq) {
      d = sqrtf(__uint_as_float(in[j]));
      s[0] += (double)d; s[1] += d < 0.05f ? 1.0 : 0.0; s[2] += d < 0.1f ? 1.0 : 0.0; s[3] += d < 0.2f ? 1.0 : 0.0;   // float32 against float32, as numpy compares
    }
    nn[j] = d;
  }
  const int lane = tid & (kWave - 1), wv = tid/kWave;
#pragma unroll
  for (int q = 0; q < 4; ++q) { const double v = ev_wave_sum(s[q]); if (lane == 0) red[wv*4 + q] = v; }
  __syncthreads();
  if (tid < 4) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < kPcBlock/kWave; ++q) v += red[q*4 + tid];
    a.stats[((size_t)bi*2 + dir)*4 + tid] = v;
  }
  if (tid == 0 && dir == 0) a.counts[bi] = n;
}

int pc_splits(int cap) { return std::max(1, std::min(32, (cap + 2047)/2048)); }

hipError_t launch_eval_pointcloud(PcArgs a, hipStream_t st) {
  a.nsplit = pc_splits(a.cap);
  hipError_t e = hipMemsetAsync(a.best, 0xff, (size_t)a.b*2*a.nqcap*sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pc_points, dim3(ceil_div(a.cap, kPcBlock), a.b), dim3(kPcBlock), 0, st, a);
  hipLaunchKernelGGL(k_pc_nn, dim3(ceil_div(a.nqcap, kPcBlock*kPcQ), a.b*a.nsplit, 2), dim3(kPcBlock), 0, st, a);
  hipLaunchKernelGGL(k_pc_finish, dim3(2, a.b), dim3(kPcBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace smd
