// smd_metrics.hip — the training-time validation metrics (`MonoDepthModule.compute_metrics`, src/core/trainer.py:531-552) as one entry point:
// resize the prediction to the target, clamp, mask by the depth range, align each sample by the ratio of the per-sample lower medians, and
// reduce MAE / RMSE / LogSI / AbsRel / Acc per sample.
//
//   pass 0..2  k_metrics_pass<0..2>: radix select over the BIT PATTERNS of the valid values (after the clamp every valid value is a positive finite
//              float, whose bits order like the value): 11 / 11 / 10 bits per pass, per-block histograms of the prediction and of the target in LDS
//              (integer atomics), merged with one global integer add per non-empty bin and block.  Pass L starts by re-deriving, in every block, the
//              prefix the passes before it selected (a block-wide scan of 2048 bins from L2: cheaper than a launch in between).
//   pass 3     k_metrics_pass<3>: the last prefix -> both medians (exact, order-independent: integer atomics only), r = med_t / med_p, and the seven
//              sums per sample as per-block fp64 partials in the workspace.
//   finish     k_metrics_finish: one wave per sample sums the partials in a fixed order and writes the five values.
// No float atomics, no host involvement: the rank (n-1)/2, the prefixes and r never leave the device.
//
// The resampled prediction is needed by all four passes, at the valid pixels only (a LiDAR target is ~5 % dense): `store` = 1 (the default, measured
// faster) writes it to the workspace in pass 0 and re-reads it, `store` = 0 recomputes the four taps per valid pixel and pass (knob metrics_store_pred;
// same bits either way).
#include <algorithm>

#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

constexpr int kMetPerThread = 4;                    // pixels per thread and chunk: four target loads in flight
constexpr int kMetChunk = kMetBlock*kMetPerThread;
constexpr int kMetWaves = kMetBlock/kWave;

struct MetricsArgs {
  const float* pred;        // (b,1,h,w)
  const float* target;      // (b,1,H,W)
  int b, h, w, H, W;
  float lo, hi;
  float sh, sw;             // h/H, w/W: ATen's area_pixel_compute_scale (align_corners = False, no scale factor)
  unsigned* hist;           // [3 passes][b][pred | target][kMetBins], zero on entry
  float* p0;                // (b,H*W): the resampled, clamped prediction at the valid pixels (store == 1)
  double* partial;          // [b][nbps][kMetSums]
  int nbps;                 // blocks per sample
  float* medians;           // (b,2) out
  int* counts;              // (b) out
};

__device__ __forceinline__ unsigned* met_hist(const MetricsArgs& a, int pass, int bi, int which) {
  return a.hist + (((size_t)pass*a.b + bi)*2 + which)*kMetBins;
}

// ATen's upsample_bilinear2d (align_corners = False, no antialias): source coordinate (dst + 0.5)*scale - 0.5 clamped at 0, second tap clamped at
// the last row / column.  Every product and sum is spelled out and contraction is off, so that the four passes — four instantiations the compiler
// optimises separately — compute the SAME bits for a pixel (the radix select narrows by bits), and equal sizes return the input bit for bit.
__device__ __forceinline__ float met_resample(const float* __restrict__ plane, int h, int w, int Y, int X, float sh, float sw) {
#pragma clang fp contract(off)
  const float fy = fmaxf(fmaf(sh, (float)Y + 0.5f, -0.5f), 0.f), fx = fmaxf(fmaf(sw, (float)X + 0.5f, -0.5f), 0.f);
  const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  const float hl1 = fy - (float)y0, hl0 = 1.f - hl1, wl1 = fx - (float)x0, wl0 = 1.f - wl1;
  const float v00 = plane[(size_t)y0*w + x0], v01 = plane[(size_t)y0*w + x1], v10 = plane[(size_t)y1*w + x0], v11 = plane[(size_t)y1*w + x1];
  const float top = fmaf(wl1, v01, wl0*v00), bot = fmaf(wl1, v11, wl0*v10);
  return fmaf(hl1, bot, hl0*top);
}

// Block-wide: the bin of hist[0, kMetBins) that holds the element of rank k (0-based, ascending) and k's rank inside that bin; -> the histogram's
// total.  With k >= total nothing is selected (bin = rank = 0).  sh: kMetWaves + 2 words of LDS.
__device__ __forceinline__ unsigned met_select(const unsigned* __restrict__ hist, unsigned k, unsigned* sh, unsigned& bin, unsigned& rank) {
  constexpr int per = kMetBins/kMetBlock;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid/kWave;
  unsigned c[per], mine = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) { c[j] = hist[tid*per + j]; mine += c[j]; }
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) { const unsigned v = __shfl_up(incl, off, kWave); if (lane >= off) incl += v; }
  if (lane == kWave - 1) sh[wv] = incl;
  if (tid == 0) { sh[kMetWaves] = 0; sh[kMetWaves + 1] = 0; }
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kMetWaves; ++q) { if (q < wv) before += sh[q]; total += sh[q]; }
  const unsigned excl = before + incl - mine;
  if (k >= excl && k < excl + mine) {          // exactly one thread when k < total
    unsigned r = k - excl, found = 0, fr = 0;
    bool done = false;
#pragma unroll
    for (int j = 0; j < per; ++j) {
      if (!done && r < c[j]) { found = (unsigned)(tid*per + j); fr = r; done = true; }
      if (!done) r -= c[j];
    }
    sh[kMetWaves] = found; sh[kMetWaves + 1] = fr;
  }
  __syncthreads();
  bin = sh[kMetWaves]; rank = sh[kMetWaves + 1];
  __syncthreads();                              // sh is reused by the next call
  return total;
}

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
  for (int off = kWave/2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// PASS 0..2: one radix pass (histograms of bits [31:21], [20:10], [9:0] of the values whose higher bits equal the selected prefix); PASS 3: the sums.
template <int PASS, bool STORE>
__global__ __launch_bounds__(kMetBlock) void k_metrics_pass(const MetricsArgs a) {
  __shared__ unsigned hp[PASS < 3 ? kMetBins : 1], ht[PASS < 3 ? kMetBins : 1];
  __shared__ unsigned sel[kMetWaves + 2];
  __shared__ double red[kMetWaves][kMetSums];
  const int bi = blockIdx.y, tid = threadIdx.x;
  const int HW = a.H*a.W;

  // the prefixes the earlier passes selected: key_x = the high bits of the median found so far, rk_x = the median's rank among the values that share them
  unsigned n = 0, key_p = 0, key_t = 0, rk_p = 0, rk_t = 0;
  if (PASS >= 1) {
    unsigned bin;
    n = met_select(met_hist(a, 0, bi, 0), 0xffffffffu, sel, bin, rk_p);      // (the total alone: nothing has rank 2^32 - 1)
    if (n == 0) {                                                             // no valid pixel: NaN medians, and `finish` writes NaN values
      if (PASS == 3 && blockIdx.x == 0 && tid == 0) { a.medians[bi*2] = a.medians[bi*2 + 1] = __builtin_nanf(""); a.counts[bi] = 0; }
      if (PASS == 3 && tid < kMetSums) a.partial[((size_t)bi*a.nbps + blockIdx.x)*kMetSums + tid] = 0.0;
      return;
    }
    rk_p = rk_t = (n - 1)/2;                                                  // torch.nanmedian's lower median
#pragma unroll
    for (int l = 0; l < PASS; ++l) {
      const int bits = l < 2 ? 11 : 10;
      unsigned bin_p, bin_t;
      met_select(met_hist(a, l, bi, 0), rk_p, sel, bin_p, rk_p);
      met_select(met_hist(a, l, bi, 1), rk_t, sel, bin_t, rk_t);
      key_p = (key_p << bits) | bin_p; key_t = (key_t << bits) | bin_t;
    }
  }
  if (PASS < 3) {
    for (int i = tid; i < kMetBins; i += kMetBlock) { hp[i] = 0; ht[i] = 0; }
    __syncthreads();
  }
  constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);               // bits below this pass's digit
  constexpr int digit = PASS == 2 ? 10 : 11;
  float r = 1.f;
  if (PASS == 3) {
    const float med_p = __uint_as_float(key_p), med_t = __uint_as_float(key_t);
    r = med_t/med_p;
    if (blockIdx.x == 0 && tid == 0) { a.medians[bi*2] = med_p; a.medians[bi*2 + 1] = med_t; a.counts[bi] = (int)n; }
  }
  double s[kMetSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  const float* __restrict__ tgt = a.target + (size_t)bi*HW;
  const float* __restrict__ plane = a.pred + (size_t)bi*a.h*a.w;
  float* __restrict__ p0s = a.p0 + (size_t)bi*HW;
  for (int base = blockIdx.x*kMetChunk; base < HW; base += a.nbps*kMetChunk) {
    float t[kMetPerThread];
#pragma unroll
    for (int k = 0; k < kMetPerThread; ++k) { const int i = base + k*kMetBlock + tid; t[k] = i < HW ? tgt[i] : 0.f; }   // (0 is never valid: lo > 0)
#pragma unroll
    for (int k = 0; k < kMetPerThread; ++k) {
      const int i = base + k*kMetBlock + tid;
      if (!(t[k] > a.lo && t[k] < a.hi)) continue;                           // a NaN target is invalid
      float p0;
      if (STORE && PASS > 0) p0 = p0s[i];
      else {
        const int Y = i/a.W, X = i - Y*a.W;
        p0 = fminf(fmaxf(met_resample(plane, a.h, a.w, Y, X, a.sh, a.sw), a.lo), a.hi);
        if (STORE) p0s[i] = p0;
      }
      if (PASS < 3) {
        const unsigned kp = __float_as_uint(p0), kt = __float_as_uint(t[k]);
        if (PASS == 0 || (kp >> (shift + digit)) == key_p) atomicAdd(&hp[(kp >> shift) & ((1u << digit) - 1u)], 1u);
        if (PASS == 0 || (kt >> (shift + digit)) == key_t) atomicAdd(&ht[(kt >> shift) & ((1u << digit) - 1u)], 1u);
      } else {
        const float p = fminf(fmaxf(p0*r, a.lo), a.hi), tt = t[k];
        // e = log p - log t as the log of the ratio: the ratio's rounding (6e-8 relative) is the whole error, where two logs of values far from 1
        // would each bring an ulp of |log| (2e-7 at 30 m) into a difference whose spread is the metric
        const float pt = p/tt, d = p - tt, ad = fabsf(d), e = logf(pt), q = fmaxf(tt/p, pt);
        s[0] += (double)ad; s[1] += (double)d*(double)d; s[2] += (double)e; s[3] += (double)e*(double)e; s[4] += (double)(ad/tt);
        s[5] += q < 1.25f ? 1.0 : 0.0; s[6] += (double)q;
      }
    }
  }
  if (PASS < 3) {
    __syncthreads();
    unsigned* gp = met_hist(a, PASS, bi, 0);
    unsigned* gt = met_hist(a, PASS, bi, 1);
    for (int i = tid; i < (1 << digit); i += kMetBlock) {
      const unsigned cp = hp[i], ct = ht[i];
      if (cp) atomicAdd(&gp[i], cp);
      if (ct) atomicAdd(&gt[i], ct);
    }
  } else {
    const int lane = tid & (kWave - 1), wv = tid/kWave;
#pragma unroll
    for (int q = 0; q < kMetSums; ++q) { const double v = met_wave_sum(s[q]); if (lane == 0) red[wv][q] = v; }
    __syncthreads();
    if (tid < kMetSums) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < kMetWaves; ++q) v += red[q][tid];
      a.partial[((size_t)bi*a.nbps + blockIdx.x)*kMetSums + tid] = v;
    }
  }
}

// One wave per sample: the blocks' partials in a fixed order -> values (b,5) = MAE, RMSE, LogSI, AbsRel, Acc.
__global__ __launch_bounds__(kWave) void k_metrics_finish(const double* __restrict__ partial, int nbps, const int* __restrict__ counts, float* __restrict__ values) {
  const int bi = blockIdx.x, lane = threadIdx.x;
  double s[kMetSums];
#pragma unroll
  for (int q = 0; q < kMetSums; ++q) {
    double v = 0.0;
    for (int j = lane; j < nbps; j += kWave) v += partial[((size_t)bi*nbps + j)*kMetSums + q];
    s[q] = met_wave_sum(v);
  }
  if (lane != 0) return;
  float* out = values + (size_t)bi*5;
  const int n = counts[bi];
  if (n == 0) {                                   // the reference's nanmean over an all-NaN row
    for (int q = 0; q < 5; ++q) out[q] = __builtin_nanf("");
    return;
  }
  const double inv = 1.0/(double)n, me = s[2]*inv;
  out[0] = (float)(s[0]*inv);
  out[1] = (float)sqrt(s[1]*inv);
  out[2] = (float)(100.0*sqrt(s[3]*inv - me*me));  // the variance is NOT clamped under the root (the reference's ScaleInvariant does not either)
  out[3] = (float)(100.0*s[4]*inv);
  out[4] = (float)(100.0*s[5]/s[6]);               // the reference's DeltaAcc divides the count by the SUM of the ratios, not by n: kept
}

int metrics_blocks_per_sample(int b, int H, int W) {
  const long HW = (long)H*W;
  const long want = (HW + 4095)/4096, cap = std::max(1L, 1024L/b);   // >= 4096 pixels per block (the LDS histograms are zeroed and merged per block), ~1024 blocks
  return (int)std::max(1L, std::min(want, cap));
}
size_t metrics_hist_bytes(int b) { return (size_t)3*b*2*kMetBins*sizeof(unsigned); }

template <bool STORE> static void launch_passes(const MetricsArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((k_metrics_pass<0, STORE>), grid, dim3(kMetBlock), 0, st, a);
  hipLaunchKernelGGL((k_metrics_pass<1, STORE>), grid, dim3(kMetBlock), 0, st, a);
  hipLaunchKernelGGL((k_metrics_pass<2, STORE>), grid, dim3(kMetBlock), 0, st, a);
  hipLaunchKernelGGL((k_metrics_pass<3, STORE>), grid, dim3(kMetBlock), 0, st, a);
}

hipError_t launch_depth_metrics(const float* pred, const float* target, int b, int h, int w, int H, int W, float lo, float hi, float* values,
                                float* medians, int* counts, unsigned* hist, double* partial, float* p0, bool store, hipStream_t st) {
  MetricsArgs a;
  a.pred = pred; a.target = target; a.b = b; a.h = h; a.w = w; a.H = H; a.W = W; a.lo = lo; a.hi = hi;
  a.sh = (float)h/(float)H; a.sw = (float)w/(float)W;
  a.hist = hist; a.p0 = p0; a.partial = partial; a.nbps = metrics_blocks_per_sample(b, H, W);
  a.medians = medians; a.counts = counts;
  hipError_t e = hipMemsetAsync(hist, 0, metrics_hist_bytes(b), st);   // a reused workspace is safe: the call zeroes what it accumulates into
  if (e != hipSuccess) return e;
  const dim3 grid(a.nbps, b);
  if (store) launch_passes<true>(a, grid, st); else launch_passes<false>(a, grid, st);
  hipLaunchKernelGGL(k_metrics_finish, dim3(b), dim3(kWave), 0, st, partial, a.nbps, counts, values);
  return hipGetLastError();
}

}  // namespace smd
