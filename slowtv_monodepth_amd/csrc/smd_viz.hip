// smd_viz.hip — image logging: `rgb_from_disp` and `rgb_from_feat` (src/tools/viz.py:20-74) and torchvision's `make_grid` as the reference's HeavyLogger
// calls it (src/core/heavy_logger.py:35-42).  fp32 in and out, nothing is copied to the host except the C x C matrix the caller decomposes.
//
// launch_viz_disp: per item vmax = np.percentile(d[d > 0], 95), then `apply_cmap` (src/utils/misc.py:54-60) with matplotlib's `Colormap.__call__`.
//   pass 0..3  the radix select of smd_eval.hip (8-bit digits over the bit patterns of the positive values) for the TWO order statistics around
//              0.95 (n - 1); the histograms are zeroed by the call and take integer atomics only (no float atomics anywhere in this file)
//   vmax       one block per item: numpy's `_lerp` between the two, in float32 as numpy evaluates it for a float32 array; n = 0 gives 0
//   colour     clip, (x - vmin)/(vmax - vmin + 1e-5), * N, the `== N -> N - 1` fix, truncation, table lookup; a NaN takes the "bad" colour (0, 0, 0)
// launch_viz_feat_moments: channel means (fp64 block sums, fixed order), then the centred C x C second-moment matrix: a block owns one 32 x 32 tile of
//   channel pairs (upper triangle) and one chunk of samples, stages 32 channels x 64 samples per operand through LDS (the planes are sample-major, the
//   matrix core wants channel-major) and accumulates in fp32 — on `v_mfma_f32_32x32x2_f32` for C >= 64 (each of the four waves takes 16 of the 64 samples),
//   on the vector ALU below; the blocks' tiles are summed into fp64 in chunk order by a second stage.
// launch_viz_feat_project: (x - mean) V to three channels with the blocks' extrema, the extrema's reduction, and `proj -= min; proj /= max` (the maximum of
//   the shifted values: rounding is monotonic, so it is fl(max - min)).
// launch_make_grid: one gather, one-channel inputs expanded, uint8 / bool read as they are; normalize=True takes the extrema of the n images first.
// Two calls give the same bits.
#include <algorithm>

#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_select_dev.h"

namespace smd {

static_assert(kVzBlock == kSelBlock && kVzBins == kSelBlock, "select_bin256 takes one bin per thread");
constexpr int kVzWaves = kVzBlock/kWave;
constexpr int kVzLevels = 4;
constexpr int kVzLds = kVzK + 1;                   // row stride of a staged operand: the 32 rows a wave reads fall into distinct banks

// ------------------------------------------------------------------------------------------------ rgb_from_disp

// `to_inv` keeps a NaN (0/NaN), which then takes the "bad" colour.
__device__ __forceinline__ float vz_value(float d, bool invert) { return invert ? (d != d ? d : to_inv1(d)) : d; }

__device__ __forceinline__ unsigned* vz_hist(const VizDispArgs& a, int level, int bi, int combo) {
  return a.hist + (((size_t)level*a.b + bi)*2 + combo)*kVzBins;
}

// np.percentile(x, 95) of a float32 array: q = 95/float32(100), the virtual index (n - 1) q in float32, its floor and fraction.
__device__ __forceinline__ void vz_ranks(unsigned n, unsigned& k0, unsigned& k1, float& t) {
#pragma clang fp contract(off)
  const float vi = (float)(n - 1)*0.95f, fl = floorf(vi);
  k0 = min((unsigned)fl, n - 1); k1 = min(k0 + 1, n - 1); t = vi - fl;
}

// The prefixes that levels [0, upto) selected for the two ranks of item bi -> n (0: nothing to select).
__device__ __forceinline__ unsigned vz_prefixes(const VizDispArgs& a, int bi, int upto, unsigned* sh, unsigned key[2], float& t) {
  unsigned bin, r, rk[2];
  const unsigned n = select_bin256(vz_hist(a, 0, bi, 0), 0xffffffffu, sh, bin, r);    // (the total alone)
  if (n == 0) return 0;
  vz_ranks(n, rk[0], rk[1], t);
  key[0] = key[1] = 0;
  for (int l = 0; l < upto; ++l)
#pragma unroll
    for (int c = 0; c < 2; ++c) { select_bin256(vz_hist(a, l, bi, c), rk[c], sh, bin, rk[c]); key[c] = (key[c] << 8) | bin; }
  return n;
}

template <int LEVEL>
__global__ __launch_bounds__(kVzBlock) void k_viz_pass(const VizDispArgs a) {
  __shared__ unsigned hs[2*kVzBins];
  __shared__ unsigned sel[kVzWaves + 2];
  const int bi = blockIdx.y, tid = threadIdx.x;
  unsigned key[2] = {0, 0};
  float t;
  if (LEVEL >= 1 && vz_prefixes(a, bi, LEVEL, sel, key, t) == 0) return;
  for (int i = tid; i < 2*kVzBins; i += kVzBlock) hs[i] = 0;
  __syncthreads();
  constexpr int shift = 24 - 8*LEVEL;
  const float* __restrict__ plane = a.disp + (size_t)bi*a.hw;
  for (long i = (long)blockIdx.x*kVzBlock + tid; i < a.hw; i += (long)a.nbps*kVzBlock) {
    const float v = vz_value(plane[i], a.invert);
    if (!(v > 0.f)) continue;                      // NaN is not positive
    const unsigned u = __float_as_uint(v);
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (LEVEL == 0 || (u >> ((shift + 8) & 31)) == key[c]) atomicAdd(&hs[c*kVzBins + ((u >> shift) & 0xffu)], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 2; ++c) { const unsigned v = hs[c*kVzBins + tid]; if (v) atomicAdd(&vz_hist(a, LEVEL, bi, c)[tid], v); }
}

__global__ __launch_bounds__(kVzBlock) void k_viz_vmax(const VizDispArgs a) {
  __shared__ unsigned sel[kVzWaves + 2];
  const int bi = blockIdx.x;
  unsigned key[2] = {0, 0};
  float t = 0.f;
  const unsigned n = vz_prefixes(a, bi, kVzLevels, sel, key, t);
  if (threadIdx.x != 0) return;
  if (n == 0) { a.vmax[bi] = 0.f; a.den[bi] = a.den0; return; }       // viz.py:16, the IndexError branch
  {
#pragma clang fp contract(off)
    // numpy's `_lerp`: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5
    const float lo = __uint_as_float(key[0]), hi = __uint_as_float(key[1]), d = hi - lo;
    float r = lo + d*t;
    if (t >= 0.5f) r = hi - d*(1.f - t);
    a.vmax[bi] = r;
    a.den[bi] = (r - a.vmin) + 1e-5f;
  }
}

__global__ __launch_bounds__(kVzBlock) void k_viz_colour(const VizDispArgs a) {
  __shared__ float lut[kVzMaxLut*3];
  const int bi = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < a.N*3; i += kVzBlock) lut[i] = a.lut[i];
  __syncthreads();
  const float vmax = a.vmax[bi], den = a.den[bi], vmin = a.vmin, fN = (float)a.N;
  const float* __restrict__ plane = a.disp + (size_t)bi*a.hw;
  float* __restrict__ out = a.rgb + (size_t)bi*3*a.hw;
  for (long i = (long)blockIdx.x*kVzBlock + tid; i < a.hw; i += (long)a.nbps*kVzBlock) {
#pragma clang fp contract(off)
    const float v = vz_value(plane[i], a.invert);
    // arr.clip(vmin, vmax) = minimum(maximum(arr, vmin), vmax): a NaN on either side stays one
    float x = (v != v || vmin != vmin) ? NAN : fmaxf(v, vmin);
    x = (x != x || vmax != vmax) ? NAN : fminf(x, vmax);
    float xa = ((x - vmin)/den)*fN;
    if (xa == fN) xa = fN - 1.f;
    float r = 0.f, g = 0.f, bl = 0.f;              // the "bad" colour
    if (xa == xa) {
      const int idx = xa < 0.f ? 0 : (xa >= fN ? a.N - 1 : (int)xa);   // under -> entry 0, over -> entry N - 1 (matplotlib's defaults)
      r = lut[idx*3]; g = lut[idx*3 + 1]; bl = lut[idx*3 + 2];
    }
    out[i] = r; out[(size_t)a.hw + i] = g; out[2*(size_t)a.hw + i] = bl;
  }
}

int viz_blocks_per_item(int b, int hw) {
  const long want = ((long)hw + 4095)/4096, cap = std::max(1L, 1024L/b);
  return (int)std::max(1L, std::min(want, cap));
}
size_t viz_hist_bytes(int b) { return (size_t)kVzLevels*b*2*kVzBins*sizeof(unsigned); }

hipError_t launch_viz_disp(VizDispArgs a, hipStream_t st) {
  a.nbps = viz_blocks_per_item(a.b, a.hw);
  const dim3 grid(a.nbps, a.b), blk(kVzBlock);
  if (a.select) {
    hipError_t e = hipMemsetAsync(a.hist, 0, viz_hist_bytes(a.b), st);   // a reused workspace is safe: the call zeroes what it accumulates into
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_viz_pass<0>, grid, blk, 0, st, a);
    hipLaunchKernelGGL(k_viz_pass<1>, grid, blk, 0, st, a);
    hipLaunchKernelGGL(k_viz_pass<2>, grid, blk, 0, st, a);
    hipLaunchKernelGGL(k_viz_pass<3>, grid, blk, 0, st, a);
    hipLaunchKernelGGL(k_viz_vmax, dim3(a.b), blk, 0, st, a);
  }
  hipLaunchKernelGGL(k_viz_colour, grid, blk, 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ rgb_from_feat

// sample ns of the batch -> its element of channel c
__device__ __forceinline__ size_t vf_index(const VizFeatArgs& a, unsigned ns, int c) {
  const unsigned bi = ns/(unsigned)a.hw, p = ns - bi*(unsigned)a.hw;
  return ((size_t)bi*a.C + c)*(size_t)a.hw + p;
}

__global__ __launch_bounds__(kVzBlock) void k_vf_mean(const VizFeatArgs a) {
  __shared__ double red[kVzWaves];
  const int c = blockIdx.y, sp = blockIdx.x;
  const long per = (a.n + a.nsplit - 1)/a.nsplit, s0 = sp*per, s1 = std::min(a.n, s0 + per);
  double v = 0.0;
  for (long ns = s0 + threadIdx.x; ns < s1; ns += kVzBlock) v += (double)a.feat[vf_index(a, (unsigned)ns, c)];
  block_store_sum<Waves::Sequential, kVzWaves, double>(v, red, a.mean_part + (size_t)c*a.nsplit + sp);
}

__global__ __launch_bounds__(kVzBlock) void k_vf_mean_fin(const VizFeatArgs a) {
  const int c = blockIdx.x*kVzBlock + threadIdx.x;
  if (c >= a.C) return;
  double v = 0.0;
  for (int j = 0; j < a.nsplit; ++j) v += a.mean_part[(size_t)c*a.nsplit + j];
  v /= (double)a.n;
  a.mean[c] = v; a.meanf[c] = (float)v;
}

__device__ __forceinline__ void vf_pair(int p, int T, int& ti, int& tj) {
  ti = 0;
  while (p >= T - ti) { p -= T - ti; ++ti; }
  tj = ti + p;
}

// 32 channels x kVzK samples of tile `tile`, centred, zero past C and past s1 -> dst[32][kVzLds]
__device__ __forceinline__ void vf_stage(const VizFeatArgs& a, int tile, long s, long s1, float* dst) {
  const int smp = threadIdx.x & (kVzK - 1), row0 = threadIdx.x/kVzK;
  const long ns = s + smp;
  const bool in = ns < s1;
  const size_t base = in ? vf_index(a, (unsigned)ns, 0) : 0;
#pragma unroll
  for (int r = 0; r < kVzTile/(kVzBlock/kVzK); ++r) {
    const int row = row0 + r*(kVzBlock/kVzK), c = tile*kVzTile + row;
    dst[row*kVzLds + smp] = (in && c < a.C) ? a.feat[base + (size_t)c*a.hw] - a.meanf[c] : 0.f;
  }
}

typedef float f16v __attribute__((ext_vector_type(16)));

template <bool MFMA>
__global__ __launch_bounds__(kVzBlock) void k_vf_cov(const VizFeatArgs a) {
  __shared__ float As[kVzTile*kVzLds];
  __shared__ float Bs[kVzTile*kVzLds];
  __shared__ float red[MFMA ? kVzWaves*kVzTileElems : 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid/kWave;
  int ti, tj;
  vf_pair(blockIdx.x, a.T, ti, tj);
  const long s0 = (long)blockIdx.y*a.chunk, s1 = std::min(a.n, s0 + a.chunk);
  const float* Bt = ti == tj ? As : Bs;
  f16v acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  float acc4[4] = {0.f, 0.f, 0.f, 0.f};
  const int gi = tid >> 3, gj = (tid & 7)*4;       // the vector form: thread -> row gi, columns gj .. gj + 3
  for (long s = s0; s < s1; s += kVzK) {
    vf_stage(a, ti, s, s1, As);
    if (ti != tj) vf_stage(a, tj, s, s1, Bs);
    __syncthreads();
    if (MFMA) {
      // lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; wave wv takes samples 16 wv .. 16 wv + 15 of the stage
#pragma unroll
      for (int kk = 0; kk < kVzK/kVzWaves/2; ++kk) {
        const int k = wv*(kVzK/kVzWaves) + kk*2 + (lane >> 5);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(lane & 31)*kVzLds + k], Bt[(lane & 31)*kVzLds + k], acc, 0, 0, 0);
      }
    } else {
#pragma unroll 8
      for (int k = 0; k < kVzK; ++k) {
        const float av = As[gi*kVzLds + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc4[q] = fmaf(av, Bt[(gj + q)*kVzLds + k], acc4[q]);
      }
    }
    __syncthreads();
  }
  float* out = a.tile_part + ((size_t)blockIdx.x*a.nchunk + blockIdx.y)*kVzTileElems;
  if (MFMA) {
    // D[row = (v & 3) + 8 (v >> 2) + 4 (l >> 5)][col = l & 31]; the four waves' tiles meet in wave order
#pragma unroll
    for (int v = 0; v < 16; ++v) red[wv*kVzTileElems + ((v & 3) + 8*(v >> 2) + 4*(lane >> 5))*kVzTile + (lane & 31)] = acc[v];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kVzTileElems/kVzBlock; ++q) {
      const int e = tid + q*kVzBlock;
      out[e] = sum_waves<Waves::Sequential, kVzWaves>(red + e, kVzTileElems, 0);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[gi*kVzTile + gj + q] = acc4[q];
  }
}

// the chunks' tiles in chunk order, in fp64 -> cov (both halves; a diagonal tile holds both of its halves itself)
__global__ __launch_bounds__(kVzBlock) void k_vf_cov_fin(const VizFeatArgs a) {
  int ti, tj;
  vf_pair(blockIdx.x, a.T, ti, tj);
  const float* part = a.tile_part + (size_t)blockIdx.x*a.nchunk*kVzTileElems;
  for (int e = threadIdx.x; e < kVzTileElems; e += kVzBlock) {
    double v = 0.0;
    for (int ch = 0; ch < a.nchunk; ++ch) v += (double)part[(size_t)ch*kVzTileElems + e];
    const int ci = ti*kVzTile + e/kVzTile, cj = tj*kVzTile + e % kVzTile;
    if (ci >= a.C || cj >= a.C) continue;
    a.cov[(size_t)ci*a.C + cj] = v;
    if (ti != tj) a.cov[(size_t)cj*a.C + ci] = v;
  }
}

void viz_feat_plan(VizFeatArgs& a) {
  a.n = (long)a.b*a.hw;
  a.nsplit = (int)std::max(1L, std::min(32L, (a.n + 32767)/32768));
  a.T = ceil_div(a.C, kVzTile);
  a.npairs = a.T*(a.T + 1)/2;
  const long want = std::max(1L, std::min((a.n + 4095)/4096, std::max(1L, 4096L/a.npairs)));
  a.chunk = ((a.n + want - 1)/want + kVzK - 1)/kVzK*kVzK;
  a.nchunk = (int)((a.n + a.chunk - 1)/a.chunk);
  a.nblk = viz_proj_blocks(a.n);
}
int viz_proj_blocks(long n) { return (int)std::max(1L, std::min(2048L, (n + kVzBlock - 1)/kVzBlock)); }

hipError_t launch_viz_feat_moments(VizFeatArgs a, hipStream_t st) {
  hipLaunchKernelGGL(k_vf_mean, dim3(a.nsplit, a.C), dim3(kVzBlock), 0, st, a);
  hipLaunchKernelGGL(k_vf_mean_fin, dim3(ceil_div(a.C, kVzBlock)), dim3(kVzBlock), 0, st, a);
  const dim3 grid(a.npairs, a.nchunk);
  if (a.C >= 64) hipLaunchKernelGGL(k_vf_cov<true>, grid, dim3(kVzBlock), 0, st, a);
  else hipLaunchKernelGGL(k_vf_cov<false>, grid, dim3(kVzBlock), 0, st, a);
  hipLaunchKernelGGL(k_vf_cov_fin, dim3(a.npairs), dim3(kVzBlock), 0, st, a);
  return hipGetLastError();
}

__device__ __forceinline__ float vz_wave_min(float v) {
#pragma unroll
  for (int off = kWave/2; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float vz_wave_max(float v) {
#pragma unroll
  for (int off = kWave/2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
// the block's minima of lo[NQ] and maxima of hi[NQ] -> dst[0, NQ) and dst[NQ, 2 NQ) (thread 0).  red: kVzWaves*2*NQ floats.
template <int NQ>
__device__ __forceinline__ void vz_block_extrema(const float* lo, const float* hi, float* red, float* dst) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x/kWave;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float mn = vz_wave_min(lo[q]), mx = vz_wave_max(hi[q]);
    if (lane == 0) { red[wv*2*NQ + q] = mn; red[wv*2*NQ + NQ + q] = mx; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float mn = red[q], mx = red[NQ + q];
#pragma unroll
      for (int w2 = 1; w2 < kVzWaves; ++w2) { mn = fminf(mn, red[w2*2*NQ + q]); mx = fmaxf(mx, red[w2*2*NQ + NQ + q]); }
      dst[q] = mn; dst[NQ + q] = mx;
    }
  }
}

__global__ __launch_bounds__(kVzBlock) void k_vf_proj(const VizFeatArgs a) {
  __shared__ float Vs[kVzMaxC*3];
  __shared__ float ms[kVzMaxC];
  __shared__ float red[kVzWaves*6];
  for (int i = threadIdx.x; i < a.C*3; i += kVzBlock) Vs[i] = a.V[i];
  for (int i = threadIdx.x; i < a.C; i += kVzBlock) ms[i] = (float)a.mean[i];
  __syncthreads();
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long ns = (long)blockIdx.x*kVzBlock + threadIdx.x; ns < a.n; ns += (long)a.nblk*kVzBlock) {
    const unsigned bi = (unsigned)ns/(unsigned)a.hw, p = (unsigned)ns - bi*(unsigned)a.hw;
    const float* __restrict__ x = a.feat + (size_t)bi*a.C*a.hw + p;
    float pr[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < a.C; ++c) {
      const float d = x[(size_t)c*a.hw] - ms[c];
#pragma unroll
      for (int q = 0; q < 3; ++q) pr[q] = fmaf(d, Vs[c*3 + q], pr[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      a.rgb[((size_t)bi*3 + q)*a.hw + p] = pr[q];
      lo[q] = fminf(lo[q], pr[q]); hi[q] = fmaxf(hi[q], pr[q]);
    }
  }
  vz_block_extrema<3>(lo, hi, red, a.ext_part + (size_t)blockIdx.x*6);
}

__global__ __launch_bounds__(kVzBlock) void k_vf_ext(const VizFeatArgs a) {
  __shared__ float red[kVzWaves*6];
  __shared__ float tot[6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = threadIdx.x; j < a.nblk; j += kVzBlock)
#pragma unroll
    for (int q = 0; q < 3; ++q) { lo[q] = fminf(lo[q], a.ext_part[(size_t)j*6 + q]); hi[q] = fmaxf(hi[q], a.ext_part[(size_t)j*6 + 3 + q]); }
  vz_block_extrema<3>(lo, hi, red, tot);
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 3; ++q) { a.ext[q] = tot[q]; a.ext[3 + q] = tot[3 + q] - tot[q]; }   // the maximum AFTER the subtraction (viz.py:69-70)
  }
}

__global__ __launch_bounds__(kVzBlock) void k_vf_norm(const VizFeatArgs a) {
  const long total = a.n*3;
  const float* __restrict__ e = a.ext;
  for (long i = (long)blockIdx.x*kVzBlock + threadIdx.x; i < total; i += (long)gridDim.x*kVzBlock) {
#pragma clang fp contract(off)
    const int q = (int)((i/a.hw) % 3);
    a.rgb[i] = (a.rgb[i] - e[q])/e[3 + q];
  }
}

hipError_t launch_viz_feat_project(VizFeatArgs a, hipStream_t st) {
  hipLaunchKernelGGL(k_vf_proj, dim3(a.nblk), dim3(kVzBlock), 0, st, a);
  hipLaunchKernelGGL(k_vf_ext, dim3(1), dim3(kVzBlock), 0, st, a);
  const int nb = (int)std::max(1L, std::min(4096L, (a.n*3 + kVzBlock - 1)/kVzBlock));
  hipLaunchKernelGGL(k_vf_norm, dim3(nb), dim3(kVzBlock), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ make_grid

template <bool U8>
__device__ __forceinline__ float gr_load(const void* x, size_t i) { return U8 ? (float)((const uint8_t*)x)[i] : ((const float*)x)[i]; }

template <bool U8>
__global__ __launch_bounds__(kVzBlock) void k_grid_ext(const GridArgs a) {
  __shared__ float red[kVzWaves*2];
  const long total = (long)a.n*a.c*a.h*a.w;
  float lo[1] = {INFINITY}, hi[1] = {-INFINITY};
  for (long i = (long)blockIdx.x*kVzBlock + threadIdx.x; i < total; i += (long)kVzGridParts*kVzBlock) {
    const float v = gr_load<U8>(a.x, (size_t)i);
    lo[0] = fminf(lo[0], v); hi[0] = fmaxf(hi[0], v);
  }
  vz_block_extrema<1>(lo, hi, red, a.ext_part + blockIdx.x*2);
}

template <bool U8>
__global__ __launch_bounds__(kVzBlock) void k_grid(const GridArgs a) {
  __shared__ float red[kVzWaves*2];
  __shared__ float ext[2];
  float lo = 0.f, den = 1.f, hi = 0.f;
  if (a.normalize) {
    static_assert(kVzGridParts == kVzBlock, "one partial per thread");
    const float l1[1] = {a.ext_part[threadIdx.x*2]}, h1[1] = {a.ext_part[threadIdx.x*2 + 1]};
    vz_block_extrema<1>(l1, h1, red, ext);
    __syncthreads();
    lo = ext[0]; hi = ext[1];
    den = (float)fmax((double)hi - (double)lo, 1e-5);          // `max(high - low, 1e-5)` on Python floats, then a float32 division
  }
  const long total = 3L*a.Hg*a.Wg, i = (long)blockIdx.x*kVzBlock + threadIdx.x;
  if (i >= total) return;
  const int X = (int)(i % a.Wg), Y = (int)((i/a.Wg) % a.Hg), ch = (int)(i/((long)a.Wg*a.Hg));
  const int sy = a.h + a.pad, sx = a.w + a.pad;
  const int ky = Y/sy, kx = X/sx, ry = Y - ky*sy - a.pad, rx = X - kx*sx - a.pad, k = ky*a.xmaps + kx;
  float v = a.pad_value;
  if (ry >= 0 && rx >= 0 && ky < a.ymaps && kx < a.xmaps && k < a.n) {
#pragma clang fp contract(off)
    v = gr_load<U8>(a.x, (((size_t)k*a.c + (a.c == 1 ? 0 : ch))*a.h + ry)*a.w + rx);
    if (a.normalize) v = ((v != v ? v : fminf(fmaxf(v, lo), hi)) - lo)/den;
  }
  a.grid[i] = v;
}

hipError_t launch_make_grid(GridArgs a, hipStream_t st) {
  const long total = 3L*a.Hg*a.Wg;
  const dim3 grid((unsigned)((total + kVzBlock - 1)/kVzBlock)), blk(kVzBlock);
  for_bool(a.u8, [&](auto u8) {
    if (a.normalize) hipLaunchKernelGGL(k_grid_ext<decltype(u8)::value>, dim3(kVzGridParts), blk, 0, st, a);
    hipLaunchKernelGGL(k_grid<decltype(u8)::value>, grid, blk, 0, st, a);
  });
  return hipGetLastError();
}

}  // namespace smd
