// smd_masks.hip — the post-process and the regularisers of predictive-mask training.
//
//   smd_upsample_stack_*: `ops.interpolate_like(mask_s, imgs, mode='bilinear')` of every scale (src/core/trainer.py:323-324; F.interpolate with
//     align_corners=False) for S tensors of (b,n,hs,ws) in ONE launch, written as the scale-major stack (S,b,n,h,w) that `handlers.image_recon` flattens
//     (src/core/handlers.py:47) — so neither S interpolate launches nor the `torch.stack` copy happen.  Backward: the exact adjoint as a gather per SOURCE
//     pixel over the output pixels whose bilinear window holds it (no atomics), one launch for all scales.  (K0, smd_depth.hip, is the one-channel,
//     to-depth form of the same resampling; it stays as it is.)
//   smd_scale_mean_*: mean over scales of the mean over elements of f(x_s), for S tensors of different sizes in one launch, f(x) = -max(log x, -100)
//     (`F.binary_cross_entropy(x, ones)`, src/regularizers/mask.py:29, with ATen's clamp of the logarithm) or f(x) = sign * x (src/regularizers/occlusion.py:39),
//     as `handlers.disp_mask` / `disp_occ` combine them (src/core/handlers.py:314-347).  Per-block partial sums in fp32, added in fp64 in block order by the
//     block that arrives last.  Backward: one element-wise launch.
#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

// ATen area_pixel_compute_source_index (align_corners=False, non-cubic) + index/lambda split (as smd_depth.hip)
__device__ __forceinline__ void up_src_index(int dst, float scale, int n_in, int& i0, int& i1, float& l1) {
  const float src = fmaxf(fmaf(scale, (float)dst + 0.5f, -0.5f), 0.f);
  i0 = min((int)src, n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// grid (blocks over h*w, planes = b*n, S)
__global__ __launch_bounds__(256) void k_upsample_stack_fwd(const ScaleSet sc, int planes, int h, int w, float* __restrict__ out) {
  const int s = blockIdx.z, pl = blockIdx.y;
  const int hs = sc.hs[s], ws = sc.ws[s];
  const float* __restrict__ src = sc.p[s] + (size_t)pl*hs*ws;
  const float sy = (float)hs/(float)h, sx = (float)ws/(float)w;
  float* __restrict__ o = out + ((size_t)s*planes + pl)*h*w;
  for (int pix = blockIdx.x*256 + threadIdx.x; pix < h*w; pix += gridDim.x*256) {
    const int v = pix/w, u = pix - v*w;
    int y0, y1, x0, x1; float ly, lx;
    up_src_index(v, sy, hs, y0, y1, ly);
    up_src_index(u, sx, ws, x0, x1, lx);
    const float p00 = src[y0*ws + x0], p01 = src[y0*ws + x1], p10 = src[y1*ws + x0], p11 = src[y1*ws + x1];
    o[pix] = (1.f - ly)*((1.f - lx)*p00 + lx*p01) + ly*((1.f - lx)*p10 + lx*p11);
  }
}

hipError_t launch_upsample_stack_fwd(const ScaleSet& sc, int planes, int h, int w, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_upsample_stack_fwd, dim3(min(ceil_div(h*w, 256), 512), planes, sc.S), dim3(256), 0, st, sc, planes, h, w, out);
  return hipGetLastError();
}

struct UpBwdMap { int first_block[SMD_MAX_SCALES + 1]; };

// Output indices whose window can hold source index j (one more on each side than the real-valued bound: the weights decide, the range only has to cover)
__device__ __forceinline__ void up_footprint(int j, float f, int n_lo, int n_hi, int& lo, int& hi) {
  lo = max((int)floorf(((float)j - 0.5f)*f - 0.5f) - 1, 0);
  hi = min((int)ceilf(((float)j + 1.5f)*f - 0.5f) + 1, n_hi - 1);
  if (j == 0) lo = 0;
  if (j == n_lo - 1) hi = n_hi - 1;
}

// grid (blocks of 256 source pixels, all scales in a row: UpBwdMap; planes): g_src[jy][jx] = sum_v wy(v -> jy) sum_u wx(u -> jx) g[v][u]
__global__ __launch_bounds__(256) void k_upsample_stack_bwd(const ScaleSet sc, const UpBwdMap map, int planes, int h, int w, const float* __restrict__ g_out) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < SMD_MAX_SCALES; ++k) if (k < sc.S && (int)blockIdx.x >= map.first_block[k]) s = k;
  const int hs = sc.hs[s], ws = sc.ws[s], pl = blockIdx.y;
  const int lp = ((int)blockIdx.x - map.first_block[s])*256 + threadIdx.x;
  if (lp >= hs*ws) return;
  const float* __restrict__ g = g_out + ((size_t)s*planes + pl)*h*w;
  float* __restrict__ o = sc.g[s] + (size_t)pl*hs*ws;
  if (hs == h && ws == w) { o[lp] = g[lp]; return; }     // identity resampling
  const int jy = lp/ws, jx = lp - jy*ws;
  const float sy = (float)hs/(float)h, sx = (float)ws/(float)w;
  int vlo, vhi, ulo, uhi;
  up_footprint(jy, (float)h/(float)hs, hs, h, vlo, vhi);
  up_footprint(jx, (float)w/(float)ws, ws, w, ulo, uhi);
  float acc = 0.f;
  for (int v = vlo; v <= vhi; ++v) {
    int y0, y1; float ly;
    up_src_index(v, sy, hs, y0, y1, ly);
    const float wy = ((y0 == jy) ? 1.f - ly : 0.f) + ((y1 == jy) ? ly : 0.f);
    if (wy == 0.f) continue;
    const float* __restrict__ row = g + (size_t)v*w;
    float racc = 0.f;
#pragma unroll 4
    for (int u = ulo; u <= uhi; ++u) {
      int x0, x1; float lx;
      up_src_index(u, sx, ws, x0, x1, lx);
      const float wx = ((x0 == jx) ? 1.f - lx : 0.f) + ((x1 == jx) ? lx : 0.f);
      racc = fmaf(wx, row[u], racc);
    }
    acc = fmaf(wy, racc, acc);
  }
  o[lp] = acc;
}

hipError_t launch_upsample_stack_bwd(const ScaleSet& sc, int planes, int h, int w, const float* g_out, hipStream_t st) {
  UpBwdMap m;
  int n = 0;
  for (int s = 0; s < SMD_MAX_SCALES; ++s) {
    m.first_block[s] = n;
    if (s < sc.S) n += ceil_div(sc.hs[s]*sc.ws[s], 256);
  }
  m.first_block[SMD_MAX_SCALES] = n;
  hipLaunchKernelGGL(k_upsample_stack_bwd, dim3(n, planes), dim3(256), 0, st, sc, m, planes, h, w, g_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kMeanPerThread = 16, kMeanPerBlock = 256*kMeanPerThread;

__device__ __forceinline__ int mean_scale_of_block(const MeanSet& ms, int blk) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < SMD_MAX_SCALES; ++k) if (k < ms.S && blk >= ms.first_block[k]) s = k;
  return s;
}

// mode 0: f(x) = -max(log x, -100);  mode 1: f(x) = x, mode 2: f(x) = -x
__device__ __forceinline__ float mean_f(float x, int mode) { return mode == 0 ? -fmaxf(logf(x), -100.f) : (mode == 1 ? x : -x); }
// ATen's binary_cross_entropy_backward with target 1: (x - 1) / max((1 - x) x, 1e-12)
__device__ __forceinline__ float mean_df(float x, int mode) { return mode == 0 ? (x - 1.f)/fmaxf((1.f - x)*x, 1e-12f) : (mode == 1 ? 1.f : -1.f); }

// partial[blk] = the block's sum of f(x); the block that arrives last (counter: zero on entry, zero again on exit) adds the partial sums of each scale in
// fp64 in block order and writes loss = mean_s(sum_s / n_s).
__global__ __launch_bounds__(256) void k_scale_mean_fwd(const MeanSet ms, int mode, float* __restrict__ partial, unsigned* __restrict__ counter, float* __restrict__ loss) {
  __shared__ float red[4];
  __shared__ unsigned last;
  const int s = mean_scale_of_block(ms, blockIdx.x);
  const long long n = ms.n[s], e0 = (long long)((int)blockIdx.x - ms.first_block[s])*kMeanPerBlock + threadIdx.x;
  const float* __restrict__ x = ms.p[s];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kMeanPerThread; ++k) {
    const long long e = e0 + (long long)k*256;
    if (e < n) acc += mean_f(x[e], mode);
  }
  acc = block_sum<Waves::Pairwise, 4>(acc, red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(partial + blockIdx.x, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) ? 1u : 0u;
  }
  __syncthreads();
  if (!last || threadIdx.x >= 64) return;
  __threadfence();
  double total = 0.0;
  for (int k = 0; k < ms.S; ++k) {
    double a = 0.0;
    for (int t = ms.first_block[k] + (int)threadIdx.x; t < ms.first_block[k + 1]; t += 64)
      a += (double)__hip_atomic_load(partial + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    total += a/(double)ms.n[k];
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(total/(double)ms.S);
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_scale_mean_bwd(const MeanSet ms, int mode, const float* __restrict__ g_loss) {
  const int s = mean_scale_of_block(ms, blockIdx.x);
  const long long n = ms.n[s], e0 = (long long)((int)blockIdx.x - ms.first_block[s])*kMeanPerBlock + threadIdx.x;
  const float* __restrict__ x = ms.p[s];
  float* __restrict__ g = ms.g[s];
  const float coef = g_loss[0]/((float)ms.S*(float)n);
#pragma unroll
  for (int k = 0; k < kMeanPerThread; ++k) {
    const long long e = e0 + (long long)k*256;
    if (e < n) g[e] = coef*mean_df(mode == 0 ? x[e] : 0.f, mode);
  }
}

int scale_mean_blocks(MeanSet& ms) {   // fills the block prefix table; -1: more blocks than a grid takes
  long long nb = 0;
  for (int s = 0; s <= SMD_MAX_SCALES; ++s) {
    ms.first_block[s] = (int)nb;
    if (s < ms.S) nb += (ms.n[s] + kMeanPerBlock - 1)/kMeanPerBlock;
    if (nb > 0x7fffffff) return -1;
  }
  return (int)nb;
}

hipError_t launch_scale_mean_fwd(MeanSet ms, int mode, float* partial, unsigned* counter, float* loss, hipStream_t st) {
  const int nb = scale_mean_blocks(ms);
  if (nb < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_scale_mean_fwd, dim3(nb), dim3(256), 0, st, ms, mode, partial, counter, loss);
  return hipGetLastError();
}

hipError_t launch_scale_mean_bwd(MeanSet ms, int mode, const float* g_loss, hipStream_t st) {
  const int nb = scale_mean_blocks(ms);
  if (nb < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_scale_mean_bwd, dim3(nb), dim3(256), 0, st, ms, mode, g_loss);
  return hipGetLastError();
}

}  // namespace smd
