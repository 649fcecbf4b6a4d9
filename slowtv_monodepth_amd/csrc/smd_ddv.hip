// smd_ddv.hip — the output head of the DDVNet decoder, fused (reference: src/networks/decoders/ddvnet.py:110, 116-124, 147-150):
//     logits = conv3x3(x)  (128 bins per output channel);  disp = sum_k softmax(logits)_k k/128.
// ATen writes the logit volume (b = 12 at 192 x 640: 755 MB for a 24 MB input and a 6 MB output), re-reads and rewrites it in the softmax and reads it
// again in the multiply and the sum.  Here the volume never leaves the registers: the convolution is the split-bf16 matrix-core scheme of
// smd_conv_mfma.hip through the stages of smd_conv_mfma_dev.h (same packed weights — `k_conv_pack_w`'s forward image —, same LDS patch with the same bank swizzle, six
// `v_mfma_f32_32x32x16_bf16` per K step with the leading product and the five small ones in accumulators of their own) and the epilogue reduces over
// the bins.  D of that MFMA is [row = output channel][column = pixel] with a lane holding 16 rows of one column (row = mfma32_row):
// a wave multiplies its pixels by ALL 128 bins of one group (four channel tiles), so a lane ends with 64 of a pixel's 128 logits in registers and lane ^ 32
// with the other 64 — maximum, sum and weighted sum are in-register loops plus one exchange between the wave's halves.  No atomics anywhere.
// A block of four waves owns 4 rows x 64 columns of one sample and one group: a wave = one row = two pixel fragments x four channel tiles = 8 + 8
// accumulators (256 registers: one wave per SIMD).  Every weight fragment a wave fetches (L1 / L2 hits: every block reads the same ones) serves two
// pixel fragments, every patch fragment four channel tiles.
// The backward recomputes the logits with the same loop and writes g_logit[k] = p_k (k/128 - disp) g_disp from the saved row maximum and reciprocal sum;
// the convolution's two gradient GEMMs then run on g_logits through the routed operators (ddv_ops.py).  The bias gradient is the plane sums of g_logits
// in a fixed order (k_ddv_bias_*), bit-reproducible from run to run.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_conv_mfma_dev.h"

namespace smd {

namespace {

constexpr int kDdvBins = 128;
struct DdvTile {
  static constexpr int TC = 64, TRB = 4, PW = TC + 2, PH = TRB + 2, NPIX = PW*PH;
};

template <bool BWD>
__global__ __launch_bounds__(256, 1) void k_ddv_head(const float* __restrict__ xp, const uint4* __restrict__ wp, const float* __restrict__ bias,
                                                     float* __restrict__ disp, float* __restrict__ stats, const float* __restrict__ g_disp,
                                                     float* __restrict__ g_logits, int C, int G, int h, int w, unsigned gx, unsigned gy, unsigned nblk) {
  using T = DdvTile;
  constexpr int P = 3, NPIX = T::NPIX, PW = T::PW, NMT = kDdvBins/32;
  __shared__ uint4 tile[P*NPIX*2];                                // one patch, [piece][pixel][half] (38 KB)
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  // XCD-aware block order: the blocks in flight on an XCD are neighbours in the image (and the groups of one tile)
  const unsigned lid = xcd_block_id(nblk);
  if (lid >= nblk) return;
  const int gi = (int)(lid % (unsigned)G);
  const unsigned tl = lid/(unsigned)G;
  const int x0 = (int)(tl % gx)*T::TC, y0 = (int)((tl/gx) % gy)*T::TRB, b = (int)(tl/(gx*gy));
  const int hi = h + 2, wi = w + 2, KC = C >> 4;
  const size_t plane = (size_t)hi*wi;
  const float* src = xp + (size_t)b*C*plane;

  // staging: as in k_conv_mfma (beyond the image: any valid address, those outputs are not stored)
  using Stage = PatchStager<256, NPIX, P, float, false>;
  Stage stage;
  stage.template rect_offsets<PW>(y0, x0, 0, hi, wi);
  float v[Stage::TRIPS][8];
  auto request = [&](int kc) { stage.request(src, plane, kc, v); };
  auto file = [&]() { stage.file(tile, 0, v); };

  f32x16 acc[NMT][2], lo[NMT][2];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[mt][nt][r] = 0.f; lo[mt][nt][r] = 0.f; }

  // weight fragments one tap ahead; tap t >= 1 of a chunk sits in slot t & 1, tap 0 in slot 2 (requested behind tap 8 of the chunk before: every index static)
  bf16x8 A[3][NMT][P];
  const uint4* wq = wp + ((size_t)(gi*NMT)*KC*9*P)*64 + lane;
  auto fetch_a = [&](bf16x8 (&dst)[NMT][P], int kc, int tap) {
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int p = 0; p < P; ++p) dst[mt][p] = as_frag(wq[((((size_t)mt*KC + kc)*9 + tap)*P + p)*64]);
  };
  auto read_b = [&](bf16x8 (&dst)[2][P], int tap) {
    const int ky = tap/3, kx = tap % 3;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      Stage::read(tile, 0, (wv + ky)*PW + nt*32 + j + kx, g, dst[nt]);
    }
  };

  request(0);
  fetch_a(A[2], 0, 0);
  file();
  __syncthreads();
  for (int kc = 0; kc < KC; ++kc) {
    const bool more = kc + 1 < KC;
    if (more) request(kc + 1);                                    // lands behind this chunk's MFMAs
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      bf16x8 Bf[2][P];
      read_b(Bf, tap);
      if (tap < 8) fetch_a(A[(tap + 1) & 1], kc, tap + 1);
      else if (more) fetch_a(A[2], kc + 1, 0);
      split_mfma<P>(A[tap == 0 ? 2 : (tap & 1)], Bf, acc, lo);
    }
    if (more) {
      __syncthreads();                                            // nobody reads this patch any more
      file();
      __syncthreads();
    }
  }

  // epilogue: the lane's 64 bins of pixel (y, x) are k = 32 mt + (r & 3) + 8 (r >> 2) + 4 g; lane ^ 32 holds the other 64
  const int M = kDdvBins*G;
  const float* bz = bias + gi*kDdvBins;
  const size_t hw = (size_t)h*w;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int y = y0 + wv, x = x0 + nt*32 + j;
    const bool ok = y < h && x < w;
    const size_t po = ((size_t)b*G + gi)*hw + (size_t)min(y, h - 1)*w + min(x, w - 1);                  // (b, gi, y, x) of a (B, G, h, w) map
    const size_t so = (((size_t)b*G + gi)*2)*hw + (size_t)min(y, h - 1)*w + min(x, w - 1);           // (b, gi, 0, y, x) of the stats
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = (acc[mt][nt][r] + lo[mt][nt][r]) + bz[32*mt + mfma32_row(r, g)];
    if constexpr (!BWD) {
      float m = acc[0][nt][0];
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[mt][nt][r]);
      m = fmaxf(m, __shfl_xor(m, 32));
      float s = 0.f, ts = 0.f;                                    // every exponent <= 0, the row's maximum contributes 1: s >= 1
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = expf(acc[mt][nt][r] - m);
          s += e;
          ts = fmaf(e, (float)(32*mt + mfma32_row(r, g))*(1.f/kDdvBins), ts);
        }
      s += __shfl_xor(s, 32);                                     // (a + b and b + a are the same float: both halves hold the same sums)
      ts += __shfl_xor(ts, 32);
      if (ok && g == 0) {
        disp[po] = ts/s;
        stats[so] = m;
        stats[so + hw] = 1.f/s;
      }
    } else {
      const float m = stats[so], rinv = stats[so + hw], d = disp[po], gd = g_disp[po];
      if (ok) {
        float* dst = g_logits + (((size_t)b*M + (size_t)gi*kDdvBins)*h + y)*w + x;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = 32*mt + mfma32_row(r, g);
            const float p = expf(acc[mt][nt][r] - m)*rinv;
            dst[(size_t)k*hw] = p*((float)k*(1.f/kDdvBins) - d)*gd;  // a register is 32 consecutive pixels of one bin per half wave (128-byte runs)
          }
      }
    }
  }
}

// g_bias[co] = sum over samples and pixels of g_logits[b][co]: a block sums one plane (a thread its stride of it, then a tree in LDS), the second kernel
// adds the samples' sums in order — every order fixed
__global__ __launch_bounds__(256) void k_ddv_bias_plane(const float* __restrict__ g_logits, float* __restrict__ partial, size_t hw) {
  __shared__ float red[256];
  const float* p = g_logits + ((size_t)blockIdx.y*gridDim.x + blockIdx.x)*hw;    // plane (b = blockIdx.y, co = blockIdx.x)
  float s = 0.f;
  for (size_t i = threadIdx.x; i < hw; i += 256) s += p[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int n = 128; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) red[threadIdx.x] += red[threadIdx.x + n];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)blockIdx.x*gridDim.y + blockIdx.y] = red[0];
}

__global__ __launch_bounds__(256) void k_ddv_bias_final(const float* __restrict__ partial, float* __restrict__ g_bias, int M, int B) {
  const int co = blockIdx.x*256 + threadIdx.x;
  if (co >= M) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (double)partial[(size_t)co*B + b];
  g_bias[co] = (float)s;
}

unsigned ddv_blocks(int B, int G, int h, int w, unsigned& gx, unsigned& gy) {
  gx = (unsigned)ceil_div(w, DdvTile::TC); gy = (unsigned)ceil_div(h, DdvTile::TRB);
  return gx*gy*(unsigned)B*(unsigned)G;
}

}  // namespace

// (B <= 65535: the samples are gridDim.y of k_ddv_bias_plane)
bool ddv_head_sizes_ok(int B, int C, int G, int h, int w) {
  if (B < 1 || B > 65535 || C < 16 || C > 4096 || C % 16 || G < 1 || G > 4 || h < 1 || w < 1) return false;
  if ((size_t)(h + 2)*(size_t)(w + 2) >= ((size_t)1 << 31)) return false;                       // offsets inside a plane are ints
  const size_t nblk = (size_t)ceil_div(w, DdvTile::TC)*(size_t)ceil_div(h, DdvTile::TRB)*(size_t)B*(size_t)G;
  return nblk < ((size_t)1 << 31) - 8;
}

size_t ddv_head_bias_partials(int B, int G) { return (size_t)B*(size_t)(kDdvBins*G); }

hipError_t launch_ddv_head_fwd(const float* xp, const void* wp, const float* bias, float* disp, float* stats, int B, int C, int G, int h, int w, hipStream_t st) {
  unsigned gx, gy;
  const unsigned nblk = ddv_blocks(B, G, h, w, gx, gy);
  hipLaunchKernelGGL(k_ddv_head<false>, dim3((nblk + 7)/8*8), dim3(256), 0, st, xp, (const uint4*)wp, bias, disp, stats, (const float*)nullptr, (float*)nullptr,
                     C, G, h, w, gx, gy, nblk);
  return hipGetLastError();
}

hipError_t launch_ddv_head_bwd_logits(const float* xp, const void* wp, const float* bias, const float* disp, const float* stats, const float* g_disp,
                                      float* g_logits, float* g_bias, float* partial, int B, int C, int G, int h, int w, hipStream_t st) {
  unsigned gx, gy;
  const unsigned nblk = ddv_blocks(B, G, h, w, gx, gy);
  hipLaunchKernelGGL(k_ddv_head<true>, dim3((nblk + 7)/8*8), dim3(256), 0, st, xp, (const uint4*)wp, bias, const_cast<float*>(disp), const_cast<float*>(stats),
                     g_disp, g_logits, C, G, h, w, gx, gy, nblk);
  if (hipError_t e = hipGetLastError()) return e;
  if (g_bias) {
    const int M = kDdvBins*G;
    hipLaunchKernelGGL(k_ddv_bias_plane, dim3(M, B), dim3(256), 0, st, g_logits, partial, (size_t)h*w);
    hipLaunchKernelGGL(k_ddv_bias_final, dim3(ceil_div(M, 256)), dim3(256), 0, st, partial, g_bias, M, B);
  }
  return hipGetLastError();
}

}  // namespace smd
