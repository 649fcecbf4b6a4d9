// smd_conv_stem.hip — the ResNet stem, conv2d(x (B,C,H,W), w (64,C,7,7), stride 2, padding 3), on the bf16 matrix cores with fp32-class results: every fp32
// operand split exactly into three bf16 pieces, six `v_mfma_f32_32x32x16_bf16` per K step of 16 (the scheme of smd_conv_mfma.hip; helpers in smd_split_dev.h and smd_conv_mfma_dev.h).
// C = 3 (the depth network's stem) and C = 6 (the pose network's); zero padding inside the kernels, NCHW fp32 in and out, any H, W >= 1.  No data gradient:
// the input is the image.
//
// Forward: implicit GEMM, M = 64 output channels, N = output pixels, K = (c, ky, kx padded 7 -> 8).  With 3 or 6 channels the "16 channels of a pixel
// contiguous" order of k_conv_mfma does not exist; here a lane's eight K slots are eight consecutive input COLUMNS of one row (c, ky), starting at
// 2 x - 3 — a K step of 16 is two such rows (lanes 0-31 row 2 s, lanes 32-63 row 2 s + 1), K = 8 ceil(7 C / 2) 2 = 176 / 336.  A block of four waves owns
// 4 output rows x 64 columns (a wave per row: two pixel fragments x two channel tiles, hi / lo accumulators) and stages the 13 x 134 x C input patch once,
// split, two columns a dword: the B operand is four consecutive dwords from dword x of the patch row whatever ky (4-byte aligned: plain ds_read_b32,
// stride-1 over the lanes).  Weight fragments come whole from k_stem_pack_w's image, one K step ahead.
//
// Weight gradient: GEMM with K = output pixels, M = 64 output channels (A = dL/dy, eight consecutive pixels of a row: the tensor's own order), N = the
// 49 C weights of an output channel (c, ky, kx) — lane column n reads input columns 2 x - 3 + kx, x = eight consecutive output pixels: a stride of two.
// The staged input rows are therefore filed DE-INTERLEAVED, even columns and odd columns apart, and a lane's fragment is eight consecutive elements of
// the plane kx selects, from an element offset that depends on kx: five dwords and a funnel shift.  A block walks a band of output rows of a strip of 64
// columns of one sample: per output row one row of dL/dy (64 channels x 64 pixels, split at filing) and TWO new input rows per channel into a ring of eight
// (output row y meets input rows 2 y - 3 .. 2 y + 3); loads for the next row are requested before the row's MFMAs and filed after.  Wave = one tile of 32
// output channels x every second tile of 32 weight columns.  Blocks leave partial sets in the weight's own order; launch_partial_sets_finalize (smd_conv_wgrad.hip) adds them in fp64 in a fixed order.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_conv_mfma_dev.h"
#include <algorithm>

namespace smd {

namespace {

template <int C> struct StemFwd {
  static constexpr int NI = 7*C, NS = (NI + 1)/2;           // operand rows (c, ky); K steps of two rows each
  static constexpr int PR = 13, PD = 67, PITCH = 68;        // patch rows, dwords (column pairs) staged per row, row pitch in dwords
  static constexpr int PLANE = C*PR*PITCH, ITEMS = C*PR*PD;
};

// w (64, C, 7, 7) -> A fragments [channel tile][K step][piece][lane]: lane l = row co & 31 of operand row i = 2 s + (l >> 5), slots kx = 0 .. 7 (kx = 7 and
// the row past 7 C: zeros)
template <int C>
__global__ __launch_bounds__(256) void k_stem_pack_w(const float* __restrict__ w, uint4* __restrict__ wp) {
  using T = StemFwd<C>;
  const int idx = blockIdx.x*256 + threadIdx.x;
  if (idx >= 2*T::NS*64) return;
  const int lane = idx & 63, s = (idx >> 6) % T::NS, mt = idx/(64*T::NS);
  const int i = 2*s + (lane >> 5), co = mt*32 + (lane & 31);
  float v[8];
#pragma unroll
  for (int kx = 0; kx < 8; ++kx) v[kx] = (i < T::NI && kx < 7) ? w[((size_t)co*T::NI + i)*7 + kx] : 0.f;
  unsigned pk[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) split_pair<3>(v[2*q], v[2*q + 1], pk[q]);
#pragma unroll
  for (int p = 0; p < 3; ++p) wp[((size_t)(mt*T::NS + s)*3 + p)*64 + lane] = uint4{pk[0][p], pk[1][p], pk[2][p], pk[3][p]};
}

template <int C>
__global__ __launch_bounds__(256, 2) void k_stem_fwd(const float* __restrict__ x, const uint4* __restrict__ wp, float* __restrict__ y, int H, int W, int ho, int wo) {
  using T = StemFwd<C>;
  constexpr int NS = T::NS, NI = T::NI, PR = T::PR, PD = T::PD, PITCH = T::PITCH, PLANE = T::PLANE, ITEMS = T::ITEMS;
  __shared__ __attribute__((aligned(16))) unsigned xs[3*PLANE];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  const int x0 = blockIdx.x*64, y0 = blockIdx.y*4, b = blockIdx.z;
  const float* xb = x + (size_t)b*C*H*W;

  // the patch: rows 2 y0 - 3 .. + 12, columns 2 x0 - 3 .. + 133, zeros outside the image
  for (int base = 0; base < ITEMS; base += 1024) {
    float v[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int item = base + u*256 + (int)threadIdx.x;
      const int d = item % PD, r = (item/PD) % PR, c = item/(PD*PR);
      const int gy = 2*y0 - 3 + r, gx = 2*x0 - 3 + 2*d;
      const bool ok = item < ITEMS && gy >= 0 && gy < H;
      v[u][0] = (ok && gx >= 0 && gx < W) ? xb[((size_t)c*H + gy)*W + gx] : 0.f;
      v[u][1] = (ok && gx + 1 >= 0 && gx + 1 < W) ? xb[((size_t)c*H + gy)*W + gx + 1] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int item = base + u*256 + (int)threadIdx.x;
      if (item < ITEMS) {
        const int d = item % PD, rc = item/PD;               // rc = c PR + r
        unsigned pk[3];
        split_pair<3>(v[u][0], v[u][1], pk);
#pragma unroll
        for (int p = 0; p < 3; ++p) xs[p*PLANE + rc*PITCH + d] = pk[p];
      }
    }
  }
  __syncthreads();

  f32x16 acc[2][2], lo[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[mt][nf][r] = 0.f; lo[mt][nf][r] = 0.f; }

  const uint4* wl = wp + lane;
  uint4 an[2][3];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int p = 0; p < 3; ++p) an[mt][p] = wl[((mt*NS + 0)*3 + p)*64];
#pragma unroll                                                    // (all 11 / 21 K steps: every patch address is then an immediate)
  for (int s = 0; s < NS; ++s) {
    bf16x8 A[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int p = 0; p < 3; ++p) A[mt][p] = as_frag(an[mt][p]);
    const int sn = min(s + 1, NS - 1);                         // (the last step requests its own fragments again)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int p = 0; p < 3; ++p) an[mt][p] = wl[((mt*NS + sn)*3 + p)*64];
    const int i = min(2*s + g, NI - 1);                        // (the row past 7 C meets zero weights: any finite data)
    const int c = i/7, ky = i - 7*c;
    const unsigned* row = xs + (c*PR + 2*wv + ky)*PITCH + j;
    bf16x8 Bf[2][3];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const unsigned* q = row + p*PLANE + nf*32;
        Bf[nf][p] = as_frag(uint4{q[0], q[1], q[2], q[3]});
      }
    split_mfma<3>(A, Bf, acc, lo);
  }

  const int yy = y0 + wv;
  if (yy >= ho) return;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int xx = x0 + nf*32 + j;
      if (xx < wo) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = mt*32 + mfma32_row(r, g);
          y[(((size_t)b*64 + co)*ho + yy)*wo + xx] = acc[mt][nf][r] + lo[mt][nf][r];
        }
      }
    }
}

template <int C> struct StemWgrad {
  static constexpr int NW = 49*C, NT = (NW + 31)/32, NTW = (NT + 1)/2;   // weights of an output channel; tiles of 32 of them; tiles per wave
  static constexpr int XP = 34, GP = 36;                                 // dwords: a de-interleaved half row (68 elements); a dL/dy row of 64 pixels + 16 bytes
  static constexpr int XPLANE = C*8*2*XP, GPLANE = 64*GP;
  static constexpr int XITEMS = C*2*XP, XTR = (XITEMS + 255)/256;        // an item = four adjacent columns of one of two input rows
};

template <int C>
__global__ __launch_bounds__(256, 2) void k_stem_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ partial,
                                                       int H, int W, int ho, int wo, int rows_per_block) {
  using T = StemWgrad<C>;
  constexpr int NW = T::NW, NT = T::NT, NTW = T::NTW, XP = T::XP, GP = T::GP, XPLANE = T::XPLANE, GPLANE = T::GPLANE, XITEMS = T::XITEMS, XTR = T::XTR;
  constexpr int NPROD = n_products(3);
  __shared__ __attribute__((aligned(16))) unsigned xs[3*XPLANE];          // [piece][c][ring slot = input row & 7][even | odd columns][XP]
  __shared__ __attribute__((aligned(16))) unsigned gs[3*GPLANE];          // [piece][co][GP]
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  const int mt = wv & 1, nh = wv >> 1;
  const int x0 = blockIdx.x*64, ybeg = blockIdx.y*rows_per_block, nrows = min(rows_per_block, ho - ybeg), b = blockIdx.z;
  const float* xb = x + (size_t)b*C*H*W;
  const float* gb = gy + (size_t)b*64*ho*wo;

  // Patch column pc = input column 2 x0 - 4 + pc; even plane E[m] = pc 2 m, odd plane O[m] = pc 2 m + 1.  Output pixel x0 + xl meets, for kx, input column
  // 2 xl + 1 + kx of the patch: kx even -> O[xl + kx / 2], kx odd -> E[xl + (kx + 1) / 2]: element offset sh = (kx + 1) >> 1 in the plane ~kx & 1.
  int xoff[NTW], sh[NTW], kyv[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int n = min((nh + 2*i)*32 + j, NW - 1);
    const int c = n/49, rem = n - 49*c, ky = rem/7, kx = rem - 7*ky;
    xoff[i] = (c*16 + ((kx & 1) ^ 1))*XP; sh[i] = (kx + 1) >> 1; kyv[i] = ky;
  }

  float xv[XTR][4], gv[4][4];
  auto load_x = [&](int ir0) {                                            // input rows ir0, ir0 + 1
#pragma unroll
    for (int t = 0; t < XTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int d = item % XP, rr = (item/XP) & 1, c = item/(2*XP);
      const int ir = ir0 + rr, gc = 2*x0 - 4 + 4*d;
      const bool ok = item < XITEMS && ir >= 0 && ir < H;
#pragma unroll
      for (int k = 0; k < 4; ++k) xv[t][k] = (ok && gc + k >= 0 && gc + k < W) ? xb[((size_t)c*H + ir)*W + gc + k] : 0.f;
    }
  };
  auto file_x = [&](int ir0) {
#pragma unroll
    for (int t = 0; t < XTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      if (item < XITEMS) {
        const int d = item % XP, rr = (item/XP) & 1, c = item/(2*XP);
        const int slot = (ir0 + rr + 8) & 7;
        unsigned pe[3], po[3];
        split_pair<3>(xv[t][0], xv[t][2], pe);
        split_pair<3>(xv[t][1], xv[t][3], po);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          xs[p*XPLANE + ((c*8 + slot)*2 + 0)*XP + d] = pe[p];
          xs[p*XPLANE + ((c*8 + slot)*2 + 1)*XP + d] = po[p];
        }
      }
    }
  };
  auto load_g = [&](int yy) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int co = item >> 4, xa = x0 + 4*(item & 15);
#pragma unroll
      for (int k = 0; k < 4; ++k) gv[t][k] = (xa + k < wo) ? gb[((size_t)co*ho + yy)*wo + xa + k] : 0.f;
    }
  };
  auto file_g = [&]() {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int co = item >> 4, q = item & 15;
      unsigned p0[3], p1[3];
      split_pair<3>(gv[t][0], gv[t][1], p0);
      split_pair<3>(gv[t][2], gv[t][3], p1);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        gs[p*GPLANE + co*GP + 2*q] = p0[p];
        gs[p*GPLANE + co*GP + 2*q + 1] = p1[p];
      }
    }
  };

  f32x16 acc[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // rows 2 ybeg - 4 .. 2 ybeg + 3 (the first only fills its slot), dL/dy row ybeg
  for (int k = 0; k < 4; ++k) { load_x(2*ybeg - 4 + 2*k); file_x(2*ybeg - 4 + 2*k); }
  load_g(ybeg); file_g();
  __syncthreads();
  for (int r = 0; r < nrows; ++r) {
    const int yy = ybeg + r;
    const bool more = r + 1 < nrows;
    if (more) { load_x(2*yy + 4); load_g(yy + 1); }
    unsigned rowa[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) rowa[i] = (unsigned)(xoff[i] + ((2*yy + 5 + kyv[i]) & 7)*2*XP);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 A[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) A[p] = as_frag(*reinterpret_cast<const uint4*>(&gs[p*GPLANE + (mt*32 + j)*GP + ks*8 + g*4]));
#pragma unroll
      for (int i = 0; i < NTW; ++i) {
        if (nh + 2*i >= NT) continue;                                     // (wave-uniform)
        const int e = ks*16 + g*8 + sh[i];
        const unsigned* q = xs + rowa[i] + (e >> 1);
        const unsigned s16 = (unsigned)(e & 1)*16u;
        bf16x8 Bf[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const unsigned d0 = q[p*XPLANE], d1 = q[p*XPLANE + 1], d2 = q[p*XPLANE + 2], d3 = q[p*XPLANE + 3], d4 = q[p*XPLANE + 4];
          Bf[p] = as_frag(uint4{__builtin_amdgcn_alignbit(d1, d0, s16), __builtin_amdgcn_alignbit(d2, d1, s16),
                                __builtin_amdgcn_alignbit(d3, d2, s16), __builtin_amdgcn_alignbit(d4, d3, s16)});
        }
#pragma unroll
        for (int t = 0; t < NPROD; ++t) acc[i] = mfma_bf16(A[prod_a(3, t)], Bf[prod_b(3, t)], acc[i]);
      }
    }
    __syncthreads();
    if (more) { file_x(2*yy + 4); file_g(); }
    __syncthreads();
  }

  const size_t blk = ((size_t)b*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x;
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int nt = nh + 2*i, n = nt*32 + j;
    if (nt < NT && n < NW) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = mt*32 + mfma32_row(r, g);
        partial[(blk*64 + co)*NW + n] = acc[i][r];
      }
    }
  }
}

// strips of 64 columns x bands of rows x samples: about one generation of blocks at two per CU, at least eight rows a block
void stem_wgrad_shape(int B, int ho, int wo, dim3& grid, int& rows) {
  const int strips = ceil_div(wo, 64);
  const long long units = (long long)strips*B;
  const int groups = (int)std::max(1ll, std::min<long long>(ceil_div(ho, 8), 512/std::max(units, 1ll)));
  rows = ceil_div(ho, groups);
  grid = dim3(strips, ceil_div(ho, rows), B);
}

}  // namespace

bool conv_stem_served(int C, int CO) { return CO == 64 && (C == 3 || C == 6); }
size_t conv_stem_packed_bytes(int C) { return (size_t)2*((7*C + 1)/2)*3*1024; }
size_t conv_stem_wgrad_floats(int B, int C, int H, int W) {
  dim3 grid; int rows;
  stem_wgrad_shape(B, (H - 1)/2 + 1, (W - 1)/2 + 1, grid, rows);
  return partial_sets_floats(grid.x*grid.y*grid.z, (size_t)64*49*C);
}
hipError_t launch_conv_stem_pack(const float* w, void* wp, int C, hipStream_t st) {
  const int n = 2*((7*C + 1)/2)*64;
  if (C == 3) hipLaunchKernelGGL(k_stem_pack_w<3>, dim3(ceil_div(n, 256)), dim3(256), 0, st, w, (uint4*)wp);
  else hipLaunchKernelGGL(k_stem_pack_w<6>, dim3(ceil_div(n, 256)), dim3(256), 0, st, w, (uint4*)wp);
  return hipGetLastError();
}
hipError_t launch_conv_stem_fwd(const float* x, const void* wp, float* y, int B, int C, int H, int W, hipStream_t st) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  const dim3 grid(ceil_div(wo, 64), ceil_div(ho, 4), B);
  if (C == 3) hipLaunchKernelGGL(k_stem_fwd<3>, grid, dim3(256), 0, st, x, (const uint4*)wp, y, H, W, ho, wo);
  else hipLaunchKernelGGL(k_stem_fwd<6>, grid, dim3(256), 0, st, x, (const uint4*)wp, y, H, W, ho, wo);
  return hipGetLastError();
}
hipError_t launch_conv_stem_bwd_wgt(const float* x, const float* gy, float* g_w, float* partial, int B, int C, int H, int W, hipStream_t st) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1, n = 64*49*C;
  dim3 grid; int rows;
  stem_wgrad_shape(B, ho, wo, grid, rows);
  if (C == 3) hipLaunchKernelGGL(k_stem_wgrad<3>, grid, dim3(256), 0, st, x, gy, partial, H, W, ho, wo, rows);
  else hipLaunchKernelGGL(k_stem_wgrad<6>, grid, dim3(256), 0, st, x, gy, partial, H, W, ho, wo, rows);
  return launch_partial_sets_finalize(partial, grid.x*grid.y*grid.z, n, SetIndexMap{}, g_w, st);   // the sets are in the weight's own order
}

}  // namespace smd
