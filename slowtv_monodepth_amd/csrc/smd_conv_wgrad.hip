// smd_conv_wgrad.hip — the weight gradient of the split-bf16 matrix-core 3x3 convolutions (the scheme: smd_conv_mfma.hip; shared stages:
// smd_conv_mfma_dev.h), and the fixed-order fp64 sum of the blocks' partial sets that the stem's weight gradient (smd_conv_stem.hip) uses too.
//
// g_w[co][c][tap] = sum over samples and pixels of g_y[co][y][x] xp[c][y + ky][x + kx]: per tap a GEMM with M = output channels, N = input channels,
// K = pixels.  Both operands want 8 consecutive K per lane = 8 consecutive pixels of a row of one channel: the tensors' own (NCHW) order.  A K step is 16
// pixels of a row (lane group g: pixels 8 g .. + 7); A = g_y, B = the padded input shifted by the tap — the shift by kx is a funnel shift of the five
// dwords a lane reads (shifted_frags).  A wave owns ONE pair (tile of output channels, tile of input channels) and all nine taps.
// The row loop runs over INPUT rows: input row r meets g_y rows r, r - 1, r - 2 as the taps' rows ky = 0, 1, 2.  Two K steps per row of a strip = the two
// waves of a pair, which meet in LDS at the end (pair_reduce_store).  The block leaves its sums as one set of partials [tap][co][c];
// launch_partial_sets_finalize adds the blocks' sets in fp64 in a fixed order (deterministic, as everywhere in this library).
//
// Two geometries (the trait structs below) x two ways of bringing the rows in (one kernel template each):
//
// WgradWide, 32 output x 64 input channels per block on `v_mfma_f32_32x32x16_bf16`, strips of 32 columns, 9 x 16 accumulator registers; four waves =
// 2 input-channel tiles x the 2 K steps.  Register-staged form (k_wgrad_staged, bf16 tensors): the block keeps a ring of four g_y rows (small: 32 channels)
// and only TWO slots of the input row (64 channels: this row, and the next one being filed), an input row's fragments are read once and serve three ky
// (15 LDS reads per 54 MFMAs), and 60 KB of LDS leave room for two blocks per CU; per row it requests one new row of each operand before the row's MFMAs
// and splits + files them after, one barrier per row.
// (First form, round 6: the ring held four INPUT rows of 64-128 channels — 93-143 KB, one block per CU, a lane's five dwords read per ky: 193 us at cfg 2's
// 96 -> 32 layer, the bf16 pipe 37 % busy, 64 % of the LDS cycles bank conflicts of the fifth-dword read.)
// LDS-DMA form (k_wgrad_dma, fp32 tensors; built for the thin stage, see below): a ring of four RAW rows — [64 input channels][36 dwords: 34 columns + 2]
// [32 g_y channels][36: 32 columns + 4], 13.8 KB a slot — three rows in flight per block instead of one; a wave splits its own slice of a row at fragment
// read (10 columns of its input channel, 8 of its g_y channel, the latter also split by the other channel tile's wave) and keeps the g_y fragments of the two
// rows before in registers.
// ZP: xp is the UNPADDED input (B, C, h, w) of a zero-padded layer (the encoders' 3x3 stride-1 convolutions): column col of padded row r is input column
// col - 1 of input row r - 1; columns outside the row carry the out-of-range offset and rows above / below the image an empty buffer resource — the DMA writes
// zeros for both, so the block sees the zero-padded rows without a padded copy of the activation.
// spb > 1 (the coarse layers, see wgrad_shape): a block walks the rows of spb samples one after the other into the same accumulators, switching the buffer
// resources per row it requests; it leaves one set of partials for all of them.
//
// WgradThin<NC>, sixteen output channels (the thin last stage) x 16 NC input channels on `v_mfma_f32_16x16x32_bf16` — a K step is 32 pixels of a row (lane
// group q: pixels 8 q .. + 7), one 16 x 16 accumulator tile per tap (36 registers).  A block walks down a strip of 64 columns: 2 K steps per row x NC tiles of
// 16 input channels = 2 NC waves.  Register-staged form: ring of four g_y rows + two slots of the input row in LDS (40-54 KB: three or four blocks per CU,
// ~100 registers), one barrier per row.  HBM-bound (128-192 B per pixel for 2304-4608 multiply-adds at 6/16 of the f32 MFMA's time).
// (Earlier forms, round 6, 16 -> 16 at 192x640 / 32 -> 16 at 96x320: tiles of 32 x 4 pixels staged through LDS with two barriers per tile 198 / 277 us; fragments
// straight from memory with a rolling register window 138 / 77 — a quarter wave of a fragment load touches 16 channel rows; the f32-MFMA kernel 112 / 76.)
// LDS-DMA form, the thin weight gradient's fourth: the rows reach LDS by LDS-DMA (`buffer_load_dword ... lds`: no staging registers, so a ring of D rows
// costs LDS only and D - 1 rows are in flight per block), RAW; a wave reads its own slice of a row — 10 columns of its input channel, 8 of its g_y channel — and
// splits it in registers (every element is split by exactly one wave of its channel tile; the g_y slice again by each of the NC tiles), keeps the g_y fragments
// of the two rows before in registers for ky = 1, 2.  The third form issued a row's loads at the top of a step and filed them at its bottom: one row (8 KB) in
// flight per block, 3.3 us per row step at 16 -> 16 (the MFMAs of a step are 0.4 us).  One barrier per row, no vector-memory wait but the in-order counter.
// A slot = [C input channels][68 dwords: 66 columns + 2] [16 g_y channels][68: 64 columns + 4] (+ one dummy piece where the pieces do not divide among the waves);
// channel stride 272 B = 16 x 17.  Pieces outside the image (columns past the row, g_y rows past the block) carry an out-of-range offset / an empty resource:
// the DMA writes zeros.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_conv_mfma_dev.h"
#include <algorithm>
#include <type_traits>

namespace smd {

// ---- block geometries ----
// MR: rows = columns of the MFMA tile (lane = MR grp + j); COB / CB: output / input channels of a block; STRIP: columns of a strip = 2 K steps;
// NT: threads, WAVES: the minimum waves per SIMD asked of the compiler; XROW / GROW: dwords of a row slot of the register-staged form's input / g_y
// ring (a channel = 2 / 4 slots + 16 bytes: an odd number of 16-byte units, the 16 lanes of a ds_read_b128 group cover all banks); CS: dwords of a channel's
// row in a slot of the LDS-DMA ring (STRIP + 4: odd in 16-byte units as well); WALKS: a block may walk several samples, TAB: the DMA pieces' offsets are parked
// in LDS (the wide form's accumulators leave no registers for 14 of them).
struct WgradWide {
  typedef f32x16 Acc;
  static constexpr int MR = 32, COB = 32, CB = 64, STRIP = 32, NT = 256, WAVES = 2, XROW = 20, GROW = 16, CS = 36;
  static constexpr bool WALKS = true, TAB = true;
  int C, CO, cg, cog, sg;                                         // channel counts; this block's input-channel group, output-channel group, sample (group)
  __device__ __forceinline__ WgradWide(int C_, int CO_) : C(C_), CO(CO_) {
    const int CGRP = (C + CB - 1)/CB, COGRP = CO/COB;
    cg = blockIdx.z % CGRP; cog = (blockIdx.z/CGRP) % COGRP; sg = blockIdx.z/(CGRP*COGRP);
  }
  static __device__ __forceinline__ int tile(int wv) { return wv & 1; }      // the wave's input-channel tile and K step
  static __device__ __forceinline__ int kstep(int wv) { return wv >> 1; }
  __device__ __forceinline__ int x_channel(int ch) const { return min(cg*CB + ch, C - 1); }   // channel tiles past C: clamped reads, not stored
  __device__ __forceinline__ bool has_channel(int c) const { return c < C; }
  static __device__ __forceinline__ int d_row(int v, int grp) { return mfma32_row(v, grp); }
};
// (Both geometries are built from the kernels' (C, CO) arguments so that one template serves them; the thin one's channel counts are compile-time, it
// ignores the two — and its kernels ignore B and spb, which only a geometry that WALKS reads.)
template <int NC> struct WgradThin {
  typedef f32x4v Acc;
  static constexpr int MR = 16, COB = 16, CB = 16*NC, STRIP = 64, NT = 128*NC, WAVES = 1, XROW = 36, GROW = 32, CS = 68;
  static constexpr bool WALKS = false, TAB = false;
  static constexpr int C = CB, CO = 16, cg = 0, cog = 0;
  int sg;
  __device__ __forceinline__ WgradThin(int, int) : sg(blockIdx.z) {}
  static __device__ __forceinline__ int tile(int wv) { return wv >> 1; }
  static __device__ __forceinline__ int kstep(int wv) { return wv & 1; }
  static __device__ __forceinline__ int x_channel(int ch) { return ch; }
  static __device__ __forceinline__ bool has_channel(int) { return true; }
  static __device__ __forceinline__ int d_row(int v, int grp) { return 4*grp + v; }   // D of the 16x16x32 MFMA: row = 4 (l >> 4) + v
};

// D[row = co][column = c] of tap t: the two K-step waves of a pair meet in LDS, the first writes the block's set of partials
template <typename G>
__device__ __forceinline__ void wgrad_store(const G& geo, float* red, float* __restrict__ partial, int wv, int lane, const typename G::Acc (&acc)[9]) {
  const int j = lane & (G::MR - 1), grp = lane/G::MR, ct = G::tile(wv);
  const size_t blk = ((size_t)geo.sg*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x;
  const int c = geo.cg*G::CB + ct*G::MR + j;
  pair_reduce_store(red, ct, G::kstep(wv) == 1, geo.has_channel(c), lane, acc, [&](int t, int v, float sum) {
    const int co = geo.cog*G::COB + G::d_row(v, grp);
    partial[((blk*9 + t)*geo.CO + co)*geo.C + c] = sum;
  });
}

// ---- rows staged through registers (bf16 tensors; any TI) ----
template <typename G, int P, typename TI>
__global__ __launch_bounds__(G::NT, G::WAVES) void k_wgrad_staged(const TI* __restrict__ xp, const TI* __restrict__ gy, float* __restrict__ partial,
                                                                    int C_, int CO_, int h, int w, int rows_per_block) {
  typedef typename G::Acc Acc;
  constexpr int NT = G::NT, COB = G::COB, CB = G::CB, MR = G::MR, XROW = G::XROW, XCH = 2*XROW + 4, GROW = G::GROW, GCH = 4*GROW + 4;
  constexpr int kXs = P*CB*XCH, kGs = P*COB*GCH;
  constexpr int kRed = (NT/128)*9*(int)(sizeof(Acc)/4)*64;        // the second wave of a pair parks its accumulators
  __shared__ __attribute__((aligned(16))) unsigned lds[(kXs + kGs) > kRed ? (kXs + kGs) : kRed];
  unsigned* const xs = lds;
  unsigned* const gs = lds + kXs;
  const G geo(C_, CO_);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & (MR - 1), grp = lane/MR;
  const int ct = G::tile(wv), kd = G::kstep(wv)*(G::STRIP/4) + grp*4;   // this wave's input-channel tile; its lanes' dword in a row (K step and lane group)
  const int x0 = blockIdx.x*G::STRIP, ybeg = blockIdx.y*rows_per_block, nrows = min(rows_per_block, h - ybeg), b = geo.sg;
  const int W = w + 2, H = h + 2;
  typedef typename RawOf<TI>::type R;
  const R* xsrc = reinterpret_cast<const R*>(xp) + (size_t)b*geo.C*H*W;
  const R* gsrc = reinterpret_cast<const R*>(gy) + ((size_t)b*geo.CO + (size_t)geo.cog*COB)*h*w;

  constexpr int XPR = G::STRIP/2 + 1, GPR = G::STRIP/2;            // an item = two adjacent columns of one channel's row
  constexpr int XITEMS = CB*XPR, XTRIPS = (XITEMS + NT - 1)/NT;
  constexpr int GITEMS = COB*GPR, GTRIPS = GITEMS/NT;
  static_assert(GITEMS % NT == 0, "g_y items per thread");
  R xv[XTRIPS][2], gv[GTRIPS][2];
  auto load_x = [&](int yy) {                                     // padded row yy (clamped: rows past the strip are requested but never used)
    yy = min(yy, H - 1);
#pragma unroll
    for (int t = 0; t < XTRIPS; ++t) {
      const int item = min(t*NT + (int)threadIdx.x, XITEMS - 1);
      const int ch = item/XPR, pr = item - ch*XPR;
      const R* rowp = xsrc + ((size_t)geo.x_channel(ch)*H + yy)*W;
      xv[t][0] = rowp[min(x0 + 2*pr, W - 1)];
      xv[t][1] = rowp[min(x0 + 2*pr + 1, W - 1)];
    }
  };
  auto file_x = [&](int slot) {
#pragma unroll
    for (int t = 0; t < XTRIPS; ++t) {
      const int item = t*NT + (int)threadIdx.x;
      if (item < XITEMS) {
        const int ch = item/XPR, pr = item - ch*XPR;
        unsigned pk[P];
        split_pair<P>(xv[t][0], xv[t][1], pk);
#pragma unroll
        for (int p = 0; p < P; ++p) xs[(p*CB + ch)*XCH + slot*XROW + pr] = pk[p];
      }
    }
  };
  auto load_g = [&](int y) {                                      // beyond the image or the block's rows: zeros, those pixels add nothing
#pragma unroll
    for (int t = 0; t < GTRIPS; ++t) {
      const int item = t*NT + (int)threadIdx.x;
      const int co = item/GPR, pr = item % GPR;
      const int xa = x0 + 2*pr;
      const bool yok = y < ybeg + nrows;
      const R* rowp = gsrc + ((size_t)co*h + (yok ? y : 0))*w;
      gv[t][0] = (yok && xa < w) ? rowp[xa] : R(0);
      gv[t][1] = (yok && xa + 1 < w) ? rowp[xa + 1] : R(0);
    }
  };
  auto file_g = [&](int slot) {
#pragma unroll
    for (int t = 0; t < GTRIPS; ++t) {
      const int item = t*NT + (int)threadIdx.x;
      const int co = item/GPR, pr = item % GPR;
      unsigned pk[P];
      split_pair<P>(gv[t][0], gv[t][1], pk);
#pragma unroll
      for (int p = 0; p < P; ++p) gs[(p*COB + co)*GCH + slot*GROW + pr] = pk[p];
    }
  };

  Acc acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = Acc{};

  // step i = 0 .. nrows + 1 works on padded input row ybeg + i (slot i & 1) against g_y rows ybeg + i - ky (ring slot (i - ky) & 3), ky = 0, 1, 2, where they
  // are rows of this block; g_y rows at or past ybeg + nrows are filed as zeros (load_g), so only the steps before the block's first rows need a guard
  load_x(ybeg); file_x(0);
  load_g(ybeg); file_g(0);
  __syncthreads();
  for (int i = 0; i < nrows + 2; ++i) {
    load_x(ybeg + i + 1);
    load_g(ybeg + i + 1);
    bf16x8 Bx[3][P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const uint4* q = reinterpret_cast<const uint4*>(&xs[(p*CB + ct*MR + j)*XCH + (i & 1)*XROW + kd]);
      const uint4 d = q[0];
      shifted_frags(d.x, d.y, d.z, d.w, q[1].x, Bx[0][p], Bx[1][p], Bx[2][p]);
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      if (i - ky < 0) continue;                                   // (wave-uniform: the block's first two steps)
      bf16x8 A[P];
#pragma unroll
      for (int p = 0; p < P; ++p) A[p] = as_frag(*reinterpret_cast<const uint4*>(&gs[(p*COB + j)*GCH + ((i - ky) & 3)*GROW + kd]));
      split_mfma_sum<P>(A, Bx, &acc[ky*3]);
    }
    file_x((i + 1) & 1);
    file_g((i + 1) & 3);
    __syncthreads();
  }
  wgrad_store(geo, reinterpret_cast<float*>(lds), partial, wv, lane, acc);   // (everybody is past the last barrier of the loop: the rings are free)
}

// ---- rows by LDS-DMA (fp32 tensors) ----
template <typename G, int P, bool ZP>
__global__ __launch_bounds__(G::NT, G::WAVES) void k_wgrad_dma(const float* __restrict__ xp, const float* __restrict__ gy, float* __restrict__ partial,
                                                                 int B, int C_, int CO_, int h, int w, int rows_per_block, int spb) {
  typedef typename G::Acc Acc;
  static_assert(!ZP || G::WALKS, "the zero-padded form exists for the wide geometry");
  constexpr int NT = G::NT, COB = G::COB, CB = G::CB, MR = G::MR, STRIP = G::STRIP, NW = NT/64, CS = G::CS, D = 4;
  constexpr int XDW = CB*CS, GDW = COB*CS, NPX = XDW/64, NPG = GDW/64, NX = (NPX + NW - 1)/NW, NG = (NPG + NW - 1)/NW, NDMA = NX + NG, SLOT = XDW + GDW + 64;
  static_assert(XDW % 64 == 0 && GDW % 64 == 0, "whole DMA pieces per region");
  static_assert((D - 2)*NDMA < 64 && D == 4, "the waits below are immediates of six bits, for a ring of four");
  constexpr int kRing = D*SLOT, kTab = G::TAB ? NW*NDMA*64 : 0, kRed = (NT/128)*9*(int)(sizeof(Acc)/4)*64;
  __shared__ __attribute__((aligned(16))) unsigned lds[(kRing + kTab) > kRed ? (kRing + kTab) : kRed];
  const G geo(C_, CO_);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & (MR - 1), grp = lane/MR;
  const int ct = G::tile(wv), kcol = G::kstep(wv)*(STRIP/2) + grp*8;    // this wave's input-channel tile; its lanes' first column of a row (K step and lane group)
  const int x0 = blockIdx.x*STRIP, ybeg = blockIdx.y*rows_per_block, nrows = min(rows_per_block, h - ybeg);
  // ZP: the input rows -1 and h are zeros.  A block that starts at the top still fetches its step 0 (g_y row 0 is the later steps' ky = 1, 2 operand) but
  // runs no MFMAs there; one that ends at the bottom drops its last step (input row h against g_y rows past the image and h - 1 x zeros) altogether.
  const bool skip0 = ZP && ybeg == 0;
  const int nsteps = nrows + 2 - ((ZP && ybeg + nrows == h) ? 1 : 0);
  // WALKS: samples b0 .. + spb - 1, one after the other: step s = sample s / nsteps, its step s % nsteps
  const int b0 = G::WALKS ? geo.sg*spb : geo.sg, nsteps_all = G::WALKS ? min(spb, B - b0)*nsteps : nsteps;
  const int W = w + 2, H = h + 2;
  const size_t xsample = ZP ? (size_t)geo.C*h*w : (size_t)geo.C*H*W;   // (ZP: unpadded planes)
  [[maybe_unused]] const rsrc_t rs_0 = make_rsrc(xp, 0);          // (ZP: the rows above and below the image — every load out of range, zeros)
  const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned*)lds);

  // piece k of a region = its dwords k 64 .. + 63; this wave takes pieces n NW + wv (a piece that does not exist: zeros into the slot's spare 256 bytes, so
  // that every wave has NX + NG loads in flight per row).  A lane's offset of a piece does not depend on the row: computed once and kept in registers, or
  // (TAB) in LDS behind the ring (the wide accumulators leave no registers for 14 of them, and recomputing them costs every row more vector instructions
  // than splitting its operands), read back by the lane that wrote it — no synchronisation.
  [[maybe_unused]] unsigned voff[G::TAB ? 1 : NDMA];
  [[maybe_unused]] unsigned* const tab = lds + kRing + wv*(NDMA*64) + lane;
  auto keep_offset = [&](int n, unsigned o) { if constexpr (G::TAB) tab[n*64] = o; else voff[n] = o; };
#pragma unroll
  for (int n = 0; n < NX; ++n) {
    const int k = n*NW + wv, d = k*64 + lane, ch = d/CS, col = d - ch*CS, c = geo.cg*CB + ch;
    if constexpr (ZP) keep_offset(n, (k < NPX && col < STRIP + 2 && x0 + col >= 1 && x0 + col <= w && geo.has_channel(c)) ? (unsigned)((c*h)*w + x0 + col - 1)*4u : 0x80000000u);
    else keep_offset(n, (k < NPX && col < STRIP + 2 && x0 + col < W && geo.has_channel(c)) ? (unsigned)((c*H)*W + x0 + col)*4u : 0x80000000u);
  }
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int k = n*NW + wv, d = k*64 + lane, co = d/CS, col = d - co*CS;
    keep_offset(NX + n, (k < NPG && col < STRIP && x0 + col < w) ? (unsigned)((co*h)*w + x0 + col)*4u : 0x80000000u);
  }
  // issue(q) is called for steps q = 0, 1, 2, ... in order, once each: step q's rows -> slot q % D (g_y rows past the block's: a valid row, unused).
  // WALKS: the next step to issue as (sample, step of that sample)
  [[maybe_unused]] int is_b = b0, is_r = 0;
  auto issue = [&](int q) {
    int r = q, b = b0;
    if constexpr (G::WALKS) { r = is_r; b = is_b; if (++is_r == nsteps) { is_r = 0; ++is_b; } }
    const unsigned base = lds0 + (unsigned)((q % D)*SLOT*4);
    const rsrc_t rs_x = make_rsrc(xp + (size_t)b*xsample, xsample*4);
    const rsrc_t rs_g = make_rsrc(gy + ((size_t)b*geo.CO + (size_t)geo.cog*COB)*h*w, (size_t)COB*h*w*4);
    rsrc_t rx = rs_x;
    unsigned sx;
    if constexpr (ZP) {                                           // input row ybeg + r - 1; rows -1 and h are the zero rows
      const int yx = ybeg + r - 1;
      const bool xin = yx >= 0 && yx < h;
      rx = xin ? rs_x : rs_0; sx = xin ? (unsigned)yx*(unsigned)w*4u : 0u;
    } else sx = (unsigned)min(ybeg + r, H - 1)*(unsigned)W*4u;
    const unsigned sg = (unsigned)min(ybeg + r, h - 1)*(unsigned)w*4u;
    unsigned v[NDMA];
#pragma unroll
    for (int n = 0; n < NDMA; ++n) { if constexpr (G::TAB) v[n] = tab[n*64]; else v[n] = voff[n]; }
#pragma unroll
    for (int n = 0; n < NX; ++n) { const int k = n*NW + wv; lds_dma_dword(rx, v[n], sx, base + (unsigned)(k < NPX ? k*256 : (XDW + GDW)*4)); }
#pragma unroll
    for (int n = 0; n < NG; ++n) { const int k = n*NW + wv; lds_dma_dword(rs_g, v[NX + n], sg, base + (unsigned)(k < NPG ? XDW*4 + k*256 : (XDW + GDW)*4)); }
  };

  Acc acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = Acc{};
  bf16x8 A[3][P];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int p = 0; p < P; ++p) A[r][p] = as_frag(uint4{0u, 0u, 0u, 0u});

  // step i of the block (step il of its sample): input row il (slot i % D) against g_y rows il - ky: this row's fragments (a0) and the two rows' before
  // (a1, a2).  A sample's last two steps carry zero g_y fragments (a0 past the block's rows), so the next sample's first two steps find zeros as the "rows
  // before" — the ring needs no reset between samples.
  [[maybe_unused]] int st_r = 0;
  auto step = [&](int i, bf16x8 (&a0)[P], const bf16x8 (&a1)[P], const bf16x8 (&a2)[P]) {
    int il = i;
    if constexpr (G::WALKS) { il = st_r; if (++st_r == nsteps) st_r = 0; }
    // this wave's pieces of step i have landed (the steps requested after it may be in flight: D - 2 of them, fewer at the block's end)
    const int after = min(D - 2, nsteps_all - 1 - i);
    if (after >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2*NDMA) : "memory");
    else if (after == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NDMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                 // ... and everybody's; nobody reads slot (i - 1) % D any more
    asm volatile("" ::: "memory");
    if (i + D - 1 < nsteps_all) issue(i + D - 1);
    const float* slot = reinterpret_cast<const float*>(lds) + (i % D)*SLOT;
    const float* xr = slot + (ct*MR + j)*CS + kcol;
    const float* gr = slot + XDW + j*CS + kcol;
    const float4 x0v = *reinterpret_cast<const float4*>(xr), x1v = *reinterpret_cast<const float4*>(xr + 4);
    const float2 x2v = *reinterpret_cast<const float2*>(xr + 8);
    const float4 g0v = *reinterpret_cast<const float4*>(gr), g1v = *reinterpret_cast<const float4*>(gr + 4);
    unsigned px[5][P], pg[4][P];
    split_pair<P>(x0v.x, x0v.y, px[0]); split_pair<P>(x0v.z, x0v.w, px[1]); split_pair<P>(x1v.x, x1v.y, px[2]); split_pair<P>(x1v.z, x1v.w, px[3]); split_pair<P>(x2v.x, x2v.y, px[4]);
    split_pair<P>(g0v.x, g0v.y, pg[0]); split_pair<P>(g0v.z, g0v.w, pg[1]); split_pair<P>(g1v.x, g1v.y, pg[2]); split_pair<P>(g1v.z, g1v.w, pg[3]);
    bf16x8 Bx[3][P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      shifted_frags(px[0][p], px[1][p], px[2][p], px[3][p], px[4][p], Bx[0][p], Bx[1][p], Bx[2][p]);
      a0[p] = as_frag(il < nrows ? uint4{pg[0][p], pg[1][p], pg[2][p], pg[3][p]} : uint4{0u, 0u, 0u, 0u});   // (past the block's rows: nothing to add)
    }
    if (skip0 && il == 0) return;                                 // (wave-uniform)
    split_mfma_sum<P>(a0, Bx, &acc[0]);
    split_mfma_sum<P>(a1, Bx, &acc[3]);
    split_mfma_sum<P>(a2, Bx, &acc[6]);
  };
#pragma unroll
  for (int r = 0; r < D - 1; ++r) if (!ZP || r < nsteps_all) issue(r);   // (nsteps >= 3, but ZP: h = 1 leaves two steps)
  for (int i = 0; i < nsteps_all; i += 3) {                       // the three roles of A[] rotate: no copies
    step(i, A[0], A[2], A[1]);
    if (i + 1 < nsteps_all) step(i + 1, A[1], A[0], A[2]);
    if (i + 2 < nsteps_all) step(i + 2, A[2], A[1], A[0]);
  }
  __syncthreads();                                                // the ring is free
  wgrad_store(geo, reinterpret_cast<float*>(lds), partial, wv, lane, acc);
}

// ---- the blocks' partial sets -> the result, fp64, fixed order ----
// partial[t][i], t < T sets of n sums each.  Many blocks' sums for few weights (the thin stage: T = 960 sets of 2304): two launches — (1) a block = 64
// sums x one of G slices of the T sets, its four waves every fourth set of the slice, added in wave order -> slice[g][i] (fp64, behind the partials in the
// workspace); (2) the G slices in order, eight loads in flight.  (One launch of ceil(n / 64) blocks over all T sets — 36 blocks reading 8.8 MB — took 67 us
// beside a 47 us kernel.)  Few sets (T < 64: the coarse levels, up to 1.2 M weights): G = 1 and the first launch writes g_w itself.
// TAPS: the sets are [tap][co][c] and g_w is [co][c][tap] (the 3x3 layers); else g_w is in the sets' own order (the stem).
template <bool TAPS> __device__ __forceinline__ size_t set_output_index(int i, SetIndexMap m) {
  if constexpr (!TAPS) return (size_t)i;
  else { const int c = i % m.C, co = (i/m.C) % m.CO, tap = i/(m.C*m.CO); return ((size_t)co*m.C + c)*9 + tap; }
}
template <bool TAPS>
__global__ __launch_bounds__(256) void k_partial_sets_sum1(const float* __restrict__ partial, unsigned T, unsigned G, int n, SetIndexMap m, double* __restrict__ slice, float* __restrict__ g_w) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = blockIdx.x*64 + lane;
  const unsigned g = blockIdx.y, t0 = (unsigned)(((unsigned long long)T*g)/G), t1 = (unsigned)(((unsigned long long)T*(g + 1))/G);
  double s = 0.0;
  if (i < n) for (unsigned t = t0 + wv; t < t1; t += 4) s += (double)partial[(size_t)t*n + i];
  part[wv][lane] = s;
  __syncthreads();
  if (wv == 0 && i < n) {
    const double tot = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    if (G == 1) g_w[set_output_index<TAPS>(i, m)] = (float)tot; else slice[(size_t)g*n + i] = tot;
  }
}
template <bool TAPS>
__global__ __launch_bounds__(256) void k_partial_sets_sum2(const double* __restrict__ slice, unsigned G, int n, SetIndexMap m, float* __restrict__ g_w) {
  const int i = blockIdx.x*256 + threadIdx.x;
  if (i >= n) return;
  double tot = 0.0;
  unsigned g = 0;
  for (; g + 8 <= G; g += 8) {                                     // eight loads in flight, added in order
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = slice[(size_t)(g + k)*n + i];
#pragma unroll
    for (int k = 0; k < 8; ++k) tot += v[k];
  }
  for (; g < G; ++g) tot += slice[(size_t)g*n + i];
  g_w[set_output_index<TAPS>(i, m)] = (float)tot;
}
static unsigned partial_set_slices(unsigned T) { return T < 64 ? 1u : std::min(32u, T/16); }
// floats of workspace: T sets of n, then the fp64 slices (G = 1: the first launch writes g_w directly, none).  T n must be even (the slices are 8-byte aligned)
size_t partial_sets_floats(unsigned T, size_t n) {
  const unsigned G = partial_set_slices(T);
  return (size_t)T*n + (G > 1 ? 2*(size_t)G*n : 0);
}
template <bool TAPS>
static void partial_sets_finalize(float* partial, unsigned T, int n, SetIndexMap m, float* g_w, hipStream_t st) {
  const unsigned G = partial_set_slices(T);
  double* slice = reinterpret_cast<double*>(partial + (size_t)T*n);
  hipLaunchKernelGGL(k_partial_sets_sum1<TAPS>, dim3(ceil_div(n, 64), G), dim3(256), 0, st, partial, T, G, n, m, slice, g_w);
  if (G > 1) hipLaunchKernelGGL(k_partial_sets_sum2<TAPS>, dim3(ceil_div(n, 256)), dim3(256), 0, st, slice, G, n, m, g_w);
}
hipError_t launch_partial_sets_finalize(float* partial, unsigned T, int n, SetIndexMap m, float* g_w, hipStream_t st) {
  if (m.CO > 0) partial_sets_finalize<true>(partial, T, n, m, g_w, st); else partial_sets_finalize<false>(partial, T, n, m, g_w, st);
  return hipGetLastError();
}

// ---- launch shapes ----
// spb: samples per block.  multi (the fp32 LDS-DMA form): where every block already takes a whole sample's rows and one block per sample would need more
// than one generation (the coarse layers: 256 - 512 channels at 12 x 40 / 6 x 20), a block walks the rows of several samples, one after the other, into the
// same accumulators — the partial sums (9 CO C floats each, written and read back by the finalize) then number strips x sample groups instead of
// strips x B.  Only groupings that still fill both block slots of every CU (>= 512 blocks) are taken: a lone block on a CU runs its rows hardly faster
// than a pair does (measured: 288 blocks of two samples at 24 x 80 b = 24, 141 us against 116 for 576 blocks of one).  Among those, the fewest
// (blocks per CU x (steps per block + the block's epilogue, about four steps)).
static void wgrad_shape(int B, int C, int CO, int h, int w, dim3& grid, int& rows, int& spb, bool multi) {
  const int cgs = ceil_div(C, 64)*(CO/32), strips = ceil_div(w, 32), base = strips*B*cgs;
  const int groups = std::max(1, std::min(512/std::max(base, 1), ceil_div(h, 12)));  // two blocks per CU: about one generation of equal blocks where the layer allows; at least
                                                                                      // twelve rows per block (a block runs two steps more than it has rows, then reduces and writes 9 x 32 x 64 sums)
  rows = ceil_div(h, groups);
  spb = 1;
  if (multi && rows == h && base > 512) {
    const long long per = (long long)strips*cgs;
    long long best = -1;
    for (int s = 1; s <= B; ++s) {
      const long long nsg = ceil_div(B, s), cost = ceil_div(nsg*per, 256ll)*(s*(h + 2) + 4);
      if (s > 1 && nsg*per < 512) break;
      if (best < 0 || cost < best) { best = cost; spb = s; }
    }
  }
  grid = dim3(strips, ceil_div(h, rows), ceil_div(B, spb)*cgs);
}
static void wgrad16_shape(int B, int C, int h, int w, dim3& grid, int& rows) {
  const int strips = ceil_div(w, 64);
  const long long units = (long long)strips*B, slots = C == 16 ? 1024 : 768;   // strips of 64 columns; ONE generation of blocks (four / three per CU), at least twelve rows per block
  const int groups = (int)std::max(1ll, std::min<long long>(ceil_div(h, 12), slots/units));
  rows = ceil_div(h, groups);
  grid = dim3(strips, ceil_div(h, rows), B);
}
// the number of partial-sum sets the weight gradient leaves (multi: the fp32 form whose blocks walk several samples)
static unsigned wgrad_sets(int B, int C, int CO, int h, int w, bool multi) {
  dim3 grid; int rows, spb = 1;
  if (CO == 16) wgrad16_shape(B, C, h, w, grid, rows); else wgrad_shape(B, C, CO, h, w, grid, rows, spb, multi);
  return grid.x*grid.y*(unsigned)ceil_div(B, spb);
}
// floats of workspace: the blocks' partial sums, then the finalize's fp64 slices (the padded form's bfloat16 path keeps one sample per block: the larger size)
size_t conv_mfma_wgrad_partials(bool zpad, int B, int C, int CO, int h, int w) { return partial_sets_floats(wgrad_sets(B, C, CO, h, w, zpad), (size_t)9*CO*C); }

// ---- launches ----
// g_w (CO, C, 3, 3) fp32: CO % 32 == 0, any C >= 1 (channel tiles past C are computed on clamped reads and not stored); or CO == 16 with C == 16 | 32.
// fp32 tensors (P = 3, or the experiment's 2; ZP: fp32 only): the LDS-DMA form; bfloat16 tensors (P = 1): the register-staged form
template <typename G, int P, bool ZP, typename T>
static void launch_wgrad_geo(const T* xp, const T* gy, float* partial, dim3 grid, int B, int C, int CO, int h, int w, int rows, int spb, hipStream_t st) {
  if constexpr (std::is_same<T, float>::value) hipLaunchKernelGGL((k_wgrad_dma<G, P, ZP>), grid, dim3(G::NT), 0, st, xp, gy, partial, B, C, CO, h, w, rows, spb);
  else hipLaunchKernelGGL((k_wgrad_staged<G, P, T>), grid, dim3(G::NT), 0, st, xp, gy, partial, C, CO, h, w, rows);
}
template <int P, bool ZP, typename T>
static void launch_wgrad(const void* xp_, const void* gy_, float* partial, int B, int C, int CO, int h, int w, hipStream_t st) {
  const T* xp = (const T*)xp_; const T* gy = (const T*)gy_;
  dim3 grid; int rows, spb = 1;
  if (!ZP && CO == 16) {
    wgrad16_shape(B, C, h, w, grid, rows);
    if (C == 16) launch_wgrad_geo<WgradThin<1>, P, false, T>(xp, gy, partial, grid, B, C, CO, h, w, rows, spb, st);
    else launch_wgrad_geo<WgradThin<2>, P, false, T>(xp, gy, partial, grid, B, C, CO, h, w, rows, spb, st);
    return;
  }
  wgrad_shape(B, C, CO, h, w, grid, rows, spb, std::is_same<T, float>::value);
  launch_wgrad_geo<WgradWide, P, ZP, T>(xp, gy, partial, grid, B, C, CO, h, w, rows, spb, st);
}
hipError_t launch_conv_mfma_bwd_wgt(const void* xp, const void* gy, float* g_w, float* partial, bool zpad, int B, int C, int CO, int h, int w, int pieces, hipStream_t st) {
  if (zpad) {
    if (pieces == 3) launch_wgrad<3, true, float>(xp, gy, partial, B, C, CO, h, w, st); else launch_wgrad<2, true, float>(xp, gy, partial, B, C, CO, h, w, st);
  } else if (pieces == 3) launch_wgrad<3, false, float>(xp, gy, partial, B, C, CO, h, w, st);
  else if (pieces == 2) launch_wgrad<2, false, float>(xp, gy, partial, B, C, CO, h, w, st);
  else launch_wgrad<1, false, bf16>(xp, gy, partial, B, C, CO, h, w, st);
  return launch_partial_sets_finalize(partial, wgrad_sets(B, C, CO, h, w, zpad || pieces != 1), 9*CO*C, SetIndexMap{CO, C}, g_w, st);
}

}  // namespace smd
