// smd_conv_s2.hip — the ResNet encoders' transition convolutions, conv2d(x (B,C,H,W), w (CO,C,3,3), stride 2, padding 1) (`conv1` of the first BasicBlock
// of layer2 / layer3 / layer4), forward, data gradient and weight gradient on the bf16 matrix cores with fp32-class results: every fp32 operand split exactly into three
// bf16 pieces, six `v_mfma_f32_32x32x16_bf16` per K step of 16 (the scheme: smd_conv_mfma.hip; the arithmetic: smd_split_dev.h; the shared stages:
// smd_conv_mfma_dev.h).  Zero padding inside the kernels, NCHW fp32 in and out, any H, W >= 1: Ho = (H - 1)/2 + 1, Wo = (W - 1)/2 + 1.
// A file of its own: the stride-1 kernels of smd_conv_mfma.hip / smd_conv_wgrad.hip are not touched and compile to the instructions they had.
//
// Forward: the implicit GEMM of k_conv_mfma (M = 32 output channels, N = 32-pixel fragments, K = 16 channels x 9 taps; the weights are
// smd_conv3x3_mfma_pack's forward image, fragments four taps ahead, the next chunk's patch requested after tap 4 and filed behind taps 6 - 8).  What differs:
//  - A block's tile is TR x TCW outputs with TR TCW <= 64 (two fragments, pixels in row-major order of the tile: a fragment may span several tile rows), chosen
//    per layer by s2_tile for the most useful pixels per block: 4 x 16 at 24 x 80, 3 x 20 at 12 x 40 and 6 x 20 (94 - 100 % useful).  Its patch is
//    (2 TR + 1) x (2 TCW + 1) inputs, at most 388 pixels — 73.5 KB for two patches of three pieces, two blocks per CU.
//  - A lane's B fragment of tap (ky, kx) sits at patch pixel (2 r + ky, 2 c + kx): a pixel stride of TWO over the lanes, for which the half-swap by bit 3 of
//    the pixel index (patch_slot) was not made — the 16 lanes that serve a ds_read_b128 together would cover 32 of the 64 banks.  So a patch row is filed
//    DE-INTERLEAVED, its TCW + 1 even columns first and its TCW odd columns behind them (as the stem's weight gradient files its rows): tap kx reads plane
//    kx & 1 from index c + (kx >> 1), consecutive pixels for consecutive lanes, and patch_slot's bank analysis holds as it stands.
//  - A staged pixel feeds 9/4 taps instead of 9, so the patch is staged once for FOUR channel tiles: the four waves of a block multiply the same two
//    fragments by the weights of four tiles of 32 output channels (k_conv_mfma: one channel tile, a wave per pixel row).  Where CO is no multiple of 128 the
//    waves past CO recompute the last tile and store nothing.
//  - Few blocks (the coarse levels): K is split over blocks in whole chunks, the partial outputs are added in split order (k_s2_split_sum): deterministic.
//
// Weight gradient: per tap a GEMM with K = output pixels, M = output channels (A = dL/dy: eight consecutive pixels of a row), N = input channels (B = the
// input at columns 2 o + kx - 1: a stride of two).  A block owns 64 output x 64 input channels and a strip of 32 output columns (two K steps) and walks
// output rows; its four waves are 2 x 2 tiles of 32 x 32, each with its nine taps' accumulators (no pair reduction).  Per output row it stages ONE row of
// dL/dy and TWO new input rows (row 2 r + 1 is kept for row r + 1: a ring of three), split at filing, the input rows de-interleaved: even patch columns and
// odd ones apart, two bf16 a dword, so that kx = 0 is four aligned dwords of the even plane, kx = 1 four of the odd plane and kx = 2 the even plane's five
// dwords funnel-shifted by one element.  The next row's loads are requested before the row's MFMAs and filed after them.  Rows -1 and H, columns -1 and W,
// channels past C / CO are filed as zeros.  Blocks leave partial sets [tap][co][c]; launch_partial_sets_finalize adds them in fp64 in a fixed order — no
// atomic add, no zeroing pass.  A block may walk several samples (spb) into the same accumulators where the layer has more blocks than a generation needs.
//
// Data gradient: by the parity of the input pixel, four stride-1 convolutions over dL/dy with 1, 2, 2 and 4 taps — nine per 2 x 2 input CELL, no zero
// insertion.  Input row 2 r meets tap ky = 1 at output row r; row 2 r + 1 meets ky = 0 at r + 1 and ky = 2 at r; columns alike.  An implicit GEMM with M = 32
// input channels (A: smd_conv3x3_mfma_pack's data-gradient image, m = c, k = co, tap slot 8 - (3 ky + kx)), N = a fragment of 32 cells, K = 16 output channels
// x the class's taps.  A block's tile is TR x TCW cells (<= 64, s2d_tile: 4 x 16 at 24 x 80, 6 x 10 at 12 x 40 and 6 x 20), its patch (TR + 1) x (TCW + 1)
// pixels of dL/dy (<= 128: one staging trip, 24 KB for two patches), zero outside dL/dy: consecutive lanes read consecutive patch pixels at every tap, so
// nothing is de-interleaved.  The four waves are two channel tiles x two cell fragments (a staged patch feeds four wave tiles; C = 64 has two channel
// tiles); a wave keeps the four classes' accumulators of its fragment (4 x (hi + lo) x 16 registers) and runs the nine (tap, class) products of a chunk
// grouped by the patch pixel they read, two classes interleaved.  A lane holds columns 2 c and 2 c + 1 of its rows: one 8-byte store each where W is even,
// contiguous over the wave; the last odd row / column of an odd H / W does not exist and is not stored.  The coarse levels split K as the forward does
// (k_s2_split_sum, split order: deterministic), but only under one block per CU: the partial gradients are four times the forward's partial outputs.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_conv_mfma_dev.h"
#include <algorithm>
#include <type_traits>

namespace smd {

namespace {

constexpr int kS2Pix = 388;                                       // the largest patch: 3 x 129 (TR = 1, TCW = 64) = 387

// ---- forward ----
template <int P>
__global__ __launch_bounds__(256, 2) void k_conv_s2_fwd(const float* __restrict__ x, const uint4* __restrict__ wp, float* __restrict__ out,
                                                        int CK, int M, int H, int W, int ho, int wo, int TR, int TCW, int KS, int kc_per_split,
                                                        size_t split_stride, unsigned gx, unsigned gy, unsigned gz) {
  constexpr int NPIX = kS2Pix, kBuf = P*NPIX*2;
  __shared__ uint4 tile[2*kBuf];                                  // two patches, [piece][pixel][half]
  const int lane = threadIdx.x & 63, wall = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  const int MT = M >> 5, MG = (MT + 3) >> 2;                      // channel tiles; groups of four of them
  const unsigned nblk = (unsigned)(MG*KS)*gx*gy*gz, lid = xcd_block_id(nblk);
  if (lid >= nblk) return;
  const int mg_own = (int)(lid % MG)*4 + wall, mg = min(mg_own, MT - 1), ks = (lid/MG) % KS;   // (a wave past CO: the last tile again, not stored)
  const unsigned tl = lid/(MG*KS);
  const int x0 = (int)(tl % gx)*TCW, y0 = (int)((tl/gx) % gy)*TR, b = (int)(tl/(gx*gy));
  const int PW = 2*TCW + 1, PWH = TCW + 1, NP = (2*TR + 1)*PW;    // a patch row: PWH even columns, then TCW odd ones
  const int KC = CK >> 4, kc0 = ks*kc_per_split, kc1 = min(KC, kc0 + kc_per_split);
  const size_t plane = (size_t)H*W;
  const float* src = x + (size_t)b*CK*plane;

  // this lane's pixel of fragment nt: pixel nt 32 + j of the tile in row-major order -> its patch pixel at tap (0, 0), or none
  int lbase[2];
  bool have[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int p = nt*32 + j, r = p/TCW, c = p - r*TCW;
    have[nt] = p < TR*TCW && y0 + r < ho && x0 + c < wo;
    lbase[nt] = have[nt] ? 2*r*PW + c : 0;
  }

  using Stage = PatchStager<256, NPIX, P, float, true>;
  constexpr int TRIPS = Stage::TRIPS;
  Stage stage;
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {                               // patch pixel -> (row, plane, index) -> input pixel; outside the image or past the patch: zeros
    const int item = Stage::item(t), half = item >= NPIX ? 1 : 0, pix = item - half*NPIX;
    const int rp = pix/PW, q = pix - rp*PW, col = q < PWH ? 2*q : 2*(q - PWH) + 1;
    const int yy = 2*y0 + rp - 1, xx = 2*x0 + col - 1;
    stage.pofs[t] = (pix < NP && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy*W + xx : -1;
  }
  float v[TRIPS][8];
  auto request = [&](int kc) { stage.request(src, plane, kc, v); };
  auto file_trip = [&](int buf, int t) { stage.file_trip(tile, buf, t, v); };

  f32x16 acc[2], lo[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[nt][r] = 0.f; lo[nt][r] = 0.f; }

  // the order of requests and waits is k_conv_mfma's (see there): weight fragments in five slots four taps ahead, the patch's fragments one tap ahead
  bf16x8 A[5][P], Bf[2][2][P];
  const uint4* wq = wp + ((size_t)mg*KC*9*P)*64 + lane;
  auto fetch_a = [&](bf16x8 (&dst)[P], int kc, int tap) {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = as_frag(wq[(size_t)((kc*9 + tap)*P + p)*64]);
  };
  auto read_b = [&](bf16x8 (&dst)[2][P], int buf, int tap) {
    const int ky = tap/3, kx = tap % 3;
    const int d = ky*PW + (kx & 1)*PWH + (kx >> 1);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) Stage::read(tile, buf, lbase[nt] + d, g, dst[nt]);
  };
  auto chunk = [&](int kc, int cur, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    read_b(Bf[0], cur, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 8) read_b(Bf[(tap + 1) & 1], cur, tap + 1);
      split_mfma<P>(A[tap % 5], Bf[tap & 1], acc, lo);
      if (tap <= 4) fetch_a(A[(tap + 4) % 5], kc, tap + 4);
      else if (MORE && tap >= 6) fetch_a(A[tap - 6], kc + 1, tap - 6);
      if (MORE && tap == 8) fetch_a(A[3], kc + 1, 3);
      if (MORE && tap == 4) request(kc + 1);
      if (MORE && tap >= 6) {
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) if (t*3/TRIPS == tap - 6) file_trip(cur ^ 1, t);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                              // the other patch is complete, and nobody reads this one any more
  };

  if (kc0 < kc1) {
    request(kc0);
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) fetch_a(A[tap], kc0, tap);
    stage.file(tile, 0, v);
  }
  __syncthreads();
  int kc = kc0;
  for (; kc + 1 < kc1; ++kc) chunk(kc, (kc - kc0) & 1, std::true_type{});
  if (kc < kc1) chunk(kc, (kc - kc0) & 1, std::false_type{});

  if (mg_own >= MT) return;
  float* dst = out + (size_t)ks*split_stride;                     // (KS > 1: `out` is the workspace the splits' sum reads)
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    if (!have[nt]) continue;
    const int p = nt*32 + j, r = p/TCW, c = p - r*TCW;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int m = mg*32 + mfma32_row(rr, g);
      dst[(((size_t)b*M + m)*ho + y0 + r)*wo + x0 + c] = acc[nt][rr] + lo[nt][rr];
    }
  }
}

// y = the sum of the K splits' partial outputs, in split order
__global__ __launch_bounds__(256) void k_s2_split_sum(const float* __restrict__ part, float* __restrict__ out, size_t n4, int KS) {
  const size_t i = (size_t)blockIdx.x*256 + threadIdx.x;
  if (i >= n4) return;
  const f4* p = reinterpret_cast<const f4*>(part);
  f4 s = p[i];
  for (int k = 1; k < KS; ++k) s += p[(size_t)k*n4 + i];
  reinterpret_cast<f4*>(out)[i] = s;
}

// The tile of a layer: TR x TCW outputs, TR TCW <= 64, the patch within kS2Pix: the most useful pixels per block, then the smallest patch, then the widest
void s2_tile(int ho, int wo, int& TR, int& TCW) {
  double best = -1.0; int best_patch = 0;
  TR = 1; TCW = 1;
  for (int tcw = std::min(wo, 64); tcw >= 1; --tcw) {
    int tr = std::min(64/tcw, ho);
    while (tr > 1 && (2*tr + 1)*(2*tcw + 1) > kS2Pix) --tr;
    const int patch = (2*tr + 1)*(2*tcw + 1);
    const double useful = (double)ho*wo/((double)ceil_div(ho, tr)*ceil_div(wo, tcw)*64.0);
    if (useful > best + 1e-9 || (useful > best - 1e-9 && patch < best_patch)) { best = useful; best_patch = patch; TR = tr; TCW = tcw; }
  }
}
struct S2Shape { int TR, TCW, KS, kcs; unsigned gx, gy, gz; dim3 grid; size_t out_elems; };
S2Shape s2_fwd_shape(int B, int C, int CO, int ho, int wo) {
  S2Shape s;
  s2_tile(ho, wo, s.TR, s.TCW);
  s.gx = ceil_div(wo, s.TCW); s.gy = ceil_div(ho, s.TR); s.gz = B;
  const int KC = C >> 4, MG = ceil_div(CO >> 5, 4);
  const long long base = (long long)s.gx*s.gy*s.gz*MG;
  int ks = 1;
  if (base < 384) ks = (int)std::min<long long>(std::max(KC/2, 1), (512 + base - 1)/base);   // under 1.5 blocks per CU: split K, at least two chunks per split
  s.kcs = ceil_div(KC, ks); s.KS = ceil_div(KC, s.kcs);
  s.grid = dim3(8*(unsigned)ceil_div(base*s.KS, 8ll));
  s.out_elems = (size_t)B*CO*ho*wo;
  return s;
}

// ---- weight gradient ----
struct S2W {
  static constexpr int CB = 64, COB = 64, STRIP = 32, P = 3;
  static constexpr int XO = 20, XCH = 36;                         // dwords: the odd plane's start in a channel's row (the even plane: 17 dwords), a channel's row
  static constexpr int GCH = 20;                                  // a dL/dy row of 32 pixels + 16 bytes (XCH, GCH: odd numbers of 16-byte units)
  static constexpr int XROW = CB*XCH, XPIECE = 3*XROW, GPIECE = COB*GCH;   // a ring slot of one piece; a piece's ring of three; a piece's dL/dy row
  static constexpr int XITEMS = CB*2*17, XTR = (XITEMS + 255)/256;         // an item = four adjacent patch columns of one of two input rows of a channel
  static constexpr int GTR = COB*8/256;                                    // an item = four adjacent pixels of a channel's dL/dy row
};

__global__ __launch_bounds__(256, 1) void k_conv_s2_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ partial,
                                                          int B, int C, int CO, int H, int W, int ho, int wo, int rows_per_block, int spb) {
  using T = S2W;
  constexpr int P = T::P, XO = T::XO, XCH = T::XCH, GCH = T::GCH, XROW = T::XROW, XPIECE = T::XPIECE, GPIECE = T::GPIECE, XTR = T::XTR, GTR = T::GTR;
  __shared__ __attribute__((aligned(16))) unsigned xs[P*XPIECE];  // [piece][ring slot][c][even plane | odd plane]
  __shared__ __attribute__((aligned(16))) unsigned gs[P*GPIECE];  // [piece][co][GCH]
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  const int ct = wv & 1, cot = wv >> 1;
  const int CG = ceil_div(C, T::CB), COG = ceil_div(CO, T::COB);
  const int cg = blockIdx.z % CG, cog = (blockIdx.z/CG) % COG, sg = blockIdx.z/(CG*COG);
  const int x0 = blockIdx.x*T::STRIP, ybeg = blockIdx.y*rows_per_block, nrows = min(rows_per_block, ho - ybeg);
  const int b0 = sg*spb, nb = min(spb, B - b0);
  const size_t xplane = (size_t)H*W, gplane = (size_t)ho*wo;

  // Patch column pc = input column 2 x0 - 1 + pc, pc = 0 .. 64: even plane E[m] = pc 2 m (33 elements), odd plane O[m] = pc 2 m + 1 (32).  Output pixel
  // x0 + xl meets input column 2 xl + kx of the patch: kx = 0 -> E[xl], kx = 1 -> O[xl], kx = 2 -> E[xl + 1].
  float xv[XTR][4], gv[GTR][4];
  auto load_x = [&](const float* xb, int ir0) {                   // input rows ir0, ir0 + 1 of this block's 64 channels
#pragma unroll
    for (int t = 0; t < XTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int d = item % 17, rr = (item/17) & 1, ch = item/34, c = cg*T::CB + ch;
      const int ir = ir0 + rr, gc = 2*x0 - 1 + 4*d;
      const bool ok = item < T::XITEMS && c < C && ir >= 0 && ir < H;
      const float* rowp = xb + ((size_t)min(c, C - 1)*H + max(min(ir, H - 1), 0))*W;
#pragma unroll
      for (int k = 0; k < 4; ++k) xv[t][k] = (ok && gc + k >= 0 && gc + k < W) ? rowp[gc + k] : 0.f;
    }
  };
  auto file_x = [&](int ir0, bool both) {                         // rows ir0 (where `both`), ir0 + 1 -> ring slots (row + 1) mod 3
#pragma unroll
    for (int t = 0; t < XTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int d = item % 17, rr = (item/17) & 1, ch = item/34;
      if (item < T::XITEMS && (both || rr == 1)) {
        const int slot = (ir0 + rr + 4) % 3;
        unsigned pe[P], po[P];
        split_pair<P>(xv[t][0], xv[t][2], pe);
        split_pair<P>(xv[t][1], xv[t][3], po);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          unsigned* row = xs + p*XPIECE + slot*XROW + ch*XCH;
          row[d] = pe[p];
          if (d < 16) row[XO + d] = po[p];
        }
      }
    }
  };
  auto load_g = [&](const float* gb, int yy) {
#pragma unroll
    for (int t = 0; t < GTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int chn = item >> 3, co = cog*T::COB + chn, xa = x0 + 4*(item & 7);
      const float* rowp = gb + ((size_t)min(co, CO - 1)*ho + yy)*wo;
#pragma unroll
      for (int k = 0; k < 4; ++k) gv[t][k] = (co < CO && xa + k < wo) ? rowp[xa + k] : 0.f;
    }
  };
  auto file_g = [&]() {
#pragma unroll
    for (int t = 0; t < GTR; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      const int chn = item >> 3, q = item & 7;
      unsigned p0[P], p1[P];
      split_pair<P>(gv[t][0], gv[t][1], p0);
      split_pair<P>(gv[t][2], gv[t][3], p1);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        gs[p*GPIECE + chn*GCH + 2*q] = p0[p];
        gs[p*GPIECE + chn*GCH + 2*q + 1] = p1[p];
      }
    }
  };

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int s = 0; s < nb; ++s) {
    const float* xb = x + (size_t)(b0 + s)*C*xplane;
    const float* gb = gy + (size_t)(b0 + s)*CO*gplane;
    // rows 2 ybeg - 1, 2 ybeg, 2 ybeg + 1 and dL/dy row ybeg (nobody reads the rings: the block's start, or behind the last row's second barrier)
    load_x(xb, 2*ybeg - 2); file_x(2*ybeg - 2, false);
    load_x(xb, 2*ybeg); file_x(2*ybeg, true);
    load_g(gb, ybeg); file_g();
    __syncthreads();
    for (int r = 0; r < nrows; ++r) {
      const int yy = ybeg + r;
      const bool more = r + 1 < nrows;
      if (more) { load_x(xb, 2*yy + 2); load_g(gb, yy + 1); }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kd = ks*8 + g*4;                                // this lane group's first dword (eight pixels = four dwords) of the K step
        bf16x8 A[P];
#pragma unroll
        for (int p = 0; p < P; ++p) A[p] = as_frag(*reinterpret_cast<const uint4*>(&gs[p*GPIECE + (cot*32 + j)*GCH + kd]));
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int slot = (2*yy + ky) % 3;                       // input row 2 yy + ky - 1
          bf16x8 Bx[3][P];
#pragma unroll
          for (int p = 0; p < P; ++p) {
            const unsigned* row = xs + p*XPIECE + slot*XROW + (ct*32 + j)*XCH;
            const uint4 e = *reinterpret_cast<const uint4*>(row + kd);
            const unsigned e4 = row[kd + 4];
            Bx[0][p] = as_frag(e);
            Bx[1][p] = as_frag(*reinterpret_cast<const uint4*>(row + XO + kd));
            Bx[2][p] = as_frag(uint4{__builtin_amdgcn_alignbit(e.y, e.x, 16), __builtin_amdgcn_alignbit(e.z, e.y, 16),
                                     __builtin_amdgcn_alignbit(e.w, e.z, 16), __builtin_amdgcn_alignbit(e4, e.w, 16)});
          }
          split_mfma_sum<P>(A, Bx, &acc[ky*3]);
        }
      }
      __syncthreads();                                            // nobody reads rows 2 yy - 1, 2 yy or the dL/dy row any more
      if (more) { file_x(2*yy + 2, true); file_g(); }
      __syncthreads();
    }
  }

  // D[row = co][column = c] of tap t -> this block's region of its set [tap][co][c]
  const size_t blk = ((size_t)sg*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x;
  const int c = cg*T::CB + ct*32 + j;
  if (c < C) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cog*T::COB + cot*32 + mfma32_row(r, g);
        if (co < CO) partial[((blk*9 + t)*CO + co)*C + c] = acc[t][r];
      }
  }
}

// strips of 32 output columns x bands of rows x sample groups x channel groups: about a generation of blocks (one per CU) where the layer allows, at least six
// rows per block; where one block per sample and channel group is more than two generations, a block walks spb samples
void s2_wgrad_shape(int B, int C, int CO, int ho, int wo, dim3& grid, int& rows, int& spb) {
  const int cgs = ceil_div(C, S2W::CB)*ceil_div(CO, S2W::COB), strips = ceil_div(wo, S2W::STRIP);
  const long long base = (long long)strips*B*cgs;
  const int groups = (int)std::max(1ll, std::min<long long>(256/std::max(base, 1ll), ceil_div(ho, 6)));
  rows = ceil_div(ho, groups);
  spb = 1;
  if (rows == ho && base > 512) spb = (int)std::min<long long>(B, base/256);
  grid = dim3(strips, ceil_div(ho, rows), ceil_div(B, spb)*cgs);
}
unsigned s2_wgrad_sets(int B, int C, int CO, int ho, int wo) {
  dim3 grid; int rows, spb;
  s2_wgrad_shape(B, C, CO, ho, wo, grid, rows, spb);
  return grid.x*grid.y*(unsigned)ceil_div(B, spb);
}

// ---- data gradient ----
constexpr int kS2DPix = 128;                                      // the largest patch: 2 x 64 (TR = 1, TCW = 63); one staging trip of 256 items

// The nine (tap, class) products of a chunk in the order they run, grouped by the patch pixel they read: B00 = (r, c) serves steps 0 - 3, B01 = (r, c + 1)
// steps 4 - 5, B10 = (r + 1, c) steps 6 - 7, B11 = (r + 1, c + 1) step 8.  Step -> the tap slot of the data-gradient image (slot 8 - (3 ky + kx) holds
// w[co][c][ky][kx]) and the class 2 (y & 1) + (x & 1) whose accumulator it feeds:
//   step        0      1      2      3      4      5      6      7      8
//   (ky, kx)  (1,1)  (1,2)  (2,1)  (2,2)  (1,0)  (2,0)  (0,1)  (0,2)  (0,0)
//   slot        4      3      1      0      5      2      7      6      8
//   class       0      1      2      3      1      3      2      3      3
__device__ __forceinline__ constexpr int s2d_slot(int s) { return (int)((0x867250134ull >> (4*s)) & 15); }

// two tiles, each with operands of its own: product t of both before product t + 1 of either (split_mfma's order and accumulators)
template <int P>
__device__ __forceinline__ void split_mfma_two(const bf16x8 (&A0)[P], const bf16x8 (&B0)[P], f32x16& acc0, f32x16& lo0,
                                               const bf16x8 (&A1)[P], const bf16x8 (&B1)[P], f32x16& acc1, f32x16& lo1) {
  constexpr int NPROD = n_products(P);
#pragma unroll
  for (int t = 0; t < NPROD; ++t) {
    if (t == NPROD - 1) { acc0 = mfma_bf16(A0[0], B0[0], acc0); acc1 = mfma_bf16(A1[0], B1[0], acc1); }
    else {
      lo0 = mfma_bf16(A0[prod_a(P, t)], B0[prod_b(P, t)], lo0);
      lo1 = mfma_bf16(A1[prod_a(P, t)], B1[prod_b(P, t)], lo1);
    }
  }
}

template <int P>
__global__ __launch_bounds__(256, 2) void k_conv_s2_bwd_data(const float* __restrict__ gy, const uint4* __restrict__ wp, float* __restrict__ out,
                                                             int CK, int M, int H, int W, int ho, int wo, int TR, int TCW, int KS, int kc_per_split,
                                                             size_t split_stride, unsigned gx, unsigned gyb, unsigned gz) {
  constexpr int NPIX = kS2DPix, kBuf = P*NPIX*2;
  __shared__ uint4 tile[2*kBuf];                                  // two patches, [piece][pixel][half]: 24 KB
  const int lane = threadIdx.x & 63, wall = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, g = lane >> 5;
  const int MT = (M + 31) >> 5, MG = (MT + 1) >> 1;               // tiles of 32 input channels; pairs of them
  const unsigned nblk = (unsigned)(MG*KS)*gx*gyb*gz, lid = xcd_block_id(nblk);
  if (lid >= nblk) return;
  const int nf = wall & 1;                                        // the wave's fragment of 32 cells; its channel tile (past C: the last tile again, not stored)
  const int mt_own = (int)(lid % MG)*2 + (wall >> 1), mt = min(mt_own, MT - 1), ks = (lid/MG) % KS;
  const unsigned tl = lid/(MG*KS);
  const int c0 = (int)(tl % gx)*TCW, r0 = (int)((tl/gx) % gyb)*TR, b = (int)(tl/(gx*gyb));
  const int PW = TCW + 1, NP = (TR + 1)*PW;
  const int KC = CK >> 4, kc0 = ks*kc_per_split, kc1 = min(KC, kc0 + kc_per_split);
  const size_t plane = (size_t)ho*wo;
  const float* src = gy + (size_t)b*CK*plane;

  // this lane's cell: cell nf 32 + j of the tile in row-major order -> its patch pixel (r, c), or none
  const int p = nf*32 + j, r = p/TCW, c = p - r*TCW;
  const bool have = p < TR*TCW && r0 + r < ho && c0 + c < wo;
  const int lbase = have ? r*PW + c : 0;

  using Stage = PatchStager<256, NPIX, P, float, true>;
  constexpr int TRIPS = Stage::TRIPS;
  Stage stage;
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {                               // patch pixel (rp, q) = dL/dy pixel (r0 + rp, c0 + q); outside dL/dy or past the patch: zeros
    const int item = Stage::item(t), half = item >= NPIX ? 1 : 0, pix = item - half*NPIX;
    const int rp = pix/PW, q = pix - rp*PW;
    const int yy = r0 + rp, xx = c0 + q;
    stage.pofs[t] = (pix < NP && yy < ho && xx < wo) ? yy*wo + xx : -1;
  }
  float v[TRIPS][8];
  auto request = [&](int kc) { stage.request(src, plane, kc, v); };

  f32x16 acc[4], lo[4];                                           // per class 2 (y & 1) + (x & 1)
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) { acc[q][rr] = 0.f; lo[q][rr] = 0.f; }

  // weight fragments in five slots (step s in A[s % 5]), steps 0 - 3 of a chunk fetched during the chunk before; the patch's four fragments in two slots
  bf16x8 A[5][P], Bf[2][P];
  const uint4* wq = wp + ((size_t)mt*KC*9*P)*64 + lane;
  auto fetch_a = [&](bf16x8 (&dst)[P], int kc, int s) {
#pragma unroll
    for (int pc = 0; pc < P; ++pc) dst[pc] = as_frag(wq[(size_t)((kc*9 + s2d_slot(s))*P + pc)*64]);
  };
  auto read_b = [&](bf16x8 (&dst)[P], int buf, int d) { Stage::read(tile, buf, lbase + d, g, dst); };
  auto chunk = [&](int kc, int cur, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    read_b(Bf[0], cur, 0);
    read_b(Bf[1], cur, 1);
    split_mfma_two<P>(A[0], Bf[0], acc[0], lo[0], A[1], Bf[0], acc[1], lo[1]);              // steps 0, 1
    fetch_a(A[4], kc, 4); fetch_a(A[0], kc, 5);
    __builtin_amdgcn_sched_barrier(0);
    split_mfma_two<P>(A[2], Bf[0], acc[2], lo[2], A[3], Bf[0], acc[3], lo[3]);              // steps 2, 3
    fetch_a(A[1], kc, 6); fetch_a(A[2], kc, 7);
    read_b(Bf[0], cur, PW);
    if (MORE) request(kc + 1);
    __builtin_amdgcn_sched_barrier(0);
    split_mfma_two<P>(A[4], Bf[1], acc[1], lo[1], A[0], Bf[1], acc[3], lo[3]);              // steps 4, 5
    fetch_a(A[3], kc, 8);
    if (MORE) fetch_a(A[0], kc + 1, 0);
    read_b(Bf[1], cur, PW + 1);
    __builtin_amdgcn_sched_barrier(0);
    split_mfma_two<P>(A[1], Bf[0], acc[2], lo[2], A[2], Bf[0], acc[3], lo[3]);              // steps 6, 7
    if (MORE) { fetch_a(A[1], kc + 1, 1); fetch_a(A[2], kc + 1, 2); }
    __builtin_amdgcn_sched_barrier(0);
    split_mfma<P>(A[3], Bf[1], acc[3], lo[3]);                                              // step 8
    if (MORE) {
      fetch_a(A[3], kc + 1, 3);
      stage.file(tile, cur ^ 1, v);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();                                              // the other patch is complete, and nobody reads this one any more
  };

  if (kc0 < kc1) {
    request(kc0);
#pragma unroll
    for (int s = 0; s < 4; ++s) fetch_a(A[s], kc0, s);
    stage.file(tile, 0, v);
  }
  __syncthreads();
  int kc = kc0;
  for (; kc + 1 < kc1; ++kc) chunk(kc, (kc - kc0) & 1, std::true_type{});
  if (kc < kc1) chunk(kc, (kc - kc0) & 1, std::false_type{});

  if (mt_own >= MT || !have) return;
  // the cell's 2 x 2 input pixels; a row's two as one 8-byte store where every such address is aligned (W even: then column 2 c + 1 exists, too)
  float* dst = out + (size_t)ks*split_stride;                     // (KS > 1: `out` is the workspace the splits' sum reads)
  const int y = 2*(r0 + r), x = 2*(c0 + c);
  const bool row1 = y + 1 < H, col1 = x + 1 < W;
  const bool pairs = (W & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int m = mt*32 + mfma32_row(rr, g);
    if (m >= M) continue;
    float* q = dst + (((size_t)b*M + m)*H + y)*W + x;
    const float v00 = acc[0][rr] + lo[0][rr], v01 = acc[1][rr] + lo[1][rr], v10 = acc[2][rr] + lo[2][rr], v11 = acc[3][rr] + lo[3][rr];
    if (pairs) {
      *reinterpret_cast<f32x2v*>(q) = f32x2v{v00, v01};
      if (row1) *reinterpret_cast<f32x2v*>(q + W) = f32x2v{v10, v11};
    } else {
      q[0] = v00;
      if (col1) q[1] = v01;
      if (row1) { q[W] = v10; if (col1) q[W + 1] = v11; }
    }
  }
}

// The data gradient's tile: TR x TCW cells of 2 x 2 input pixels, TR TCW <= 64, the patch (TR + 1) x (TCW + 1) within kS2DPix: s2_tile's order of preference
void s2d_tile(int ho, int wo, int& TR, int& TCW) {
  double best = -1.0; int best_patch = 0;
  TR = 1; TCW = 1;
  for (int tcw = std::min(wo, 63); tcw >= 1; --tcw) {
    int tr = std::min(64/tcw, ho);
    while (tr > 1 && (tr + 1)*(tcw + 1) > kS2DPix) --tr;
    const int patch = (tr + 1)*(tcw + 1);
    const double useful = (double)ho*wo/((double)ceil_div(ho, tr)*ceil_div(wo, tcw)*64.0);
    if (useful > best + 1e-9 || (useful > best - 1e-9 && patch < best_patch)) { best = useful; best_patch = patch; TR = tr; TCW = tcw; }
  }
}
// Blocks of two channel tiles x two cell fragments.  The partial outputs of a K split are four times the forward's (H x W against ho x wo), so K is split
// only under one block per CU: at least two chunks per split, about two blocks per CU
S2Shape s2d_shape(int B, int C, int CO, int H, int W) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  S2Shape s;
  s2d_tile(ho, wo, s.TR, s.TCW);
  s.gx = ceil_div(wo, s.TCW); s.gy = ceil_div(ho, s.TR); s.gz = B;
  const int KC = CO >> 4, MG = ceil_div(ceil_div(C, 32), 2);
  const long long base = (long long)s.gx*s.gy*s.gz*MG;
  int ks = 1;
  if (base < 256) ks = (int)std::min<long long>(std::max(KC/2, 1), (512 + base - 1)/base);
  s.kcs = ceil_div(KC, ks); s.KS = ceil_div(KC, s.kcs);
  s.grid = dim3(8*(unsigned)ceil_div(base*s.KS, 8ll));
  s.out_elems = (size_t)B*C*H*W;
  return s;
}

}  // namespace

bool conv_s2_served(int C, int CO) { return C >= 16 && C % 16 == 0 && CO >= 32 && CO % 32 == 0; }
// floats of workspace: the forward's K-split partial outputs, or the weight gradient's partial sets with the finalize's fp64 slices
size_t conv_s2_workspace_floats(int B, int C, int CO, int H, int W) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  const S2Shape s = s2_fwd_shape(B, C, CO, ho, wo);
  return std::max({(size_t)64, s.KS > 1 ? (size_t)s.KS*s.out_elems : (size_t)0, partial_sets_floats(s2_wgrad_sets(B, C, CO, ho, wo), (size_t)9*CO*C)});
}
hipError_t launch_conv_s2_fwd(const float* x, const void* wp_fwd, float* y, float* split_ws, int B, int C, int CO, int H, int W, hipStream_t st) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  const S2Shape s = s2_fwd_shape(B, C, CO, ho, wo);
  hipLaunchKernelGGL(k_conv_s2_fwd<3>, s.grid, dim3(256), 0, st, x, (const uint4*)wp_fwd, s.KS > 1 ? split_ws : y, C, CO, H, W, ho, wo, s.TR, s.TCW, s.KS, s.kcs,
                     s.out_elems, s.gx, s.gy, s.gz);
  if (s.KS > 1) {
    const size_t n4 = s.out_elems/4;                              // (B CO ho wo is a multiple of 4: CO is a multiple of 32)
    hipLaunchKernelGGL(k_s2_split_sum, dim3((unsigned)((n4 + 255)/256)), dim3(256), 0, st, split_ws, y, n4, s.KS);
  }
  return hipGetLastError();
}
hipError_t launch_conv_s2_bwd_wgt(const float* x, const float* gy, float* g_w, float* partial, int B, int C, int CO, int H, int W, hipStream_t st) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  dim3 grid; int rows, spb;
  s2_wgrad_shape(B, C, CO, ho, wo, grid, rows, spb);
  hipLaunchKernelGGL(k_conv_s2_wgrad, grid, dim3(256), 0, st, x, gy, partial, B, C, CO, H, W, ho, wo, rows, spb);
  return launch_partial_sets_finalize(partial, grid.x*grid.y*(unsigned)ceil_div(B, spb), 9*CO*C, SetIndexMap{CO, C}, g_w, st);
}

// the data gradient: its blocks (the grid is 32-bit), its workspace (the K splits' partial gradients) and its launch
long long conv_s2d_blocks(int B, int C, int CO, int H, int W) { return (long long)s2d_shape(B, C, CO, H, W).grid.x; }
size_t conv_s2d_workspace_floats(int B, int C, int CO, int H, int W) {
  const S2Shape s = s2d_shape(B, C, CO, H, W);
  return std::max((size_t)64, s.KS > 1 ? (size_t)s.KS*s.out_elems : (size_t)0);
}
hipError_t launch_conv_s2_bwd_data(const float* gy, const void* wp_bwd, float* g_x, float* split_ws, int B, int C, int CO, int H, int W, hipStream_t st) {
  const int ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  const S2Shape s = s2d_shape(B, C, CO, H, W);
  hipLaunchKernelGGL(k_conv_s2_bwd_data<3>, s.grid, dim3(256), 0, st, gy, (const uint4*)wp_bwd, s.KS > 1 ? split_ws : g_x, CO, C, H, W, ho, wo, s.TR, s.TCW, s.KS,
                     s.kcs, s.out_elems, s.gx, s.gy, s.gz);
  if (s.KS > 1) {
    const size_t n4 = s.out_elems/4;                              // (B C H W is a multiple of 4: C is a multiple of 16)
    hipLaunchKernelGGL(k_s2_split_sum, dim3((unsigned)((n4 + 255)/256)), dim3(256), 0, st, split_ws, g_x, n4, s.KS);
  }
  return hipGetLastError();
}

}  // namespace smd
