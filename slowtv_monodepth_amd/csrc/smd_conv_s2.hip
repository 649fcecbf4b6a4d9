// smd_conv_s2.hip — the ResNet encoders' transition convolutions, conv2d(x (B,C,H,W), w (CO,C,3,3), stride 2, padding 1) (`conv1` of the first BasicBlock
// of layer2 / layer3 / layer4), forward and weight gradient on the bf16 matrix cores with fp32-class results: every fp32 operand split exactly into three
// bf16 pieces, six `v_mfma_f32_32x32x16_bf16` per K step of 16 (the scheme: smd_conv_mfma.hip; the arithmetic: smd_split_dev.h; the shared stages:
// smd_conv_mfma_dev.h).  Zero padding inside the kernels, NCHW fp32 in and out, any H, W >= 1: Ho = (H - 1)/2 + 1, Wo = (W - 1)/2 + 1.  No data gradient.
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

}  // namespace smd
