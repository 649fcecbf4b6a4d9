// smd_conv_mfma.hip — the Monodepth decoder's wide 3x3 convolutions on the bf16 matrix cores with fp32-class results (SURVEY.md §8f rank 4, round 6;
// reference: src/networks/decoders/monodepth.py:40-50, 71-84 — `ConvELU(cin, cout)` = reflection-padded conv3x3 + ELU; decoders/utils.py:44-54).
//
// Why not the f32 MFMA (smd_conv_thin.hip): on gfx950 `v_mfma_f32_32x32x2_f32` runs at the vector rate, 157 TFLOP/s — 1/16 of the bf16 matrix rate — and
// there is no xf32/TF32 form.  MIOpen's fp32 Winograd reaches 87-93 TFLOP/s effective on these layers forward and 55-75 backward.  Here every fp32 operand
// is SPLIT EXACTLY into three bf16 pieces, x = x0 + x1 + x2 (8 + 8 + 8 significant bits: x0 = bf16(x), x1 = bf16(x - x0), x2 = x - x0 - x1, each
// difference exact in fp32), and a product a.b is formed as the six bf16 products with i + j <= 2,
//     a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0),
// each exact in the fp32 accumulator's product stage; what is dropped (a1 b2 + a2 b1 + a2 b2) is below 2^-25 |a b|, under the rounding of an fp32
// multiply-add.  Six `v_mfma_f32_32x32x16_bf16` per K step of 16 = 6/16 of the f32 MFMA's time for the same arithmetic: a ceiling of 2.67 x the fp32
// matrix peak with fp32-class error (tests: <= 2e-6 of the tensor's max against fp64 `conv2d`, the same bound the f32-MFMA kernels are held to).
// That bound is the kernels' own fp32 accumulation noise (1e-7 to 1e-6 of the maximum), and a third-order product is at most 2^-18 of a product: one wrong
// piece at one tap, channel half, K chunk or fragment slot stays under it.  tests/test_gpu_conv_exact.py therefore also runs these kernels (and the stem's) on
// operands where nothing rounds — piece-built values whose dropped products are exactly zero, one product per output element, and dense small integers
// (tests/conv_exact.py) — and asks for the fp64 result bit for bit: any kept product missing, doubled or read from the wrong place fails there.
// PIECES = 2 (three products, 16 significant bits, "better than TF32") exists as an experiment knob only; PIECES = 1 is plain bf16.
// Round 7: the same kernels serve the ResNet encoders' zero-padded 3x3 stride-1 layers (OFF = 1 below, k_wgrad_dma's ZP form in smd_conv_wgrad.hip; profiles/r07_encoder_convs.txt).
//
// This file: the weights' packing, forward and data gradient — one kernel (implicit GEMM, M = output channels, N = pixels, K = (tap, input channel)) — and
// the sixteen-channel form.  The weight gradient, a GEMM with K = pixels (M = output channels, N = input channels, one accumulator tile per tap), is
// smd_conv_wgrad.hip; the stages the kernels of both files, the stem and the DDVNet head share are smd_conv_mfma_dev.h.  Operand layouts, per `v_mfma_f32_32x32x16_bf16`:
// A: lane l holds row i = l & 31, K slots 8 (l >> 5) .. + 7; B: column j = l & 31, same K slots; D: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5).
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_conv_mfma_dev.h"
#include <algorithm>

namespace smd {

template <typename T> __device__ __forceinline__ void store_out(T* p, size_t i, float v);
template <> __device__ __forceinline__ void store_out<float>(float* p, size_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void store_out<bf16>(bf16* p, size_t i, float v) { p[i] = __float2bfloat16(v); }

// ---- weights -> bf16 pieces in the A-operand order of both convolution forms (one launch per layer and step; the backward reads what the forward packed) ----
// forward form:       Wt[m = co][k = c][tap]      = w[co][c][tap]          (M = CO, CK = C)
// data-gradient form: Wt[m = c][k = co][tap]      = w[co][c][8 - tap]      (M = C, CK = CO): the convolution of the zero-extended dL/dy with the flipped kernel
// element (m, k, tap, piece) at ((((m >> 5) KC + (k >> 4)) 9 + tap) P + piece) 512 + (((k >> 3) & 1) 32 + (m & 31)) 8 + (k & 7): a wave's fragment is 1 KiB, lane-major
template <int P>
__global__ __launch_bounds__(256) void k_conv_pack_w(const float* __restrict__ w, unsigned short* __restrict__ wp_fwd, unsigned short* __restrict__ wp_bwd, int CO, int C) {
  const int idx = blockIdx.x*256 + threadIdx.x;
  if (idx >= CO*C*9) return;
  const int tap = idx % 9, c = (idx/9) % C, co = idx/(9*C);
  unsigned pk[P];
  split_pair<P>(w[idx], 0.f, pk);
  if (wp_fwd) {
    const size_t base = ((((size_t)(co >> 5)*(C >> 4) + (c >> 4))*9 + tap)*P)*512 + (((c >> 3) & 1)*32 + (co & 31))*8 + (c & 7);
#pragma unroll
    for (int p = 0; p < P; ++p) wp_fwd[base + (size_t)p*512] = (unsigned short)(pk[p] & 0xffffu);
  }
  if (wp_bwd) {
    const size_t base = ((((size_t)(c >> 5)*(CO >> 4) + (co >> 4))*9 + (8 - tap))*P)*512 + (((co >> 3) & 1)*32 + (c & 31))*8 + (co & 7);
#pragma unroll
    for (int p = 0; p < P; ++p) wp_bwd[base + (size_t)p*512] = (unsigned short)(pk[p] & 0xffffu);
  }
}

// ---- forward / data gradient ----
// out[b][m][y][x] = sum over k < CK and taps of in[b][k][y + ky - OFF][x + kx - OFF] Wt[m][k][tap]; OFF = 0 for the forward (in = the reflection-padded input,
// every read of a stored output is inside it), OFF = 2 for the data gradient (in = dL/dy, zero outside; out = the gradient of the PADDED input), OFF = 1 for a
// zero-padded "same" layer (the encoders' 3x3 stride-1 convolutions: in and out both h x w, reads outside the image are zeros) — with the forward operand image
// its forward, with the data-gradient image (flipped taps) its data gradient, which lands on the unpadded input's gradient directly.
// A block of four waves owns 8 pixel tiles of 32 consecutive pixels (TC = 64: 4 rows x 64 columns, a wave per row; TC = 32: 8 rows x 32 columns, a wave
// per row pair) and one tile of 32 output channels; K runs in chunks of 16 input channels x 9 taps.  Per chunk the block stages its (TRB + 2) x (TC + 2)
// patch of the 16 channels in LDS — coalesced row pieces, split into the bf16 pieces ONCE per element (it is used by 9 taps x every output channel),
// filed pixel-major with the 16 channels of a pixel contiguous (32 B per piece): the B operand of a tap is then one ds_read_b128 per lane whatever the tap's
// shift.  The two 16-byte halves of a pixel are swapped where bit 3 of the pixel index is set: the 16-lane groups that serve a ds_read_b128
// ({0-3, 12-15, 20-27}, ...) then cover all 64 banks instead of colliding two ways.  Two patches: the next chunk's loads are requested after tap 4's fetch
// and filed behind the MFMAs of taps 6 - 8, one barrier per chunk.  The weights come as whole fragments from `k_conv_pack_w`'s image (1 KiB per wave and piece, lane-major:
// every block reads the same ones, L1 / L2 hits), five slots requested four taps ahead (see below why).
// What was measured on the way to this form (cfg 2's 96 -> 32 layer at 96x320, MIOpen 217 us; scripts/dev/conv_mfma_check.py, profiles/r06_conv_mfma_*):
// one load per loop trip, 134 us; every staging load before its first use + the ring, 135 (the pieces — MFMAs alone 59 us, operand reads 40, staging 79-97 —
// hardly overlap: a CU's one memory pipeline carries the staging loads AND four waves' copies of the weight fragments, 133 KB per chunk and block);
// weights through LDS as well (one patch + one weight image, two barriers per chunk), 171; the chunk's loads spread over the taps, 205 (284 registers: one
// wave per SIMD); two producer waves + four MFMA waves per block, 158-174; chunks of 8 channels (two taps per MFMA K step) so that patch AND weight fragments
// fit twice in 68 KB and the MFMA loop touches no vector memory, 158.  What the series says: the limiter is the bytes a CU pulls through its vector-memory path
// (~10 B/clk for L2 / HBM data: 25 KB of patch per chunk and block = 2.5 k cycles against 3.5 k of MFMAs for 32 output channels) — weight fragments fetched
// once per block from L2 cost more than four waves' L1-hit copies.  Later in the round (profiles/r06_conv_mfma_ablations.txt): the in-order load counter (a fragment wait
// drained the staging loads: fragments four taps ahead, staging request behind the chunk's last fetch, -5 %), a phase trace (scripts/dev/conv_trace.py), eight waves with
// the weights in LDS and persistent blocks (both slower).  The lever left is MFMA work per wave and staged byte: two or three channel tiles per patch.
#ifdef SMD_CONV_TRACE   // diagnosis builds only (scripts/dev/conv_trace.py): shader-clock stamps of wave 0 of every block of the forward / data-gradient form
__device__ unsigned long long g_conv_trace[8192][40];
#define SMD_CT(slot) do { if (wall == 0 && lid < 8192u && (slot) < 40) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) g_conv_trace[lid][(slot)] = t_; } } while (0)
#else
#define SMD_CT(slot) do { } while (0)
#endif
template <int TC> struct ConvTile {
  static constexpr int TRB = (TC == 64) ? 4 : 8;
  static constexpr int PW = TC + 2, PH = TRB + 2, NPIX = PW*PH;
};
// TC = 0: ROW-BAND tiles for narrow maps (the coarse levels: 24 x 80, 12 x 40, 6 x 20 and their padded-gradient forms).  A block's 256 pixels are R whole
// output rows of one sample, or — where a whole image is at most 128 pixels — S whole samples (R = ho); the eight fragments are 32 CONSECUTIVE pixels of
// the band in flattened order, so a fragment may cross row ends and sample boundaries.  The patch is the band's input rows with their halos, each row
// wo + 2 wide, and each sample's rows stacked with their own two halo rows; a lane decodes its pixel once per block and reads tap (ky, kx) at
// lane base + ky (wo + 2) + kx.  The rectangular tiles of 64 x 4 / 32 x 8 carry 47 % useful pixels at 12 x 40 and 6 x 20 and 62.5 % at 24 x 80; bands of
// 240 pixels (6 rows, 2 samples, 3 rows) carry 94 %.  The patch buffer is sized for the largest band patch (420 pixels: 5 x 84 at 26 x 82), 79 KB for
// two patches — still two blocks per CU.
template <> struct ConvTile<0> {
  static constexpr int TRB = 0, PW = 0, NPIX = 420;
};

// NM: channel tiles per block.  NM = 2 (knob conv_two_tiles, layers with a multiple of 64 output channels): EIGHT waves, waves 4 .. 7 multiply the same patch by
// the next 32 output channels' weights — the patch is staged once for 64 channels (by all 512 lanes).  Built to halve what a block pulls through the CU's
// vector-memory path per MFMA; measured neutral (128 -> 64 at 48x160: 103.0 vs 104.7 us forward, 108.0 vs 104.7 data gradient; 512 -> 256 at 12x40: 183 vs 171;
// 128 -> 64 at 24x80 data gradient 42.7 vs 52.3), so the default stays one tile per block.  Same bits either way.
template <int TC, int P, int OFF, typename TI, typename TO, int NM>
__global__ __launch_bounds__(256*NM, 2/NM) void k_conv_mfma(const TI* __restrict__ in_, const uint4* __restrict__ wp, TO* __restrict__ out,
                                                   int CK, int M, int hi, int wi, int ho, int wo, int KS, int kc_per_split, size_t split_stride,
                                                   unsigned gx, unsigned gy, unsigned gz, int S, int B) {
  using T = ConvTile<TC>;
  constexpr bool BAND = TC == 0;                                  // row-band tiles: gx = R (rows of a band, BR), gy = bands per sample, gz = groups of S samples
  constexpr int NPIX = T::NPIX, off = OFF;
  const int PW = BAND ? wo + 2 : T::PW;
  constexpr bool ZERO = OFF != 0;                                 // reads outside the image are zeros (OFF = 0: every read of a stored output is inside)
  constexpr int kBuf = P*NPIX*2;
  __shared__ uint4 tile[2*kBuf];                                  // two patches, [piece][pixel][half]
  const int lane = threadIdx.x & 63, wall = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wv = wall & 3, mt = wall >> 2, j = lane & 31, g = lane >> 5;
  constexpr int NT = 256*NM;
  // Block -> (channel tile, K split, tile column, tile row, sample), in the XCD-aware order of xcd_block_id
  const int MG = M/(32*NM);
  const unsigned nblk = (unsigned)(MG*KS)*(BAND ? 1u : gx)*gy*gz, lid = xcd_block_id(nblk);
  if (lid >= nblk) return;
  const int mg = (int)(lid % MG)*NM + mt, ks = (lid/MG) % KS;     // mg: this wave's tile of 32 output channels
  const unsigned tl = lid/(MG*KS);
  const int BR = BAND ? (int)gx : 0, SEGP = (BR + 2)*PW;            // (band: a sample's patch rows, R + 2 of PW pixels)
  const int x0 = BAND ? 0 : (int)(tl % gx)*TC, y0 = BAND ? (int)(tl % gy)*BR : (int)((tl/gx) % gy)*T::TRB;
  const int b = BAND ? (int)(tl/gy)*S : (int)(tl/(gx*gy));         // (band: the first of its S samples)
  const int KC = CK >> 4, kc0 = ks*kc_per_split, kc1 = min(KC, kc0 + kc_per_split);
  const size_t plane = (size_t)hi*wi;
  typedef typename RawOf<TI>::type R;
  const R* src = reinterpret_cast<const R*>(in_) + (size_t)b*CK*plane;
  // band: this lane's pixel of fragment nt (the wave's fragments 2 wv, 2 wv + 1) -> its sample (0 .. S - 1 in the band), row and column; -1: none
  auto band_pixel = [&](int nt, int& seg, int& ry, int& x) {
    const int p = (2*wv + nt)*32 + j, spx = BR*wo;
    seg = p/spx; const int q = p - seg*spx; ry = q/wo; x = q - ry*wo;
    if (seg >= S || b + seg >= B || y0 + ry >= ho) seg = -1;
  };
  int lbase[2] = {0, 0};                                          // band: the lane's patch pixel at tap (0, 0)
  if constexpr (BAND) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      int seg, ry, x;
      band_pixel(nt, seg, ry, x);
      lbase[nt] = seg >= 0 ? (seg*(BR + 2) + ry)*PW + x : 0;
    }
  }

  // staging (PatchStager): the rectangular tiles' offsets are the stager's; a row band computes its own and feeds the same request / file_trip
  using Stage = PatchStager<NT, NPIX, P, R, ZERO>;
  constexpr int TRIPS = Stage::TRIPS;
  Stage stage;
  if constexpr (BAND) {
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {                             // patch pixel -> (sample of the band, row, column); past the patch or the batch: zeros /
      const int item = Stage::item(t), half = item >= NPIX ? 1 : 0, pix = item - half*NPIX;   //   any valid address (OFF = 0)
      const int seg = pix/SEGP, rp = pix - seg*SEGP, r = rp/PW, cc = rp - r*PW;
      const int yy = y0 + r - off, xx = cc - off;
      const bool in_b = seg < S && b + seg < B;
      const int sofs = min(seg, B - 1 - b)*CK*(int)plane;        // (the host keeps B CK hi wi below 2^31 for band tiles)
      if (ZERO) stage.pofs[t] = (in_b && yy >= 0 && yy < hi && xx >= 0 && xx < wi) ? sofs + yy*wi + xx : -1;
      else stage.pofs[t] = sofs + min(yy, hi - 1)*wi + min(xx, wi - 1);
    }
  } else stage.template rect_offsets<T::PW>(y0, x0, off, hi, wi);
  R v[TRIPS][8];
  auto request = [&](int kc) { stage.request(src, plane, kc, v); };
  auto file_trip = [&](int buf, int t) { stage.file_trip(tile, buf, t, v); };

  f32x16 acc[2], lo[2];                                           // the leading product's and the small ones' accumulators (split_mfma)
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[nt][r] = 0.f; lo[nt][r] = 0.f; }

  // the weights' fragments: five slots, requested FOUR taps ahead (tap t of a chunk sits in slot t mod 5; a chunk counts as ten steps, the tenth empty, so the
  // positions repeat every chunk), and the next patch's staging loads requested after tap 4's fetch.  The counter of outstanding loads retires in order: a wait
  // for a fragment also waits for every load requested before it.  With a ring of three (two taps ahead) and the staging request at the chunk's start, tap 2's
  // fragments were requested after the staging loads and the wait for them drained those: the staging latency stood exposed in every chunk.  Now the fragments
  // of taps 4 .. 8 are requested before the staging loads and every later fetch belongs to the next chunk, whose first wait comes after the staging loads
  // have been filed anyway: they have four taps to land and are waited for only where they are filed.  (Six slots / nine: 256 registers and 400 / 72 bytes of
  // spills per lane.)  The patch's fragments (LDS) one tap ahead.
  bf16x8 A[5][P], Bf[2][2][P];
  const uint4* wq = wp + ((size_t)mg*KC*9*P)*64 + lane;
  auto fetch_a = [&](bf16x8 (&dst)[P], int kc, int tap) {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = as_frag(wq[(size_t)((kc*9 + tap)*P + p)*64]);
  };
  auto read_b = [&](bf16x8 (&dst)[2][P], int buf, int tap) {
    const int ky = tap/3, kx = tap % 3;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int r = (TC == 64) ? wv : 2*wv + nt, cb = (TC == 64) ? nt*32 : 0;
      Stage::read(tile, buf, BAND ? lbase[nt] + ky*PW + kx : (r + ky)*PW + cb + j + kx, g, dst[nt]);
    }
  };
  // one chunk; MORE is compile-time (the last chunk is peeled): no load sits behind a run-time branch, the compiler keeps count of what is outstanding
  auto chunk = [&](int kc, int cur, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    [[maybe_unused]] const int cslot = 3 + 4*(kc - kc0);
    SMD_CT(cslot);
    read_b(Bf[0], cur, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 8) read_b(Bf[(tap + 1) & 1], cur, tap + 1);
      split_mfma<P>(A[tap % 5], Bf[tap & 1], acc, lo);
      if (tap <= 4) fetch_a(A[(tap + 4) % 5], kc, tap + 4);
      else if (MORE && tap >= 6) fetch_a(A[tap - 6], kc + 1, tap - 6);
      if (MORE && tap == 8) fetch_a(A[3], kc + 1, 3);             // (the empty tenth step's fetch; slot 3 is tap 8's, whose MFMAs have been issued)
      if (MORE && tap == 4) request(kc + 1);                      // after this chunk's last fetch: lands during taps 5 .. 8
      // the next patch is filed trip by trip behind the last taps' MFMAs (its splits run in the matrix pipe's shadow) instead of after them
      if (MORE && tap >= 6) {
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) if (t*3/TRIPS == tap - 6) file_trip(cur ^ 1, t);
      }
      // a tap's instructions stay in their tap: left free, the scheduler sinks the fetches of taps 0 - 2 (for taps 4 - 6) behind tap 3's MFMAs and every later
      // fragment is then requested one tap before its use and waited for with vmcnt(0) — the four taps of distance exist in the source only
      __builtin_amdgcn_sched_barrier(0);
    }
    SMD_CT(cslot + 1);
    SMD_CT(cslot + 2);
    __syncthreads();                                              // the other patch is complete, and nobody reads this one any more
    SMD_CT(cslot + 3);
  };

  SMD_CT(0);
  if (kc0 < kc1) {
    request(kc0);
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) fetch_a(A[tap], kc0, tap);
    stage.file(tile, 0, v);
  }
  SMD_CT(1);
  __syncthreads();
  SMD_CT(2);
  int kc = kc0;
  for (; kc + 1 < kc1; ++kc) chunk(kc, (kc - kc0) & 1, std::true_type{});
  if (kc < kc1) chunk(kc, (kc - kc0) & 1, std::false_type{});
  // D[row = output channel][column = pixel]: a register is 32 consecutive pixels of one channel per half wave (128-byte runs)
  // (a K split's partial output is always fp32: `out` is then the workspace the splits' sum reads)
  float* dstf = reinterpret_cast<float*>(out) + (size_t)ks*split_stride;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    int y, x, bo = b;
    bool ok;
    if constexpr (BAND) {
      int seg, ry;
      band_pixel(nt, seg, ry, x);
      ok = seg >= 0; y = y0 + ry; bo = b + seg;
    } else {
      const int r = (TC == 64) ? wv : 2*wv + nt, cb = (TC == 64) ? nt*32 : 0;
      y = y0 + r; x = x0 + cb + j; ok = y < ho && x < wo;
    }
    if (ok) {
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int m = mg*32 + mfma32_row(rr, g);
        const size_t o = (((size_t)bo*M + m)*ho + y)*wo + x;
        if (KS > 1) dstf[o] = acc[nt][rr] + lo[nt][rr];
        else store_out<TO>(out, o, acc[nt][rr] + lo[nt][rr]);
      }
    }
  }
  SMD_CT(39);
}

// ---- sixteen output channels (the decoder's thin last stage: 32 -> 16 at half resolution, 16 -> 16 at full resolution) ----
// The same split-bf16 arithmetic on `v_mfma_f32_16x16x32_bf16` (A: row i = l & 15, K slots 8 (l >> 4) .. + 7; B: column j = l & 15; D: column = l & 15,
// row = 4 (l >> 4) + v), pixels as rows, output channels as columns: a lane ends with four consecutive pixels of one channel — a 16-byte store.  A K step of
// 32 = TWO taps x 16 channels (lane group q: tap 2 s + (q >> 1), channels 8 (q & 1) .. + 7); the ninth tap's partner is a zero weight.  With 2304 multiply-adds
// per pixel on 128 bytes the layer is HBM-bound once its arithmetic costs 6/16 of the f32 MFMA's time (the f32-MFMA kernel of smd_conv_thin.hip: 82 us
// forward at cfg 2, its K loop at half the f32 matrix rate; 189 MB / 5 TB/s = 38 us).  The weights (<= 2 chunks x 5 K steps x P fragments) stay in registers;
// a wave owns 16 columns x 4 rows of a 64 x 4 tile (four accumulator pairs); the patch is staged and read exactly as in k_conv_mfma.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte store that is only 4-byte aligned (the padded gradient's rows)

// thin operand image: element (chunk, K step s, piece, lane = 16 q + j, e) = Wt[m = j][k = 16 chunk + 8 (q & 1) + e][tap = 2 s + (q >> 1)] (zero for tap 9)
template <int P>
__global__ __launch_bounds__(256) void k_conv_pack_w16(const float* __restrict__ w, unsigned short* __restrict__ wp_fwd, unsigned short* __restrict__ wp_bwd, int C) {
  const int idx = blockIdx.x*256 + threadIdx.x;                   // w is (16, C, 3, 3)
  const int nslots = (C >> 4)*5*64*8;
  if (idx < nslots && wp_fwd) {                                   // forward form: m = co, k = c
    const int e = idx & 7, lane = (idx >> 3) & 63, s = (idx >> 9) % 5, ch = idx/(512*5);
    const int j = lane & 15, q = lane >> 4, tap = 2*s + (q >> 1), k = 16*ch + 8*(q & 1) + e;
    unsigned pk[P];
    split_pair<P>(tap < 9 ? w[((size_t)j*C + k)*9 + tap] : 0.f, 0.f, pk);
#pragma unroll
    for (int p = 0; p < P; ++p) wp_fwd[(((size_t)(ch*5 + s)*P + p)*64 + lane)*8 + e] = (unsigned short)(pk[p] & 0xffffu);
  }
  if (idx < 5*64*8 && wp_bwd && C == 16) {                        // data-gradient form (16 -> 16 only): m = c, k = co, flipped taps
    const int e = idx & 7, lane = (idx >> 3) & 63, s = idx >> 9;
    const int j = lane & 15, q = lane >> 4, tap = 2*s + (q >> 1), k = 8*(q & 1) + e;
    unsigned pk[P];
    split_pair<P>(tap < 9 ? w[((size_t)k*C + j)*9 + (8 - tap)] : 0.f, 0.f, pk);
#pragma unroll
    for (int p = 0; p < P; ++p) wp_bwd[(((size_t)s*P + p)*64 + lane)*8 + e] = (unsigned short)(pk[p] & 0xffffu);
  }
}

template <int NCH, int P, bool BWD, typename TI, typename TO>
__global__ __launch_bounds__(256) void k_conv16_mfma(const TI* __restrict__ in_, const uint4* __restrict__ wp, TO* __restrict__ out,
                                                     int hi, int wi, int ho, int wo, unsigned gx, unsigned gy, unsigned gz) {
  using T = ConvTile<64>;
  constexpr int NPIX = T::NPIX, PW = T::PW, off = BWD ? 2 : 0, CK = 16*NCH;
  __shared__ uint4 tile[P*NPIX*2];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 15, q = lane >> 4;
  const unsigned nblk = gx*gy*gz, lid = xcd_block_id(nblk);
  if (lid >= nblk) return;
  const int x0 = (int)(lid % gx)*64, y0 = (int)((lid/gx) % gy)*4, b = (int)(lid/(gx*gy));
  const size_t plane = (size_t)hi*wi;
  typedef typename RawOf<TI>::type R;
  const R* src = reinterpret_cast<const R*>(in_) + (size_t)b*CK*plane;

  bf16x8 Wr[NCH][5][P];                                           // every weight fragment of the layer: requested first, used last
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int s = 0; s < 5; ++s)
#pragma unroll
      for (int p = 0; p < P; ++p) Wr[ch][s][p] = as_frag(wp[((ch*5 + s)*P + p)*64 + lane]);

  // The patch is PatchStager's (same layout, patch_slot, Stage::read), but the three staging loops below are this kernel's own copies of the stager's
  // rect_offsets / request / file.  Through the stager the compiler's register allocation of this straight-line kernel comes out differently: called from
  // lambdas, the fp32 16 -> 16 forward took 130 registers instead of 109 (a wave per SIMD less, 67 us instead of 56); with only the request loop written
  // out, the data gradient reused a load's destination in the last load's address and drained the 31 loads before it (79 us instead of 71).  Written out,
  // every instance issues all of a chunk's loads before its first wait, as before.  Keep the loops in step with PatchStager.
  using Stage = PatchStager<256, NPIX, P, R, BWD>;
  constexpr int ITEMS = Stage::ITEMS, TRIPS = Stage::TRIPS;
  int pofs[TRIPS];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int item = min(t*256 + (int)threadIdx.x, ITEMS - 1);
    const int half = item >= NPIX ? 1 : 0, pix = item - half*NPIX;
    const int r = pix/PW, cc = pix - r*PW;
    const int yy = y0 + r - off, xx = x0 + cc - off;
    if (BWD) pofs[t] = (yy >= 0 && yy < hi && xx >= 0 && xx < wi) ? yy*wi + xx : -1;
    else pofs[t] = min(yy, hi - 1)*wi + min(xx, wi - 1);
  }
  int dpix[5];                                                    // this lane group's tap of K step s, as an offset inside the patch
#pragma unroll
  for (int s = 0; s < 5; ++s) { const int tq = min(2*s + (q >> 1), 8); dpix[s] = (tq/3)*PW + tq % 3; }

  f32x4v acc[4], lo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { acc[r] = f32x4v{0.f, 0.f, 0.f, 0.f}; lo[r] = f32x4v{0.f, 0.f, 0.f, 0.f}; }

#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    R v[TRIPS][8];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {                             // every load of the chunk before its first use
      const int item = min(t*256 + (int)threadIdx.x, ITEMS - 1);
      const int half = item >= NPIX ? 1 : 0;
      const R* p = src + (size_t)(ch*16 + half*8)*plane + (size_t)max(pofs[t], 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[t][e] = (!BWD || pofs[t] >= 0) ? p[(size_t)e*plane] : R(0);
    }
    if (ch > 0) __syncthreads();                                  // nobody reads the previous chunk any more
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int item = t*256 + (int)threadIdx.x;
      if (item < ITEMS) {
        const int half = item >= NPIX ? 1 : 0, pix = item - half*NPIX;
        unsigned pk[4][P];
#pragma unroll
        for (int k = 0; k < 4; ++k) split_pair<P>(v[t][2*k], v[t][2*k + 1], pk[k]);
        const int slot = patch_slot(pix, half);
#pragma unroll
        for (int p = 0; p < P; ++p) tile[p*NPIX*2 + slot] = uint4{pk[0][p], pk[1][p], pk[2][p], pk[3][p]};
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 5; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bf16x8 A[P];
        Stage::read(tile, 0, r*PW + 16*wv + i + dpix[s], q & 1, A);
        split_mfma<P>(A, Wr[ch][s], acc[r], lo[r]);
      }
    }
  }
  // D[row = pixel 4 q + v][column = channel i]: four consecutive pixels of one channel per lane
  const int x = x0 + 16*wv + 4*q;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = y0 + r;
    if (y >= ho || x >= wo) continue;
    TO* dstp = out + (((size_t)b*16 + i)*ho + y)*wo + x;
    const f32x4v o = acc[r] + lo[r];
    if constexpr (sizeof(TO) == 4) {
      if (x + 3 < wo) *reinterpret_cast<f32x4u*>(dstp) = o;
      else { dstp[0] = o[0]; if (x + 1 < wo) dstp[1] = o[1]; if (x + 2 < wo) dstp[2] = o[2]; }
    } else {                                                      // bfloat16: dword stores where the row pitch keeps pixel pairs 4-byte aligned
      const unsigned lo2 = pack_bf16_rne(o[0], o[1]), hi2 = pack_bf16_rne(o[2], o[3]);
      if (x + 3 < wo && (wo & 1) == 0) { reinterpret_cast<unsigned*>(dstp)[0] = lo2; reinterpret_cast<unsigned*>(dstp)[1] = hi2; }
      else {
        unsigned short* d16 = reinterpret_cast<unsigned short*>(dstp);
        d16[0] = (unsigned short)(lo2 & 0xffffu);
        if (x + 1 < wo) d16[1] = (unsigned short)(lo2 >> 16);
        if (x + 2 < wo) d16[2] = (unsigned short)(hi2 & 0xffffu);
        if (x + 3 < wo) d16[3] = (unsigned short)(hi2 >> 16);
      }
    }
  }
}

// out = the sum of the K splits' partial outputs, in split order (the coarse decoder levels: few pixels, thousands of K — the splits are what fills the chip)
template <typename TO>
__global__ __launch_bounds__(256) void k_conv_split_sum(const float* __restrict__ part, TO* __restrict__ out, size_t n4, int KS) {
  const size_t i = (size_t)blockIdx.x*256 + threadIdx.x;
  if (i >= n4) return;
  const f4* p = reinterpret_cast<const f4*>(part);
  f4 s = p[i];
  for (int k = 1; k < KS; ++k) s += p[(size_t)k*n4 + i];
  if constexpr (sizeof(TO) == 4) reinterpret_cast<f4*>(out)[i] = s;
  else { unsigned* o = reinterpret_cast<unsigned*>(out) + 2*i; o[0] = pack_bf16_rne(s.x, s.y); o[1] = pack_bf16_rne(s.z, s.w); }
}

// ---- launch shapes ----  (the weight gradient: smd_conv_wgrad.hip)
static size_t thin_packed_elems(int C, int pieces) { return (size_t)(C >> 4)*5*pieces*512; }
size_t conv_mfma_packed_elems(int C, int CO, int pieces) { return std::max((size_t)CO*C*9*pieces, CO == 16 ? thin_packed_elems(C, pieces) : (size_t)0); }

// ---- launches.  `pieces`: 3 (or the experiment's 2): fp32 tensors, split operands; 1: bfloat16 tensors in and out (fp32 weights, packed as their bf16 rounding;
// fp32 accumulation, fp32 weight gradient) — the decoder under bf16 autocast ----
#define SMD_BY_PIECES(pieces, CALL) do { if ((pieces) == 3) { CALL(3, float); } else if ((pieces) == 2) { CALL(2, float); } else { CALL(1, bf16); } } while (0)

// 16 output channels: the thin operand image (forward: C = 16 or 32; data gradient: the thin image for C = 16, the wide one — 32 rows — for C = 32)
template <int P, typename T>
static void launch_conv16(const void* in, const void* wp, void* out, int B, int CK, bool bwd, int hi, int wi, int ho, int wo, hipStream_t st) {
  const unsigned gx = ceil_div(wo, 64), gy = ceil_div(ho, 4), gz = B;
  const dim3 grid(8*(unsigned)ceil_div((long long)gx*gy*gz, 8ll));
  const uint4* wq = (const uint4*)wp;
  const T* i_ = (const T*)in; T* o_ = (T*)out;
  if (bwd) hipLaunchKernelGGL((k_conv16_mfma<1, P, true, T, T>), grid, dim3(256), 0, st, i_, wq, o_, hi, wi, ho, wo, gx, gy, gz);
  else if (CK == 16) hipLaunchKernelGGL((k_conv16_mfma<1, P, false, T, T>), grid, dim3(256), 0, st, i_, wq, o_, hi, wi, ho, wo, gx, gy, gz);
  else hipLaunchKernelGGL((k_conv16_mfma<2, P, false, T, T>), grid, dim3(256), 0, st, i_, wq, o_, hi, wi, ho, wo, gx, gy, gz);
}

hipError_t launch_conv_mfma_pack(const float* w, void* wp_fwd, void* wp_bwd, int C, int CO, int pieces, hipStream_t st) {
  if (CO == 16) {
    void* thin_bwd = (C == 16) ? wp_bwd : nullptr;
    if (wp_fwd || thin_bwd) {
      const dim3 g16(ceil_div((C >> 4)*5*512, 256));
#define SMD_CALL(P, T) hipLaunchKernelGGL((k_conv_pack_w16<P>), g16, dim3(256), 0, st, w, (unsigned short*)wp_fwd, (unsigned short*)thin_bwd, C)
      SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
    }
    if (C == 16 || !wp_bwd) return hipGetLastError();
    wp_fwd = nullptr;                                             // C = 32: the data gradient is a 32-row layer of the wide kernel
  }
  const dim3 grid(ceil_div(CO*C*9, 256));
#define SMD_CALL(P, T) hipLaunchKernelGGL((k_conv_pack_w<P>), grid, dim3(256), 0, st, w, (unsigned short*)wp_fwd, (unsigned short*)wp_bwd, CO, C)
  SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
  return hipGetLastError();
}

// Launch shape of the forward / data-gradient form: tile columns, channel tiles per block, K splits (each split a whole number of 16-channel chunks).
struct ConvShape { int TC, TRB, NM, KS, kcs, S; unsigned gx, gy, gz; dim3 grid; size_t out_elems; };
// Row-band tiles (TC = 0): BR rows of one sample, or S whole samples (BR = ho) where an image has at most 128 pixels; the patch (S (BR + 2) (wo + 2) pixels)
// must fit ConvTile<0>::NPIX.  Returns the useful share of the band blocks' 256 pixels, 0 where no band fits.
static double band_shape(int B, int CK, int ho, int wo, int& BR, int& S) {
  constexpr int NP = ConvTile<0>::NPIX;
  const int PW = wo + 2;
  if (3*PW > NP || (long long)B*CK*(ho + 2)*PW >= (1ll << 31)) return 0.0;   // (the kernel's patch offsets are int)
  if (ho*wo <= 128) {
    BR = ho; S = std::min(256/(ho*wo), B);
    while (S > 1 && S*(ho + 2)*PW > NP) --S;
  } else {
    S = 1; BR = std::min(ho, 256/wo);
    while (BR > 0 && (BR + 2)*PW > NP) --BR;
    if (BR == 0) return 0.0;
  }
  return (double)B*ho*wo/((double)ceil_div(ho, BR)*ceil_div(B, S)*256.0);
}
static ConvShape conv_shape(int B, int CK, int M, int ho, int wo, bool two_tiles) {
  ConvShape s;
  s.TC = wo >= 48 ? 64 : 32; s.TRB = wo >= 48 ? 4 : 8; s.S = 1;
  const int KC = CK >> 4;
  {
    // band tiles where the rectangular ones waste clearly more (under 90 % useful, and the band at least 5 points better); their K split is chosen by
    // whole generations of the 512 block slots (256 CUs x 2): the fewest (generations x (chunks per split + one for the block's prologue / epilogue)),
    // plus the split partials' round trip through memory (~25 MB per chunk's time), instead of the rectangular tiles' "under 1.5 blocks per CU" rule
    const double rect = (double)B*ho*wo/((double)ceil_div(wo, s.TC)*s.TC*ceil_div(ho, s.TRB)*s.TRB*B);
    int BR = 0, S = 1;
    const double band = rect < 0.9 ? band_shape(B, CK, ho, wo, BR, S) : 0.0;
    if (band > rect + 0.05) {
      s.TC = 0; s.TRB = BR; s.S = S; s.NM = 1;
      s.gx = BR; s.gy = ceil_div(ho, BR); s.gz = ceil_div(B, S);
      s.out_elems = (size_t)B*M*ho*wo;
      const long long base = (long long)s.gy*s.gz*(M/32);
      double best = -1.0;
      for (int kcs = std::min(2, KC); kcs <= KC; ++kcs) {
        const int KS = ceil_div(KC, kcs);
        if (ceil_div(KC, KS) != kcs) continue;                    // (the same split count with fewer chunks per split)
        const double cost = (double)ceil_div(base*KS, 512ll)*(kcs + 1) + (KS > 1 ? (2.0*KS + 1.0)*s.out_elems*4.0/25e6 : 0.0);
        if (best < 0.0 || cost < best - 1e-9) { best = cost; s.kcs = kcs; s.KS = KS; }
      }
      s.grid = dim3(8*(unsigned)ceil_div(base*s.KS, 8ll));
      return s;
    }
  }
  const long long tiles = (long long)ceil_div(wo, s.TC)*ceil_div(ho, s.TRB)*B;
  s.NM = (M % 64 == 0 && tiles*(M/64) >= 256 && two_tiles) ? 2 : 1;   // two channel tiles over one patch where that still leaves a block per CU
  const long long base = tiles*(M/(32*s.NM));
  int ks = 1;
  if (base < 384) ks = (int)std::min<long long>(std::max(KC/2, 1), (512 + base - 1)/base);   // under 1.5 blocks per CU: split K, at least two chunks per split
  s.kcs = ceil_div(KC, ks); s.KS = ceil_div(KC, s.kcs);
  s.gx = ceil_div(wo, s.TC); s.gy = ceil_div(ho, s.TRB); s.gz = B;
  s.grid = dim3(8*(unsigned)ceil_div((long long)s.gx*s.gy*s.gz*(M/(32*s.NM))*s.KS, 8ll));
  s.out_elems = (size_t)B*M*ho*wo;
  return s;
}
// forward: CK = C, M = CO; data gradient: CK = CO, M = C, the output the padded size; the thin stage's 16-channel kernels (fwd CO = 16; data C = CO = 16) never split
size_t conv_mfma_split_elems(ConvOp op, bool zpad, int B, int C, int CO, int h, int w, bool two_tiles) {
  if (op == ConvOp::Wgt || !conv_mfma_served(op, zpad, C, CO) || (CO == 16 && (op == ConvOp::Fwd || C == 16))) return 0;
  const int e = zpad ? 0 : 2;
  const ConvShape s = op == ConvOp::Fwd ? conv_shape(B, C, CO, h, w, two_tiles) : conv_shape(B, CO, C, h + e, w + e, two_tiles);
  return s.KS > 1 ? (size_t)s.KS*s.out_elems : 0;
}

template <int P, int OFF, typename T>
static void launch_conv_form(const void* in, const void* wp, void* out, float* split_ws, int B, int CK, int M, int hi, int wi, int ho, int wo, bool two_tiles, hipStream_t st) {
  const ConvShape s = conv_shape(B, CK, M, ho, wo, two_tiles);
  const uint4* wq = (const uint4*)wp;
  const T* i_ = (const T*)in;
  T* dst = s.KS > 1 ? reinterpret_cast<T*>(split_ws) : (T*)out;    // (the kernel writes a split's partial output as fp32 whatever T)
  if (s.TC == 0) hipLaunchKernelGGL((k_conv_mfma<0, P, OFF, T, T, 1>), s.grid, dim3(256), 0, st, i_, wq, dst, CK, M, hi, wi, ho, wo, s.KS, s.kcs, s.out_elems, s.gx, s.gy, s.gz, s.S, B);
  else if (s.NM == 2) {
    if (s.TC == 64) hipLaunchKernelGGL((k_conv_mfma<64, P, OFF, T, T, 2>), s.grid, dim3(512), 0, st, i_, wq, dst, CK, M, hi, wi, ho, wo, s.KS, s.kcs, s.out_elems, s.gx, s.gy, s.gz, 1, B);
    else hipLaunchKernelGGL((k_conv_mfma<32, P, OFF, T, T, 2>), s.grid, dim3(512), 0, st, i_, wq, dst, CK, M, hi, wi, ho, wo, s.KS, s.kcs, s.out_elems, s.gx, s.gy, s.gz, 1, B);
  } else if (s.TC == 64) hipLaunchKernelGGL((k_conv_mfma<64, P, OFF, T, T, 1>), s.grid, dim3(256), 0, st, i_, wq, dst, CK, M, hi, wi, ho, wo, s.KS, s.kcs, s.out_elems, s.gx, s.gy, s.gz, 1, B);
  else hipLaunchKernelGGL((k_conv_mfma<32, P, OFF, T, T, 1>), s.grid, dim3(256), 0, st, i_, wq, dst, CK, M, hi, wi, ho, wo, s.KS, s.kcs, s.out_elems, s.gx, s.gy, s.gz, 1, B);
  if (s.KS > 1) {
    const size_t n4 = s.out_elems/4;                              // (B M ho wo is a multiple of 4: M is a multiple of 32)
    hipLaunchKernelGGL((k_conv_split_sum<T>), dim3((unsigned)((n4 + 255)/256)), dim3(256), 0, st, split_ws, (T*)out, n4, s.KS);
  }
}

#define SMD_BY_PIECES_F32(pieces, CALL) do { if ((pieces) == 3) { CALL(3); } else { CALL(2); } } while (0)   // the zero-padded forms: fp32 tensors only
// y (B, CO, h, w) = conv3x3(xp (B, C, h + 2, w + 2)), or zpad: conv2d(x (B, C, h, w), padding = 1); what is served: conv_mfma_served (smd_kernels.h)
hipError_t launch_conv_mfma_fwd(const void* x, const void* wp_fwd, void* y, float* split_ws, bool zpad, int B, int C, int CO, int h, int w, int pieces, bool two_tiles, hipStream_t st) {
  if (zpad) {
#define SMD_CALL(P) launch_conv_form<P, 1, float>(x, wp_fwd, y, split_ws, B, C, CO, h, w, h, w, two_tiles, st)
    SMD_BY_PIECES_F32(pieces, SMD_CALL);
#undef SMD_CALL
  } else if (CO == 16) {
#define SMD_CALL(P, T) launch_conv16<P, T>(x, wp_fwd, y, B, C, false, h + 2, w + 2, h, w, st)
    SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
  } else {
#define SMD_CALL(P, T) launch_conv_form<P, 0, T>(x, wp_fwd, y, split_ws, B, C, CO, h + 2, w + 2, h, w, two_tiles, st)
    SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
  }
  return hipGetLastError();
}
// g_xp (B, C, h + 2, w + 2) from g_y (B, CO, h, w), or zpad: g_x (B, C, h, w)
hipError_t launch_conv_mfma_bwd_data(const void* gy, const void* wp_bwd, void* g_x, float* split_ws, bool zpad, int B, int C, int CO, int h, int w, int pieces, bool two_tiles, hipStream_t st) {
  if (zpad) {
#define SMD_CALL(P) launch_conv_form<P, 1, float>(gy, wp_bwd, g_x, split_ws, B, CO, C, h, w, h, w, two_tiles, st)
    SMD_BY_PIECES_F32(pieces, SMD_CALL);
#undef SMD_CALL
  } else if (CO == 16 && C == 16) {
#define SMD_CALL(P, T) launch_conv16<P, T>(gy, wp_bwd, g_x, B, 16, true, h, w, h + 2, w + 2, st)
    SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
  } else {
#define SMD_CALL(P, T) launch_conv_form<P, 2, T>(gy, wp_bwd, g_x, split_ws, B, CO, C, h, w, h + 2, w + 2, two_tiles, st)
    SMD_BY_PIECES(pieces, SMD_CALL);
#undef SMD_CALL
  }
  return hipGetLastError();
}

}  // namespace smd

#ifdef SMD_CONV_TRACE
extern "C" int smd_debug_conv_trace(unsigned long long* host_out, int blocks) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(smd::g_conv_trace), (size_t)blocks*40*sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif
