// smd_conv_mfma_dev.h — the stages the split-bf16 matrix-core convolutions share, each written once: block order, the D-fragment row map, the swizzled
// LDS patch and its stager, the product sequence, the weight gradients' shifted fragments, the LDS-DMA load and the K-step pair reduction.  The scheme is
// described in smd_conv_mfma.hip, the arithmetic (the split and the products kept) is smd_split_dev.h.  Users: smd_conv_mfma.hip, smd_conv_wgrad.hip,
// smd_conv_stem.hip, smd_ddv.hip.
#pragma once
#include "smd_common.h"
#include "smd_split_dev.h"

namespace smd {

typedef float f32x4v __attribute__((ext_vector_type(4)));

// bfloat16 tensors (the decoder under bf16 autocast, `pieces` = 1): an element IS its one piece — loaded as 16 raw bits, two of them a dword
template <int P> __device__ __forceinline__ void split_pair(unsigned short a, unsigned short b, unsigned (&p)[P]) {
  static_assert(P == 1, "bfloat16 operands have one piece");
  p[0] = (unsigned)a | ((unsigned)b << 16);
}
template <typename T> struct RawOf { typedef float type; };                  // what a staging load leaves in a register
template <> struct RawOf<bf16> { typedef unsigned short type; };

// Block -> logical block id (channel tile, K split, tile column, tile row, sample: the caller's decode), XCD-aware: the hardware deals consecutive workgroup
// ids round-robin to the 8 XCDs, each with its own L2.  Here XCD k works through the k-th eighth of the tile list in order, so the blocks in flight on an XCD
// are neighbours in the image — the halo rows / columns two tiles share, and the one patch the channel tiles of a pixel tile all read, come from HBM once
// (the natural order sends every neighbour to another L2: 329 MB fetched for a 145 MB input at cfg 2's 96 -> 32 layer).  The grid is a multiple of 8
// blocks: an id at or past nblk means "no work", the block returns.
__device__ __forceinline__ unsigned xcd_block_id(unsigned nblk) {
  const unsigned per = (nblk + 7)/8;
  return (blockIdx.x & 7)*per + (blockIdx.x >> 3);
}

// D of `v_mfma_f32_32x32x16_bf16`: register r (0 .. 15) of a lane of group g = lane >> 5 holds this row of column lane & 31
__device__ __forceinline__ constexpr int mfma32_row(int r, int g) { return (r & 3) + 8*(r >> 2) + 4*g; }

// one MFMA of the accumulator's shape: 16 registers -> 32x32x16, 4 -> 16x16x32
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4v mfma_bf16(bf16x8 a, bf16x8 b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// The product sequence over NA x NB accumulator tiles: product t of every tile before product t + 1 of any (no MFMA waits for the one before it).  The
// leading product a0 b0 and the five small ones run in accumulators of their own: adding a term 2^-8 or 2^-16 the size of the sum costs a rounding of the
// SUM's size, so six products in one accumulator carry six times the roundings of one (measured: 2.5e-6 of the output's max at K = 4608 against MIOpen's
// 6e-7; split: 1.0e-6 against 6e-7 there, at or below MIOpen's elsewhere); the small accumulator's roundings are 2^-8 of that.
template <int P, int NA, int NB, typename Acc>
__device__ __forceinline__ void split_mfma(const bf16x8 (&A)[NA][P], const bf16x8 (&B)[NB][P], Acc (&acc)[NA][NB], Acc (&lo)[NA][NB]) {
  constexpr int NPROD = n_products(P);
#pragma unroll
  for (int t = 0; t < NPROD; ++t)
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (t == NPROD - 1) acc[a][b] = mfma_bf16(A[a][0], B[b][0], acc[a][b]);
        else lo[a][b] = mfma_bf16(A[a][prod_a(P, t)], B[b][prod_b(P, t)], lo[a][b]);
      }
}
template <int P, int NB, typename Acc>                            // one A tile
__device__ __forceinline__ void split_mfma(const bf16x8 (&A)[P], const bf16x8 (&B)[NB][P], Acc (&acc)[NB], Acc (&lo)[NB]) {
  constexpr int NPROD = n_products(P);
#pragma unroll
  for (int t = 0; t < NPROD; ++t)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (t == NPROD - 1) acc[b] = mfma_bf16(A[0], B[b][0], acc[b]);
      else lo[b] = mfma_bf16(A[prod_a(P, t)], B[b][prod_b(P, t)], lo[b]);
    }
}
template <int P, typename Acc>                                    // one tile
__device__ __forceinline__ void split_mfma(const bf16x8 (&A)[P], const bf16x8 (&B)[P], Acc& acc, Acc& lo) {
  constexpr int NPROD = n_products(P);
#pragma unroll
  for (int t = 0; t < NPROD; ++t) {
    if (t == NPROD - 1) acc = mfma_bf16(A[0], B[0], acc);
    else lo = mfma_bf16(A[prod_a(P, t)], B[prod_b(P, t)], lo);
  }
}
// the weight gradients' form: every product into the one accumulator of its tile (K = pixels: the sums are short), acc[0 .. NB - 1]
template <int P, int NB, typename Acc>
__device__ __forceinline__ void split_mfma_sum(const bf16x8 (&A)[P], const bf16x8 (&B)[NB][P], Acc* acc) {
#pragma unroll
  for (int t = 0; t < n_products(P); ++t)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = mfma_bf16(A[prod_a(P, t)], B[b][prod_b(P, t)], acc[b]);
}

// ---- the LDS patch of the forward / data-gradient forms: [piece][pixel][half], a half = 8 of the chunk's 16 channels of one pixel (16 bytes) ----
// The two 16-byte halves of a pixel are swapped where bit 3 of the pixel index is set: the 16-lane groups that serve a ds_read_b128 ({0-3, 12-15,
// 20-27}, ...) then cover all 64 banks instead of colliding two ways.
__device__ __forceinline__ int patch_slot(int pix, int half) { return pix*2 + (half ^ ((pix >> 3) & 1)); }

// Staging of a patch of NPIX pixels by NT threads: an item = 8 channels of one patch pixel; its address inside a channel plane does not depend on the chunk
// (`pofs`: offset inside the plane, or -1: outside).  ZERO: reads outside the image are zeros; else they are clamped to any valid address (those outputs
// are not stored).  The caller owns the registers the loads land in (R v[TRIPS][8]) and decides when a chunk is requested and when each trip is filed.
template <int NT, int NPIX, int P, typename R, bool ZERO>
struct PatchStager {
  static constexpr int ITEMS = 2*NPIX, TRIPS = (ITEMS + NT - 1)/NT, kBuf = P*NPIX*2;   // kBuf: uint4 of one patch
  int pofs[TRIPS];
  static __device__ __forceinline__ int item(int t) { return min(t*NT + (int)threadIdx.x, ITEMS - 1); }
  // rectangular patch, PW pixels wide, whose pixel (0, 0) is input pixel (y0 - off, x0 - off)
  template <int PW> __device__ __forceinline__ void rect_offsets(int y0, int x0, int off, int hi, int wi) {
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int it = item(t), half = it >= NPIX ? 1 : 0, pix = it - half*NPIX;
      const int r = pix/PW, cc = pix - r*PW;
      const int yy = y0 + r - off, xx = x0 + cc - off;
      if (ZERO) pofs[t] = (yy >= 0 && yy < hi && xx >= 0 && xx < wi) ? yy*wi + xx : -1;
      else pofs[t] = min(yy, hi - 1)*wi + min(xx, wi - 1);
    }
  }
  // every load of chunk kc (16 channels from `src`) is issued before anything waits for one
  __device__ __forceinline__ void request(const R* src, size_t plane, int kc, R (&v)[TRIPS][8]) const {
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int half = item(t) >= NPIX ? 1 : 0;
      const R* p = src + (size_t)(kc*16 + half*8)*plane + (size_t)max(pofs[t], 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[t][e] = (!ZERO || pofs[t] >= 0) ? p[(size_t)e*plane] : R(0);
    }
  }
  // split trip t's eight values ONCE per element and file them in patch `buf` of `tile`
  __device__ __forceinline__ void file_trip(uint4* tile, int buf, int t, const R (&v)[TRIPS][8]) const {
    const int it = t*NT + (int)threadIdx.x;
    if (it < ITEMS) {
      const int half = it >= NPIX ? 1 : 0, pix = it - half*NPIX;
      unsigned pk[4][P];
#pragma unroll
      for (int q = 0; q < 4; ++q) split_pair<P>(v[t][2*q], v[t][2*q + 1], pk[q]);
      const int slot = patch_slot(pix, half);
#pragma unroll
      for (int p = 0; p < P; ++p) tile[buf*kBuf + p*NPIX*2 + slot] = uint4{pk[0][p], pk[1][p], pk[2][p], pk[3][p]};
    }
  }
  __device__ __forceinline__ void file(uint4* tile, int buf, const R (&v)[TRIPS][8]) const {
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) file_trip(tile, buf, t, v);
  }
  // the P fragments of patch pixel `pix`, channel half `half`
  static __device__ __forceinline__ void read(const uint4* tile, int buf, int pix, int half, bf16x8 (&dst)[P]) {
    const int slot = patch_slot(pix, half);
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = as_frag(tile[buf*kBuf + p*NPIX*2 + slot]);
  }
};

// ---- the weight gradients ----
// Five consecutive dwords (ten bf16 of a row) -> the fragments of the three taps kx = 0, 1, 2: elements 0 .. 7, 1 .. 8 (a funnel shift, v_alignbit), 2 .. 9
__device__ __forceinline__ void shifted_frags(unsigned d0, unsigned d1, unsigned d2, unsigned d3, unsigned d4, bf16x8& k0, bf16x8& k1, bf16x8& k2) {
  k0 = as_frag(uint4{d0, d1, d2, d3});
  k1 = as_frag(uint4{__builtin_amdgcn_alignbit(d1, d0, 16), __builtin_amdgcn_alignbit(d2, d1, 16), __builtin_amdgcn_alignbit(d3, d2, 16), __builtin_amdgcn_alignbit(d4, d3, 16)});
  k2 = as_frag(uint4{d1, d2, d3, d4});
}

// LDS-DMA: each lane's dword at (rsrc, voffset + soffset) lands at LDS byte lds_dst + 4 lane (out of range: zero); m0 is restored
__device__ __forceinline__ void lds_dma_dword(const rsrc_t& rsrc, unsigned voffset, unsigned soffset, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voffset), "s"(rsrc), "s"(soffset), "s"(lds_dst) : "memory");
}

// The two waves of a pair hold the two K steps' halves of the same NT accumulator tiles: the second parks its accumulators in `red` (LDS, free by now:
// 64 NT sizeof(Acc) bytes per pair), one barrier, the first adds them to its own and hands every sum to store(t, v, sum) where `keep` (this lane's column exists).
template <int NT, typename Acc, typename Store>
__device__ __forceinline__ void pair_reduce_store(float* red, int pair, bool second, bool keep, int lane, const Acc (&acc)[NT], Store store) {
  constexpr int NV = sizeof(Acc)/sizeof(float);
  if (second) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < NV; ++v) red[((pair*NT + t)*NV + v)*64 + lane] = acc[t][v];
  }
  __syncthreads();
  if (!second && keep) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < NV; ++v) store(t, v, acc[t][v] + red[((pair*NT + t)*NV + v)*64 + lane]);
  }
}

}  // namespace smd
