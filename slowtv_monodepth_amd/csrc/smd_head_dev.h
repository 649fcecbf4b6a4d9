// smd_head_dev.h — what the one-channel output head (smd_conv_head.hip) and the n-channel one (smd_conv_headn.hip) share: the tile constants and the
// three-element row reader.
#pragma once
#include "smd_common.h"

namespace smd {

constexpr int kHeadRows = 4;                   // output rows per thread: (kHeadRows + 2) x 3 loads feed 9 kHeadRows multiply-adds per channel
constexpr int kHeadTileW = 64, kHeadTileH = 4*kHeadRows;   // a block of 256 threads: 64 columns x 4 row groups
constexpr long long kHeadEnoughWaves = 4096;   // four generations of waves on the chip: below that a launch is a chain of latencies, split the channels as well

// Three consecutive elements of a padded row for a thread's column.  bfloat16 with an even row pitch (every decoder level: w is even): the two ALIGNED dwords that
// hold them and a funnel shift by the column's parity, the aligned base and the parity computed once per thread (2-byte loads made the bf16 forward three times
// slower than the fp32 one on half the bytes: 152 vs 50 us at 16 -> 1, 384x640).
template <typename TX, bool DW> struct Row3 {             // DW: bfloat16 rows read as aligned dwords (chosen at launch: even pitch); no run-time branch around a load
  const TX* base; size_t e0; unsigned par;                // (offsets from the tensor's base, a 4-byte-aligned kernel argument: the pointer never passes through an integer —
                                                          // that made every load a flat_load with vmcnt(0) behind it and cost 222 registers)
  __device__ __forceinline__ Row3(const TX* base_, size_t e0_) : base(base_), e0(e0_), par((unsigned)(e0_ & 1)) {}
  __device__ __forceinline__ void next_channel(size_t elems) { e0 += elems; }    // (an even number of elements: the parity stays)
  // the loads of a channel's rows are all issued before the first is converted (left to the scheduler the dword form waited after every row: 23 waits per three
  // channels where the fp32 form has 5)
  __device__ __forceinline__ void request(size_t row_off, unsigned& d0, unsigned& d1) const {
    const unsigned* pw = reinterpret_cast<const unsigned*>(base) + (e0 >> 1) + (row_off >> 1);   // (the pitch is even: the lane's part and the wave-uniform row part separate)
    d0 = pw[0]; d1 = pw[1];
  }
  __device__ __forceinline__ void unpack(unsigned d0, unsigned d1, float& a, float& b, float& c) const {
    const unsigned r = __builtin_amdgcn_alignbit(d1, d0, par*16), t = d1 >> (par*16);
    a = __builtin_bit_cast(float, r << 16); b = __builtin_bit_cast(float, r & 0xffff0000u); c = __builtin_bit_cast(float, t << 16);
  }
  __device__ __forceinline__ void load(size_t row_off, float& a, float& b, float& c) const {   // row_off: elements from the thread's first row (a multiple of the pitch)
    if constexpr (DW) { unsigned d0, d1; request(row_off, d0, d1); unpack(d0, d1, a, b, c); }
    else { a = ld_as_float<TX>(base, e0 + row_off); b = ld_as_float<TX>(base, e0 + row_off + 1); c = ld_as_float<TX>(base, e0 + row_off + 2); }
  }
};

}  // namespace smd
