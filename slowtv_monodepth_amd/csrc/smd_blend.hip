// smd_blend.hip — Monodepth's flip-and-blend post-process (reference: blend_stereo, src/tools/geometry.py:94-129, followed by the disparity half of
// to_scaled, src/tools/geometry.py:63-76) over a whole pyramid in one launch, and its adjoint.
//
//   m_l = the caller's ramp (w,): clamp(20 (linspace(0,1,w) - 0.05), 0, 1) with torch's bits       m_r[j] = m_l[w-1-j]       m_mu = (1 - m_l) - m_r
//   out = (m_r l + m_l r) + m_mu ((l + r)/2)                 [out = scale out + offset]
//
// `r` is the prediction for the mirrored image.  With SMD_BLEND_MIRROR it arrives as the network wrote it and the kernel reads r_raw[w-1-j]: the
// `flip` copy of the reference is never made.  The adjoint is written from the side of the INCOMING gradient: the thread that owns columns j..j+3 of a
// row stores g_l[j..j+3] and the four values of g_r_raw at the mirrored columns, so every output element is written exactly once, by one thread, from
// one product chain: no atomics, no sums whose order could move, two runs are bit-equal.
//
// Streaming shape: two reads and one write per element and nothing to reuse, so a thread owns groups of four columns of one row and moves them as
// 16-byte vectors; the mirrored operand is the 16-byte vector at the mirrored address with its lanes swapped in registers.  A group is moved as a vector
// only where every address it touches is 16-byte aligned — decided per group from the pointers, since an operand may be a storage-offset view and a row
// of a width that is no multiple of four starts anywhere; all other groups, and the w % 4 columns at the end of a row, go element by element.  The ramp
// is w floats that every row re-reads: it stays in the caches.
//
// The grid is one dimension over (level, chunk of kBlendItems groups) units, large levels first: the 1x3 level of a pyramid is one more block of the
// launch, not a launch.  Every product and sum is a separately rounded fp32 operation (contraction is switched off where they are written): the reference's ATen sequence has no
// fused multiply-add, and with the ramp's bits shared the kernel repeats its roundings one for one.
#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

namespace {

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ f4 reversed(f4 v) { return f4{v.w, v.z, v.y, v.x}; }

// (hipcc's __fmul_rn / __fadd_rn are plain `*` and `+` compiled with contraction allowed: the pragma is what keeps the roundings apart, as in smd_metrics.hip)
template <bool SCALE> __device__ __forceinline__ float blend1(float l, float r, float ml, float mr, float scale, float offset) {
#pragma clang fp contract(off)
  const float mmu = (1.f - ml) - mr;
  const float mu = (l + r)*0.5f;
  const float a = mr*l, b = ml*r, c = mmu*mu;
  float o = (a + b) + c;
  if (SCALE) { const float t = scale*o; o = t + offset; }
  return o;
}

// d out / d l and d out / d r at one column, times the incoming gradient, in autograd's order: (g m_r) + (g m_mu)/2 and (g m_l) + (g m_mu)/2
template <bool SCALE> __device__ __forceinline__ void blend1_adj(float g, float ml, float mr, float scale, float& gl, float& gr) {
#pragma clang fp contract(off)
  if (SCALE) g = g*scale;
  const float mmu = (1.f - ml) - mr;
  const float half = (g*mmu)*0.5f;
  const float a = g*mr, b = g*ml;
  gl = a + half;
  gr = b + half;
}

// the level of unit `u` and the unit's index inside it (S <= 8: a scalar scan)
__device__ __forceinline__ int level_of(const BlendSet& bs, int u, int& local) {
  int s = 0;
  while (s + 1 < bs.S && u >= bs.unit0[s + 1]) ++s;
  local = u - bs.unit0[s];
  return s;
}

}  // namespace

template <bool MIRROR, bool SCALE>
__global__ __launch_bounds__(256) void k_flip_blend_fwd(const BlendSet bs, float scale, float offset) {
  int local;
  const int s = level_of(bs, blockIdx.x, local);
  const int w = bs.w[s], ng = bs.ng[s];
  const unsigned items = (unsigned)bs.rows[s]*(unsigned)ng;                   // < 2^31: blend_plan refuses more
  const float* __restrict__ L = bs.a[s];
  const float* __restrict__ R = bs.b[s];
  const float* __restrict__ M = bs.ramp[s];
  float* __restrict__ O = bs.o0[s];
  const unsigned first = (unsigned)local*kBlendItems;
  const unsigned last = items - first > kBlendItems ? first + kBlendItems : items;
  for (unsigned it = first + threadIdx.x; it < last; it += 256) {
    const int row = (int)(it/(unsigned)ng), c0 = (int)(it - (unsigned)row*(unsigned)ng)*4;
    const size_t base = (size_t)row*w;
    const int cm = w - 4 - c0;                           // first column of the mirrored group (>= 0 where the group is whole)
    const float* pl = L + base + c0;
    const float* pr = R + base + (MIRROR ? cm : c0);
    float* po = O + base + c0;
    if (c0 + 4 <= w && aligned16(pl) && aligned16(pr) && aligned16(po) && aligned16(M + c0) && aligned16(M + cm)) {
      const f4 l = *(const f4*)pl, ml = *(const f4*)(M + c0), mr = reversed(*(const f4*)(M + cm));
      f4 r = *(const f4*)pr;
      if (MIRROR) r = reversed(r);
      f4 o;
      o.x = blend1<SCALE>(l.x, r.x, ml.x, mr.x, scale, offset); o.y = blend1<SCALE>(l.y, r.y, ml.y, mr.y, scale, offset);
      o.z = blend1<SCALE>(l.z, r.z, ml.z, mr.z, scale, offset); o.w = blend1<SCALE>(l.w, r.w, ml.w, mr.w, scale, offset);
      *(f4*)po = o;
    } else {
      const int n = w - c0 < 4 ? w - c0 : 4;
      for (int i = 0; i < n; ++i) {
        const int j = c0 + i, jm = w - 1 - j;
        O[base + j] = blend1<SCALE>(L[base + j], R[base + (MIRROR ? jm : j)], M[j], M[jm], scale, offset);
      }
    }
  }
}

template <bool MIRROR, bool SCALE>
__global__ __launch_bounds__(256) void k_flip_blend_bwd(const BlendSet bs, float scale) {
  int local;
  const int s = level_of(bs, blockIdx.x, local);
  const int w = bs.w[s], ng = bs.ng[s];
  const unsigned items = (unsigned)bs.rows[s]*(unsigned)ng;                   // < 2^31: blend_plan refuses more
  const float* __restrict__ G = bs.a[s];
  const float* __restrict__ M = bs.ramp[s];
  float* __restrict__ GL = bs.o0[s];
  float* __restrict__ GR = bs.o1[s];
  const unsigned first = (unsigned)local*kBlendItems;
  const unsigned last = items - first > kBlendItems ? first + kBlendItems : items;
  for (unsigned it = first + threadIdx.x; it < last; it += 256) {
    const int row = (int)(it/(unsigned)ng), c0 = (int)(it - (unsigned)row*(unsigned)ng)*4;
    const size_t base = (size_t)row*w;
    const int cm = w - 4 - c0;
    const float* pg = G + base + c0;
    float* pgl = GL ? GL + base + c0 : nullptr;
    float* pgr = GR ? GR + base + (MIRROR ? cm : c0) : nullptr;
    if (c0 + 4 <= w && aligned16(pg) && aligned16(pgl) && aligned16(pgr) && aligned16(M + c0) && aligned16(M + cm)) {
      const f4 g = *(const f4*)pg, ml = *(const f4*)(M + c0), mr = reversed(*(const f4*)(M + cm));
      float l4[4], r4[4];
      blend1_adj<SCALE>(g.x, ml.x, mr.x, scale, l4[0], r4[0]); blend1_adj<SCALE>(g.y, ml.y, mr.y, scale, l4[1], r4[1]);
      blend1_adj<SCALE>(g.z, ml.z, mr.z, scale, l4[2], r4[2]); blend1_adj<SCALE>(g.w, ml.w, mr.w, scale, l4[3], r4[3]);
      const f4 gl = {l4[0], l4[1], l4[2], l4[3]}, gr = {r4[0], r4[1], r4[2], r4[3]};
      if (pgl) *(f4*)pgl = gl;
      if (pgr) *(f4*)pgr = MIRROR ? reversed(gr) : gr;
    } else {
      const int n = w - c0 < 4 ? w - c0 : 4;
      for (int i = 0; i < n; ++i) {
        const int j = c0 + i, jm = w - 1 - j;
        float gl, gr;
        blend1_adj<SCALE>(G[base + j], M[j], M[jm], scale, gl, gr);
        if (GL) GL[base + j] = gl;
        if (GR) GR[base + (MIRROR ? jm : j)] = gr;
      }
    }
  }
}

// rows, groups per row and the first unit of every level; -> the number of units (0: a level of 2^31 elements or more, or 2^31 units)
long blend_plan(BlendSet& bs, const int* hs, const int* ws, int S, int planes) {
  long units = 0;
  bs.S = S;
  for (int s = 0; s < S; ++s) {
    const long rows = (long)planes*hs[s], ng = (ws[s] + 3)/4;
    if (rows*ws[s] >= (1L << 31)) return 0;
    bs.rows[s] = (int)rows; bs.w[s] = ws[s]; bs.ng[s] = (int)ng;
    bs.unit0[s] = (int)units;
    units += (rows*ng + kBlendItems - 1)/kBlendItems;
    if (units >= (1L << 31)) return 0;
  }
  bs.unit0[S] = (int)units;
  return units;
}

hipError_t launch_flip_blend_fwd(const BlendSet& bs, int flags, float scale, float offset, hipStream_t st) {
  const dim3 grid((unsigned)bs.unit0[bs.S]);
  for_bool(flags & SMD_BLEND_MIRROR, [&](auto mirror) {
    for_bool(flags & SMD_BLEND_SCALE, [&](auto scaled) {
      hipLaunchKernelGGL((k_flip_blend_fwd<decltype(mirror)::value, decltype(scaled)::value>), grid, dim3(256), 0, st, bs, scale, offset);
    });
  });
  return hipGetLastError();
}

hipError_t launch_flip_blend_bwd(const BlendSet& bs, int flags, float scale, hipStream_t st) {
  const dim3 grid((unsigned)bs.unit0[bs.S]);
  for_bool(flags & SMD_BLEND_MIRROR, [&](auto mirror) {
    for_bool(flags & SMD_BLEND_SCALE, [&](auto scaled) {
      hipLaunchKernelGGL((k_flip_blend_bwd<decltype(mirror)::value, decltype(scaled)::value>), grid, dim3(256), 0, st, bs, scale);
    });
  });
  return hipGetLastError();
}

}  // namespace smd
