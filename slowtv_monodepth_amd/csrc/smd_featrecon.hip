// smd_featrecon.hip — FeatDepth's feature-metric reconstruction loss (reference: `handlers.feat_recon`, src/core/handlers.py:70-119) from the LOW-resolution
// features: the bilinear up-sampling of the target and support features to the depth map, the warp of the up-sampled supports (`ViewSynth`), the dense
// l1 / l2 error (`DenseL1Error` / `DenseL2Error`, src/losses/photometric.py:11-20), the static error of the automask and `ReconstructionLoss`'s reduction
// over the supports (src/losses/reconstruction.py:43-44, 59-77, 125) in one sweep.  Nothing of size (C, H, W) is written unless the caller asks for the warp.
//
// Per full-resolution pixel (x, y) and support i, in the order of the un-fused operators (smd_unfused.hip):
//   geometry   the projection of k_view_synth_fwd -> (sx, sy) -> `make_taps`: the north-west full-resolution tap (x0, y0) and the fractions (fx, fy);
//   up-sample  ATen's `upsample_bilinear2d(align_corners=False)`: source = max(r (d + 0.5) - 0.5, 0), r = in/out, taps (i0, i0 + [i0 < in - 1]), weight l1 = source - i0;
//   warp       the four neighbours U(x0 + j, y0 + i), i, j in {0, 1}, are up-samples of the support's low-resolution plane L, formed on the fly in ATen's statement.
//              For a ratio in/out <= 1 the low-resolution taps of two adjacent full-resolution columns (rows) lie in three adjacent columns (rows): nine loads per
//              channel, indices and weights once per (pixel, support); then `bilerp`'s statement (smd_common.h) on the four values, as k_view_synth_fwd;
//   errors     d = warp - target (target: the four-tap up-sample at (x, y)); l1: sum_c |d| / C, l2: sqrt(max(sum_c d^2, eps)); with the automask the same against
//              the un-warped up-sample of the support at (x, y);
//   reduce     k_recon_reduce_fwd's statements: min (first index wins ties) or mean over the supports, the static candidate + eps * noise, sel = 255 where it wins.
//              The noise is the caller's tensor or `gauss_noise(seed, b*H*W index)` (smd_common.h), as in smd_recon_reduce_fwd: equal seeds draw equal noise.
// The loss is the mean of the reduced error: one fp64 sum per block, added by a one-block second stage in a fixed order (`launch_sum_partials_f64`; no atomics, bit-reproducible).
//
// Backward, one sweep: `sel` names the support(s) that carry a gradient (the winner for min, all for mean, none where the automask won).  For those the samples
// are recomputed together with d warp / d fx and d warp / d fy (the same nine loads), summed over the channels into d err / d sx, d err / d sy, and pushed through
// k_view_synth_bwd's statements to g_depth and the twelve pose sums per (support, sample) and block, which `launch_pose_finalize` (smd_pose_fin.h) turns into
// g_T in fp64 in a fixed order.  <WT, WD>: the instantiation without g_T never forms the pose sums, the one without g_depth never stores it; the arithmetic of
// what remains is the same statements (contraction is off in this file, so that no instantiation fuses what another does not).
//
// Shape: a block is 64 columns x 4 rows (a wave per row, lanes along x): its four rows share their low-resolution rows, four adjacent lanes their target-side
// taps, and the L1 holds the few hundred bytes per channel they touch.  The feature tensors are read through buffer resources (base + size in SGPRs, the
// channel plane as the scalar offset, the tap as the per-lane offset: DESIGN §3); an offset outside the tensor would read 0 instead of faulting.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_photo_dev.h"

#pragma clang fp contract(off)

namespace smd {

namespace {

constexpr int kFrCols = 64, kFrRows = 4, kFrBlock = kFrCols*kFrRows;

// (the projection `pix_geom`, the dense errors, the reduction over the supports and ViewSynth's adjoint: smd_photo_dev.h, the un-fused operators' own statements)

// ATen's bilinear up-sampling along one axis (align_corners=False): out[d] = (1 - l1) in[i0] + l1 in[i1]
struct UpTap { int i0, i1; float l1; };
__device__ __forceinline__ UpTap up_tap(int d, float r, int n_in) {
  const float s = fmaxf(fmaf(r, (float)d + 0.5f, -0.5f), 0.f);
  UpTap t;
  t.i0 = min((int)s, n_in - 1);
  t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
  t.l1 = s - (float)t.i0;
  return t;
}

// One axis of the warp: the full-resolution taps d0 and d0 + 1 as ATen up-samples them, on three low-resolution slots idx[] = min(i0(d0) + {0, 1, 2}, n_in - 1):
// tap d0 reads slots (0, 1) with weights (1 - la, la), tap d0 + 1 slots (delta, delta + 1) with (1 - lb, lb), delta = i0(d0 + 1) - i0(d0) in {0, 1}.
struct Axis3 { int idx[3]; float la, lb; int delta; };
__device__ __forceinline__ Axis3 make_axis(int d0, float r, int n_in) {
  const UpTap ta = up_tap(d0, r, n_in), tb = up_tap(d0 + 1, r, n_in);
  Axis3 ax;
  ax.delta = min(max(tb.i0 - ta.i0, 0), 1);      // 0 or 1 for every size the entry points accept: tests/test_featrecon_host.py checks every (n_out <= kFrMaxSize, n_in, d)
  ax.la = ta.l1; ax.lb = tb.l1;
#pragma unroll
  for (int k = 0; k < 3; ++k) ax.idx[k] = min(ta.i0 + k, n_in - 1);
  return ax;
}

struct FrArgs {
  const float* depth; const float* feat; const float* supp; const float* T; const float* K; const float* Kinv;
  const float* noise; uint8_t* sel; float* warp; double* part;                                         // forward
  const float* g_loss; float* g_depth; float* pose_partial;                                            // backward
  int b, n, C, H, W, hf, wf;
  int l1, use_min, automask;
  float wscale, hscale, rx, ry;
  uint32_t seed_lo, seed_hi;
};

// the four-tap up-sample of one low-resolution plane (ATen's statement: h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11))
struct Up4 { unsigned o00, o01, o10, o11; float w0, w1, h0, h1; };
__device__ __forceinline__ Up4 make_up4(int x, int y, const FrArgs& a) {
  const UpTap tx = up_tap(x, a.rx, a.wf), ty = up_tap(y, a.ry, a.hf);
  Up4 u;
  u.o00 = (unsigned)(ty.i0*a.wf + tx.i0)*4u; u.o01 = (unsigned)(ty.i0*a.wf + tx.i1)*4u;
  u.o10 = (unsigned)(ty.i1*a.wf + tx.i0)*4u; u.o11 = (unsigned)(ty.i1*a.wf + tx.i1)*4u;
  u.w1 = tx.l1; u.w0 = 1.f - tx.l1; u.h1 = ty.l1; u.h0 = 1.f - ty.l1;
  return u;
}
__device__ __forceinline__ float up4(rsrc_t r, const Up4& u, unsigned plane) {
  const float v00 = bld(r, u.o00, plane), v01 = bld(r, u.o01, plane), v10 = bld(r, u.o10, plane), v11 = bld(r, u.o11, plane);
  const float top = fmaf(u.w1, v01, u.w0*v00), bot = fmaf(u.w1, v11, u.w0*v10);
  return fmaf(u.h1, bot, u.h0*top);
}

// the warp's nine taps: the four full-resolution neighbours U(x0 + j, y0 + i) in ATen's statement, then `bilerp`'s (smd_common.h) on them
struct Warp9 { unsigned o[3][3]; float xa0, xa1, xb0, xb1, ya0, ya1, yb0, yb1, fx, fy; int dx, dy; };
__device__ __forceinline__ Warp9 make_warp9(const Taps& tp, int W, const FrArgs& a) {
  const int y0 = tp.off/W, x0 = tp.off - y0*W;
  const Axis3 cx = make_axis(x0, a.rx, a.wf), cy = make_axis(y0, a.ry, a.hf);
  Warp9 w;
  w.xa1 = cx.la; w.xa0 = 1.f - cx.la; w.xb1 = cx.lb; w.xb0 = 1.f - cx.lb; w.dx = cx.delta;
  w.ya1 = cy.la; w.ya0 = 1.f - cy.la; w.yb1 = cy.lb; w.yb0 = 1.f - cy.lb; w.dy = cy.delta;
  w.fx = tp.fx; w.fy = tp.fy;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) w.o[k][l] = (unsigned)(cy.idx[k]*a.wf + cx.idx[l])*4u;
  return w;
}
// -> U(x0, y0), U(x0 + 1, y0), U(x0, y0 + 1), U(x0 + 1, y0 + 1)
__device__ __forceinline__ void corners9(rsrc_t r, const Warp9& w, unsigned plane, float& u00, float& u01, float& u10, float& u11) {
  float ha[3], hb[3];      // the horizontal half per low-resolution row: columns x0 and x0 + 1
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float l0 = bld(r, w.o[k][0], plane), l1 = bld(r, w.o[k][1], plane), l2 = bld(r, w.o[k][2], plane);
    ha[k] = fmaf(w.xa1, l1, w.xa0*l0);
    hb[k] = fmaf(w.xb1, w.dx ? l2 : l1, w.xb0*(w.dx ? l1 : l0));
  }
  u00 = fmaf(w.ya1, ha[1], w.ya0*ha[0]); u01 = fmaf(w.ya1, hb[1], w.ya0*hb[0]);
  u10 = fmaf(w.yb1, w.dy ? ha[2] : ha[1], w.yb0*(w.dy ? ha[1] : ha[0]));
  u11 = fmaf(w.yb1, w.dy ? hb[2] : hb[1], w.yb0*(w.dy ? hb[1] : hb[0]));
}
__device__ __forceinline__ float warp9(rsrc_t r, const Warp9& w, unsigned plane) {
  float u00, u01, u10, u11;
  corners9(r, w, plane, u00, u01, u10, u11);
  const float top = fmaf(w.fx, u01 - u00, u00), bot = fmaf(w.fx, u11 - u10, u10);
  return fmaf(w.fy, bot - top, top);
}
// ... and its derivatives with respect to the fractions (fx, fy)
__device__ __forceinline__ float warp9(rsrc_t r, const Warp9& w, unsigned plane, float& ddx, float& ddy) {
  float u00, u01, u10, u11;
  corners9(r, w, plane, u00, u01, u10, u11);
  const float top = fmaf(w.fx, u01 - u00, u00), bot = fmaf(w.fx, u11 - u10, u10);
  ddx = fmaf(w.fy, (u11 - u10) - (u01 - u00), u01 - u00);
  ddy = bot - top;
  return fmaf(w.fy, bot - top, top);
}

// ------------------------------------------------------------------------------------------------- forward
template <bool WARP>
__global__ __launch_bounds__(kFrBlock) void k_feat_recon_fwd(const FrArgs a) {
  __shared__ double red[kFrRows];
  const int bi = blockIdx.z;
  const int x = blockIdx.x*kFrCols + (threadIdx.x & 63), y = blockIdx.y*kFrRows + (threadIdx.x >> 6);
  const bool live = x < a.W && y < a.H;
  const size_t HW = (size_t)a.H*a.W, pix = (size_t)y*a.W + x;
  const unsigned plane = (unsigned)(a.hf*a.wf)*4u;
  const rsrc_t rt = make_rsrc(a.feat, (size_t)a.b*a.C*plane), rs = make_rsrc(a.supp, (size_t)a.n*a.b*a.C*plane);
  const float rc = 1.f/(float)a.C;
  float e = 0.f;
  float best = 0.f, acc = 0.f, sb = 0.f, sa = 0.f;
  int bsel = 0;
  Up4 ut = {};
  float D = 0.f;
  if (live) { ut = make_up4(x, y, a); D = a.depth[(size_t)bi*HW + pix]; }
  for (int i = 0; i < a.n; ++i) {
    Cam cm;
    make_cam(cm, a.T + ((size_t)i*a.b + bi)*16, a.K + (size_t)bi*16, a.Kinv + (size_t)bi*16);
    if (!live) continue;
    const PixGeom g = pix_geom(cm, D, (float)x, (float)y, a.wscale, a.hscale);
    const Taps tp = make_taps(g.sx, g.sy, a.H, a.W, a.W);
    const Warp9 w9 = make_warp9(tp, a.W, a);
    const unsigned pt0 = (unsigned)bi*(unsigned)a.C*plane, ps0 = ((unsigned)i*(unsigned)a.b + (unsigned)bi)*(unsigned)a.C*plane;
    float w1 = 0.f, w2 = 0.f, s1 = 0.f, s2 = 0.f;
    float* wp = WARP ? a.warp + (((size_t)i*a.b + bi)*a.C)*HW + pix : nullptr;
    for (int c = 0; c < a.C; ++c) {
      const unsigned pt = pt0 + (unsigned)c*plane, ps = ps0 + (unsigned)c*plane;
      const float t = up4(rt, ut, pt);
      const float v = warp9(rs, w9, ps);
      if (WARP) wp[(size_t)c*HW] = v;
      const float d = v - t;
      w1 += fabsf(d); w2 = fmaf(d, d, w2);
      if (a.automask) {
        const float ds = up4(rs, ut, ps) - t;
        s1 += fabsf(ds); s2 = fmaf(ds, ds, s2);
      }
    }
    const float ew = dense_err(w1, w2, a.l1, rc), es = dense_err(s1, s2, a.l1, rc);
    if (i == 0) { best = ew; acc = ew; sb = es; sa = es; }
    else {
      acc += ew; if (ew < best) { best = ew; bsel = i; }
      sa += es; sb = fminf(sb, es);
    }
  }
  if (live) {
    e = a.use_min ? best : acc/(float)a.n;
    if (!a.use_min) bsel = 0;
    if (a.automask) {
      const size_t idx = (size_t)bi*HW + pix;
      float est = a.use_min ? sb : sa/(float)a.n;
      est = fmaf(kEps32, a.noise ? a.noise[idx] : gauss_noise(a.seed_lo, a.seed_hi, (uint32_t)idx), est);
      if (est < e) { e = est; bsel = SMD_SEL_MASKED; }
    }
    a.sel[(size_t)bi*HW + pix] = (uint8_t)bsel;
  }
  block_store_sum<Waves::Sequential, kFrRows, double>(live ? (double)e : 0.0, red, a.part + ((size_t)bi*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------- backward
template <bool WT, bool WD>
__global__ __launch_bounds__(kFrBlock) void k_feat_recon_bwd(const FrArgs a) {
  __shared__ float red[kFrRows][kPoseSums];
  const int bi = blockIdx.z;
  const int x = blockIdx.x*kFrCols + (threadIdx.x & 63), y = blockIdx.y*kFrRows + (threadIdx.x >> 6);
  const bool live = x < a.W && y < a.H;
  const size_t HW = (size_t)a.H*a.W, pix = (size_t)y*a.W + x;
  const unsigned plane = (unsigned)(a.hf*a.wf)*4u;
  const rsrc_t rt = make_rsrc(a.feat, (size_t)a.b*a.C*plane), rs = make_rsrc(a.supp, (size_t)a.n*a.b*a.C*plane);
  const unsigned blk = blockIdx.y*gridDim.x + blockIdx.x, nblk = gridDim.x*gridDim.y;
  const float gq = a.g_loss[0]/(float)((size_t)a.b*HW);                      // k_recon_reduce_bwd: g / total, / n for the mean
  const float ge = a.use_min ? gq : gq/(float)a.n;
  Up4 ut = {};
  float D = 0.f, gd = 0.f;
  int s = SMD_SEL_MASKED;
  if (live) { ut = make_up4(x, y, a); D = a.depth[(size_t)bi*HW + pix]; s = a.sel[(size_t)bi*HW + pix]; }
  for (int i = 0; i < a.n; ++i) {
    Cam cm;
    make_cam(cm, a.T + ((size_t)i*a.b + bi)*16, a.K + (size_t)bi*16, a.Kinv + (size_t)bi*16);
    float ps[kPoseSums] = {};
    if (live && (a.use_min ? s == i : s != SMD_SEL_MASKED)) {
      const float uf = (float)x, vf = (float)y;
      const PixGeom g = pix_geom(cm, D, uf, vf, a.wscale, a.hscale);
      const Taps tp = make_taps(g.sx, g.sy, a.H, a.W, a.W);
      const Warp9 w9 = make_warp9(tp, a.W, a);
      const unsigned pt0 = (unsigned)bi*(unsigned)a.C*plane, ps0 = ((unsigned)i*(unsigned)a.b + (unsigned)bi)*(unsigned)a.C*plane;
      float e2 = 0.f, sx_ = 0.f, sy_ = 0.f;
      for (int c = 0; c < a.C; ++c) {
        const float t = up4(rt, ut, pt0 + (unsigned)c*plane);
        float ddx, ddy;
        const float d = warp9(rs, w9, ps0 + (unsigned)c*plane, ddx, ddy) - t;
        if (a.l1) {
          const float sg = sgn(d);
          sx_ = fmaf(sg, ddx, sx_); sy_ = fmaf(sg, ddy, sy_);
        } else {
          e2 = fmaf(d, d, e2); sx_ = fmaf(d, ddx, sx_); sy_ = fmaf(d, ddy, sy_);
        }
      }
      // d err / d warp_c = d / sqrt(e2) (0 where clamp(min=eps) is active: k_photo_error_bwd) | sign(d) / C
      const float k = a.l1 ? ge/(float)a.C : dense_l2_gfac(ge, e2);
      float gnx, gny, gz;
      synth_adj(g, tp, k*sx_, k*sy_, a.wscale, a.hscale, gnx, gny, gz);
      gd += synth_adj_depth(g, gnx, gny, gz);
      if (WT) pose_sums(ps, gnx, gny, gz, D, uf, vf);
    }
    if (WT) {
      store_pose_sums<kFrRows>(ps, &red[0][0], a.pose_partial + (((size_t)i*a.b + bi)*nblk + blk)*kPoseSums);
      __syncthreads();      // `red` is written again for the next support
    }
  }
  if (WD && live) a.g_depth[(size_t)bi*HW + pix] = gd;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- host
// Sizes the kernels serve: 2 <= H, W <= kFrMaxSize (up to it the fp32 source coordinates of two adjacent columns lie at most one low-resolution column apart:
// their exact values differ by r <= 1 - 1/2048 or by exactly 1 and half an ulp below 2048 is 2^-14; checked exhaustively on the host by
// tests/test_featrecon_host.py.  Nothing beyond it is claimed), hf <= H, wf <= W, n <= SMD_MAX_SUPPORTS, b*H*W < 2^31, every feature tensor below 4 GiB (32-bit buffer offsets).
constexpr int kFrMaxSize = 2048;
bool feat_recon_sizes_ok(int b, int n, int C, int H, int W, int hf, int wf) {
  if (b < 1 || n < 1 || C < 1 || H < 2 || W < 2 || hf < 1 || wf < 1) return false;
  if (n > SMD_MAX_SUPPORTS || b > 65535 || H > kFrMaxSize || W > kFrMaxSize || hf > H || wf > W) return false;
  if ((size_t)b*H*W >= ((size_t)1 << 31)) return false;
  if ((size_t)n*b*C*hf*wf*sizeof(float) >= ((size_t)1 << 32)) return false;
  return true;
}
int feat_recon_blocks(int b, int H, int W) { return ceil_div(W, kFrCols)*ceil_div(H, kFrRows)*b; }

static FrArgs fr_args(const float* depth, const float* feat, const float* supp, const float* T, const float* K, const float* Kinv, int b, int n, int C, int H, int W,
                      int hf, int wf, int flags) {
  FrArgs a = {};
  a.depth = depth; a.feat = feat; a.supp = supp; a.T = T; a.K = K; a.Kinv = Kinv;
  a.b = b; a.n = n; a.C = C; a.H = H; a.W = W; a.hf = hf; a.wf = wf;
  recon_switches(flags, a.l1, a.use_min, a.automask);
  a.wscale = synth_scale(W); a.hscale = synth_scale(H);
  a.rx = (float)wf/(float)W; a.ry = (float)hf/(float)H;                                              // ATen: area_pixel_compute_scale<float>
  return a;
}

hipError_t launch_feat_recon_fwd(const float* depth, const float* feat, const float* supp, const float* T, const float* K, const float* Kinv, const float* noise,
                                 uint64_t seed, float* loss, uint8_t* sel, float* warp, double* part, int b, int n, int C, int H, int W, int hf, int wf, int flags,
                                 hipStream_t st) {
  FrArgs a = fr_args(depth, feat, supp, T, K, Kinv, b, n, C, H, W, hf, wf, flags);
  a.noise = noise; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sel = sel; a.warp = warp; a.part = part;
  const dim3 grid(ceil_div(W, kFrCols), ceil_div(H, kFrRows), b);
  for_bool(warp != nullptr, [&](auto w) { hipLaunchKernelGGL((k_feat_recon_fwd<decltype(w)::value>), grid, dim3(kFrBlock), 0, st, a); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_sum_partials_f64(part, feat_recon_blocks(b, H, W), 1.0/((double)b*H*W), loss, st);
}

hipError_t launch_feat_recon_bwd(const float* depth, const float* feat, const float* supp, const float* T, const float* K, const float* Kinv, const uint8_t* sel,
                                 const float* g_loss, float* g_depth, float* g_T, float* pose_partial, int b, int n, int C, int H, int W, int hf, int wf, int flags,
                                 hipStream_t st) {
  FrArgs a = fr_args(depth, feat, supp, T, K, Kinv, b, n, C, H, W, hf, wf, flags);
  a.sel = const_cast<uint8_t*>(sel); a.g_loss = g_loss; a.g_depth = g_depth; a.pose_partial = pose_partial;
  const dim3 grid(ceil_div(W, kFrCols), ceil_div(H, kFrRows), b);
  if (g_T && g_depth) hipLaunchKernelGGL((k_feat_recon_bwd<true, true>), grid, dim3(kFrBlock), 0, st, a);
  else if (g_T) hipLaunchKernelGGL((k_feat_recon_bwd<true, false>), grid, dim3(kFrBlock), 0, st, a);
  else hipLaunchKernelGGL((k_feat_recon_bwd<false, true>), grid, dim3(kFrBlock), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !g_T) return e;
  const int per_sample = (int)(grid.x*grid.y);
  return launch_pose_finalize(pose_partial, per_sample, per_sample, T, K, Kinv, g_T, nullptr, nullptr, b, n, st);
}

}  // namespace smd
