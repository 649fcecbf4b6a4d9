// smd_maskrecon.hip — the image reconstruction loss with a predictive weighting mask (SfM-Learner's explainability mask, Klodt's uncertainty) in one forward
// and one backward sweep.  Replaces, for a criterion built with `mask_name`, `handlers.image_recon` (reference: src/core/handlers.py:14-67) on the un-fused
// operators: the warp of every support at every scale (`ViewSynth.forward`, src/tools/geometry.py:366-391), the photometric error of the warps and, for the
// automask, of the un-warped supports (`PhotoError`, src/losses/photometric.py:54-88), the mask applied to the per-support errors
// (`ReconstructionLoss.apply_mask`, src/losses/reconstruction.py:46-57), the reduction over the supports, the automask and the mean
// (src/losses/reconstruction.py:59-77, 79-96, 125).  Nothing of size (n, S, b, 3, h, w) or (n, S, b, h, w) is written: the plain route writes and reads back the
// warps and both error stacks, this one writes `sel`, one byte of static winner and a sum per block.
//
// The un-masked fused kernels (smd_recon_fwd.hip / smd_recon_bwd.hip) keep the identity error reduced over the supports; the mask weights the per-support
// identity errors BEFORE that reduction, so this is an operator of its own.  Its statements are those of the un-fused kernels (smd_unfused.hip), shared
// through smd_photo_dev.h and smd_common.h, in their order, so that `sel` is the plain route's pixel for pixel:
//   geometry   `pix_geom` + `make_taps` + `bilerp`: k_view_synth_fwd;
//   error      the nine-tap window sums walked rows first, `ssim_win_err`, `photo_mix` (weight 0.85) or the plain mean of |d|: k_photo_error_fwd.  PhotoError
//              pads the WARPED image by reflection, so the halo of a tile at an image border holds the warp of the mirrored pixel (its own depth, its own
//              projection), never a sample at an out-of-range coordinate;
//   reduce     `masked_err` on the warped and the static errors, min (first index wins) or mean over the supports, static + eps * noise, the two-way
//              minimum: k_recon_reduce_fwd.  The noise is the caller's tensor or `gauss_noise(seed, (s*b + bi)*h*w + pixel)`: equal seeds, equal noise.
//
// Forward, a block = a tile of 32 x 8 pixels of one (scale, sample): per support the warp of the tile and a halo of one goes to LDS (three channels), next to
// the target's and, with the automask, the un-warped support's; a barrier; every thread forms its pixel's errors from LDS.  The loss is the mean of the
// reduced error: one fp64 sum per block, added by a one-block second stage in a fixed order (`launch_sum_partials_f64`).  `stat` keeps the static winner where min and automask are both
// on: the backward reads decisions, it never re-decides.
//
// Backward, one sweep, per tile and support: the warp with a halo of two; the three SSIM coefficients of every pixel of the tile and a halo of one
// (k_photo_coef's statements, times the gradient `sel` and the mask route to that pixel's error); the adjoint of the reflection-padded 3x3 sum
// (k_photo_error_bwd) at the tile's pixels; the bilinear weights' derivatives and k_view_synth_bwd's statements to g_depth and the twelve pose sums per block,
// which `launch_pose_finalize` (smd_pose_fin.h) turns into g_T in fp64 in a fixed order.  g_mask is written directly for every element, the static branch
// included (k_recon_reduce_bwd).  <WT, WD, WM>: an instantiation without an output never forms its terms; what remains is the same statements (contraction is
// off in this file, so that no instantiation fuses what another does not).  No floating-point atomics: two runs give the same bits.
//
// LDS: three planes of (8 + 2R) x (32 + 2R) floats per image (R = 1 forward, 2 backward) and nine coefficient planes in the backward: 12 KB / 28 KB of the 160.
// A wave is two tile rows of 32 lanes; the 32 lanes of a half read consecutive floats of one LDS row, so no pitch gives a bank conflict.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_photo_dev.h"

#pragma clang fp contract(off)

namespace smd {

namespace {

constexpr int kMrTW = 32, kMrTH = 8, kMrBlock = kMrTW*kMrTH, kMrWaves = kMrBlock/64;
constexpr int kMrC = 3;

struct MrArgs {
  const float* depth; const float* mask; const float* tgt; const float* supp; const float* T; const float* K; const float* Kinv;
  const float* noise; uint8_t* sel; uint8_t* stat; float* warp; double* part;                          // forward
  const float* g_loss; float* g_depth; float* g_mask; float* pose_partial;                             // backward
  int b, n, S, h, w;
  int l1, use_min, automask, mask_mode;
  float wscale, hscale;
  uint32_t seed_lo, seed_hi;
};

// a plane of the tile with a halo of R, row-major
template <int R> struct Tile {
  static constexpr int PW = kMrTW + 2*R, PH = kMrTH + 2*R, N = PW*PH;
  float v[kMrC][PH][PW];
};

// The photometric error of the pixel whose tile coordinates in planes with a halo of R are (lx, ly) (k_photo_error_fwd's statements; x: prediction, y: target).
template <bool SSIM, int R>
__device__ __forceinline__ float photo_err(const Tile<R>& x, const Tile<R>& y, int lx, int ly, int l1) {
  float es = 0.f, el = 0.f;
#pragma unroll
  for (int c = 0; c < kMrC; ++c) {
    const float d = x.v[c][ly][lx] - y.v[c][ly][lx];
    el += fabsf(d);
    if (SSIM) {
      float sx, sxx, sxy, sy, syy;
      window_walk([&](int dv, int du, float& p, float& t) { p = x.v[c][ly + dv][lx + du]; t = y.v[c][ly + dv][lx + du]; }, sx, sxx, sxy, sy, syy);
      es += ssim_win_err(sx, sxx, sxy, sy, syy);
    }
  }
  const float rc = 1.f/(float)kMrC;
  return (!SSIM || l1) ? el*rc : photo_mix(es, el, rc, kWSsim);
}

// Position `idx` of a plane with a halo of R -> its local coordinates and the image pixel it holds (the mirrored one beyond a border); false where no window
// of an image pixel reads it (more than one beyond the image: the remainder of a border tile).
template <int R>
__device__ __forceinline__ bool halo_pos(int idx, int x0, int y0, int h, int w, int& lx, int& ly, int& gx, int& gy, bool& inside) {
  ly = idx/Tile<R>::PW; lx = idx - ly*Tile<R>::PW;
  const int rx = x0 + lx - R, ry = y0 + ly - R;
  inside = rx >= 0 && rx < w && ry >= 0 && ry < h;
  if (rx < -1 || rx > w || ry < -1 || ry > h) { gx = gy = 0; return false; }
  gx = reflect1(rx, w); gy = reflect1(ry, h);
  return true;
}

// the target's planes (and nothing else) of a tile
template <int R>
__device__ __forceinline__ void load_target(Tile<R>& tg, const float* __restrict__ tgt_b, int x0, int y0, int h, int w) {
  const size_t hw = (size_t)h*w;
  for (int idx = threadIdx.x; idx < Tile<R>::N; idx += kMrBlock) {
    int lx, ly, gx, gy; bool inside;
    const bool on = halo_pos<R>(idx, x0, y0, h, w, lx, ly, gx, gy, inside);
#pragma unroll
    for (int c = 0; c < kMrC; ++c) tg.v[c][ly][lx] = on ? tgt_b[(size_t)c*hw + (size_t)gy*w + gx] : 0.f;
  }
}

// the warp of support i (and, with STATIC, the un-warped support) of a tile: k_view_synth_fwd's statements at every position's image pixel
template <int R, bool STATIC, bool WARP>
__device__ __forceinline__ void synth_tile(Tile<R>& wp, Tile<R>& sp, const MrArgs& a, const Cam& cm, const float* __restrict__ depth_z,
                                           const float* __restrict__ supp_ib, float* __restrict__ warp_ib, int x0, int y0) {
  const int h = a.h, w = a.w;
  const size_t hw = (size_t)h*w;
  for (int idx = threadIdx.x; idx < Tile<R>::N; idx += kMrBlock) {
    int lx, ly, gx, gy; bool inside;
    const bool on = halo_pos<R>(idx, x0, y0, h, w, lx, ly, gx, gy, inside);
    if (!on) {
#pragma unroll
      for (int c = 0; c < kMrC; ++c) { wp.v[c][ly][lx] = 0.f; if (STATIC) sp.v[c][ly][lx] = 0.f; }
      continue;
    }
    const size_t pix = (size_t)gy*w + gx;
    const PixGeom g = pix_geom(cm, depth_z[pix], (float)gx, (float)gy, a.wscale, a.hscale);
    const Taps tp = make_taps(g.sx, g.sy, h, w, w);
    const bool own = WARP && warp_ib && inside && lx >= R && lx < R + kMrTW && ly >= R && ly < R + kMrTH;
#pragma unroll
    for (int c = 0; c < kMrC; ++c) {
      const float v = bilerp(supp_ib + (size_t)c*hw, tp, w);
      wp.v[c][ly][lx] = v;
      if (own) warp_ib[(size_t)c*hw + pix] = v;
      if (STATIC) sp.v[c][ly][lx] = supp_ib[(size_t)c*hw + pix];
    }
  }
}

// ------------------------------------------------------------------------------------------------- forward
template <bool SSIM, bool WARP>
__global__ __launch_bounds__(kMrBlock) void k_mask_recon_fwd(const MrArgs a) {
  constexpr int R = SSIM ? 1 : 0;
  __shared__ Tile<R> tg, wp, sp;
  __shared__ double red[kMrWaves];
  const int z = blockIdx.z, s = z/a.b, bi = z - s*a.b;
  const int h = a.h, w = a.w, n = a.n;
  const int x0 = blockIdx.x*kMrTW, y0 = blockIdx.y*kMrTH;
  const int tx = threadIdx.x & (kMrTW - 1), ty = threadIdx.x/kMrTW;
  const int x = x0 + tx, y = y0 + ty;
  const bool live = x < w && y < h;
  const size_t hw = (size_t)h*w, pix = (size_t)y*w + x, idx = (size_t)z*hw + pix;
  load_target<R>(tg, a.tgt + (size_t)bi*kMrC*hw, x0, y0, h, w);
  float best = 0.f, acc = 0.f, sb = 0.f, sa = 0.f;
  int bsel = 0, jstat = 0;
  for (int i = 0; i < n; ++i) {
    Cam cm;
    make_cam(cm, a.T + ((size_t)i*a.b + bi)*16, a.K + (size_t)bi*16, a.Kinv + (size_t)bi*16);
    const float* supp_ib = a.supp + ((size_t)i*a.b + bi)*kMrC*hw;
    float* warp_ib = WARP ? a.warp + ((size_t)i*a.b + bi)*kMrC*hw : nullptr;
    if (i) __syncthreads();      // the planes are written again
    if (a.automask) synth_tile<R, true, WARP>(wp, sp, a, cm, a.depth + (size_t)z*hw, supp_ib, (WARP && s == 0) ? warp_ib : nullptr, x0, y0);
    else synth_tile<R, false, WARP>(wp, sp, a, cm, a.depth + (size_t)z*hw, supp_ib, (WARP && s == 0) ? warp_ib : nullptr, x0, y0);
    __syncthreads();
    if (!live) continue;
    const float m = a.mask[((size_t)z*n + i)*hw + pix];
    const float v = masked_err(photo_err<SSIM, R>(wp, tg, tx + R, ty + R, a.l1), m, a.mask_mode);
    if (i == 0) { best = v; acc = v; }
    else { acc += v; if (v < best) { best = v; bsel = i; } }
    if (a.automask) {
      const float vs = masked_err(photo_err<SSIM, R>(sp, tg, tx + R, ty + R, a.l1), m, a.mask_mode);
      if (i == 0) { sb = vs; sa = vs; }
      else { sa += vs; if (vs < sb) { sb = vs; jstat = i; } }
    }
  }
  float e = 0.f;
  if (live) {
    e = a.use_min ? best : acc/(float)n;
    if (!a.use_min) bsel = 0;
    if (a.automask) {
      float est = a.use_min ? sb : sa/(float)n;
      est = fmaf(kEps32, a.noise ? a.noise[idx] : gauss_noise(a.seed_lo, a.seed_hi, (uint32_t)idx), est);
      if (est < e) { e = est; bsel = SMD_SEL_MASKED; }
      if (a.stat) a.stat[idx] = (uint8_t)jstat;
    }
    a.sel[idx] = (uint8_t)bsel;
  }
  block_store_sum<Waves::Sequential, kMrWaves, double>(live ? (double)e : 0.0, red, a.part + ((size_t)z*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------- backward
template <bool SSIM, bool WT, bool WD, bool WM>
__global__ __launch_bounds__(kMrBlock) void k_mask_recon_bwd(const MrArgs a) {
  constexpr int R = SSIM ? 2 : 0, RC = SSIM ? 1 : 0;       // halo of the images, of the coefficients
  constexpr int CW = kMrTW + 2*RC, CH = kMrTH + 2*RC;
  constexpr bool GEO = WT || WD;
  __shared__ Tile<R> tg, wp, sp;
  __shared__ float cf[SSIM && GEO ? 3*kMrC : 1][CH][CW];
  __shared__ float red[kMrWaves][kPoseSums];
  const int z = blockIdx.z, s = z/a.b, bi = z - s*a.b;
  const int h = a.h, w = a.w, n = a.n;
  const int x0 = blockIdx.x*kMrTW, y0 = blockIdx.y*kMrTH;
  const int tx = threadIdx.x & (kMrTW - 1), ty = threadIdx.x/kMrTW;
  const int x = x0 + tx, y = y0 + ty;
  const bool live = x < w && y < h;
  const size_t hw = (size_t)h*w, pix = (size_t)y*w + x, idx = (size_t)z*hw + pix;
  const unsigned blk = blockIdx.y*gridDim.x + blockIdx.x, nblk = gridDim.x*gridDim.y;
  const float g = a.g_loss[0]/(float)((size_t)a.S*a.b*hw), gn = g/(float)n;      // k_recon_reduce_bwd: g / total, / n for the mean
  const bool stat_on = WM && a.automask;
  load_target<R>(tg, a.tgt + (size_t)bi*kMrC*hw, x0, y0, h, w);
  int sq = SMD_SEL_MASKED, jq = 0;
  float D = 0.f, gd = 0.f;
  if (live) { sq = a.sel[idx]; D = a.depth[idx]; if (a.stat) jq = a.stat[idx]; }
  for (int i = 0; i < n; ++i) {
    Cam cm;
    make_cam(cm, a.T + ((size_t)i*a.b + bi)*16, a.K + (size_t)bi*16, a.Kinv + (size_t)bi*16);
    const float* supp_ib = a.supp + ((size_t)i*a.b + bi)*kMrC*hw;
    const float* mask_i = a.mask + ((size_t)z*n + i)*hw;
    if (i) __syncthreads();      // the planes are written again
    if (stat_on) synth_tile<R, true, false>(wp, sp, a, cm, a.depth + (size_t)z*hw, supp_ib, nullptr, x0, y0);
    else synth_tile<R, false, false>(wp, sp, a, cm, a.depth + (size_t)z*hw, supp_ib, nullptr, x0, y0);
    __syncthreads();
    if (SSIM && GEO) {
      // the three coefficients per channel of every image pixel of the tile and a halo of one (k_photo_coef)
      for (int q = threadIdx.x; q < CW*CH; q += kMrBlock) {
        const int cy = q/CW, cx = q - cy*CW;
        const int px = x0 + cx - RC, py = y0 + cy - RC;
        float ge = 0.f;
        if (px >= 0 && px < w && py >= 0 && py < h) {
          const size_t pp = (size_t)py*w + px;
          const float v = routed(a.sel[(size_t)z*hw + pp], i, g, gn, a.use_min);
          if (v != 0.f) { const float m = mask_i[pp]; ge = v*(a.mask_mode == 1 ? m : __expf(-m)); }
        }
        const float gc = ge*(kWSsim/(float)kMrC);
        const int lx = cx - RC + R, ly = cy - RC + R;
#pragma unroll
        for (int c = 0; c < kMrC; ++c) {
          float ca = 0.f, cb = 0.f, cc = 0.f;
          if (ge != 0.f && !a.l1) {
            float sx, sxx, sxy, sy, syy;
            window_walk([&](int dv, int du, float& p, float& t) { p = wp.v[c][ly + dv][lx + du]; t = tg.v[c][ly + dv][lx + du]; }, sx, sxx, sxy, sy, syy);
            ssim_win_coef(sx, sxx, sxy, sy, syy, gc, ca, cb, cc);
          }
          cf[c*3][cy][cx] = ca; cf[c*3 + 1][cy][cx] = cb; cf[c*3 + 2][cy][cx] = cc;
        }
      }
      __syncthreads();
    }
    float ps[kPoseSums] = {};
    if (live) {
      const int lx = tx + R, ly = ty + R;
      const float m = mask_i[pix];
      float v = routed(sq, i, g, gn, a.use_min);
      const float dm = a.mask_mode == 1 ? m : __expf(-m);      // d masked / d err
      if (WM) {
        const float gs = routed_static(sq, i, jq, g, gn, a.use_min, a.automask);      // reaches the masked STATIC error of support i
        const float ew = (v != 0.f) ? photo_err<SSIM, R>(wp, tg, lx, ly, a.l1) : 0.f;
        const float es = (gs != 0.f) ? photo_err<SSIM, R>(sp, tg, lx, ly, a.l1) : 0.f;
        a.g_mask[((size_t)z*n + i)*hw + pix] = a.mask_mode == 1 ? v*ew + gs*es : v*fmaf(-ew, dm, 1.f) + gs*fmaf(-es, dm, 1.f);      // (`mask_grad`, smd_photo_dev.h)
      }
      v *= dm;
      if (GEO) {
        // k_photo_error_bwd: the L1 term and the adjoint of (reflection pad + 3x3 sum) on the coefficient planes
        const float gl = v*((!SSIM || a.l1) ? 1.f : (1.f - kWSsim))/(float)kMrC;
        float wv[3], wu[3];
        reflect_weights_adj(y, h, wv[0], wv[2]); wv[1] = 1.f;
        reflect_weights_adj(x, w, wu[0], wu[2]); wu[1] = 1.f;
        const PixGeom pg = pix_geom(cm, D, (float)x, (float)y, a.wscale, a.hscale);
        const Taps tp = make_taps(pg.sx, pg.sy, h, w, w);
        float gsx = 0.f, gsy = 0.f;
#pragma unroll
        for (int c = 0; c < kMrC; ++c) {
          const float xv = wp.v[c][ly][lx], yv = tg.v[c][ly][lx];
          const float d = xv - yv;
          float gx = gl*sgn(d);
          if (SSIM && !a.l1) {
            float SA = 0.f, SB = 0.f, SC = 0.f;
#pragma unroll
            for (int dv = -1; dv <= 1; ++dv) {
              const int pv = y + dv;
              if (pv < 0 || pv >= h) continue;
#pragma unroll
              for (int du = -1; du <= 1; ++du) {
                const int pu = x + du;
                if (pu < 0 || pu >= w) continue;
                const float wt = wv[dv + 1]*wu[du + 1];
                const int cy = ty + RC + dv, cx = tx + RC + du;
                SA = fmaf(wt, cf[c*3][cy][cx], SA); SB = fmaf(wt, cf[c*3 + 1][cy][cx], SB); SC = fmaf(wt, cf[c*3 + 2][cy][cx], SC);
              }
            }
            gx += fmaf(2.f*xv, SB, fmaf(yv, SC, SA));
          }
          float ddx, ddy;
          (void)bilerp(supp_ib + (size_t)c*hw, tp, w, ddx, ddy);
          gsx = fmaf(gx, ddx, gsx); gsy = fmaf(gx, ddy, gsy);
        }
        // k_view_synth_bwd's statements
        float gnx, gny, gz;
        synth_adj(pg, tp, gsx, gsy, a.wscale, a.hscale, gnx, gny, gz);
        gd += synth_adj_depth(pg, gnx, gny, gz);
        if (WT) pose_sums(ps, gnx, gny, gz, D, (float)x, (float)y);
      }
    }
    if (WT) store_pose_sums<kMrWaves>(ps, &red[0][0], a.pose_partial + ((((size_t)i*a.b + bi)*a.S + s)*nblk + blk)*kPoseSums);
  }
  if (WD && live) a.g_depth[idx] = gd;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- host
// Sizes the kernels serve: 2 <= h, w <= 2048, 1 <= n <= SMD_MAX_SUPPORTS, 1 <= S <= SMD_MAX_SCALES, S*b <= 65535 (grid z), S*b*h*w < 2^31 (the noise index).
bool mask_recon_sizes_ok(int S, int b, int n, int h, int w) {
  if (S < 1 || b < 1 || n < 1 || h < 2 || w < 2) return false;
  if (S > SMD_MAX_SCALES || n > SMD_MAX_SUPPORTS || h > 2048 || w > 2048 || (long long)S*b > 65535) return false;
  return (size_t)S*b*h*w < ((size_t)1 << 31);
}
int mask_recon_tiles(int h, int w) { return ceil_div(w, kMrTW)*ceil_div(h, kMrTH); }

static MrArgs mr_args(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* Kinv,
                      int S, int b, int n, int h, int w, int flags) {
  MrArgs a = {};
  a.depth = depth; a.mask = mask; a.tgt = tgt; a.supp = supp; a.T = T; a.K = K; a.Kinv = Kinv;
  a.S = S; a.b = b; a.n = n; a.h = h; a.w = w;
  recon_switches(flags, a.l1, a.use_min, a.automask);
  a.mask_mode = (flags & SMD_MASK_UNCERTAINTY) ? 2 : 1;
  a.wscale = synth_scale(w); a.hscale = synth_scale(h);
  return a;
}

hipError_t launch_mask_recon_fwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* Kinv,
                                 const float* noise, uint64_t seed, float* loss, uint8_t* sel, uint8_t* stat, float* warp0, double* part,
                                 int S, int b, int n, int h, int w, int flags, hipStream_t st) {
  MrArgs a = mr_args(depth, mask, tgt, supp, T, K, Kinv, S, b, n, h, w, flags);
  a.noise = noise; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sel = sel; a.stat = (a.use_min && a.automask) ? stat : nullptr;
  a.warp = warp0; a.part = part;
  const dim3 grid(ceil_div(w, kMrTW), ceil_div(h, kMrTH), S*b);
  for_bool(!a.l1, [&](auto ss) { for_bool(warp0 != nullptr, [&](auto wr) {
    hipLaunchKernelGGL((k_mask_recon_fwd<decltype(ss)::value, decltype(wr)::value>), grid, dim3(kMrBlock), 0, st, a); }); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_sum_partials_f64(part, mask_recon_tiles(h, w)*S*b, 1.0/((double)S*b*h*w), loss, st);
}

hipError_t launch_mask_recon_bwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* Kinv,
                                 const uint8_t* sel, const uint8_t* stat, const float* g_loss, float* g_depth, float* g_mask, float* g_T, float* pose_partial,
                                 int S, int b, int n, int h, int w, int flags, hipStream_t st) {
  MrArgs a = mr_args(depth, mask, tgt, supp, T, K, Kinv, S, b, n, h, w, flags);
  a.sel = const_cast<uint8_t*>(sel); a.stat = (a.use_min && a.automask) ? const_cast<uint8_t*>(stat) : nullptr;
  a.g_loss = g_loss; a.g_depth = g_depth; a.g_mask = g_mask; a.pose_partial = pose_partial;
  const dim3 grid(ceil_div(w, kMrTW), ceil_div(h, kMrTH), S*b);
  for_bool(!a.l1, [&](auto ss) { for_bool(g_T != nullptr, [&](auto wt) { for_bool(g_depth != nullptr, [&](auto wd) { for_bool(g_mask != nullptr, [&](auto wm) {
    hipLaunchKernelGGL((k_mask_recon_bwd<decltype(ss)::value, decltype(wt)::value, decltype(wd)::value, decltype(wm)::value>), grid, dim3(kMrBlock), 0, st, a);
  }); }); }); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !g_T) return e;
  const int per_sample = S*mask_recon_tiles(h, w);
  return launch_pose_finalize(pose_partial, per_sample, per_sample, T, K, Kinv, g_T, nullptr, nullptr, b, n, st);
}

}  // namespace smd
