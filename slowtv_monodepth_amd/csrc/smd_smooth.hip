// smd_smooth.hip — edge-aware disparity smoothness over the whole scale pyramid, forward and adjoint.
//
// Restates `handlers.disp_smooth` (src/core/handlers.py:262-281): per scale s, resize the target image to the
// disparity's size (bilinear, align_corners=False), `SmoothReg.forward` (src/regularizers/smooth.py:71-97) with
// `ops.mean_normalize` (src/tools/ops.py:279-286) and `compute_grad` (smooth.py:12-30), then mean_s(loss_s / 2^s).
// All scales run in one launch per phase (the reference issues ~170 launches here).
//
// Per image the loss is E/N with E = sum_edges w|dhat_p - dhat_q|, dhat = d / max(mean(d), eps).  E is 1-homogeneous
// in dhat, so sum_p (dE/ddhat_p) dhat_p = E and the mean-normalisation term of the adjoint needs only (mean, E):
//   dL/dd_q = g_s/N * [ G_q / m  -  [mean >= eps] * E / (m * hs*ws) ],   G_q = dE/ddhat_q.
#include <stdlib.h>
#include <string.h>

#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_smooth_dev.h"

namespace smd {

// kSmoothChunk (pixels per block, smd_kernels.h) / 256 pixels per thread

__device__ __forceinline__ void src_index_s(int dst, float scale, int n_in, int& i0, int& i1, float& l1) {
  float src = fmaxf(fmaf(scale, (float)dst + 0.5f, -0.5f), 0.f);
  i0 = min((int)src, n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// Bilinearly resized target image at low-res pixel (v, u), three channels.
__device__ __forceinline__ void img_at(const float* __restrict__ img, int h, int w, int hs, int ws, int v, int u, float out[3]) {
  if (hs == h && ws == w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = img[(size_t)c*h*w + (size_t)v*w + u];
    return;
  }
  int y0, y1, x0, x1; float ly, lx;
  src_index_s(v, (float)h/(float)hs, h, y0, y1, ly);
  src_index_s(u, (float)w/(float)ws, w, x0, x1, lx);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = img + (size_t)c*h*w;
    float p00 = p[(size_t)y0*w + x0], p01 = p[(size_t)y0*w + x1], p10 = p[(size_t)y1*w + x0], p11 = p[(size_t)y1*w + x1];
    out[c] = (1.f - ly)*((1.f - lx)*p00 + lx*p01) + ly*((1.f - lx)*p10 + lx*p11);
  }
}

// Frame-only half (round 4): the edge weights {exp(-mean_c |dI/dx|), exp(-mean_c |dI/dy|)} of every pyramid level depend on the target
// frames alone — `SmoothReg` resizes the image to each level and differentiates it (src/core/handlers.py:272-277, smooth.py:12-30,
// 91-94) — so they are computed by a launch of their own that the trainer enqueues with the reconstruction's frame-only prep, under
// the networks; the sweep over the disparities (k_smooth_main) and the adjoint then read 8 bytes per pixel and never touch the image.
// Streaming form: a wave owns 63 columns + one halo lane and walks down kSmoothRows rows; the (resized) image pixel is computed once
// per pixel — 3 loads at the image's own scale, 6 eight-byte tap pairs at the coarser ones; the right-hand neighbour is the next lane
// (DPP), the neighbour below the next row's registers.  Also zeroes the arrival counters of the sweep's in-launch second stage.
__global__ __launch_bounds__(256) void k_smooth_edges(const ScaleSet sc, int b, const float* __restrict__ img, int h, int w, float* __restrict__ edge_w,
                                                      unsigned* __restrict__ arrive) {
  const int s = sc.S - 1 - (int)blockIdx.z, bi = blockIdx.y;   // coarse scales first (few pixels, strided taps: the longest latency chains)
  if (arrive != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
    for (int e = threadIdx.x; e < sc.S*b + 2; e += 256) arrive[e] = 0u;   // pairs, pairs done, loss combination (fused loss path)
  const int lane = threadIdx.x & 63, unit = blockIdx.x*4 + (threadIdx.x >> 6);
  const int hs = sc.hs[s], ws = sc.ws[s], n = hs*ws;
  if (unit >= smooth_units_of(hs, ws)) return;
  const int nsx = (ws + kSmoothCols - 1)/kSmoothCols;
  const int sxi = unit % nsx, syi = unit/nsx;
  const int r0 = syi*kSmoothRows, r1 = min(r0 + kSmoothRows, hs);
  const int u = sxi*kSmoothCols + lane, uc = min(u, ws - 1);        // lanes right of the image repeat its last column
  const bool live = lane < kSmoothCols && u < ws;
  const float* __restrict__ im = img + (size_t)bi*3*h*w;
  const bool ident = (hs == h && ws == w);
  float2* __restrict__ ew = (float2*)edge_w + edge_offset(sc, b, s) + (size_t)bi*n;
  // horizontal half of the bilinear resize: constant per lane
  int x0 = uc, x1 = uc; float lx = 0.f;
  if (!ident) src_index_s(uc, (float)w/(float)ws, w, x0, x1, lx);
  const bool pair = (x1 == x0 + 1);                                  // false only where the right tap is clamped onto the left one
  const size_t hw = (size_t)h*w;
  struct Row { float ic[3]; };
  auto load_row = [&](int v) {
    Row r;
    if (ident) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r.ic[c] = im[(size_t)c*hw + (size_t)v*w + uc];
    } else {
      int y0, y1; float ly;
      src_index_s(v, (float)h/(float)hs, h, y0, y1, ly);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* p0 = im + (size_t)c*hw + (size_t)y0*w + x0;
        const float* p1 = im + (size_t)c*hw + (size_t)y1*w + x0;
        // the two columns are adjacent: one 8-byte (4-byte aligned) load per image row; p0[1] / p1[1] stay inside the plane
        // because x0 + 1 <= w - 1 whenever `pair` holds
        typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
        float p00, p01, p10, p11;
        if (pair) { const f2u a = *(const f2u*)p0, bb = *(const f2u*)p1; p00 = a.x; p01 = a.y; p10 = bb.x; p11 = bb.y; }
        else { p00 = p0[0]; p01 = p00; p10 = p1[0]; p11 = p10; }
        r.ic[c] = (1.f - ly)*((1.f - lx)*p00 + lx*p01) + ly*((1.f - lx)*p10 + lx*p11);
      }
    }
    return r;
  };
  // every row of the strip (and the one below it) is requested before the first is used: the loop is latency-shaped
  Row rows[kSmoothRows + 1];
#pragma unroll
  for (int k = 0; k <= kSmoothRows; ++k) rows[k] = load_row(min(r0 + k, hs - 1));   // the last image row pairs with itself
#pragma unroll
  for (int k = 0; k < kSmoothRows; ++k) {
    const int v = r0 + k;
    const Row& cur = rows[k];
    const Row& nxt = rows[k + 1];
    const float ir0 = lane_right(cur.ic[0]), ir1 = lane_right(cur.ic[1]), ir2 = lane_right(cur.ic[2]);
    const float wx = __expf(-(fabsf(cur.ic[0] - ir0) + fabsf(cur.ic[1] - ir1) + fabsf(cur.ic[2] - ir2))*(1.f/3.f));
    const float wy = __expf(-(fabsf(cur.ic[0] - nxt.ic[0]) + fabsf(cur.ic[1] - nxt.ic[1]) + fabsf(cur.ic[2] - nxt.ic[2]))*(1.f/3.f));
    if (live && v < r1) ew[(size_t)v*ws + u] = make_float2(wx, wy);
  }
}

// The sweep over the disparities as a kernel of its own (body: smd_smooth_dev.h).
__global__ __launch_bounds__(256) void k_smooth_main(const ScaleSet sc, int b, const SmoothFwdJob jb) { smooth_main_block(sc, b, jb, (int)blockIdx.x); }

// Second stage as a launch of its own (used when the pyramid has more (scale, sample) pairs than arrival slots): per image mean m
// and E = E'/max(m, eps) -> stats; loss = mean_s( 2^-key_s * sum_b E / (b*hs*ws) ).  One wave per pair, 16 waves, one block.
__global__ __launch_bounds__(1024) void k_smooth_finalize(const ScaleSet sc, int b, const float* __restrict__ partial, int max_chunks,
                                                          float* __restrict__ stats, float* __restrict__ loss, int per_pixel_units) {
  // (Tried in round 4: requesting the partials of a wave's three pairs before summing the first — 8.2 us instead of 6.7: the kernel is
  // launch + a few dependent round trips whichever way they are arranged.)
  __shared__ double contrib[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double mine = 0.0;
  for (int pair = wv; pair < sc.S*b; pair += 16) {
    const int s = pair/b;
    const int n = sc.hs[s]*sc.ws[s];
    const int chunks = per_pixel_units ? ceil_div(n, 256) : smooth_units_main(sc.hs[s], sc.ws[s]);
    double e = 0.0, dsum = 0.0;
    const float2* __restrict__ pp = (const float2*)partial + (size_t)pair*max_chunks;
    int c = lane;
    for (; c + 192 < chunks; c += 256) {   // four independent loads in flight; the order of the additions is fixed
      const float2 v0 = pp[c], v1 = pp[c + 64], v2 = pp[c + 128], v3 = pp[c + 192];
      e += ((double)v0.x + (double)v1.x) + ((double)v2.x + (double)v3.x); dsum += ((double)v0.y + (double)v1.y) + ((double)v2.y + (double)v3.y);
    }
    for (; c < chunks; c += 64) { const float2 v = pp[c]; e += (double)v.x; dsum += (double)v.y; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { e += __shfl_xor(e, off, 64); dsum += __shfl_xor(dsum, off, 64); }
    const float mean = (float)(dsum/n);
    const float E = (float)(e/(double)fmaxf(mean, kEps32));
    if (lane == 0) { stats[(size_t)pair*2] = mean; stats[(size_t)pair*2 + 1] = E; }
    mine += ldexp((double)E/((double)b*n), -sc.key[s]);   // 2^-key exactly, without the double-precision exp2 routine
  }
  if (lane == 0) contrib[wv] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int k = 0; k < 16; ++k) total += contrib[k];
    loss[0] = (float)(total/sc.S);
  }
}


// ---------------------------------------------------------------------------------------------
// SmoothReg(use_laplacian=True) (src/regularizers/smooth.py:33-48): second-order differences
//   a[u] = |x[u] - x[u+1]| (0 in the last column),  xx[u] = |a[u] - a[u+1]| (0 in the last column),  likewise in y.
// Still 1-homogeneous in the disparity, so the mean-normalisation algebra of the first-order form carries over unchanged
// (E = E'/m; the adjoint needs only (mean, E) and signs).  No BASELINE configuration enables it: one thread per pixel, the
// two-launch second stage; the edge weights exp(-image xx), exp(-image yy) are always cached for the adjoint.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float lap1(float x0, float x1, float x2, int i, int n) {   // xx at position i of a line of n values x0 = x[i], x1 = x[i+1], x2 = x[i+2]
  if (i >= n - 1) return 0.f;
  const float a0 = fabsf(x0 - x1), a1 = (i + 1 < n - 1) ? fabsf(x1 - x2) : 0.f;
  return fabsf(a0 - a1);
}

__global__ __launch_bounds__(256) void k_smooth_lap_main(const ScaleSet sc, int b, const float* __restrict__ img, int h, int w, int flags,
                                                         float* __restrict__ partial, int max_units, float* __restrict__ edge_w) {
  __shared__ float red[2*4];
  const int s = blockIdx.z, bi = blockIdx.y;
  const int hs = sc.hs[s], ws = sc.ws[s], n = hs*ws;
  const int pix = blockIdx.x*256 + threadIdx.x;
  if ((int)blockIdx.x*256 >= n) return;
  const float* __restrict__ d = sc.p[s] + (size_t)bi*n;
  const float* __restrict__ im = img + (size_t)bi*3*h*w;
  const bool edges = flags & SMD_USE_EDGES;
  float2* __restrict__ ew = (edges && edge_w) ? (float2*)edge_w + edge_offset(sc, b, s) + (size_t)bi*n : nullptr;
  float e = 0.f, dsum = 0.f;
  if (pix < n) {
    const int v = pix/ws, u = pix - v*ws;
    auto D = [&](int vv, int uu) { return d[(size_t)min(vv, hs - 1)*ws + min(uu, ws - 1)]; };
    const float dc = D(v, u);
    const float dxx = lap1(dc, D(v, u + 1), D(v, u + 2), u, ws), dyy = lap1(dc, D(v + 1, u), D(v + 2, u), v, hs);
    float wx = 1.f, wy = 1.f;
    if (edges) {
      float c0[3], r1[3], r2[3], b1[3], b2[3];
      img_at(im, h, w, hs, ws, v, u, c0);
      img_at(im, h, w, hs, ws, v, min(u + 1, ws - 1), r1); img_at(im, h, w, hs, ws, v, min(u + 2, ws - 1), r2);
      img_at(im, h, w, hs, ws, min(v + 1, hs - 1), u, b1); img_at(im, h, w, hs, ws, min(v + 2, hs - 1), u, b2);
      float ix = 0.f, iy = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) { ix += lap1(c0[c], r1[c], r2[c], u, ws); iy += lap1(c0[c], b1[c], b2[c], v, hs); }
      wx = __expf(-ix*(1.f/3.f)); wy = __expf(-iy*(1.f/3.f));
      if (ew) ew[pix] = make_float2(wx, wy);
    }
    e = dxx*wx + dyy*wy; dsum = dc;
  }
  block_sum2<Waves::Sequential, 4>(e, dsum, red);
  if (threadIdx.x == 0) {
    float* pp = partial + (((size_t)s*b + bi)*max_units + blockIdx.x)*2;
    pp[0] = e; pp[1] = dsum;
  }
}

// dE'/dd at pixel i of a line (un-normalised disparities x[-2..2] around it, weights wgt[-2..0] of the three terms that contain it)
__device__ __forceinline__ float lap1_grad(const float x[5], const float wgt[3], int i, int n) {
  auto sg = [](float t) { return (t > 0.f) ? 1.f : ((t < 0.f) ? -1.f : 0.f); };
  float G = 0.f;
#pragma unroll
  for (int t = -2; t <= 0; ++t) {                 // term at position p = i + t: | a[p] - a[p+1] |, a[k] = |x[k] - x[k+1]| (0 for k >= n-1)
    const int p = i + t;
    if (p < 0 || p >= n - 1) continue;
    const float xa = x[t + 2], xb = x[t + 3], xc = (t + 4 <= 4) ? x[t + 4] : 0.f;       // x[p], x[p+1], x[p+2]
    const float a0 = fabsf(xa - xb), a1 = (p + 1 < n - 1) ? fabsf(xb - xc) : 0.f;
    // d a0 / d x[i]: i == p -> sg(xa - xb), i == p+1 -> -sg(xa - xb);  d a1 / d x[i]: i == p+1 -> sg(xb - xc), i == p+2 -> -sg(xb - xc)
    float da0 = 0.f, da1 = 0.f;
    if (t == 0) da0 = sg(xa - xb);
    else if (t == -1) { da0 = -sg(xa - xb); if (p + 1 < n - 1) da1 = sg(xb - xc); }
    else if (p + 1 < n - 1) da1 = -sg(xb - xc);
    G = fmaf(wgt[t + 2]*sg(a0 - a1), da0 - da1, G);
  }
  return G;
}

__global__ __launch_bounds__(256) void k_smooth_lap_bwd(const ScaleSet sc, int b, int flags, const float* __restrict__ stats, const float* __restrict__ g_loss,
                                                        const float* __restrict__ edge_w) {
  const int s = blockIdx.z, bi = blockIdx.y;
  const int hs = sc.hs[s], ws = sc.ws[s], n = hs*ws;
  const int pix = blockIdx.x*256 + threadIdx.x;
  if (pix >= n) return;
  const float* __restrict__ d = sc.p[s] + (size_t)bi*n;
  float* __restrict__ gd = sc.g[s] + (size_t)bi*n;
  const float mean = stats[((size_t)s*b + bi)*2], E = stats[((size_t)s*b + bi)*2 + 1];
  const float m = fmaxf(mean, kEps32), inv_m = 1.f/m;
  const float gs = g_loss[0]*exp2f(-(float)sc.key[s])/((float)sc.S*(float)b*(float)n);
  const float mean_term = (mean >= kEps32) ? E*inv_m/(float)n : 0.f;
  const float2* __restrict__ ew = ((flags & SMD_USE_EDGES) && edge_w) ? (const float2*)edge_w + edge_offset(sc, b, s) + (size_t)bi*n : nullptr;
  const int v = pix/ws, u = pix - v*ws;
  float xh[5], xv[5], wh[3], wv[3];
#pragma unroll
  for (int t = -2; t <= 2; ++t) {
    xh[t + 2] = d[(size_t)v*ws + min(max(u + t, 0), ws - 1)];
    xv[t + 2] = d[(size_t)min(max(v + t, 0), hs - 1)*ws + u];
  }
#pragma unroll
  for (int t = -2; t <= 0; ++t) {
    wh[t + 2] = ew ? ew[(size_t)v*ws + max(u + t, 0)].x : 1.f;
    wv[t + 2] = ew ? ew[(size_t)max(v + t, 0)*ws + u].y : 1.f;
  }
  const float G = lap1_grad(xh, wh, u, ws) + lap1_grad(xv, wv, v, hs);
  gd[pix] = gs*(G*inv_m - mean_term);
}

// aux maps of the first scale for the second-order form (smooth.py:86, 89 on the laplacian's (xx, yy))
__global__ __launch_bounds__(256) void k_smooth_lap_aux(const ScaleSet sc, int b, const float* __restrict__ img, int h, int w,
                                                        const float* __restrict__ stats, float* __restrict__ disp_grad, float* __restrict__ image_grad) {
  const int bi = blockIdx.y;
  const int hs = sc.hs[0], ws = sc.ws[0], n = hs*ws;
  const float* __restrict__ d = sc.p[0] + (size_t)bi*n;
  const float* __restrict__ im = img + (size_t)bi*3*h*w;
  const float inv_m = 1.f/fmaxf(stats[(size_t)bi*2], kEps32);
  for (int pix = blockIdx.x*256 + threadIdx.x; pix < n; pix += gridDim.x*256) {
    const int v = pix/ws, u = pix - v*ws;
    auto D = [&](int vv, int uu) { return d[(size_t)min(vv, hs - 1)*ws + min(uu, ws - 1)]*inv_m; };
    const float dc = D(v, u);
    const float gx = lap1(dc, D(v, u + 1), D(v, u + 2), u, ws), gy = lap1(dc, D(v + 1, u), D(v + 2, u), v, hs);
    float c0[3], r1[3], r2[3], b1[3], b2[3];
    img_at(im, h, w, hs, ws, v, u, c0);
    img_at(im, h, w, hs, ws, v, min(u + 1, ws - 1), r1); img_at(im, h, w, hs, ws, v, min(u + 2, ws - 1), r2);
    img_at(im, h, w, hs, ws, min(v + 1, hs - 1), u, b1); img_at(im, h, w, hs, ws, min(v + 2, hs - 1), u, b2);
    float ax = 0.f, ay = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ax += lap1(c0[c], r1[c], r2[c], u, ws); ay += lap1(c0[c], b1[c], b2[c], v, hs); }
    ax *= (1.f/3.f); ay *= (1.f/3.f);
    if (disp_grad) disp_grad[(size_t)bi*n + pix] = sqrtf(fmaxf(gx*gx + gy*gy, kEps32));
    if (image_grad) image_grad[(size_t)bi*n + pix] = sqrtf(fmaxf(ax*ax + ay*ay, kEps32));
  }
}

// Optional aux maps of the first scale (`disp_grad`, `image_grad` of smooth.py:86,89) — logging only, not on the timed path.
__global__ __launch_bounds__(256) void k_smooth_aux(const ScaleSet sc, int b, const float* __restrict__ img, int h, int w,
                                                    const float* __restrict__ stats, float* __restrict__ disp_grad, float* __restrict__ image_grad) {
  const int bi = blockIdx.y;
  const int hs = sc.hs[0], ws = sc.ws[0], n = hs*ws;
  const float* __restrict__ d = sc.p[0] + (size_t)bi*n;
  const float* __restrict__ im = img + (size_t)bi*3*h*w;
  const float inv_m = 1.f/fmaxf(stats[(size_t)bi*2], kEps32);
  for (int pix = blockIdx.x*256 + threadIdx.x; pix < n; pix += gridDim.x*256) {
    const int v = pix/ws, u = pix - v*ws;
    const float dc = d[pix]*inv_m;
    float gx = 0.f, gy = 0.f, ax = 0.f, ay = 0.f, ic[3];
    img_at(im, h, w, hs, ws, v, u, ic);
    if (u < ws - 1) {
      gx = fabsf(dc - d[pix + 1]*inv_m);
      float ir[3]; img_at(im, h, w, hs, ws, v, u + 1, ir);
      ax = (fabsf(ic[0] - ir[0]) + fabsf(ic[1] - ir[1]) + fabsf(ic[2] - ir[2]))*(1.f/3.f);
    }
    if (v < hs - 1) {
      gy = fabsf(dc - d[pix + ws]*inv_m);
      float ib[3]; img_at(im, h, w, hs, ws, v + 1, u, ib);
      ay = (fabsf(ic[0] - ib[0]) + fabsf(ic[1] - ib[1]) + fabsf(ic[2] - ib[2]))*(1.f/3.f);
    }
    if (disp_grad) disp_grad[(size_t)bi*n + pix] = sqrtf(fmaxf(gx*gx + gy*gy, kEps32));
    if (image_grad) image_grad[(size_t)bi*n + pix] = sqrtf(fmaxf(ax*ax + ay*ay, kEps32));
  }
}

// ---------------------------------------------------------------------------------------------------
// SmoothReg(use_blur=True) (src/regularizers/smooth.py:21): kornia.filters.gaussian_blur2d(x, kernel_size=(3, 3), sigma=(1, 1)) =
// filter2d_separable(x, k, k, border_type='reflect') with k = exp(-d^2/2)/sum, d in {-1, 0, 1}: a horizontal then a vertical 3-tap pass over
// the reflect-padded plane (kornia 0.6.10; the library is absent from the build image: restated from its published source, parity unpinned).
// One thread per pixel; a cold option (no reference configuration sets it), so no streaming form.
constexpr float kBlurSide = 0.27406862f, kBlurMid = 0.45186276f;   // exp(-1/2) / (1 + 2 exp(-1/2)),  1 / (1 + 2 exp(-1/2))
__device__ __forceinline__ int refl1(int i, int n) { return (i < 0) ? -i : ((i >= n) ? 2*(n - 1) - i : i); }   // F.pad(mode='reflect') by one
__global__ __launch_bounds__(256) void k_blur3_fwd(const float* __restrict__ x, float* __restrict__ out, int planes, int h, int w) {
  const size_t hw = (size_t)h*w;
  for (size_t i = (size_t)blockIdx.x*256 + threadIdx.x; i < (size_t)planes*hw; i += (size_t)gridDim.x*256) {
    const size_t pl = i/hw; const int v = (int)((i - pl*hw)/w), u = (int)(i - pl*hw - (size_t)v*w);
    const float* p = x + pl*hw;
    const int ul = refl1(u - 1, w), ur = refl1(u + 1, w);
    float r[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float* q = p + (size_t)refl1(v + d - 1, h)*w; r[d] = fmaf(kBlurSide, q[ul], fmaf(kBlurSide, q[ur], kBlurMid*q[u])); }
    out[i] = fmaf(kBlurSide, r[0], fmaf(kBlurSide, r[2], kBlurMid*r[1]));
  }
}
// weight with which input position j enters output position i of a reflect-padded 3-tap line of n values
__device__ __forceinline__ float blur_w(int i, int j, int n) {
  return ((i == j) ? kBlurMid : 0.f) + kBlurSide*(float)((refl1(i - 1, n) == j) + (refl1(i + 1, n) == j));
}
// adjoint: g_x[v, u] = sum over the outputs (i, j) within one pixel of (v, u) of W_v(i -> v) W_h(j -> u) g_out[i, j]
__global__ __launch_bounds__(256) void k_blur3_bwd(const float* __restrict__ g_out, float* __restrict__ g_x, int planes, int h, int w) {
  const size_t hw = (size_t)h*w;
  for (size_t i = (size_t)blockIdx.x*256 + threadIdx.x; i < (size_t)planes*hw; i += (size_t)gridDim.x*256) {
    const size_t pl = i/hw; const int v = (int)((i - pl*hw)/w), u = (int)(i - pl*hw - (size_t)v*w);
    const float* p = g_out + pl*hw;
    float acc = 0.f;
    for (int a = max(v - 1, 0); a <= min(v + 1, h - 1); ++a) {
      const float wv = blur_w(a, v, h);
      float row = 0.f;
      for (int c = max(u - 1, 0); c <= min(u + 1, w - 1); ++c) row = fmaf(blur_w(c, u, w), p[(size_t)a*w + c], row);
      acc = fmaf(wv, row, acc);
    }
    g_x[i] = acc;
  }
}
hipError_t launch_blur3(const float* x, float* out, int planes, int h, int w, bool adjoint, hipStream_t st) {
  const size_t n = (size_t)planes*h*w;
  const size_t nb = (n + 255)/256;
  const unsigned blocks = (unsigned)(nb < (size_t)(1u << 16) ? nb : (size_t)(1u << 16));
  if (adjoint) hipLaunchKernelGGL(k_blur3_bwd, dim3(blocks), dim3(256), 0, st, x, out, planes, h, w);
  else hipLaunchKernelGGL(k_blur3_fwd, dim3(blocks), dim3(256), 0, st, x, out, planes, h, w);
  return hipGetLastError();
}

hipError_t launch_smooth_edges(const ScaleSet& sc, int b, const float* img, int h, int w, float* edge_w, hipStream_t st) {
  int max_chunks = 1;
  for (int s = 0; s < sc.S; ++s) max_chunks = max(max_chunks, smooth_units_of(sc.hs[s], sc.ws[s]));
  hipLaunchKernelGGL(k_smooth_edges, dim3(ceil_div(max_chunks, 4), b, sc.S), dim3(256), 0, st, sc, b, img, h, w, edge_w, (unsigned*)((char*)edge_w + edge_arrive_offset(sc, b)));
  return hipGetLastError();
}
size_t smooth_edge_bytes(const ScaleSet& sc, int b) { return edge_arrive_offset(sc, b) + ((((size_t)sc.S*b + 2)*sizeof(unsigned) + 255) & ~(size_t)255); }

// The sweep's partials [S*b][max_units] pairs + [S*b] doubles in `ws_sums` (smd_disp_smooth_workspace_bytes), its counters behind the edge weights.
void smooth_fwd_job(const ScaleSet& sc, int b, float* loss, float* stats, float* ws_sums, float* edge_w, SmoothFwdJob* job) {
  int max_chunks = 1;   // units (waves) of the largest scale; the partial sums of a (scale, sample) are strided by it
  for (int s = 0; s < sc.S; ++s) max_chunks = max(max_chunks, smooth_units_of(sc.hs[s], sc.ws[s]));
  memset(job, 0, sizeof(*job));
  job->edge_w = edge_w; job->partial = ws_sums; job->max_units = max_chunks; job->stats = stats; job->loss = loss;
  job->arrive = edge_w ? (unsigned*)((char*)edge_w + edge_arrive_offset(sc, b)) : nullptr;
  job->contrib = (double*)(ws_sums + (size_t)sc.S*b*max_chunks*2);
}
hipError_t launch_smooth_main(const ScaleSet& sc, int b, const SmoothFwdJob& job, hipStream_t st) {
  hipLaunchKernelGGL(k_smooth_main, dim3(smooth_main_blocks(sc, b)), dim3(256), 0, st, sc, b, job);
  return hipGetLastError();
}

hipError_t launch_smooth_fwd(const ScaleSet& sc, int b, const float* img, int h, int w, int flags, float* loss, float* stats,
                             float* disp_grad, float* image_grad, float* ws_sums, float* edge_w, bool edges_ready, hipStream_t st) {
  int max_chunks = 1;   // units (waves) of the largest scale; the partial sums of a (scale, sample) are strided by it
  for (int s = 0; s < sc.S; ++s) max_chunks = max(max_chunks, smooth_units_of(sc.hs[s], sc.ws[s]));
  if (flags & SMD_USE_LAPLACIAN) {   // second-order form: one thread per pixel, two-launch second stage
    int mu = 1;
    for (int s = 0; s < sc.S; ++s) mu = max(mu, ceil_div(sc.hs[s]*sc.ws[s], 256));
    // (the C ABI sizes the workspace for these units too: smd_disp_smooth_workspace_bytes)
    hipLaunchKernelGGL(k_smooth_lap_main, dim3(mu, b, sc.S), dim3(256), 0, st, sc, b, img, h, w, flags, ws_sums, mu, edge_w);
    hipLaunchKernelGGL(k_smooth_finalize, dim3(1), dim3(1024), 0, st, sc, b, ws_sums, mu, stats, loss, 1);
    if (disp_grad || image_grad)
      hipLaunchKernelGGL(k_smooth_lap_aux, dim3(min(ceil_div(sc.hs[0]*sc.ws[0], 256), 480), b), dim3(256), 0, st, sc, b, img, h, w, stats, disp_grad, image_grad);
    return hipGetLastError();
  }
  // Edge-aware: the weights come from k_smooth_edges (already run by smd_disp_smooth_prep when `edges_ready`), whose buffer also
  // carries the arrival counters of the in-launch second stage; without edge weighting: the two-launch form.
  const bool edges = (flags & SMD_USE_EDGES) && edge_w;
  unsigned* arrive = edges ? (unsigned*)((char*)edge_w + edge_arrive_offset(sc, b)) : nullptr;
  // The alternative, the second stage as a launch of its own (k_smooth_finalize), lost.  Measured at cfg 2 (rocprofv3, profiles/r04_smooth_ab.txt):
  // round 3's sweep (8-row units) 18.0 us with the in-launch chain against 7.1 + 6.7 us in two launches — the chain's five dependent round
  // trips at the end of a launch that is itself one generation of tiny waves cost 11 us; with 16-row units (half the blocks and partials)
  // 13.2 us with the chain against 7.4 + 7.4: the chain stays, now a launch cheaper AND faster.
  if (edges && !edges_ready) hipLaunchKernelGGL(k_smooth_edges, dim3(ceil_div(max_chunks, 4), b, sc.S), dim3(256), 0, st, sc, b, img, h, w, edge_w, (unsigned*)((char*)edge_w + edge_arrive_offset(sc, b)));
  SmoothFwdJob job;
  smooth_fwd_job(sc, b, loss, stats, ws_sums, edges ? edge_w : nullptr, &job);
  job.arrive = arrive;
  hipLaunchKernelGGL(k_smooth_main, dim3(smooth_main_blocks(sc, b)), dim3(256), 0, st, sc, b, job);
  if (!arrive) hipLaunchKernelGGL(k_smooth_finalize, dim3(1), dim3(1024), 0, st, sc, b, ws_sums, job.max_units, stats, loss, 0);
  if (disp_grad || image_grad)
    hipLaunchKernelGGL(k_smooth_aux, dim3(min(ceil_div(sc.hs[0]*sc.ws[0], 256), 480), b), dim3(256), 0, st, sc, b, img, h, w, stats, disp_grad, image_grad);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_smooth_bwd(const ScaleSet sc, int b, const float* __restrict__ img, int h, int w, int flags,
                                                    const float* __restrict__ stats, const float* __restrict__ g_loss,
                                                    const float* __restrict__ edge_w) {
  const int s = blockIdx.z, bi = blockIdx.y;
  const int hs = sc.hs[s], ws = sc.ws[s], n = hs*ws;
  const float* __restrict__ d = sc.p[s] + (size_t)bi*n;
  float* __restrict__ gd = sc.g[s] + (size_t)bi*n;
  const float* __restrict__ im = img + (size_t)bi*3*h*w;
  const float mean = stats[((size_t)s*b + bi)*2], E = stats[((size_t)s*b + bi)*2 + 1];
  const float m = fmaxf(mean, kEps32), inv_m = 1.f/m;
  const bool edges = flags & SMD_USE_EDGES;
  const float gs = g_loss[0]*exp2f(-(float)sc.key[s])/((float)sc.S*(float)b*(float)n);
  const float mean_term = (mean >= kEps32) ? E*inv_m/(float)n : 0.f;
  const int cpx = smooth_chunk_px(n), ppt = cpx/256;
  if ((int)blockIdx.x*cpx >= n) return;
  if (edges && edge_w) {   // weights cached by the forward sweep: 4 weight + 5 disparity loads per pixel, no image access, no exp
    const float2* __restrict__ ew = (const float2*)edge_w + edge_offset(sc, b, s) + (size_t)bi*n;
    auto sg = [](float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); };
    // Branch-free loads: a neighbour outside the image is addressed as the pixel itself and its term masked afterwards, so every
    // load of the thread's pixels is unconditional and they are all in flight together (the loop is latency-shaped).
#pragma unroll 4
    for (int kk = 0; kk < ppt; ++kk) {
      const int pix = min((int)blockIdx.x*cpx + kk*256 + (int)threadIdx.x, n - 1);
      const bool live = (int)blockIdx.x*cpx + kk*256 + (int)threadIdx.x < n;
      const int v = pix/ws, u = pix - v*ws;
      const int pr = v*ws + min(u + 1, ws - 1), pl = v*ws + max(u - 1, 0), pb = min(v + 1, hs - 1)*ws + u, pa = max(v - 1, 0)*ws + u;
      const float dc = d[pix]*inv_m, dr = d[pr]*inv_m, dl = d[pl]*inv_m, db = d[pb]*inv_m, da = d[pa]*inv_m;
      const float2 wc = ew[pix], wl = ew[pl], wa = ew[pa];
      const float G = (u < ws - 1 ? wc.x*sg(dc - dr) : 0.f) - (u > 0 ? wl.x*sg(dl - dc) : 0.f) + (v < hs - 1 ? wc.y*sg(dc - db) : 0.f) - (v > 0 ? wa.y*sg(da - dc) : 0.f);
      if (live) gd[pix] = gs*(G*inv_m - mean_term);
    }
    return;
  }
  for (int kk = 0; kk < ppt; ++kk) {
    const int pix = blockIdx.x*cpx + kk*256 + threadIdx.x;
    if (pix >= n) continue;
    const int v = pix/ws, u = pix - v*ws;
    const float dc = d[pix]*inv_m;
    float ic[3];
    if (edges) img_at(im, h, w, hs, ws, v, u, ic);
    float G = 0.f;
    auto sgn = [](float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); };
    auto wgt = [&](const float a[3], const float bb[3]) {
      return __expf(-(fabsf(a[0] - bb[0]) + fabsf(a[1] - bb[1]) + fabsf(a[2] - bb[2]))*(1.f/3.f));
    };
    if (u < ws - 1) {
      float wgt_ = 1.f;
      if (edges) { float io[3]; img_at(im, h, w, hs, ws, v, u + 1, io); wgt_ = wgt(ic, io); }
      G += wgt_*sgn(dc - d[pix + 1]*inv_m);
    }
    if (u > 0) {
      float wgt_ = 1.f;
      if (edges) { float io[3]; img_at(im, h, w, hs, ws, v, u - 1, io); wgt_ = wgt(io, ic); }
      G -= wgt_*sgn(d[pix - 1]*inv_m - dc);
    }
    if (v < hs - 1) {
      float wgt_ = 1.f;
      if (edges) { float io[3]; img_at(im, h, w, hs, ws, v + 1, u, io); wgt_ = wgt(ic, io); }
      G += wgt_*sgn(dc - d[pix + ws]*inv_m);
    }
    if (v > 0) {
      float wgt_ = 1.f;
      if (edges) { float io[3]; img_at(im, h, w, hs, ws, v - 1, u, io); wgt_ = wgt(io, ic); }
      G -= wgt_*sgn(d[pix - ws]*inv_m - dc);
    }
    gd[pix] = gs*(G*inv_m - mean_term);
  }
}

// Streaming adjoint as a kernel of its own (body: smd_smooth_dev.h): 1-D grid, coarse scales first, ceil(units / 4) blocks per (scale, sample).
__global__ __launch_bounds__(256) void k_smooth_bwd_stream(const ScaleSet sc, int b, const float* __restrict__ stats, const float* __restrict__ g_loss, float g_scale,
                                                           const float* __restrict__ edge_w, int accumulate_scale) {
  int s = sc.S - 1, blk = (int)blockIdx.x;
  for (; s > 0; --s) { const int nb = ceil_div(smooth_units_bwd(sc.hs[s], sc.ws[s]), 4)*b; if (blk < nb) break; blk -= nb; }
  const int bpi = ceil_div(smooth_units_bwd(sc.hs[s], sc.ws[s]), 4);
  smooth_bwd_block(sc, b, s, blk/bpi, blk % bpi, stats, g_loss, g_scale, edge_w, s == accumulate_scale);
}

hipError_t launch_smooth_bwd(const ScaleSet& sc, int b, const float* img, int h, int w, int flags, const float* stats,
                             const float* g_loss, const float* edge_w, hipStream_t st, float g_scale, int accumulate_scale) {
  if (flags & SMD_USE_LAPLACIAN) {
    int mu = 1;
    for (int s = 0; s < sc.S; ++s) mu = max(mu, ceil_div(sc.hs[s]*sc.ws[s], 256));
    hipLaunchKernelGGL(k_smooth_lap_bwd, dim3(mu, b, sc.S), dim3(256), 0, st, sc, b, flags, stats, g_loss, edge_w);
    return hipGetLastError();
  }
  if (!(flags & SMD_USE_EDGES) || edge_w) {   // the streaming adjoint reads the cached weights (or none); the per-pixel form below re-derives them from the image
    int blocks = 0;
    for (int s = 0; s < sc.S; ++s) blocks += ceil_div(smooth_units_bwd(sc.hs[s], sc.ws[s]), 4)*b;
    hipLaunchKernelGGL(k_smooth_bwd_stream, dim3(blocks), dim3(256), 0, st, sc, b, stats, g_loss, g_scale, (flags & SMD_USE_EDGES) ? edge_w : nullptr, accumulate_scale);
    return hipGetLastError();
  }
  int max_chunks = 1;
  for (int s = 0; s < sc.S; ++s) max_chunks = max(max_chunks, smooth_chunks_of(sc.hs[s]*sc.ws[s]));
  hipLaunchKernelGGL(k_smooth_bwd, dim3(max_chunks, b, sc.S), dim3(256), 0, st, sc, b, img, h, w, flags, stats, g_loss, edge_w);
  return hipGetLastError();
}

}  // namespace smd
