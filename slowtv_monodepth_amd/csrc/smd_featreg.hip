// smd_featreg.hip — FeatDepth's two feature regularisers (reference: FeatPeakReg and FeatSmoothReg, src/regularizers/smooth.py:100-176, with compute_grad /
// compute_laplacian, :12-48) for every level of a feature pyramid in one launch, and their adjoint.
//
//   dx[i][j] = |x[i][j] - x[i][j+1]|  (0 in the last column)        dy[i][j] = |x[i][j] - x[i+1][j]|  (0 in the last row)
//   dxx = |dx[i][j] - dx[i][j+1]|, dyx = |dy[i][j] - dy[i][j+1]|  (0 in the last column; the neighbour in the last column is the padded 0)
//   dxy = |dx[i][j] - dx[i+1][j]|, dyy = |dy[i][j] - dy[i+1][j]|  (0 in the last row)
//   peaky  = -(mean(wx dx) + mean(wy dy))                              w* = exp(-channel mean of the same difference of the image), or 1 without edges
//   smooth = mean(wxx dxx) + mean(wyy dyy) + mean(wxy dxy) + mean(wyx dyx)
//
// Both regularisers read the same features and the same image, so one sweep serves both.  A thread owns four columns of one row of a tile of one image and
// keeps the image weights of its four pixels in registers while it walks a chunk of channels: the weights are formed once per tile and channel chunk, not
// per channel.  The differences live in registers; the forward writes two fp64 sums per block and nothing else, a one-block second stage adds them in a fixed
// order: no atomics, no full-size intermediates, two runs are bit-equal and the result does not depend on how the grid is scheduled.
//
// The adjoint is a gather: the thread that owns x[i][j..j+3] recomputes the differences of the 5 x 8 window around them, forms the gradients with respect to
// the first-order differences it needs (dx at columns j-1..j+3 of its row, dy at rows i-1, i) with sign(0) = 0 and the padded zeros constant, and stores
// g_x once.  Nothing is scattered.
//
// Streaming shape: where a level's rows are 16-byte aligned (w % 4 == 0 and an aligned base) a group of four columns moves as one 16-byte vector and its
// two-column halos as 8-byte vectors; other levels, and groups that touch the border, go element by element under explicit bounds.  No LDS beyond the
// block reduction.
#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

namespace {

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// out[0 .. LEFT+6) = row[j-LEFT .. j+6), zeros outside [0, w); `vec`: the row is 16-byte aligned and j % 4 == 0
template <int LEFT> __device__ __forceinline__ void load_row(const float* __restrict__ row, bool row_ok, int j, int w, bool vec, float* out) {
#pragma unroll
  for (int k = 0; k < LEFT + 6; ++k) out[k] = 0.f;
  if (!row_ok) return;
  if (vec && j + 4 <= w) {
    const f4 v = *(const f4*)(row + j);
    out[LEFT] = v.x; out[LEFT + 1] = v.y; out[LEFT + 2] = v.z; out[LEFT + 3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (j + k < w) out[LEFT + k] = row[j + k];
  }
  if (vec && j + 6 <= w) {
    const f2 v = *(const f2*)(row + j + 4);
    out[LEFT + 4] = v.x; out[LEFT + 5] = v.y;
  } else {
#pragma unroll
    for (int k = 4; k < 6; ++k) if (j + k < w) out[LEFT + k] = row[j + k];
  }
  if (LEFT == 2) {
    if (vec && j >= 4) {
      const f2 v = *(const f2*)(row + j - 2);
      out[0] = v.x; out[1] = v.y;
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k) if (j - 2 + k >= 0 && j - 2 + k < w) out[k] = row[j - 2 + k];
    }
  }
}

// the unit's level and its coordinates: (image b, channel chunk, row i, first column j) of this thread
struct Where { int s, b, c0, c1, i, j; };
__device__ __forceinline__ Where locate(const FeatRegSet& fs) {
  int s = 0;
  const int u = blockIdx.x;
  while (s + 1 < fs.S && u >= fs.L[s + 1].unit0) ++s;
  const FeatLevel& L = fs.L[s];
  int t = u - L.unit0;
  const int chunk = t % L.nchunk; t /= L.nchunk;
  const int tx = t % L.tiles_x; t /= L.tiles_x;
  const int ty = t % L.tiles_y;
  Where q;
  q.s = s; q.b = t/L.tiles_y;
  q.c0 = chunk*kFeatChunk; q.c1 = q.c0 + kFeatChunk < L.C ? q.c0 + kFeatChunk : L.C;
  const int tg = 1 << L.tg_log2;
  q.i = ty*(256 >> L.tg_log2) + ((int)threadIdx.x >> L.tg_log2);
  q.j = (tx*tg + ((int)threadIdx.x & (tg - 1)))*4;
  return q;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- forward
// X rows i..i+2, columns j..j+5.  d?[k] are the differences at column j+k of row i; e?[k] of row i+1.
struct Fwd4 { float dx[5], dy[5], ex[4], ey[4]; };
__device__ __forceinline__ void first_order_fwd(const float X[3][6], int i, int j, int h, int w, Fwd4& f) {
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    f.dx[k] = (j + k < w - 1) ? fabsf(X[0][k] - X[0][k + 1]) : 0.f;
    f.dy[k] = (i < h - 1 && j + k < w) ? fabsf(X[0][k] - X[1][k]) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f.ex[k] = (i + 1 < h && j + k < w - 1) ? fabsf(X[1][k] - X[1][k + 1]) : 0.f;
    f.ey[k] = (i + 1 < h - 1 && j + k < w) ? fabsf(X[1][k] - X[2][k]) : 0.f;
  }
}
// the four second-order differences of column j+k of row i
__device__ __forceinline__ void second_order_fwd(const Fwd4& f, int k, bool col1, bool row1, float& xx, float& xy, float& yx, float& yy) {
  xx = col1 ? fabsf(f.dx[k] - f.dx[k + 1]) : 0.f;
  yx = col1 ? fabsf(f.dy[k] - f.dy[k + 1]) : 0.f;
  xy = row1 ? fabsf(f.dx[k] - f.ex[k]) : 0.f;
  yy = row1 ? fabsf(f.dy[k] - f.ey[k]) : 0.f;
}

__global__ __launch_bounds__(256) void k_feat_regs_fwd(const FeatRegSet fs, int flags, double* __restrict__ part) {
  __shared__ double red[8];
  const Where q = locate(fs);
  const FeatLevel& L = fs.L[q.s];
  const int h = L.h, w = L.w, i = q.i, j = q.j;
  const bool active = i < h && j < w;
  const bool want_p = flags & SMD_FEATREG_PEAKY, want_s = flags & SMD_FEATREG_SMOOTH;
  double acc[2] = {0.0, 0.0};
  if (active) {
    const size_t plane = (size_t)h*w;
    const bool row1 = i < h - 1;
    float wx[4], wy[4], wxx[4], wxy[4], wyx[4], wyy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wx[k] = wy[k] = wxx[k] = wxy[k] = wyx[k] = wyy[k] = 1.f;
    const bool pe = want_p && (flags & SMD_FEATREG_PEAKY_EDGES), se = want_s && (flags & SMD_FEATREG_SMOOTH_EDGES);
    if (pe || se) {
      float a[6][4] = {};
      for (int c = 0; c < 3; ++c) {
        const float* p = L.img + ((size_t)q.b*3 + c)*plane + (size_t)i*w;
        float X[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) load_row<0>(p + (size_t)r*w, i + r < h, j, w, L.vec_img, X[r]);
        Fwd4 f;
        first_order_fwd(X, i, j, h, w, f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float xx, xy, yx, yy;
          second_order_fwd(f, k, j + k < w - 1, row1, xx, xy, yx, yy);
          a[0][k] += f.dx[k]; a[1][k] += f.dy[k]; a[2][k] += xx; a[3][k] += xy; a[4][k] += yx; a[5][k] += yy;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (pe) { wx[k] = expf(-(a[0][k]/3.f)); wy[k] = expf(-(a[1][k]/3.f)); }
        if (se) { wxx[k] = expf(-(a[2][k]/3.f)); wxy[k] = expf(-(a[3][k]/3.f)); wyx[k] = expf(-(a[4][k]/3.f)); wyy[k] = expf(-(a[5][k]/3.f)); }
      }
    }
    for (int c = q.c0; c < q.c1; ++c) {
      const float* p = L.x + ((size_t)q.b*L.C + c)*plane + (size_t)i*w;
      float X[3][6];
#pragma unroll
      for (int r = 0; r < 3; ++r) load_row<0>(p + (size_t)r*w, i + r < h, j, w, L.vec_x, X[r]);
      Fwd4 f;
      first_order_fwd(X, i, j, h, w, f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (want_p) acc[0] += (double)(wx[k]*f.dx[k]) + (double)(wy[k]*f.dy[k]);
        if (want_s) {
          float xx, xy, yx, yy;
          second_order_fwd(f, k, j + k < w - 1, row1, xx, xy, yx, yy);
          acc[1] += ((double)(wxx[k]*xx) + (double)(wyy[k]*yy)) + ((double)(wxy[k]*xy) + (double)(wyx[k]*yx));
        }
      }
    }
  }
  stage_wave_sums(acc, red);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x*2] = sum_waves<Waves::Sequential, 4>(red, 2, 0);
    part[(size_t)blockIdx.x*2 + 1] = sum_waves<Waves::Sequential, 4>(red, 2, 1);
  }
}

// second stage, one block: per level the blocks' sums in a fixed order, times the level's coefficient 1/(N_s 2^s S); out_p = -(peaky), out_s = smooth
__global__ __launch_bounds__(256) void k_feat_regs_fin(const FeatRegSet fs, const double* __restrict__ part, float* __restrict__ out_p, float* __restrict__ out_s) {
  __shared__ double red[8];
  double total[2] = {0.0, 0.0};
  for (int s = 0; s < fs.S; ++s) {
    const int first = fs.L[s].unit0, last = s + 1 < fs.S ? fs.L[s + 1].unit0 : fs.units;
    double acc[2] = {0.0, 0.0};
    for (int u = first + (int)threadIdx.x; u < last; u += 256) { acc[0] += part[(size_t)u*2]; acc[1] += part[(size_t)u*2 + 1]; }
    stage_wave_sums(acc, red);
    total[0] += sum_waves<Waves::Sequential, 4>(red, 2, 0)*fs.L[s].coef;
    total[1] += sum_waves<Waves::Sequential, 4>(red, 2, 1)*fs.L[s].coef;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (out_p) *out_p = (float)(-total[0]);
    if (out_s) *out_s = (float)total[1];
  }
}

// ------------------------------------------------------------------------------------------------- backward
// The window: rows i-2..i+2 (r = 0..4), columns j-2..j+5 (k = 0..7).  DX[r][k] (r = 1..3 -> rows i-1..i+1, stored at r-1; k = 0..6) and DY[r][k] (r = 0..3
// -> rows i-2..i+1; k = 1..6, stored at k-1) are the padded first-order differences: 0 outside the map and in the last column / row.
struct Win {
  float DX[3][7], DY[4][6];
};
__device__ __forceinline__ void first_order_bwd(const float X[5][8], int i, int j, int h, int w, Win& d) {
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const int row = i - 2 + r;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int col = j - 2 + k;
      d.DX[r - 1][k] = (row >= 0 && row < h && col >= 0 && col < w - 1) ? fabsf(X[r][k] - X[r][k + 1]) : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i - 2 + r;
#pragma unroll
    for (int k = 1; k < 7; ++k) {
      const int col = j - 2 + k;
      d.DY[r][k - 1] = (row >= 0 && row < h - 1 && col >= 0 && col < w) ? fabsf(X[r][k] - X[r + 1][k]) : 0.f;
    }
  }
}
// accessors in window coordinates (r: 0..4 = rows i-2..i+2, k: 0..7 = columns j-2..j+5)
#define DXW(d, r, k) ((d).DX[(r) - 1][(k)])
#define DYW(d, r, k) ((d).DY[(r)][(k) - 1])

// The image weights the adjoint of a thread reads, in window coordinates:
//   x[k], k = 1..5 (row i)   xx[k], k = 0..5 (row i)   xy[r][k], r = 1, 2 (rows i-1, i), k = 1..5
//   y[r][k], r = 1, 2, k = 2..5   yx[r][k], r = 1, 2, k = 1..5   yy[r][k], r = 0..2, k = 2..5
struct Wts { float x[5], xx[6], xy[2][5], y[2][4], yx[2][5], yy[3][4]; };

template <class F> __device__ __forceinline__ void for_weights(Wts& a, F f) {
#pragma unroll
  for (int k = 0; k < 5; ++k) f(a.x[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) f(a.xx[k]);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int k = 0; k < 5; ++k) { f(a.xy[r][k]); f(a.yx[r][k]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) f(a.y[r][k]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f(a.yy[r][k]);
  }
}

// the second-order differences of one plane at the positions of `Wts`, added to `a` (masked exactly as the forward masks them)
template <bool P, bool S2> __device__ __forceinline__ void add_second_order(const Win& d, int i, int j, int h, int w, Wts& a) {
  if (P) {
#pragma unroll
    for (int k = 1; k < 6; ++k) a.x[k - 1] += DXW(d, 2, k);
#pragma unroll
    for (int r = 1; r < 3; ++r) {
#pragma unroll
      for (int k = 2; k < 6; ++k) a.y[r - 1][k - 2] += DYW(d, r, k);
    }
  }
  if (S2) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.xx[k] += (j - 2 + k < w - 1) ? fabsf(DXW(d, 2, k) - DXW(d, 2, k + 1)) : 0.f;
#pragma unroll
    for (int r = 1; r < 3; ++r) {
      const bool row1 = i - 2 + r < h - 1;
#pragma unroll
      for (int k = 1; k < 6; ++k) {
        a.xy[r - 1][k - 1] += row1 ? fabsf(DXW(d, r, k) - DXW(d, r + 1, k)) : 0.f;
        a.yx[r - 1][k - 1] += (j - 2 + k < w - 1) ? fabsf(DYW(d, r, k) - DYW(d, r, k + 1)) : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const bool row1 = i - 2 + r < h - 1;
#pragma unroll
      for (int k = 2; k < 6; ++k) a.yy[r][k - 2] += row1 ? fabsf(DYW(d, r, k) - DYW(d, r + 1, k)) : 0.f;
    }
  }
}

template <bool P, bool S2>
__global__ __launch_bounds__(256) void k_feat_regs_bwd(const FeatRegSet fs, int flags, const float* __restrict__ g_peaky, const float* __restrict__ g_smooth) {
  const Where q = locate(fs);
  const FeatLevel& L = fs.L[q.s];
  const int h = L.h, w = L.w, i = q.i, j = q.j;
  if (!(i < h && j < w)) return;
  // d loss / d (a level's sums): the incoming gradients times the level's coefficient; peaky is negated
  const double gp = P ? -(double)*g_peaky*L.coef : 0.0, gs = S2 ? (double)*g_smooth*L.coef : 0.0;
  const size_t plane = (size_t)h*w;
  Wts wt;
  for_weights(wt, [](float& v) { v = 1.f; });
  const bool pe = P && (flags & SMD_FEATREG_PEAKY_EDGES), se = S2 && (flags & SMD_FEATREG_SMOOTH_EDGES);
  if (pe || se) {
    Wts a;
    for_weights(a, [](float& v) { v = 0.f; });
    for (int c = 0; c < 3; ++c) {
      const float* p = L.img + ((size_t)q.b*3 + c)*plane;
      float X[5][8];
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const int row = i - 2 + r;
        load_row<2>(p + (size_t)(row < 0 ? 0 : row)*w, row >= 0 && row < h, j, w, L.vec_img, X[r]);
      }
      Win d;
      first_order_bwd(X, i, j, h, w, d);
      add_second_order<P, S2>(d, i, j, h, w, a);
    }
    for_weights(a, [](float& v) { v = expf(-(v/3.f)); });
    if (pe) {
#pragma unroll
      for (int k = 0; k < 5; ++k) wt.x[k] = a.x[k];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wt.y[r][k] = a.y[r][k];
      }
    }
    if (se) {
#pragma unroll
      for (int k = 0; k < 6; ++k) wt.xx[k] = a.xx[k];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int k = 0; k < 5; ++k) { wt.xy[r][k] = a.xy[r][k]; wt.yx[r][k] = a.yx[r][k]; }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wt.yy[r][k] = a.yy[r][k];
      }
    }
  }
  for (int c = q.c0; c < q.c1; ++c) {
    const size_t base = ((size_t)q.b*L.C + c)*plane;
    const float* p = L.x + base;
    float X[5][8];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int row = i - 2 + r;
      load_row<2>(p + (size_t)(row < 0 ? 0 : row)*w, row >= 0 && row < h, j, w, L.vec_x, X[r]);
    }
    Win d;
    first_order_bwd(X, i, j, h, w, d);
    // d loss / d dx at row i, columns j-1..j+3 (k = 1..5); the padded zero of the last column is a constant
    double Gx[5];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
      const int col = j - 2 + k;
      double g = 0.0;
      if (col >= 0 && col < w - 1) {
        if (P) g = gp*wt.x[k - 1];
        if (S2) {
          double t = (double)(wt.xx[k]*sgn(DXW(d, 2, k) - DXW(d, 2, k + 1)));
          if (col >= 1) t -= (double)(wt.xx[k - 1]*sgn(DXW(d, 2, k - 1) - DXW(d, 2, k)));
          if (i < h - 1) t += (double)(wt.xy[1][k - 1]*sgn(DXW(d, 2, k) - DXW(d, 3, k)));
          if (i >= 1) t -= (double)(wt.xy[0][k - 1]*sgn(DXW(d, 1, k) - DXW(d, 2, k)));
          g += gs*t;
        }
      }
      Gx[k - 1] = g;
    }
    // d loss / d dy at rows i-1, i (r = 1, 2), columns j..j+3 (k = 2..5)
    double Gy[2][4];
#pragma unroll
    for (int r = 1; r < 3; ++r) {
      const int row = i - 2 + r;
#pragma unroll
      for (int k = 2; k < 6; ++k) {
        const int col = j - 2 + k;
        double g = 0.0;
        if (row >= 0 && row < h - 1 && col < w) {
          if (P) g = gp*wt.y[r - 1][k - 2];
          if (S2) {
            double t = 0.0;
            if (col < w - 1) t += (double)(wt.yx[r - 1][k - 1]*sgn(DYW(d, r, k) - DYW(d, r, k + 1)));
            if (col >= 1) t -= (double)(wt.yx[r - 1][k - 2]*sgn(DYW(d, r, k - 1) - DYW(d, r, k)));
            t += (double)(wt.yy[r][k - 2]*sgn(DYW(d, r, k) - DYW(d, r + 1, k)));        // row < h-1 holds here
            if (row >= 1) t -= (double)(wt.yy[r - 1][k - 2]*sgn(DYW(d, r - 1, k) - DYW(d, r, k)));
            g += gs*t;
          }
        }
        Gy[r - 1][k - 2] = g;
      }
    }
    float o[4];
#pragma unroll
    for (int k = 2; k < 6; ++k) {
      // Gx / Gy are 0 where the difference does not exist, so no further bounds are needed
      const double g = (Gx[k - 1]*sgn(X[2][k] - X[2][k + 1]) - Gx[k - 2]*sgn(X[2][k - 1] - X[2][k]))
                     + (Gy[1][k - 2]*sgn(X[2][k] - X[3][k]) - Gy[0][k - 2]*sgn(X[1][k] - X[2][k]));
      o[k - 2] = (float)g;
    }
    float* po = L.gx + base + (size_t)i*w + j;
    if (L.vec_gx && j + 4 <= w) {
      *(f4*)po = f4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (j + k < w) po[k] = o[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------- host
// tiles, chunks and the first unit of every level; -> the number of units (0: a level of 2^31 elements or more, or 2^31 units)
long feat_regs_plan(FeatRegSet& fs, const int* Cs, const int* hs, const int* ws, int S, int B) {
  long units = 0;
  fs.S = S;
  for (int s = 0; s < S; ++s) {
    FeatLevel& L = fs.L[s];
    const long n = (long)B*Cs[s]*hs[s]*ws[s];
    if (n >= (1L << 31)) return 0;
    const int ng = (ws[s] + 3)/4;
    int tgl = 0;
    while (tgl < 5 && (1 << tgl) < ng) ++tgl;
    const int tg = 1 << tgl, tr = 256 >> tgl;
    L.C = Cs[s]; L.h = hs[s]; L.w = ws[s]; L.tg_log2 = tgl;
    L.tiles_x = (ng + tg - 1)/tg; L.tiles_y = (hs[s] + tr - 1)/tr;
    L.nchunk = (Cs[s] + kFeatChunk - 1)/kFeatChunk;
    L.unit0 = (int)units;
    L.coef = 1.0/((double)n*(double)(1L << s)*(double)S);
    units += (long)B*L.tiles_y*L.tiles_x*L.nchunk;
    if (units >= (1L << 31)) return 0;
  }
  fs.units = (int)units;
  return units;
}

hipError_t launch_feat_regs_fwd(const FeatRegSet& fs, int flags, double* part, float* out_p, float* out_s, hipStream_t st) {
  hipLaunchKernelGGL(k_feat_regs_fwd, dim3((unsigned)fs.units), dim3(256), 0, st, fs, flags, part);
  hipLaunchKernelGGL(k_feat_regs_fin, dim3(1), dim3(256), 0, st, fs, (const double*)part, out_p, out_s);
  return hipGetLastError();
}

hipError_t launch_feat_regs_bwd(const FeatRegSet& fs, int flags, const float* g_peaky, const float* g_smooth, hipStream_t st) {
  for_bool(g_peaky != nullptr, [&](auto p) {
    for_bool(g_smooth != nullptr, [&](auto s2) {
      hipLaunchKernelGGL((k_feat_regs_bwd<decltype(p)::value, decltype(s2)::value>), dim3((unsigned)fs.units), dim3(256), 0, st, fs, flags, g_peaky, g_smooth);
    });
  });
  return hipGetLastError();
}

}  // namespace smd
