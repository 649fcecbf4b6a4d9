// smd_subpixel.hip — the SuperDepth decoder's sub-pixel convolution (reference: src/networks/decoders/superdepth.py:13-26) with what stands around it.
//
// The reference runs  ELU -> Conv2d(C, C r^2, 3, groups=C, padding=1) -> PixelShuffle(r) -> ReLU | sigmoid -> [cat(skip) -> reflection pad]  as separate ATen
// kernels, each a full pass over a tensor r^2 times the input's size.  Here one gather reads the raw (bias-free) convolution output x and writes the next
// convolution's padded input:
//   u = pre_act(x + pre_bias[c]);  v[b,c,r y+dy,r x+dx] = bias[o] + sum_ij weight[o,0,i,j] u[b,c,y+i-1,x+j-1]  (o = c r^2 + dy r + dx, zero padding);
//   z = act(v);  out = z | reflect_pad1(cat(z, skip))
//   k_sp_fwd       a lane owns one OUTPUT column (adjacent lanes: adjacent columns, whatever r), so its dx and its three input columns are fixed: the 9 r
//                  weights it needs stay in registers, a wave walks down the input rows with a rolling 3 x 3 window (x comes through the cache: the halo
//                  re-reads never reach HBM) and writes r output rows per input row; the mirrored border rows of the padding are second stores of the same
//                  value, the mirrored border columns are lanes of their own.
//   k_sp_skip_fwd  the skip channels of the padded concatenation.
// Backward (the pad adjoint folded in on the fly, dL/dv = G act'(z) with z read from `out`, u recomputed):
//   k_sp_bwd_x     a thread owns one input pixel and gathers its 9 r^2 contributions (the channel's weights in LDS), rows, columns, dy, dx in order;
//                  in fp64 to the store; its per-block sums (fp64) are the pre-bias gradient's.
//   k_sp_bwd_w     the forward's lane map on the un-padded plane: 10 r accumulators a lane (9 taps and the bias for each dy), the lanes of one dx by a
//                  butterfly, the four waves in order, one set of 10 r^2 sums per block to the workspace; k_sp_w_finalize adds the sets in fp64, samples
//                  and blocks in order.
//   k_sp_skip_bwd  the pad adjoint of the skip channels.
// Every sum has a fixed order: no atomics, two runs are bit-equal.
#include "smd_glue_dev.h"

namespace smd {

enum { kSpNone = 0, kSpRelu = 1, kSpSigmoid = 2 };
constexpr int kSpBlock = 256;
constexpr int kSpWaves = kSpBlock/64;
constexpr int kSpRowsFwd = 8;     // input rows a wave of the forward walks at most
constexpr int kSpRowsWgt = 16;    // ... of the weight gradient: one butterfly per block, so longer walks

static inline int sp_rows_per_wave(int h, int most) {
  const int r = ceil_div(h, kSpWaves);
  return r < 1 ? 1 : (r > most ? most : r);
}
struct SpGrid { int rpw; unsigned strips, bands; };
static inline SpGrid sp_grid(int h, int width, int most) {
  SpGrid g;
  g.rpw = sp_rows_per_wave(h, most);
  g.strips = (unsigned)ceil_div(width, 64);
  g.bands = (unsigned)ceil_div(h, g.rpw*kSpWaves);
  return g;
}
static inline int sp_pre(const SubPixel& s) { return s.pre_act ? kActElu : kActNone; }

bool subpixel_sizes_ok(const SubPixel& s) {
  if (s.B < 1 || s.C < 1 || s.Cs < 0 || s.h < 1 || s.w < 1 || (s.r != 2 && s.r != 4 && s.r != 8)) return false;
  if (s.pre_act < 0 || s.pre_act > 1 || s.act < 0 || s.act > 2 || (s.pad != 0 && s.pad != 1) || (s.Cs > 0 && !s.pad)) return false;
  const long long H = (long long)s.r*s.h + 2, W = (long long)s.r*s.w + 2, HW = H*W;
  if (HW >= (1ll << 30)) return false;
  const long long planes = (long long)s.B*((long long)s.C + s.Cs);
  if (planes*((HW + kDecChunk - 1)/kDecChunk) >= (1ll << 31)) return false;
  const long long tiles = ((W + 63)/64)*(long long)s.h;      // at least as many as any launch's strips x bands
  return planes*tiles < (1ll << 31) && (long long)s.C*s.r*s.r*10 < (1ll << 31);
}
static size_t sp_pb_partials(const SubPixel& s) { return ((2*(size_t)s.B*s.C*ceil_div(s.h*s.w, kDecChunk)) + 3) & ~(size_t)3; }   // floats; the sums are doubles
size_t subpixel_workspace_floats(const SubPixel& s) {
  const SpGrid g = sp_grid(s.h, s.r*s.w, kSpRowsWgt);
  return sp_pb_partials(s) + (size_t)s.B*s.C*g.strips*g.bands*10*s.r*s.r;
}

// u at (yy, xx) of an h x w plane: pre_act(x + pb) inside, the convolution's zero padding outside
__device__ __forceinline__ float sp_u(const float* __restrict__ xp, int yy, int xx, int h, int w, float pb, int pre) {
  return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? glue_act(xp[yy*w + xx] + pb, pre) : 0.f;
}
__device__ __forceinline__ float sp_act(float v, int act) {
  return act == kSpRelu ? fmaxf(v, 0.f) : (act == kSpSigmoid ? 1.f/(1.f + expf(-v)) : v);
}
// dL/dv at the un-padded position (rr, q) of an RH x RW plane: g / z are this channel's plane of g_out / out (padded: the pad adjoint of g, z at the centre cell)
__device__ __forceinline__ float sp_gv(const float* __restrict__ g, const float* __restrict__ z, int rr, int q, int RH, int RW, int pad, int act) {
  const int W = RW + 2;
  const float G = pad ? pad_adj_at(g, rr, q, RH, RW, W) : g[rr*RW + q];
  if (act == kSpNone) return G;
  const float zz = pad ? z[(rr + 1)*W + q + 1] : z[rr*RW + q];
  return act == kSpRelu ? (zz > 0.f ? G : 0.f) : G*zz*(1.f - zz);
}

template <int R>
__global__ __launch_bounds__(kSpBlock) void k_sp_fwd(const float* __restrict__ x, const float* __restrict__ pre_bias, const float* __restrict__ weight,
                                                     const float* __restrict__ bias, float* __restrict__ out, SubPixel s, SpGrid gr) {
  const unsigned strip = blockIdx.x % gr.strips, t = blockIdx.x/gr.strips, band = t % gr.bands, plane = t/gr.bands;   // plane = b*C + c
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int h = s.h, w = s.w, RH = R*h, RW = R*w, p = s.pad, W = RW + 2*p, H = RH + 2*p;
  const int px = (int)strip*64 + lane;
  if (px >= W) return;
  const unsigned b = plane/s.C, c = plane - b*s.C;
  const int q = p ? unpad_reflect(px, RW) : px;
  const int ix = q/R, dx = q - ix*R;
  float wr[R][9], br[R];
#pragma unroll
  for (int dy = 0; dy < R; ++dy) {
    const size_t o = (size_t)c*R*R + dy*R + dx;
    br[dy] = bias[o];
#pragma unroll
    for (int k = 0; k < 9; ++k) wr[dy][k] = weight[o*9 + k];
  }
  const float pb = pre_bias ? pre_bias[c] : 0.f;
  const int pre = s.pre_act ? kActElu : kActNone, act = s.act;
  const float* xp = x + (size_t)plane*h*w;
  float* op = out + ((size_t)b*(s.C + s.Cs) + c)*H*W + px;
  const int y0 = ((int)band*kSpWaves + wv)*gr.rpw, y1 = y0 + gr.rpw < h ? y0 + gr.rpw : h;
  float u[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { u[0][j] = sp_u(xp, y0 - 1, ix + j - 1, h, w, pb, pre); u[1][j] = sp_u(xp, y0, ix + j - 1, h, w, pb, pre); }
  for (int y = y0; y < y1; ++y) {
#pragma unroll
    for (int j = 0; j < 3; ++j) u[2][j] = sp_u(xp, y + 1, ix + j - 1, h, w, pb, pre);
#pragma unroll
    for (int dy = 0; dy < R; ++dy) {
      float v = br[dy];
#pragma unroll
      for (int k = 0; k < 9; ++k) v = fmaf(wr[dy][k], u[k/3][k % 3], v);
      const float z = sp_act(v, act);
      const int rr = R*y + dy;
      op[(size_t)(rr + p)*W] = z;
      if (p && rr == 1) op[0] = z;
      if (p && rr == RH - 2) op[(size_t)(RH + 1)*W] = z;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) { u[0][j] = u[1][j]; u[1][j] = u[2][j]; }
  }
}

// out[:, C + cs] = reflect_pad1(skip[:, cs])
__global__ __launch_bounds__(kDecBlock) void k_sp_skip_fwd(const float* __restrict__ skip, float* __restrict__ out, int C, int Cs, int RH, int RW, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Cs + cs
  const unsigned b = plane/Cs, cs = plane - b*Cs;
  const int H = RH + 2, W = RW + 2;
  const float* src = skip + (size_t)plane*RH*RW;
  float* dst = out + ((size_t)b*(C + Cs) + C + cs)*H*W;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H*W) break;
    const int py = idx/W, px = idx - py*W;
    dst[idx] = src[unpad_reflect(py, RH)*RW + unpad_reflect(px, RW)];
  }
}
__global__ __launch_bounds__(kDecBlock) void k_sp_skip_bwd(const float* __restrict__ g_out, float* __restrict__ g_skip, int C, int Cs, int RH, int RW, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Cs + cs
  const unsigned b = plane/Cs, cs = plane - b*Cs;
  const int W = RW + 2;
  const float* g = g_out + ((size_t)b*(C + Cs) + C + cs)*(RH + 2)*W;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= RH*RW) break;
    const int r = idx/RW, q = idx - r*RW;
    g_skip[(size_t)plane*RH*RW + idx] = pad_adj_at(g, r, q, RH, RW, W);
  }
}

// g_x = pre_act'(x + pb) sum_{i,j,dy,dx} weight[c r^2 + dy r + dx][i][j] dL/dv[r (y - i + 1) + dy][r (x - j + 1) + dx]; g_x may be NULL (its sums alone)
template <int R>
__global__ __launch_bounds__(kDecBlock) void k_sp_bwd_x(const float* __restrict__ x, const float* __restrict__ pre_bias, const float* __restrict__ weight,
                                                        const float* __restrict__ out, const float* __restrict__ g_out, float* __restrict__ g_x,
                                                        double* __restrict__ pb_partial, SubPixel s, unsigned chunks) {
  __shared__ float wl[9*R*R];
  __shared__ double red[kDecBlock/64];
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*C + c
  const unsigned b = plane/s.C, c = plane - b*s.C;
  const int h = s.h, w = s.w, RH = R*h, RW = R*w, p = s.pad, act = s.act, pre = s.pre_act ? kActElu : kActNone;
  for (int i = threadIdx.x; i < 9*R*R; i += kDecBlock) wl[i] = weight[(size_t)c*9*R*R + i];
  __syncthreads();
  const size_t po = ((size_t)b*(s.C + s.Cs) + c)*(size_t)(RH + 2*p)*(RW + 2*p);
  const float* g = g_out + po;
  const float* z = out ? out + po : nullptr;
  const float pb = pre_bias ? pre_bias[c] : 0.f;
  double bsum = 0.0;
#pragma unroll 1
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= h*w) break;
    const int yq = idx/w, xq = idx - yq*w;
    double acc = 0.0;      // 9 r^2 terms of either sign, and the pre-bias gradient is the (cancelling) sum of the results: fp64 to the store
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int yy = yq - i + 1;
      if (yy < 0 || yy >= h) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int xx = xq - j + 1;
        if (xx < 0 || xx >= w) continue;
#pragma unroll 2
        for (int dy = 0; dy < R; ++dy)
#pragma unroll
          for (int dx = 0; dx < R; ++dx) acc = fma((double)wl[(dy*R + dx)*9 + i*3 + j], (double)sp_gv(g, z, R*yy + dy, R*xx + dx, RH, RW, p, act), acc);
      }
    }
    if (pre) { const float xv = x[(size_t)plane*h*w + idx] + pb; if (!(xv > 0.f)) acc *= (double)expf(xv); }      // elu'(x) = x > 0 ? 1 : exp(x)
    if (g_x) g_x[(size_t)plane*h*w + idx] = (float)acc;
    bsum += acc;
  }
  if (pb_partial) block_store_sum<Waves::Sequential, kDecBlock/64>(bsum, red, pb_partial + blockIdx.x);
}

// partial[block][(dy r + dx) 10 + t] = the block's sum of dL/dv u[tap t] (t < 9) and of dL/dv (t = 9) over its rows and its 64 output columns
template <int R>
__global__ __launch_bounds__(kSpBlock) void k_sp_bwd_w(const float* __restrict__ x, const float* __restrict__ pre_bias, const float* __restrict__ out,
                                                       const float* __restrict__ g_out, float* __restrict__ partial, SubPixel s, SpGrid gr) {
  __shared__ float red[kSpWaves][10*R*R];
  const unsigned strip = blockIdx.x % gr.strips, t = blockIdx.x/gr.strips, band = t % gr.bands, plane = t/gr.bands;   // plane = b*C + c
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int h = s.h, w = s.w, RH = R*h, RW = R*w, p = s.pad, act = s.act, pre = s.pre_act ? kActElu : kActNone;
  const unsigned b = plane/s.C, c = plane - b*s.C;
  const int q = (int)strip*64 + lane;
  const bool valid = q < RW;
  const int ix = q/R, dx = lane % R;              // (64 is a multiple of R: dx = q % R)
  const size_t po = ((size_t)b*(s.C + s.Cs) + c)*(size_t)(RH + 2*p)*(RW + 2*p);
  const float* g = g_out + po;
  const float* z = out ? out + po : nullptr;
  const float* xp = x + (size_t)plane*h*w;
  const float pb = pre_bias ? pre_bias[c] : 0.f;
  float acc[R][10];
#pragma unroll
  for (int dy = 0; dy < R; ++dy)
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[dy][k] = 0.f;
  const int y0 = ((int)band*kSpWaves + wv)*gr.rpw, y1 = y0 + gr.rpw < h ? y0 + gr.rpw : h;
  if (valid) {
    float u[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { u[0][j] = sp_u(xp, y0 - 1, ix + j - 1, h, w, pb, pre); u[1][j] = sp_u(xp, y0, ix + j - 1, h, w, pb, pre); }
    for (int y = y0; y < y1; ++y) {
#pragma unroll
      for (int j = 0; j < 3; ++j) u[2][j] = sp_u(xp, y + 1, ix + j - 1, h, w, pb, pre);
#pragma unroll
      for (int dy = 0; dy < R; ++dy) {
        const float gv = sp_gv(g, z, R*y + dy, q, RH, RW, p, act);
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[dy][k] = fmaf(gv, u[k/3][k % 3], acc[dy][k]);
        acc[dy][9] += gv;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) { u[0][j] = u[1][j]; u[1][j] = u[2][j]; }
    }
  }
  // the lanes of one dx: butterfly over the lane bits above log2(R); lanes 0..R-1 then hold their dx's sums
#pragma unroll
  for (int dy = 0; dy < R; ++dy)
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      float v = acc[dy][k];
#pragma unroll
      for (int off = 32; off >= R; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane < R) red[wv][(dy*R + dx)*10 + k] = v;
    }
  __syncthreads();
  for (int n = threadIdx.x; n < 10*R*R; n += kSpBlock) partial[(size_t)blockIdx.x*10*R*R + n] = sum_waves<Waves::Sequential, kSpWaves>(&red[0][0], 10*R*R, n);
}

// g_weight[(c r^2 + k) 9 + t] (t < 9) / g_bias[c r^2 + k] (t = 9) = the sum over samples and blocks of partial[((b C + c) per + p) 10 r^2 + k 10 + t] (fp64, fixed order)
__global__ __launch_bounds__(64) void k_sp_w_finalize(const float* __restrict__ partial, int B, int C, unsigned per, int rr, float* __restrict__ g_weight,
                                                      float* __restrict__ g_bias) {
  const int n10 = 10*rr, c = blockIdx.x/n10, n = blockIdx.x - c*n10, k = n/10, t = n - k*10;
  double acc = 0.0;
  const unsigned total = (unsigned)B*per;
  for (unsigned i = threadIdx.x; i < total; i += 64) { const unsigned b = i/per, pp = i - b*per; acc += (double)partial[(((size_t)b*C + c)*per + pp)*n10 + n]; }
  acc = wave_sum_f64(acc);
  if (threadIdx.x != 0) return;
  if (t < 9) { if (g_weight) g_weight[((size_t)c*rr + k)*9 + t] = (float)acc; }
  else if (g_bias) g_bias[(size_t)c*rr + k] = (float)acc;
}
__global__ __launch_bounds__(64) void k_sp_pb_finalize(const double* __restrict__ partial, int B, int C, unsigned chunks, float* __restrict__ g_pb) {
  const int c = blockIdx.x;
  double acc = 0.0;
  const unsigned n = (unsigned)B*chunks;
  for (unsigned i = threadIdx.x; i < n; i += 64) { const unsigned b = i/chunks, k = i - b*chunks; acc += partial[((size_t)b*C + c)*chunks + k]; }
  acc = wave_sum_f64(acc);
  if (threadIdx.x == 0) g_pb[c] = (float)acc;
}

// f(std::integral_constant<int, r>) for the served r
template <class F> static void for_factor(int r, F f) {
  if (r == 2) f(std::integral_constant<int, 2>{}); else if (r == 4) f(std::integral_constant<int, 4>{}); else f(std::integral_constant<int, 8>{});
}

hipError_t launch_subpixel_fwd(const SubPixel& s, const float* x, const float* pre_bias, const float* weight, const float* bias, const float* skip, float* out,
                               hipStream_t st) {
  const int RH = s.r*s.h, RW = s.r*s.w;
  const SpGrid g = sp_grid(s.h, RW + 2*s.pad, kSpRowsFwd);
  const unsigned blocks = (unsigned)((size_t)s.B*s.C*g.bands*g.strips);
  for_factor(s.r, [&](auto r) { hipLaunchKernelGGL((k_sp_fwd<decltype(r)::value>), dim3(blocks), dim3(kSpBlock), 0, st, x, pre_bias, weight, bias, out, s, g); });
  if (s.Cs > 0) {
    const unsigned chunks = ceil_div((RH + 2)*(RW + 2), kDecChunk);
    hipLaunchKernelGGL(k_sp_skip_fwd, dim3((unsigned)((size_t)s.B*s.Cs*chunks)), dim3(kDecBlock), 0, st, skip, out, s.C, s.Cs, RH, RW, chunks);
  }
  return hipGetLastError();
}

hipError_t launch_subpixel_bwd(const SubPixel& s, const float* x, const float* pre_bias, const float* weight, const float* out, const float* g_out, float* g_x,
                               float* g_pre_bias, float* g_weight, float* g_bias, float* g_skip, float* ws, hipStream_t st) {
  const int RH = s.r*s.h, RW = s.r*s.w;
  if (g_x || g_pre_bias) {
    const unsigned chunks = ceil_div(s.h*s.w, kDecChunk);
    const unsigned blocks = (unsigned)((size_t)s.B*s.C*chunks);
    for_factor(s.r, [&](auto r) {
      hipLaunchKernelGGL((k_sp_bwd_x<decltype(r)::value>), dim3(blocks), dim3(kDecBlock), 0, st, x, pre_bias, weight, out, g_out, g_x, g_pre_bias ? (double*)ws : nullptr, s, chunks);
    });
    if (g_pre_bias) hipLaunchKernelGGL(k_sp_pb_finalize, dim3(s.C), dim3(64), 0, st, (const double*)ws, s.B, s.C, chunks, g_pre_bias);
  }
  if (g_weight || g_bias) {
    float* partial = ws + sp_pb_partials(s);
    const SpGrid g = sp_grid(s.h, RW, kSpRowsWgt);
    const unsigned per = g.strips*g.bands, blocks = (unsigned)((size_t)s.B*s.C*per);
    for_factor(s.r, [&](auto r) { hipLaunchKernelGGL((k_sp_bwd_w<decltype(r)::value>), dim3(blocks), dim3(kSpBlock), 0, st, x, pre_bias, out, g_out, partial, s, g); });
    hipLaunchKernelGGL(k_sp_w_finalize, dim3((unsigned)(s.C*10*s.r*s.r)), dim3(64), 0, st, partial, s.B, s.C, per, s.r*s.r, g_weight, g_bias);
  }
  if (g_skip && s.Cs > 0) {
    const unsigned chunks = ceil_div(RH*RW, kDecChunk);
    hipLaunchKernelGGL(k_sp_skip_bwd, dim3((unsigned)((size_t)s.B*s.Cs*chunks)), dim3(kDecBlock), 0, st, g_out, g_skip, s.C, s.Cs, RH, RW, chunks);
  }
  return hipGetLastError();
}

}  // namespace smd
