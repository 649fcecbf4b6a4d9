// smd_conv_headn.hip — output heads with a FEW output channels: reflect-pad -> conv3x3(C -> n) -> act, 1 <= n <= 4.  The predictive-mask decoder's heads
// (reference: src/networks/depth.py:12, 108-114 — `MonodepthDecoder(out_ch=num_ch_mask, out_act=MASKS[mask_name])`, one weight per support frame and pixel,
// sigmoid for explainability masks and relu for uncertainty masks; src/networks/decoders/monodepth.py:52, 86-87).
//
// n output channels on C input channels are still a stencil: 9 C n multiply-adds per pixel on the same 4 C bytes of input.  The kernels are those of
// smd_conv_head.hip with n accumulators per output row: the padded activation is read ONCE for all n channels (n passes of the one-channel head would read it
// n times; the weights are wave-uniform scalar loads either way).
//   k_headn_fwd      y[o] = act(bias[o] + sum_c sum_3x3 w[o,c,ky,kx] xp[c, i+ky, j+kx])
//   k_headn_bwd_data g_xp[c, p, q] = sum_o sum_3x3 w[o,c,ky,kx] gp[o, p-ky, q-kx]
//   k_headn_bwd_wgt  g_w[o,c,ky,kx] = sum_pixels gp[o,i,j] xp[c, i+ky, j+kx];  g_bias[o] = sum gp[o]   per-block partial sums, then a fixed-order fp64 sum
// with gp = g_y * act'(y) recomputed from the saved output (sigmoid: y (1 - y); relu: y > 0).  Deterministic (no atomics), fp32 arithmetic in a fixed order.
#include "smd_common.h"
#include "smd_kernels.h"
#include "smd_head_dev.h"

namespace smd {

constexpr int kHeadnWgtTiles = 3;   // vertically adjacent 64 x 16 tiles per block of the weight gradient (as the one-channel head)

// act: 0 identity, 1 sigmoid, 2 relu
__device__ __forceinline__ float headn_act(float v, int act) { return act == 1 ? 1.f/(1.f + __expf(-v)) : (act == 2 ? fmaxf(v, 0.f) : v); }

// The launch shapes are k_head_fwd's: R rows per thread; SPLIT: the block's four waves share one row group and take the input channels in turn.
template <int N, int R, bool SPLIT, typename TX, bool DW>
__global__ __launch_bounds__(256) void k_headn_fwd(const TX* __restrict__ xp, const float* __restrict__ wgt, const float* __restrict__ bias, float* __restrict__ y,
                                                   int C, int h, int w, int act) {
  __shared__ float red[SPLIT ? 3 : 1][SPLIT ? N : 1][R][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x*kHeadTileW + lane, y0 = SPLIT ? blockIdx.y*R : (blockIdx.y*4 + wv)*R, b = blockIdx.z;
  const bool live = x < w && y0 < h;
  const int W = w + 2, H = h + 2;
  const int rows = live ? min(R, h - y0) : 0;
  float acc[N][R];
#pragma unroll
  for (int o = 0; o < N; ++o)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[o][r] = 0.f;
  if (live) {
    const int c0 = SPLIT ? wv : 0, cs = SPLIT ? 4 : 1;
    Row3<TX, DW> rp(xp, (((size_t)b*C + c0)*H + y0)*W + x);
#pragma unroll 2
    for (int c = c0; c < C; c += cs, rp.next_channel((size_t)cs*H*W)) {
      float v[R + 2][3];
      if constexpr (DW) {
        unsigned d0[R + 2], d1[R + 2];
#pragma unroll
        for (int r = 0; r < R + 2; ++r) rp.request((size_t)min(r, rows + 1)*W, d0[r], d1[r]);   // (rows beyond the image's last: the last one again, unused)
#pragma unroll
        for (int r = 0; r < R + 2; ++r) {
          rp.unpack(d0[r], d1[r], v[r][0], v[r][1], v[r][2]);
          if (r >= rows + 2) v[r][0] = v[r][1] = v[r][2] = 0.f;
        }
      } else {
#pragma unroll
        for (int r = 0; r < R + 2; ++r) {
          if (r < rows + 2) rp.load((size_t)r*W, v[r][0], v[r][1], v[r][2]);   // (rows beyond the image's last: not read)
          else v[r][0] = v[r][1] = v[r][2] = 0.f;
        }
      }
#pragma unroll
      for (int o = 0; o < N; ++o) {
        const float* wc = wgt + ((size_t)o*C + c)*9;               // wave-uniform: scalar loads
        const float w00 = wc[0], w01 = wc[1], w02 = wc[2], w10 = wc[3], w11 = wc[4], w12 = wc[5], w20 = wc[6], w21 = wc[7], w22 = wc[8];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float s = acc[o][r];
          s = fmaf(w00, v[r][0], s); s = fmaf(w01, v[r][1], s); s = fmaf(w02, v[r][2], s);
          s = fmaf(w10, v[r + 1][0], s); s = fmaf(w11, v[r + 1][1], s); s = fmaf(w12, v[r + 1][2], s);
          s = fmaf(w20, v[r + 2][0], s); s = fmaf(w21, v[r + 2][1], s); s = fmaf(w22, v[r + 2][2], s);
          acc[o][r] = s;
        }
      }
    }
  }
  if (SPLIT) {
    if (wv > 0) {
#pragma unroll
      for (int o = 0; o < N; ++o)
#pragma unroll
        for (int r = 0; r < R; ++r) red[wv - 1][o][r][lane] = acc[o][r];
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int o = 0; o < N; ++o)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[o][r] = ((acc[o][r] + red[0][o][r][lane]) + red[1][o][r][lane]) + red[2][o][r][lane];
  }
#pragma unroll
  for (int o = 0; o < N; ++o) {
    const float bc = bias ? bias[o] : 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) if (r < rows) y[(((size_t)b*N + o)*h + y0 + r)*w + x] = headn_act(acc[o][r] + bc, act);
  }
}

// gp = g_y * act'(y) at (i, j) of the plane that starts at `base`, zero outside the image
__device__ __forceinline__ float headn_gp(const float* __restrict__ gy, const float* __restrict__ y, size_t base, int i, int j, int h, int w, int act) {
  if (i < 0 || i >= h || j < 0 || j >= w) return 0.f;
  const float g = gy[base + (size_t)i*w + j];
  if (act == 0) return g;
  const float s = y[base + (size_t)i*w + j];
  return act == 1 ? g*s*(1.f - s) : (s > 0.f ? g : 0.f);
}

// grid (ceil(W/64), ceil(H/4), B * G): channel group blockIdx.z % G takes channels [g * Cg, (g + 1) * Cg); a thread owns one padded position
template <int N, typename TX, bool DW>
__global__ __launch_bounds__(256) void k_headn_bwd_data(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ wgt, TX* __restrict__ g_xp,
                                                        int C, int h, int w, int G, int Cg, int act) {
  const int W = w + 2, H = h + 2;
  const int q = blockIdx.x*64 + (threadIdx.x & 63), p = blockIdx.y*4 + (threadIdx.x >> 6), b = blockIdx.z/G, g = blockIdx.z - b*G;
  if (q >= W || p >= H) return;                                 // (DW: W even, the last column W - 1 is odd and its partner W - 2 is a live lane of the same wave)
  float nb[N][9];                              // nb[o][ky*3 + kx] = gp[o, p - ky, q - kx]: the outputs whose window holds padded position (p, q) at (ky, kx)
#pragma unroll
  for (int o = 0; o < N; ++o) {
    const size_t base = ((size_t)b*N + o)*h*w;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) nb[o][ky*3 + kx] = headn_gp(gy, y, base, p - ky, q - kx, h, w, act);
  }
  const int c0 = g*Cg, c1 = min(c0 + Cg, C);
  TX* o_ = g_xp + (((size_t)b*C + c0)*H + p)*W + q;
  for (int c = c0; c < c1; ++c, o_ += (size_t)H*W) {
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < N; ++o) {
      const float* wc = wgt + ((size_t)o*C + c)*9;
#pragma unroll
      for (int k = 0; k < 9; ++k) s = fmaf(wc[k], nb[o][k], s);
    }
    if constexpr (sizeof(TX) == 2 && DW) {                      // bfloat16, even pitch: an even lane stores its neighbour's value with its own, one dword
      const float nx = __shfl_down(s, 1, 64);
      if ((q & 1) == 0) {
        typedef float f2 __attribute__((ext_vector_type(2))); typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        const f2 pr = {s, nx};
        *reinterpret_cast<unsigned*>(o_) = __builtin_bit_cast(unsigned, __builtin_convertvector(pr, b2));
      }
    } else st_from_float<TX>(o_, 0, s);
  }
}

// grid (tiles_x, B * chunks_y, C + 1): a block walks kHeadnWgtTiles vertically adjacent 64 x 16 tiles of its (tile column, sample, input channel) and leaves
// N x 9 sums; input channel C is the biases' job (sums of gp).  partial[((c * T + tile) * N + o) * 9 + k], T = tiles_x * B * chunks_y.
template <int N, typename TX, bool DW>
__global__ __launch_bounds__(256) void k_headn_bwd_wgt(const TX* __restrict__ xp, const float* __restrict__ gy, const float* __restrict__ y, float* __restrict__ partial,
                                                       int C, int h, int w, int chunks_y, int act) {
  __shared__ float red[4][N*9];
  const int W = w + 2, H = h + 2;
  const int b = blockIdx.y/chunks_y, chunk = blockIdx.y - b*chunks_y, c = blockIdx.z;
  const int x = blockIdx.x*kHeadTileW + (threadIdx.x & 63);
  float acc[N][9];
#pragma unroll
  for (int o = 0; o < N; ++o)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[o][k] = 0.f;
  if (x < w) {
    const int ylo = chunk*kHeadnWgtTiles*kHeadTileH, yhi = min(ylo + kHeadnWgtTiles*kHeadTileH, h);
    for (int y0 = ylo + (threadIdx.x >> 6)*kHeadRows; y0 < yhi; y0 += kHeadTileH) {
      const int rows = min(kHeadRows, h - y0);
      float g[N][kHeadRows];
#pragma unroll
      for (int o = 0; o < N; ++o)
#pragma unroll
        for (int r = 0; r < kHeadRows; ++r) g[o][r] = r < rows ? headn_gp(gy, y, ((size_t)b*N + o)*h*w, y0 + r, x, h, w, act) : 0.f;
      if (c == C) {
#pragma unroll
        for (int o = 0; o < N; ++o)
#pragma unroll
          for (int r = 0; r < kHeadRows; ++r) acc[o][0] += g[o][r];
      } else {
        const Row3<TX, DW> rp(xp, (((size_t)b*C + c)*H + y0)*W + x);
        float v[kHeadRows + 2][3];
        if constexpr (DW) {
          unsigned d0[kHeadRows + 2], d1[kHeadRows + 2];
#pragma unroll
          for (int r = 0; r < kHeadRows + 2; ++r) rp.request((size_t)min(r, rows + 1)*W, d0[r], d1[r]);
#pragma unroll
          for (int r = 0; r < kHeadRows + 2; ++r) {
            rp.unpack(d0[r], d1[r], v[r][0], v[r][1], v[r][2]);
            if (r >= rows + 2) v[r][0] = v[r][1] = v[r][2] = 0.f;
          }
        } else {
#pragma unroll
          for (int r = 0; r < kHeadRows + 2; ++r) {
            if (r < rows + 2) rp.load((size_t)r*W, v[r][0], v[r][1], v[r][2]);
            else v[r][0] = v[r][1] = v[r][2] = 0.f;
          }
        }
#pragma unroll
        for (int o = 0; o < N; ++o)
#pragma unroll
          for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
              for (int kx = 0; kx < 3; ++kx) acc[o][ky*3 + kx] = fmaf(g[o][r], v[r + ky][kx], acc[o][ky*3 + kx]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < N; ++o)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float t = wave_sum(acc[o][k]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][o*9 + k] = t;
    }
  __syncthreads();
  if (threadIdx.x < N*9) {
    const size_t T = (size_t)gridDim.x*gridDim.y;
    const size_t tile = (size_t)blockIdx.y*gridDim.x + blockIdx.x;
    partial[((size_t)c*T + tile)*(N*9) + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// g_w[(o*C + c)*9 + k] (c < C) and g_bias[o] = fp64 sums of the blocks' partial sums in block order; grid (C + 1, N), one wave each
__global__ __launch_bounds__(64) void k_headn_wgt_finalize(const float* __restrict__ partial, unsigned T, int C, int N, float* __restrict__ g_w, float* __restrict__ g_bias) {
  const int c = blockIdx.x, o = blockIdx.y;
  const int nk = c == C ? 1 : 9;
  for (int k = 0; k < nk; ++k) {
    double acc = 0.0;
    for (unsigned t = threadIdx.x; t < T; t += 64) acc += (double)partial[(((size_t)c*T + t)*N + o)*9 + k];
    acc = wave_sum_f64(acc);
    if (threadIdx.x == 0) {
      if (c == C) { if (g_bias) g_bias[o] = (float)acc; }
      else g_w[((size_t)o*C + c)*9 + k] = (float)acc;
    }
  }
}

static inline int headn_wgt_chunks(int h) { return ceil_div(ceil_div(h, kHeadTileH), kHeadnWgtTiles); }
size_t conv_headn_partials(int B, int C, int N, int h, int w) { return (size_t)(C + 1)*ceil_div(w, kHeadTileW)*B*headn_wgt_chunks(h)*9*N; }

template <int N, typename TX, bool DW>
static void headn_fwd_t(const TX* xp, const float* wgt, const float* bias, float* y, int B, int C, int h, int w, int act, hipStream_t st) {
  const int tx = ceil_div(w, kHeadTileW);
  if ((long long)B*tx*ceil_div(h, kHeadTileH)*4 >= kHeadEnoughWaves || C < 8)
    hipLaunchKernelGGL((k_headn_fwd<N, kHeadRows, false, TX, DW>), dim3(tx, ceil_div(h, kHeadTileH), B), dim3(256), 0, st, xp, wgt, bias, y, C, h, w, act);
  else if ((long long)B*tx*ceil_div(h, 2)*4 >= kHeadEnoughWaves)
    hipLaunchKernelGGL((k_headn_fwd<N, 2, true, TX, DW>), dim3(tx, ceil_div(h, 2), B), dim3(256), 0, st, xp, wgt, bias, y, C, h, w, act);
  else
    hipLaunchKernelGGL((k_headn_fwd<N, 1, true, TX, DW>), dim3(tx, h, B), dim3(256), 0, st, xp, wgt, bias, y, C, h, w, act);
}

template <int N, typename TX, bool DW>
static void headn_bwd_t(const TX* xp, const float* wgt, const float* y, const float* gy, TX* g_xp, float* g_w, float* g_bias, float* partial,
                        int B, int C, int h, int w, int act, hipStream_t st) {
  if (g_xp) {
    const long long waves = (long long)B*ceil_div(w + 2, 64)*ceil_div(h + 2, 4)*4;
    int G = (int)((kHeadEnoughWaves + waves - 1)/waves);
    if (G > C) G = C;
    if (G < 1) G = 1;
    if ((long long)B*G > 65535) G = 65535/B > 0 ? 65535/B : 1;
    const int Cg = ceil_div(C, G);
    G = ceil_div(C, Cg);
    hipLaunchKernelGGL((k_headn_bwd_data<N, TX, DW>), dim3(ceil_div(w + 2, 64), ceil_div(h + 2, 4), B*G), dim3(256), 0, st, gy, y, wgt, g_xp, C, h, w, G, Cg, act);
  }
  if (g_w) {
    const int tx = ceil_div(w, kHeadTileW);
    const int cy = headn_wgt_chunks(h);
    hipLaunchKernelGGL((k_headn_bwd_wgt<N, TX, DW>), dim3(tx, B*cy, C + 1), dim3(256), 0, st, xp, gy, y, partial, C, h, w, cy, act);
    hipLaunchKernelGGL(k_headn_wgt_finalize, dim3(C + 1, N), dim3(64), 0, st, partial, (unsigned)(tx*B*cy), C, N, g_w, g_bias);
  }
}

template <int N>
static void headn_fwd_n(const void* xp, int x_bf16, const float* wgt, const float* bias, float* y, int B, int C, int h, int w, int act, hipStream_t st) {
  if (x_bf16 && (w & 1) == 0) headn_fwd_t<N, bf16, true>((const bf16*)xp, wgt, bias, y, B, C, h, w, act, st);      // (every decoder level has an even width)
  else if (x_bf16) headn_fwd_t<N, bf16, false>((const bf16*)xp, wgt, bias, y, B, C, h, w, act, st);
  else headn_fwd_t<N, float, false>((const float*)xp, wgt, bias, y, B, C, h, w, act, st);
}
template <int N>
static void headn_bwd_n(const void* xp, int x_bf16, const float* wgt, const float* y, const float* gy, void* g_xp, float* g_w, float* g_bias, float* partial,
                        int B, int C, int h, int w, int act, hipStream_t st) {
  if (x_bf16 && (w & 1) == 0) headn_bwd_t<N, bf16, true>((const bf16*)xp, wgt, y, gy, (bf16*)g_xp, g_w, g_bias, partial, B, C, h, w, act, st);
  else if (x_bf16) headn_bwd_t<N, bf16, false>((const bf16*)xp, wgt, y, gy, (bf16*)g_xp, g_w, g_bias, partial, B, C, h, w, act, st);
  else headn_bwd_t<N, float, false>((const float*)xp, wgt, y, gy, (float*)g_xp, g_w, g_bias, partial, B, C, h, w, act, st);
}

hipError_t launch_conv_headn_fwd(const void* xp, int x_bf16, const float* wgt, const float* bias, float* y, int B, int C, int N, int h, int w, int act, hipStream_t st) {
  switch (N) {
    case 1: headn_fwd_n<1>(xp, x_bf16, wgt, bias, y, B, C, h, w, act, st); break;
    case 2: headn_fwd_n<2>(xp, x_bf16, wgt, bias, y, B, C, h, w, act, st); break;
    case 3: headn_fwd_n<3>(xp, x_bf16, wgt, bias, y, B, C, h, w, act, st); break;
    case 4: headn_fwd_n<4>(xp, x_bf16, wgt, bias, y, B, C, h, w, act, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_conv_headn_bwd(const void* xp, int x_bf16, const float* wgt, const float* y, const float* gy, void* g_xp, float* g_w, float* g_bias, float* partial,
                                 int B, int C, int N, int h, int w, int act, hipStream_t st) {
  switch (N) {
    case 1: headn_bwd_n<1>(xp, x_bf16, wgt, y, gy, g_xp, g_w, g_bias, partial, B, C, h, w, act, st); break;
    case 2: headn_bwd_n<2>(xp, x_bf16, wgt, y, gy, g_xp, g_w, g_bias, partial, B, C, h, w, act, st); break;
    case 3: headn_bwd_n<3>(xp, x_bf16, wgt, y, gy, g_xp, g_w, g_bias, partial, B, C, h, w, act, st); break;
    case 4: headn_bwd_n<4>(xp, x_bf16, wgt, y, gy, g_xp, g_w, g_bias, partial, B, C, h, w, act, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace smd
