// smd_decoder.hip — glue between the 3x3 convolutions of the Monodepth decoder.
//
// The reference decoder (src/networks/decoders/monodepth.py:71-89, decoders/utils.py:44-54) runs, per stage,
//   reflect-pad -> conv3x3 -> ELU -> nearest x2 -> cat(skip) -> reflect-pad -> conv3x3 -> ELU -> [reflect-pad -> conv3x3 -> sigmoid]
// as separate ATen kernels, each a full read + write of the activation.  The convolutions stay with MIOpen; everything
// between them collapses into two gather kernels that write the NEXT convolution's already-padded input:
//   k_elu_pad         out = reflect_pad1(elu(x + bias))                              (B,C,h,w)           -> (B,C,h+2,w+2)
//   k_elu_up_cat_pad  out = reflect_pad1(cat(nearest_x2(elu(a + bias)), skip))       (B,Ca,h,w),(B,Cs,2h,2w) -> (B,Ca+Cs,2h+2,2w+2)
// and two adjoint gathers (deterministic, no atomics).  The convolution's bias is added here (the convolution itself runs
// bias-free), so MIOpen's separate bias pass and ATen's bias-gradient reduction over the full tensor both disappear: the
// adjoint gathers already hold the pre-activation gradient and emit its per-block channel sums.  ELU is recomputed from the saved pre-activation in the backward
// (elu'(x) = x > 0 ? 1 : exp(x)), so no activated tensor is kept.
#include "smd_common.h"
#include "smd_kernels.h"

namespace smd {

constexpr int kDecBlock = 256;
constexpr int kDecPerThread = 4;   // block-strided elements per thread: 4 independent load->store chains, 4x fewer blocks
constexpr int kDecChunk = kDecBlock*kDecPerThread;

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : __expf(x) - 1.f; }
__device__ __forceinline__ float elu1_grad(float x) { return x > 0.f ? 1.f : __expf(x); }
// the activation the pad kernels apply to x + bias: the Monodepth stages' ELU, the DiffNet attention stages' ReLU
enum { kActNone = 0, kActElu = 1, kActRelu = 2 };
__device__ __forceinline__ float glue_act(float x, int act) { return act == kActElu ? elu1(x) : (act == kActRelu ? fmaxf(x, 0.f) : x); }
__device__ __forceinline__ float glue_act_grad(float x, int act) { return act == kActElu ? elu1_grad(x) : (act == kActRelu ? (x > 0.f ? 1.f : 0.f) : 1.f); }
__device__ __forceinline__ int unpad_reflect(int p, int n) { const int r = p - 1; return r < 0 ? -r : (r >= n ? 2*(n - 1) - r : r); }

__device__ __forceinline__ void block_store_sum(float v, float* red, float* dst) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) { float t = 0.f; for (int k = 0; k < kDecBlock/64; ++k) t += red[k]; *dst = t; }
}

// g_bias[c] = sum over samples and chunks of the per-block partial sums of the pre-activation gradient (fp64, fixed order).
__global__ __launch_bounds__(64) void k_bias_finalize(const float* __restrict__ partial, int B, int C, unsigned chunks, float* __restrict__ g_bias) {
  const int c = blockIdx.x;
  double acc = 0.0;
  const unsigned per = chunks, n = (unsigned)B*per;
  for (unsigned i = threadIdx.x; i < n; i += 64) { const unsigned b = i/per, k = i - b*per; acc += (double)partial[((size_t)b*C + c)*per + k]; }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (threadIdx.x == 0) g_bias[c] = (float)acc;
}

// Sum of g over the padded positions that read un-padded index r along one axis of length n: p = r+1, plus the mirrored
// border cell when r is the second / second-to-last element.
#define SMD_PAD_ADJ_POS(r, n, p0, p1, p2) const int p0 = (r) + 1, p1 = ((r) == 1) ? 0 : -1, p2 = ((r) == (n) - 2) ? (n) + 1 : -1

template <typename TA, typename TO>
__global__ __launch_bounds__(kDecBlock) void k_elu_pad_fwd(const TA* __restrict__ x, const float* __restrict__ bias, TO* __restrict__ out, int C, int h, int w, int act,
                                                           unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;
  const int H = h + 2, W = w + 2;
  const float bc = bias ? bias[plane % C] : 0.f;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H*W) break;
    const int py = idx/W, px = idx - py*W;
    const float v = ld_as_float<TA>(x, (size_t)plane*h*w + unpad_reflect(py, h)*w + unpad_reflect(px, w)) + bc;
    st_from_float<TO>(out, (size_t)plane*H*W + idx, glue_act(v, act));
  }
}

template <typename TA, typename TO>
__global__ __launch_bounds__(kDecBlock) void k_elu_pad_bwd(const TA* __restrict__ x, const float* __restrict__ bias, const TO* __restrict__ g_out,
                                                           TA* __restrict__ g_x, float* __restrict__ bias_partial, int C, int h, int w, int act,
                                                           unsigned chunks) {
  __shared__ float red[kDecBlock/64];
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;
  const int W = w + 2;
  const float bc = bias ? bias[plane % C] : 0.f;
  float bsum = 0.f;
  const TO* g = g_out + (size_t)plane*(h + 2)*W;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= h*w) break;
    const int i = idx/w, j = idx - i*w;
    float acc = ld_as_float<TO>(g, (i + 1)*W + j + 1);
    if (i == 1 || i == h - 2 || j == 1 || j == w - 2) {   // rare: mirrored border cells
      SMD_PAD_ADJ_POS(i, h, y0, y1, y2); SMD_PAD_ADJ_POS(j, w, x0, x1, x2);
      const int ys[3] = {y0, y1, y2}, xs[3] = {x0, x1, x2};
      acc = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (ys[a] < 0) continue;
#pragma unroll
        for (int b = 0; b < 3; ++b) if (xs[b] >= 0) acc += ld_as_float<TO>(g, ys[a]*W + xs[b]);
      }
    }
    const float gv = act ? acc*glue_act_grad(ld_as_float<TA>(x, (size_t)plane*h*w + idx) + bc, act) : acc;
    st_from_float<TA>(g_x, (size_t)plane*h*w + idx, gv); bsum += gv;
  }
  if (bias_partial) block_store_sum(bsum, red, bias_partial + blockIdx.x);
}

template <typename TA, typename TS, typename TO>
__global__ __launch_bounds__(kDecBlock) void k_elu_up_cat_pad_fwd(const TA* __restrict__ a, const float* __restrict__ bias, const TS* __restrict__ skip,
                                                                  TO* __restrict__ out, int Ca, int Cs, int h, int w, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*(Ca+Cs) + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, H = H2 + 2, W = W2 + 2;
  const unsigned b = plane/C, c = plane - b*C;
  const bool from_a = (int)c < Ca;
  const float bc = (from_a && bias) ? bias[c] : 0.f;
  const TA* src_a = a + ((size_t)b*Ca + (from_a ? c : 0))*h*w;
  const TS* src_s = from_a ? nullptr : skip + ((size_t)b*Cs + (c - Ca))*H2*W2;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H*W) break;
    const int py = idx/W, px = idx - py*W;
    const int r = unpad_reflect(py, H2), q = unpad_reflect(px, W2);
    st_from_float<TO>(out, (size_t)plane*H*W + idx, from_a ? elu1(ld_as_float<TA>(src_a, (r >> 1)*w + (q >> 1)) + bc) : ld_as_float<TS>(src_s, r*W2 + q));
  }
}

// Adjoint w.r.t. `a` (low resolution): each source pixel feeds a 2x2 block of the up-sampled map, each cell of which
// feeds its padded position plus (on the second / second-to-last row or column) the mirrored border cell.
template <typename TA, typename TO>
__global__ __launch_bounds__(kDecBlock) void k_elu_up_cat_pad_bwd_a(const TA* __restrict__ a, const float* __restrict__ bias, const TO* __restrict__ g_out,
                                                                    TA* __restrict__ g_a, float* __restrict__ bias_partial, int Ca, int Cs, int h, int w,
                                                                    unsigned chunks) {
  __shared__ float red[kDecBlock/64];
  float bsum = 0.f;
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Ca + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, W = W2 + 2;
  const unsigned b = plane/Ca, c = plane - b*Ca;
  const TO* g = g_out + ((size_t)b*C + c)*(H2 + 2)*W;
  const float bc = bias ? bias[c] : 0.f;
  for (int k = 0; k < kDecPerThread; ++k) {
  const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
  if (idx >= h*w) break;
  const int i = idx/w, j = idx - i*w;
  float acc = 0.f;
  if (i > 0 && i < h - 1 && j > 0 && j < w - 1) {   // interior: the plain 2x2 block
    const TO* gp = g + (2*i + 1)*W + 2*j + 1;
    acc = (ld_as_float<TO>(gp, 0) + ld_as_float<TO>(gp, 1)) + (ld_as_float<TO>(gp, W) + ld_as_float<TO>(gp, W + 1));
  } else
#pragma unroll
  for (int dr = 0; dr < 2; ++dr) {
    const int r = 2*i + dr;
    SMD_PAD_ADJ_POS(r, H2, y0, y1, y2);
    const int ys[3] = {y0, y1, y2};
#pragma unroll
    for (int dq = 0; dq < 2; ++dq) {
      const int q = 2*j + dq;
      SMD_PAD_ADJ_POS(q, W2, x0, x1, x2);
      const int xs[3] = {x0, x1, x2};
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        if (ys[m] < 0) continue;
#pragma unroll
        for (int n = 0; n < 3; ++n) if (xs[n] >= 0) acc += ld_as_float<TO>(g, ys[m]*W + xs[n]);
      }
    }
  }
  const float gv = acc*elu1_grad(ld_as_float<TA>(a, (size_t)plane*h*w + idx) + bc);
  st_from_float<TA>(g_a, (size_t)plane*h*w + idx, gv); bsum += gv;
  }
  if (bias_partial) block_store_sum(bsum, red, bias_partial + blockIdx.x);
}

// Adjoint w.r.t. the skip tensor (full resolution): plain reflection-pad adjoint of its channel slice.
template <typename TS, typename TO>
__global__ __launch_bounds__(kDecBlock) void k_elu_up_cat_pad_bwd_skip(const TO* __restrict__ g_out, TS* __restrict__ g_skip,
                                                                       int Ca, int Cs, int h, int w, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Cs + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, W = W2 + 2;
  const unsigned b = plane/Cs, c = plane - b*Cs;
  const TO* g = g_out + ((size_t)b*C + Ca + c)*(H2 + 2)*W;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H2*W2) break;
    const int r = idx/W2, q = idx - r*W2;
    float acc = ld_as_float<TO>(g, (r + 1)*W + q + 1);
    if (r == 1 || r == H2 - 2 || q == 1 || q == W2 - 2) {
      SMD_PAD_ADJ_POS(r, H2, y0, y1, y2); SMD_PAD_ADJ_POS(q, W2, x0, x1, x2);
      const int ys[3] = {y0, y1, y2}, xs[3] = {x0, x1, x2};
      acc = 0.f;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        if (ys[m] < 0) continue;
#pragma unroll
        for (int n = 0; n < 3; ++n) if (xs[n] >= 0) acc += ld_as_float<TO>(g, ys[m]*W + xs[n]);
      }
    }
    st_from_float<TS>(g_skip, (size_t)plane*H2*W2 + idx, acc);
  }
}

// dtypes: bit 0 = x / a (and their gradients) are bf16, bit 1 = skip (and its gradient), bit 2 = out (and its gradient).
#define SMD_DT_A 1
#define SMD_DT_S 2
#define SMD_DT_O 4

static hipError_t launch_act_pad_fwd(const void* x, const float* bias, void* out, int B, int C, int h, int w, int act, int dt, hipStream_t st) {
  const unsigned chunks = ceil_div((h + 2)*(w + 2), kDecChunk);
  const dim3 grid((unsigned)((size_t)B*C*chunks)), blk(kDecBlock);
#define SMD_GO(TA_, TO_) hipLaunchKernelGGL((k_elu_pad_fwd<TA_, TO_>), grid, blk, 0, st, (const TA_*)x, bias, (TO_*)out, C, h, w, act, chunks)
  if (dt & SMD_DT_A) { if (dt & SMD_DT_O) SMD_GO(bf16, bf16); else SMD_GO(bf16, float); }
  else { if (dt & SMD_DT_O) SMD_GO(float, bf16); else SMD_GO(float, float); }
#undef SMD_GO
  return hipGetLastError();
}
size_t decoder_bias_partials(int B, int C, int h, int w) { return (size_t)B*C*ceil_div(h*w, kDecChunk); }
static hipError_t launch_act_pad_bwd(const void* x, const float* bias, const void* g_out, void* g_x, float* g_bias, float* ws, int B, int C, int h, int w,
                                     int act, int dt, hipStream_t st) {
  const unsigned chunks = ceil_div(h*w, kDecChunk);
  const dim3 grid((unsigned)((size_t)B*C*chunks)), blk(kDecBlock);
#define SMD_GO(TA_, TO_) hipLaunchKernelGGL((k_elu_pad_bwd<TA_, TO_>), grid, blk, 0, st, (const TA_*)x, bias, (const TO_*)g_out, (TA_*)g_x, g_bias ? ws : nullptr, C, h, w, act, chunks)
  if (dt & SMD_DT_A) { if (dt & SMD_DT_O) SMD_GO(bf16, bf16); else SMD_GO(bf16, float); }
  else { if (dt & SMD_DT_O) SMD_GO(float, bf16); else SMD_GO(float, float); }
#undef SMD_GO
  if (g_bias) hipLaunchKernelGGL(k_bias_finalize, dim3(C), dim3(64), 0, st, ws, B, C, chunks, g_bias);
  return hipGetLastError();
}
// the public forms: `apply_elu` keeps its meaning (any non-zero value: ELU); the ReLU form is fp32 only
hipError_t launch_elu_pad_fwd(const void* x, const float* bias, void* out, int B, int C, int h, int w, int apply_elu, int dt, hipStream_t st) {
  return launch_act_pad_fwd(x, bias, out, B, C, h, w, apply_elu ? kActElu : kActNone, dt, st);
}
hipError_t launch_elu_pad_bwd(const void* x, const float* bias, const void* g_out, void* g_x, float* g_bias, float* ws, int B, int C, int h, int w,
                              int apply_elu, int dt, hipStream_t st) {
  return launch_act_pad_bwd(x, bias, g_out, g_x, g_bias, ws, B, C, h, w, apply_elu ? kActElu : kActNone, dt, st);
}
hipError_t launch_relu_pad_fwd(const float* x, const float* bias, float* out, int B, int C, int h, int w, hipStream_t st) {
  return launch_act_pad_fwd(x, bias, out, B, C, h, w, kActRelu, 0, st);
}
hipError_t launch_relu_pad_bwd(const float* x, const float* bias, const float* g_out, float* g_x, float* g_bias, float* ws, int B, int C, int h, int w,
                               hipStream_t st) {
  return launch_act_pad_bwd(x, bias, g_out, g_x, g_bias, ws, B, C, h, w, kActRelu, 0, st);
}
hipError_t launch_elu_up_cat_pad_fwd(const void* a, const float* bias, const void* skip, void* out, int B, int Ca, int Cs, int h, int w, int dt,
                                     hipStream_t st) {
  const unsigned chunks = ceil_div((2*h + 2)*(2*w + 2), kDecChunk);
  const dim3 grid((unsigned)((size_t)B*(Ca + Cs)*chunks)), blk(kDecBlock);
#define SMD_GO(TA_, TS_, TO_) hipLaunchKernelGGL((k_elu_up_cat_pad_fwd<TA_, TS_, TO_>), grid, blk, 0, st, (const TA_*)a, bias, (const TS_*)skip, (TO_*)out, Ca, Cs, h, w, chunks)
  switch (dt & 7) {
    case 0: SMD_GO(float, float, float); break;  case 1: SMD_GO(bf16, float, float); break;
    case 2: SMD_GO(float, bf16, float); break;   case 3: SMD_GO(bf16, bf16, float); break;
    case 4: SMD_GO(float, float, bf16); break;   case 5: SMD_GO(bf16, float, bf16); break;
    case 6: SMD_GO(float, bf16, bf16); break;    default: SMD_GO(bf16, bf16, bf16); break;
  }
#undef SMD_GO
  return hipGetLastError();
}
hipError_t launch_elu_up_cat_pad_bwd(const void* a, const float* bias, const void* g_out, void* g_a, void* g_skip, float* g_bias, float* ws,
                                     int B, int Ca, int Cs, int h, int w, int dt, hipStream_t st) {
  if (g_a) {
    const unsigned chunks = ceil_div(h*w, kDecChunk);
    const dim3 grid((unsigned)((size_t)B*Ca*chunks)), blk(kDecBlock);
#define SMD_GO(TA_, TO_) hipLaunchKernelGGL((k_elu_up_cat_pad_bwd_a<TA_, TO_>), grid, blk, 0, st, (const TA_*)a, bias, (const TO_*)g_out, (TA_*)g_a, g_bias ? ws : nullptr, Ca, Cs, h, w, chunks)
    if (dt & SMD_DT_A) { if (dt & SMD_DT_O) SMD_GO(bf16, bf16); else SMD_GO(bf16, float); }
    else { if (dt & SMD_DT_O) SMD_GO(float, bf16); else SMD_GO(float, float); }
#undef SMD_GO
    if (g_bias) hipLaunchKernelGGL(k_bias_finalize, dim3(Ca), dim3(64), 0, st, ws, B, Ca, chunks, g_bias);
  }
  if (g_skip && Cs > 0) {
    const unsigned chunks = ceil_div(4*h*w, kDecChunk);
    const dim3 grid((unsigned)((size_t)B*Cs*chunks)), blk(kDecBlock);
#define SMD_GO(TS_, TO_) hipLaunchKernelGGL((k_elu_up_cat_pad_bwd_skip<TS_, TO_>), grid, blk, 0, st, (const TO_*)g_out, (TS_*)g_skip, Ca, Cs, h, w, chunks)
    if (dt & SMD_DT_S) { if (dt & SMD_DT_O) SMD_GO(bf16, bf16); else SMD_GO(bf16, float); }
    else { if (dt & SMD_DT_O) SMD_GO(float, bf16); else SMD_GO(float, float); }
#undef SMD_GO
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- DiffNet attention stage
// reflect_pad1(gate o cat(nearest_x2(act(a + bias)), skip)) with gate = sigmoid(W2 relu(W1 mean_hw(cat(..)))) (reference: src/networks/decoders/diffnet.py:44-47,
// 70-74): on ATen everything in front of the stage's convolution is five full-size passes over the concatenation (interpolate, cat, the pooling read, the
// multiply, the reflection pad).  Here the concatenation is never written.
//   forward:  k_ucg_pool (per-block sums of act(a + bias) over the LOW-resolution plane — the mean of its nearest x2 up-sampling is the same number — and of
//             skip; in fp64 from the first add to the sigmoid: with large Linear weights the gate amplifies a rounding of the mean by the product of the two
//             layers' gains, and an fp32 mean then decides the error of the output and of every gradient) -> k_ucg_gate_fwd (one block per sample: means, the two small matrix-vector products) -> k_ucg_apply_fwd (the gather of
//             k_elu_up_cat_pad_fwd times the gate).
//   backward: k_ucg_reduce_bwd (per-block sums of G o src, G the pad adjoint of g_out, folded on the fly) -> k_ucg_gate_bwd (one block per sample: back
//             through the sigmoid, W2, the ReLU, W1) -> k_ucg_param_grad (the samples in order) -> k_ucg_apply_bwd_a / _skip (gate G + dmean / n).
// Every sum has a fixed order: no float atomics, two runs are bit-equal.
constexpr int kUcgItems = 4096;            // floats of a plane one block of the pooling sweep handles
constexpr int kUcgMaxChunks = 256;
constexpr int kUcgGateBlock = 1024;        // the per-sample block of the matrix-vector products
constexpr int kUcgGateWaves = kUcgGateBlock/64;

static int ucg_pool_chunks(int n) {
  const int c = ceil_div(n, kUcgItems);
  return c < 1 ? 1 : (c > kUcgMaxChunks ? kUcgMaxChunks : c);
}
// where the per-block sums of the two halves live and how many each plane has: the a planes first ((b Ca + c) cha + k), then the skip planes
struct UcgPartial { unsigned na; int cha, chs; };
static UcgPartial ucg_partial(const UpCatGate& s, bool bwd) {
  UcgPartial p;
  p.cha = bwd ? ceil_div(s.h*s.w, kDecChunk) : ucg_pool_chunks(s.h*s.w);
  p.chs = bwd ? ceil_div(4*s.h*s.w, kDecChunk) : ucg_pool_chunks(4*s.h*s.w);
  p.na = (unsigned)((size_t)s.B*s.Ca*p.cha);
  return p;
}
static size_t ucg_partial_floats(const UpCatGate& s, bool bwd) {
  const UcgPartial p = ucg_partial(s, bwd);
  return (((size_t)s.B*s.Ca*p.cha + (size_t)s.B*s.Cs*p.chs) + 3) & ~(size_t)3;
}
static size_t ucg_vec_floats(const UpCatGate& s) { return (((size_t)s.B*(2*(s.Ca + s.Cs) + s.R)) + 3) & ~(size_t)3; }   // dz2 (B,C), dmean (B,C), dz1 (B,R)

bool up_cat_gate_sizes_ok(const UpCatGate& s) {
  if (s.B < 1 || s.Ca < 1 || s.Cs < 1 || s.h < 1 || s.w < 1 || s.R < 1 || (s.act != 0 && s.act != 1)) return false;
  const long long C = (long long)s.Ca + s.Cs, HW = ((long long)2*s.h + 2)*((long long)2*s.w + 2);
  return HW < (1ll << 30) && (long long)s.B*C*((HW + kDecChunk - 1)/kDecChunk) < (1ll << 31) && C*s.R < (1ll << 31) && (long long)s.B*(2*C + s.R) < (1ll << 31);
}
size_t up_cat_gate_workspace_floats(const UpCatGate& s) {
  const size_t fwd = 2*(ucg_partial_floats(s, false) + (size_t)s.B*(s.Ca + s.Cs + s.R));      // doubles: the per-block sums, the means, the hidden layer
  const size_t bwd = ucg_partial_floats(s, true) + ucg_vec_floats(s) + decoder_bias_partials(s.B, s.Ca, s.h, s.w);
  return fwd > bwd ? fwd : bwd;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// partial[block] = the sum of src over chunk k of a plane: blocks [0, na) take act(a + bias) on an h x w plane, the others skip on a 2h x 2w plane
__global__ __launch_bounds__(kDecBlock) void k_ucg_pool(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ skip, int Ca,
                                                        int hw, int act, UcgPartial pp, double* __restrict__ partial) {
  __shared__ double red[kDecBlock/64];
  const bool from_a = blockIdx.x < pp.na;
  const unsigned id = from_a ? blockIdx.x : blockIdx.x - pp.na;
  const int ch = from_a ? pp.cha : pp.chs, n = from_a ? hw : 4*hw;
  const unsigned plane = id/ch, k = id - plane*ch;
  int len = ceil_div(n, ch);
  len = (len + 3) & ~3;
  const long long l = (long long)k*len;
  const int lo = l < n ? (int)l : n, hi = l + len < n ? (int)(l + len) : n;
  const float* p = (from_a ? a : skip) + (size_t)plane*n;
  const double bc = (from_a && bias) ? (double)bias[plane % Ca] : 0.0;
  const bool relu = from_a && act;
  auto term = [&](float v) { const double t = (double)v + bc; return relu ? fmax(t, 0.0) : t; };
  double s = 0.0;
  if ((n & 3) == 0) {        // (a skip plane always: 4 h w)
    for (int i = lo + (int)threadIdx.x*4; i < hi; i += kDecBlock*4) {
      const f4 v = *(const f4*)(p + i);
      s += (term(v[0]) + term(v[1])) + (term(v[2]) + term(v[3]));
    }
  } else {
    for (int i = lo + (int)threadIdx.x; i < hi; i += kDecBlock) s += term(p[i]);
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < kDecBlock/64; ++k) t += red[k]; partial[blockIdx.x] = t; }
}

// the sum of src (backward: of G o src) over plane (b, c): its per-block sums in order, fp64
template <typename T> __device__ __forceinline__ double ucg_plane_sum(const T* __restrict__ partial, UcgPartial pp, int b, int c, int Ca, int Cs) {
  const bool from_a = c < Ca;
  const T* p = from_a ? partial + ((size_t)b*Ca + c)*pp.cha : partial + pp.na + ((size_t)b*Cs + (c - Ca))*pp.chs;
  const int n = from_a ? pp.cha : pp.chs;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += (double)p[k];
  return s;
}

// store(r, sum_c M[r][c] v[c]) for the rows of a row-major rows x cols matrix: one wave per row
template <class F> __device__ __forceinline__ void ucg_matvec_rows(const float* __restrict__ M, const double* v, int rows, int cols, F store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < rows; r += kUcgGateWaves) {
    double s = 0.0;
    for (int c = lane; c < cols; c += 64) s += (double)M[(size_t)r*cols + c]*v[c];
    s = wave_sum_f64(s);
    if (lane == 0) store(r, s);
  }
}
// store(c, sum_r M[r][c] v[r]): the product with the transpose.  Lanes own columns (coalesced rows), the waves split the rows, `red` (waves x 64) sums them.
template <class F> __device__ __forceinline__ void ucg_matvec_cols(const float* __restrict__ M, const float* v, int rows, int cols, double* red, F store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = 0; c0 < cols; c0 += 64) {
    const int c = c0 + lane;
    double s = 0.0;
    if (c < cols) for (int r = wave; r < rows; r += kUcgGateWaves) s += (double)M[(size_t)r*cols + c]*(double)v[r];
    __syncthreads();
    red[wave*64 + lane] = s;
    __syncthreads();
    if (wave == 0 && c < cols) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < kUcgGateWaves; ++w) t += red[w*64 + lane];
      store(c, t);
    }
  }
}

// One block per sample: mean (B,C) from the per-block sums, hid (B,R) = relu(W1 mean), gate (B,C) = sigmoid(W2 hid).  The chain runs in fp64 (mean64, hid64:
// the workspace); what the backward reads is stored in fp32.
__global__ __launch_bounds__(kUcgGateBlock) void k_ucg_gate_fwd(const double* __restrict__ partial, UcgPartial pp, const float* __restrict__ w1,
                                                               const float* __restrict__ w2, float* __restrict__ gate, float* __restrict__ mean,
                                                               float* __restrict__ hid, double* mean64, double* hid64, int Ca, int Cs, int R, int hw) {
  const int b = blockIdx.x, C = Ca + Cs;
  double* mb = mean64 + (size_t)b*C;
  double* hb = hid64 + (size_t)b*R;
  for (int c = threadIdx.x; c < C; c += kUcgGateBlock) {
    const double m = ucg_plane_sum(partial, pp, b, c, Ca, Cs)/(double)(c < Ca ? hw : 4*hw);
    mb[c] = m; mean[(size_t)b*C + c] = (float)m;
  }
  __threadfence_block(); __syncthreads();
  ucg_matvec_rows(w1, mb, R, C, [&](int r, double s) { const double t = fmax(s, 0.0); hb[r] = t; hid[(size_t)b*R + r] = (float)t; });
  __threadfence_block(); __syncthreads();
  ucg_matvec_rows(w2, hb, C, R, [&](int c, double s) { gate[(size_t)b*C + c] = (float)(1.0/(1.0 + exp(-s))); });
}

__global__ __launch_bounds__(kDecBlock) void k_ucg_apply_fwd(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ skip,
                                                             const float* __restrict__ gate, float* __restrict__ out, int Ca, int Cs, int h, int w, int act,
                                                             unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*(Ca+Cs) + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, H = H2 + 2, W = W2 + 2;
  const unsigned b = plane/C, c = plane - b*C;
  const bool from_a = (int)c < Ca;
  const float bc = (from_a && bias) ? bias[c] : 0.f, gt = gate[plane];
  const int av = act ? kActRelu : kActNone;
  const float* src = from_a ? a + ((size_t)b*Ca + c)*h*w : skip + ((size_t)b*Cs + (c - Ca))*H2*W2;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H*W) break;
    const int py = idx/W, px = idx - py*W;
    const int r = unpad_reflect(py, H2), q = unpad_reflect(px, W2);
    out[(size_t)plane*H*W + idx] = gt*(from_a ? glue_act(src[(r >> 1)*w + (q >> 1)] + bc, av) : src[r*W2 + q]);
  }
}

// G(r, q): the reflection-pad adjoint at the un-padded position (r, q) of an nr x nq plane whose padded gradient g has rows of W = nq + 2 floats
__device__ __forceinline__ float pad_adj_at(const float* __restrict__ g, int r, int q, int nr, int nq, int W) {
  if (!(r == 1 || r == nr - 2 || q == 1 || q == nq - 2)) return g[(r + 1)*W + q + 1];
  SMD_PAD_ADJ_POS(r, nr, y0, y1, y2); SMD_PAD_ADJ_POS(q, nq, x0, x1, x2);       // rare: mirrored border cells
  const int ys[3] = {y0, y1, y2}, xs[3] = {x0, x1, x2};
  float acc = 0.f;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (ys[m] < 0) continue;
#pragma unroll
    for (int n = 0; n < 3; ++n) if (xs[n] >= 0) acc += g[ys[m]*W + xs[n]];
  }
  return acc;
}
// the sum of G over the 2 x 2 children of the low-resolution pixel (i, j) of an h x w plane
__device__ __forceinline__ float up_pad_adj_at(const float* __restrict__ g, int i, int j, int h, int w, int W) {
  if (i > 0 && i < h - 1 && j > 0 && j < w - 1) {   // interior: the plain 2x2 block
    const float* gp = g + (2*i + 1)*W + 2*j + 1;
    return (gp[0] + gp[1]) + (gp[W] + gp[W + 1]);
  }
  return (pad_adj_at(g, 2*i, 2*j, 2*h, 2*w, W) + pad_adj_at(g, 2*i, 2*j + 1, 2*h, 2*w, W)) +
         (pad_adj_at(g, 2*i + 1, 2*j, 2*h, 2*w, W) + pad_adj_at(g, 2*i + 1, 2*j + 1, 2*h, 2*w, W));
}

// partial[block] = the sum of G o src over a chunk of a plane (the a planes at low resolution: their 2 x 2 children share one src value)
__global__ __launch_bounds__(kDecBlock) void k_ucg_reduce_bwd(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ skip,
                                                              const float* __restrict__ g_out, int Ca, int Cs, int h, int w, int act, UcgPartial pp,
                                                              float* __restrict__ partial) {
  __shared__ float red[kDecBlock/64];
  const bool from_a = blockIdx.x < pp.na;
  const unsigned id = from_a ? blockIdx.x : blockIdx.x - pp.na;
  const int ch = from_a ? pp.cha : pp.chs, Ch = from_a ? Ca : Cs;
  const unsigned plane = id/ch, chunk = id - plane*ch;
  const unsigned b = plane/Ch, c = plane - b*Ch;
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, W = W2 + 2, n = from_a ? h*w : H2*W2;
  const float* g = g_out + ((size_t)b*C + (from_a ? c : Ca + c))*(H2 + 2)*W;
  const float* src = (from_a ? a : skip) + (size_t)plane*n;
  const float bc = (from_a && bias) ? bias[c] : 0.f;
  const int av = act ? kActRelu : kActNone;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= n) break;
    if (from_a) { const int i = idx/w, j = idx - i*w; s = fmaf(up_pad_adj_at(g, i, j, h, w, W), glue_act(src[idx] + bc, av), s); }
    else { const int r = idx/W2, q = idx - r*W2; s = fmaf(pad_adj_at(g, r, q, H2, W2, W), src[idx], s); }
  }
  block_store_sum(s, red, partial + blockIdx.x);
}

// One block per sample: dgate = sum G o src (from the per-block sums) -> dz2 = dgate gate (1 - gate) -> dhid = W2^T dz2 -> dz1 = dhid [hid > 0] ->
// dmean = W1^T dz1, stored divided by the elements of the plane it was the mean of.  vec = dz2 (B,C), dmean (B,C), dz1 (B,R).
__global__ __launch_bounds__(kUcgGateBlock) void k_ucg_gate_bwd(const float* __restrict__ partial, UcgPartial pp, const float* __restrict__ w1,
                                                               const float* __restrict__ w2, const float* __restrict__ gate, const float* __restrict__ hid,
                                                               float* vec, int B, int Ca, int Cs, int R, int hw) {
  __shared__ double red[kUcgGateWaves*64];
  const int b = blockIdx.x, C = Ca + Cs;
  const float* gb = gate + (size_t)b*C;
  const float* hb = hid + (size_t)b*R;
  float* dz2 = vec + (size_t)b*C;
  float* dmean = vec + ((size_t)B + b)*C;
  float* dz1 = vec + (size_t)2*B*C + (size_t)b*R;
  for (int c = threadIdx.x; c < C; c += kUcgGateBlock) {
    const double gv = (double)gb[c];
    dz2[c] = (float)(ucg_plane_sum(partial, pp, b, c, Ca, Cs)*gv*(1.0 - gv));
  }
  __threadfence_block(); __syncthreads();
  ucg_matvec_cols(w2, dz2, C, R, red, [&](int r, double s) { dz1[r] = hb[r] > 0.f ? (float)s : 0.f; });
  __threadfence_block(); __syncthreads();
  ucg_matvec_cols(w1, dz1, R, C, red, [&](int c, double s) { dmean[c] = (float)(s/(double)(c < Ca ? hw : 4*hw)); });
}

// g_w1[r][c] = sum_b dz1[b][r] mean[b][c],  g_w2[c][r] = sum_b dz2[b][c] hid[b][r]: the samples in order.
__global__ __launch_bounds__(256) void k_ucg_param_grad(const float* __restrict__ mean, const float* __restrict__ hid, const float* __restrict__ vec,
                                                        float* __restrict__ g_w1, float* __restrict__ g_w2, int B, int C, int R) {
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if (idx >= (size_t)C*R) return;
  const float* dz2 = vec;
  const float* dz1 = vec + (size_t)2*B*C;
  const int r1 = (int)(idx/C), c1 = (int)(idx - (size_t)r1*C), c2 = (int)(idx/R), r2 = (int)(idx - (size_t)c2*R);
  float t1 = 0.f, t2 = 0.f;
  for (int b = 0; b < B; ++b) {
    t1 = fmaf(dz1[(size_t)b*R + r1], mean[(size_t)b*C + c1], t1);
    t2 = fmaf(dz2[(size_t)b*C + c2], hid[(size_t)b*R + r2], t2);
  }
  g_w1[idx] = t1; g_w2[idx] = t2;
}

// g_a = act'(a + bias) (gate sum-of-children G + dmean) at low resolution; its per-block sums are the bias gradient's.  g_a may be NULL (g_bias alone).
__global__ __launch_bounds__(kDecBlock) void k_ucg_apply_bwd_a(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ g_out,
                                                               const float* __restrict__ gate, const float* __restrict__ dmean, float* __restrict__ g_a,
                                                               float* __restrict__ bias_partial, int Ca, int Cs, int h, int w, int act, unsigned chunks) {
  __shared__ float red[kDecBlock/64];
  float bsum = 0.f;
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Ca + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, W = W2 + 2;
  const unsigned b = plane/Ca, c = plane - b*Ca;
  const float* g = g_out + ((size_t)b*C + c)*(H2 + 2)*W;
  const float bc = bias ? bias[c] : 0.f, gt = gate[(size_t)b*C + c], dm = dmean[(size_t)b*C + c];
  const int av = act ? kActRelu : kActNone;
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= h*w) break;
    const int i = idx/w, j = idx - i*w;
    float gv = fmaf(gt, up_pad_adj_at(g, i, j, h, w, W), dm);
    if (av) gv *= glue_act_grad(a[(size_t)plane*h*w + idx] + bc, av);
    if (g_a) g_a[(size_t)plane*h*w + idx] = gv;
    bsum += gv;
  }
  if (bias_partial) block_store_sum(bsum, red, bias_partial + blockIdx.x);
}

// g_skip = gate G + dmean at full resolution
__global__ __launch_bounds__(kDecBlock) void k_ucg_apply_bwd_skip(const float* __restrict__ g_out, const float* __restrict__ gate, const float* __restrict__ dmean,
                                                                  float* __restrict__ g_skip, int Ca, int Cs, int h, int w, unsigned chunks) {
  const unsigned plane = blockIdx.x/chunks, chunk = blockIdx.x - plane*chunks;   // plane = b*Cs + c
  const int C = Ca + Cs, H2 = 2*h, W2 = 2*w, W = W2 + 2;
  const unsigned b = plane/Cs, c = plane - b*Cs;
  const float* g = g_out + ((size_t)b*C + Ca + c)*(H2 + 2)*W;
  const float gt = gate[(size_t)b*C + Ca + c], dm = dmean[(size_t)b*C + Ca + c];
#pragma unroll
  for (int k = 0; k < kDecPerThread; ++k) {
    const int idx = chunk*kDecChunk + k*kDecBlock + threadIdx.x;
    if (idx >= H2*W2) break;
    const int r = idx/W2, q = idx - r*W2;
    g_skip[(size_t)plane*H2*W2 + idx] = fmaf(gt, pad_adj_at(g, r, q, H2, W2, W), dm);
  }
}

hipError_t launch_up_cat_gate_pad_fwd(const UpCatGate& s, const float* a, const float* bias, const float* skip, const float* w1, const float* w2, float* out,
                                      float* gate, float* mean, float* hid, float* ws, hipStream_t st) {
  const UcgPartial pp = ucg_partial(s, false);
  const int C = s.Ca + s.Cs, hw = s.h*s.w;
  const unsigned blocks = pp.na + (unsigned)((size_t)s.B*s.Cs*pp.chs);
  double* partial = (double*)ws;
  double* mean64 = partial + ucg_partial_floats(s, false);
  double* hid64 = mean64 + (size_t)s.B*C;
  hipLaunchKernelGGL(k_ucg_pool, dim3(blocks), dim3(kDecBlock), 0, st, a, bias, skip, s.Ca, hw, s.act, pp, partial);
  hipLaunchKernelGGL(k_ucg_gate_fwd, dim3(s.B), dim3(kUcgGateBlock), 0, st, partial, pp, w1, w2, gate, mean, hid, mean64, hid64, s.Ca, s.Cs, s.R, hw);
  const unsigned chunks = ceil_div((2*s.h + 2)*(2*s.w + 2), kDecChunk);
  hipLaunchKernelGGL(k_ucg_apply_fwd, dim3((unsigned)((size_t)s.B*C*chunks)), dim3(kDecBlock), 0, st, a, bias, skip, gate, out, s.Ca, s.Cs, s.h, s.w, s.act, chunks);
  return hipGetLastError();
}

hipError_t launch_up_cat_gate_pad_bwd(const UpCatGate& s, const float* a, const float* bias, const float* skip, const float* w1, const float* w2,
                                      const float* gate, const float* mean, const float* hid, const float* g_out, float* g_a, float* g_skip, float* g_bias,
                                      float* g_w1, float* g_w2, float* ws, hipStream_t st) {
  const UcgPartial pp = ucg_partial(s, true);
  const int C = s.Ca + s.Cs, hw = s.h*s.w;
  float* partial = ws;
  float* vec = partial + ucg_partial_floats(s, true);
  float* bias_partial = vec + ucg_vec_floats(s);
  const float* dmean = vec + (size_t)s.B*C;
  const unsigned blocks = pp.na + (unsigned)((size_t)s.B*s.Cs*pp.chs);
  hipLaunchKernelGGL(k_ucg_reduce_bwd, dim3(blocks), dim3(kDecBlock), 0, st, a, bias, skip, g_out, s.Ca, s.Cs, s.h, s.w, s.act, pp, partial);
  hipLaunchKernelGGL(k_ucg_gate_bwd, dim3(s.B), dim3(kUcgGateBlock), 0, st, partial, pp, w1, w2, gate, hid, vec, s.B, s.Ca, s.Cs, s.R, hw);
  if (g_w1) hipLaunchKernelGGL(k_ucg_param_grad, dim3((unsigned)(((size_t)C*s.R + 255)/256)), dim3(256), 0, st, mean, hid, vec, g_w1, g_w2, s.B, C, s.R);
  if (g_a || g_bias) {
    hipLaunchKernelGGL(k_ucg_apply_bwd_a, dim3(pp.na), dim3(kDecBlock), 0, st, a, bias, g_out, gate, dmean, g_a, g_bias ? bias_partial : nullptr, s.Ca, s.Cs,
                       s.h, s.w, s.act, (unsigned)pp.cha);
    if (g_bias) hipLaunchKernelGGL(k_bias_finalize, dim3(s.Ca), dim3(64), 0, st, bias_partial, s.B, s.Ca, (unsigned)pp.cha, g_bias);
  }
  if (g_skip) hipLaunchKernelGGL(k_ucg_apply_bwd_skip, dim3((unsigned)((size_t)s.B*s.Cs*pp.chs)), dim3(kDecBlock), 0, st, g_out, gate, dmean, g_skip, s.Ca, s.Cs,
                                 s.h, s.w, (unsigned)pp.chs);
  return hipGetLastError();
}

}  // namespace smd
