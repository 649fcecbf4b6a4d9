// smd_decoder.hip — glue between the 3x3 convolutions of the decoders.
//
// The reference decoder (src/networks/decoders/monodepth.py:71-89, decoders/utils.py:44-54) runs, per stage,
//   reflect-pad -> conv3x3 -> ELU -> nearest x2 -> cat(skip) -> reflect-pad -> conv3x3 -> ELU -> [reflect-pad -> conv3x3 -> sigmoid]
// as separate ATen kernels, each a full read + write of the activation.  The convolutions run on this library's split-bf16 MFMA kernels
// (smd_conv_mfma.hip, smd_conv_thin.hip, the heads; MIOpen only where the routing table serves no kernel); everything between them collapses into
// gather kernels that write the NEXT convolution's already-padded input:
//   k_elu_pad         out = reflect_pad1(act(x + bias))                              (B,C,h,w)           -> (B,C,h+2,w+2)
//   k_elu_up_cat_pad  out = reflect_pad1(cat(nearest_x2(elu(a + bias)), skip))       (B,Ca,h,w),(B,Cs,2h,2w) -> (B,Ca+Cs,2h+2,2w+2)
//   k_ucg_*           the same times DiffNet's channel gate (second half of this file)
// and their adjoint gathers (deterministic, no atomics).  The convolution's bias is added here (the convolution itself runs bias-free), so a separate
// bias pass and a bias-gradient reduction over the full tensor both disappear: the adjoint gathers already hold the pre-activation gradient and emit
// its per-block channel sums.  The activation is recomputed from the saved pre-activation in the backward (elu'(x) = x > 0 ? 1 : exp(x)), so no
// activated tensor is kept.  The stages themselves (source map, pad adjoint, reductions, the gate's matrix-vector products) are in smd_glue_dev.h;
// this file holds the kernels assembled from them, the backward of the two-layer gate (shared with the squeeze-excite gate of smd_attention.hip) and
// the launchers.
#include "smd_glue_dev.h"

namespace smd {

// g_bias[c] = sum over samples and chunks of the per-block partial sums of the pre-activation gradient (fp64, fixed order).
__global__ __launch_bounds__(64) void k_bias_finalize(const float* __restrict__ partial, int B, int C, unsigned chunks, float* __restrict__ g_bias) {
  const int c = blockIdx.x;
  double acc = 0.0;
  const unsigned per = chunks, n = (unsigned)B*per;
  for (unsigned i = threadIdx.x; i < n; i += 64) { const unsigned b = i/per, k = i - b*per; acc += (double)partial[((size_t)b*C + c)*per + k]; }
  acc = wave_sum_f64(acc);
  if (threadIdx.x == 0) g_bias[c] = (float)acc;
}

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
    const float acc = pad_adj_at(g, i, j, h, w, W);
    const float gv = act ? acc*glue_act_grad(ld_as_float<TA>(x, (size_t)plane*h*w + idx) + bc, act) : acc;
    st_from_float<TA>(g_x, (size_t)plane*h*w + idx, gv); bsum += gv;
  }
  if (bias_partial) block_store_sum<Waves::Sequential, kDecBlock/64>(bsum, red, bias_partial + blockIdx.x);
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
    const float gv = up_pad_adj_at<true>(g, i, j, h, w, W)*elu1_grad(ld_as_float<TA>(a, (size_t)plane*h*w + idx) + bc);   // <true>: this kernel's border order
    st_from_float<TA>(g_a, (size_t)plane*h*w + idx, gv); bsum += gv;
  }
  if (bias_partial) block_store_sum<Waves::Sequential, kDecBlock/64>(bsum, red, bias_partial + blockIdx.x);
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
    st_from_float<TS>(g_skip, (size_t)plane*H2*W2 + idx, pad_adj_at(g, r, q, H2, W2, W));
  }
}

// dtypes: bit 0 = x / a (and their gradients) are bf16, bit 1 = skip (and its gradient), bit 2 = out (and its gradient).
#define SMD_DT_A 1
#define SMD_DT_S 2
#define SMD_DT_O 4
template <typename T> struct ElemTag { typedef T type; };
// f(a, s, o): ElemTags of the element types the three dtype bits select.  A kernel launched from f is instantiated for the types f names only.
template <class F> static void for_dtypes(int dt, F f) {
  auto pick = [](bool is_bf16, auto g) { if (is_bf16) g(ElemTag<bf16>{}); else g(ElemTag<float>{}); };
  pick(dt & SMD_DT_A, [&](auto a) { pick(dt & SMD_DT_S, [&](auto s) { pick(dt & SMD_DT_O, [&](auto o) { f(a, s, o); }); }); });
}
#define SMD_ELEM(tag) typename decltype(tag)::type

static hipError_t launch_act_pad_fwd(const void* x, const float* bias, void* out, int B, int C, int h, int w, int act, int dt, hipStream_t st) {
  const unsigned chunks = ceil_div((h + 2)*(w + 2), kDecChunk);
  const dim3 grid((unsigned)((size_t)B*C*chunks)), blk(kDecBlock);
  for_dtypes(dt, [&](auto ta, auto, auto to) {
    typedef SMD_ELEM(ta) TA; typedef SMD_ELEM(to) TO;
    hipLaunchKernelGGL((k_elu_pad_fwd<TA, TO>), grid, blk, 0, st, (const TA*)x, bias, (TO*)out, C, h, w, act, chunks);
  });
  return hipGetLastError();
}
size_t decoder_bias_partials(int B, int C, int h, int w) { return (size_t)B*C*ceil_div(h*w, kDecChunk); }
static hipError_t launch_act_pad_bwd(const void* x, const float* bias, const void* g_out, void* g_x, float* g_bias, float* ws, int B, int C, int h, int w,
                                     int act, int dt, hipStream_t st) {
  const unsigned chunks = ceil_div(h*w, kDecChunk);
  const dim3 grid((unsigned)((size_t)B*C*chunks)), blk(kDecBlock);
  for_dtypes(dt, [&](auto ta, auto, auto to) {
    typedef SMD_ELEM(ta) TA; typedef SMD_ELEM(to) TO;
    hipLaunchKernelGGL((k_elu_pad_bwd<TA, TO>), grid, blk, 0, st, (const TA*)x, bias, (const TO*)g_out, (TA*)g_x, g_bias ? ws : nullptr, C, h, w, act, chunks);
  });
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
  for_dtypes(dt, [&](auto ta, auto ts, auto to) {
    typedef SMD_ELEM(ta) TA; typedef SMD_ELEM(ts) TS; typedef SMD_ELEM(to) TO;
    hipLaunchKernelGGL((k_elu_up_cat_pad_fwd<TA, TS, TO>), grid, blk, 0, st, (const TA*)a, bias, (const TS*)skip, (TO*)out, Ca, Cs, h, w, chunks);
  });
  return hipGetLastError();
}
hipError_t launch_elu_up_cat_pad_bwd(const void* a, const float* bias, const void* g_out, void* g_a, void* g_skip, float* g_bias, float* ws,
                                     int B, int Ca, int Cs, int h, int w, int dt, hipStream_t st) {
  if (g_a) {
    const unsigned chunks = ceil_div(h*w, kDecChunk);
    const dim3 grid((unsigned)((size_t)B*Ca*chunks)), blk(kDecBlock);
    for_dtypes(dt, [&](auto ta, auto, auto to) {
      typedef SMD_ELEM(ta) TA; typedef SMD_ELEM(to) TO;
      hipLaunchKernelGGL((k_elu_up_cat_pad_bwd_a<TA, TO>), grid, blk, 0, st, (const TA*)a, bias, (const TO*)g_out, (TA*)g_a, g_bias ? ws : nullptr, Ca, Cs, h, w, chunks);
    });
    if (g_bias) hipLaunchKernelGGL(k_bias_finalize, dim3(Ca), dim3(64), 0, st, ws, B, Ca, chunks, g_bias);
  }
  if (g_skip && Cs > 0) {
    const unsigned chunks = ceil_div(4*h*w, kDecChunk);
    const dim3 grid((unsigned)((size_t)B*Cs*chunks)), blk(kDecBlock);
    for_dtypes(dt, [&](auto, auto ts, auto to) {
      typedef SMD_ELEM(ts) TS; typedef SMD_ELEM(to) TO;
      hipLaunchKernelGGL((k_elu_up_cat_pad_bwd_skip<TS, TO>), grid, blk, 0, st, (const TO*)g_out, (TS*)g_skip, Ca, Cs, h, w, chunks);
    });
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
//   backward: k_ucg_reduce_bwd (per-block sums of G o src, G the pad adjoint of g_out, folded on the fly) -> k_gate_bwd (one block per sample: back
//             through the sigmoid, W2, the ReLU, W1) -> k_gate_param_grad (the samples in order) -> k_ucg_apply_bwd_a / _skip (gate G + dmean / n).
// Every sum has a fixed order: no float atomics, two runs are bit-equal.
// where the per-block sums of the two halves live and how many each plane has: the a planes first, then the skip planes
static GatePartial ucg_partial(const UpCatGate& s, bool bwd) {
  GatePartial p;
  p.cha = bwd ? ceil_div(s.h*s.w, kDecChunk) : pool_chunks(s.h*s.w);
  p.chs = bwd ? ceil_div(4*s.h*s.w, kDecChunk) : pool_chunks(4*s.h*s.w);
  p.na = (unsigned)((size_t)s.B*s.Ca*p.cha);
  return p;
}
static size_t ucg_partial_floats(const UpCatGate& s, bool bwd) {
  const GatePartial p = ucg_partial(s, bwd);
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

// partial[block] = the sum of src over chunk k of a plane: blocks [0, na) take act(a + bias) on an h x w plane, the others skip on a 2h x 2w plane
__global__ __launch_bounds__(kDecBlock) void k_ucg_pool(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ skip, int Ca,
                                                        int hw, int act, GatePartial pp, double* __restrict__ partial) {
  __shared__ double red[kDecBlock/64];
  const bool from_a = blockIdx.x < pp.na;
  const unsigned id = from_a ? blockIdx.x : blockIdx.x - pp.na;
  const int ch = from_a ? pp.cha : pp.chs, n = from_a ? hw : 4*hw;
  const unsigned plane = id/ch, k = id - plane*ch;
  int lo, hi;
  pool_range(n, ch, k, lo, hi);
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
  block_store_sum<Waves::Sequential, kDecBlock/64>(s, red, partial + blockIdx.x);
}

// One block per sample: mean (B,C) from the per-block sums, hid (B,R) = relu(W1 mean), gate (B,C) = sigmoid(W2 hid).  The chain runs in fp64 (mean64, hid64:
// the workspace); what the backward reads is stored in fp32.
__global__ __launch_bounds__(kGateBlock) void k_ucg_gate_fwd(const double* __restrict__ partial, GatePartial pp, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, float* __restrict__ gate, float* __restrict__ mean,
                                                            float* __restrict__ hid, double* mean64, double* hid64, int Ca, int Cs, int R, int hw) {
  const int b = blockIdx.x, C = Ca + Cs;
  double* mb = mean64 + (size_t)b*C;
  double* hb = hid64 + (size_t)b*R;
  for (int c = threadIdx.x; c < C; c += kGateBlock) {
    const double m = gate_plane_sum(partial, pp, b, c, Ca, Cs)/(double)(c < Ca ? hw : 4*hw);
    mb[c] = m; mean[(size_t)b*C + c] = (float)m;
  }
  __threadfence_block(); __syncthreads();
  matvec_rows(w1, mb, R, C, [&](int r, double s) { const double t = fmax(s, 0.0); hb[r] = t; hid[(size_t)b*R + r] = (float)t; });
  __threadfence_block(); __syncthreads();
  matvec_rows(w2, hb, C, R, [&](int c, double s) { gate[(size_t)b*C + c] = (float)(1.0/(1.0 + exp(-s))); });
}

// (k_elu_up_cat_pad_fwd's source map with one source pointer: its blocks are four elements a thread, and the two-pointer prologue of a shared body cost
// this kernel 18 instructions a block, 0.3 - 0.6 % of the decoder's forward.  tests/test_gpu_diffnet.py pins that the two maps stay one.)
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

// partial[block] = the sum of G o src over a chunk of a plane (the a planes at low resolution: their 2 x 2 children share one src value)
__global__ __launch_bounds__(kDecBlock) void k_ucg_reduce_bwd(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ skip,
                                                              const float* __restrict__ g_out, int Ca, int Cs, int h, int w, int act, GatePartial pp,
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
    if (from_a) { const int i = idx/w, j = idx - i*w; s = fmaf(up_pad_adj_at<false>(g, i, j, h, w, W), glue_act(src[idx] + bc, av), s); }
    else { const int r = idx/W2, q = idx - r*W2; s = fmaf(pad_adj_at(g, r, q, H2, W2, W), src[idx], s); }
  }
  block_store_sum<Waves::Sequential, kDecBlock/64>(s, red, partial + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- the backward of a two-layer gate
// One block per sample: dgate (from the per-block sums) -> dz2 = dgate gate (1 - gate) -> dhid = W2^T dz2 -> dz1 = dhid [hid > 0] -> dmean = W1^T dz1,
// stored divided by the elements of the plane it was the mean of.
__global__ __launch_bounds__(kGateBlock) void k_gate_bwd(GateBwd g) {
  __shared__ double red[kGateWaves*64];
  const int b = blockIdx.x, C = g.Ca + g.Cs, Ca = g.Ca, R = g.R, hw = g.hw;
  const float* gb = g.gate + (size_t)b*C;
  const float* hb = g.hid + (size_t)b*R;
  float* dz2 = g.dz2 + (size_t)b*C;
  float* dz1 = g.dz1 + (size_t)b*R;
  float* dmean = g.dmean + (size_t)b*C;
  for (int c = threadIdx.x; c < C; c += kGateBlock) {
    const double gv = (double)gb[c];
    dz2[c] = (float)(gate_plane_sum(g.partial, g.pp, b, c, Ca, g.Cs)*gv*(1.0 - gv));
  }
  __threadfence_block(); __syncthreads();
  matvec_cols(g.w2, dz2, C, R, red, [&](int r, double s) { dz1[r] = hb[r] > 0.f ? (float)s : 0.f; });
  __threadfence_block(); __syncthreads();
  matvec_cols(g.w1, dz1, R, C, red, [&](int c, double s) { dmean[c] = (float)(s/(double)(c < Ca ? hw : 4*hw)); });
}

// g_w1[r][c] = sum_b dz1[b][r] mean[b][c],  g_w2[c][r] = sum_b dz2[b][c] hid[b][r],  with biases g_b1 = sum_b dz1, g_b2 = sum_b dz2: the samples in order.
__global__ __launch_bounds__(256) void k_gate_param_grad(const float* __restrict__ mean, const float* __restrict__ hid, const float* __restrict__ dz2,
                                                         const float* __restrict__ dz1, float* __restrict__ g_w1, float* __restrict__ g_b1,
                                                         float* __restrict__ g_w2, float* __restrict__ g_b2, int B, int C, int R) {
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if (idx >= (size_t)C*R) return;
  const int r1 = (int)(idx/C), c1 = (int)(idx - (size_t)r1*C), c2 = (int)(idx/R), r2 = (int)(idx - (size_t)c2*R);
  float t1 = 0.f, t2 = 0.f;
  for (int b = 0; b < B; ++b) {
    t1 = fmaf(dz1[(size_t)b*R + r1], mean[(size_t)b*C + c1], t1);
    t2 = fmaf(dz2[(size_t)b*C + c2], hid[(size_t)b*R + r2], t2);
  }
  g_w1[idx] = t1; g_w2[idx] = t2;
  if (!g_b1) return;
  if (idx < (size_t)R) { float u = 0.f; for (int b = 0; b < B; ++b) u += dz1[(size_t)b*R + idx]; g_b1[idx] = u; }
  if (idx < (size_t)C) { float u = 0.f; for (int b = 0; b < B; ++b) u += dz2[(size_t)b*C + idx]; g_b2[idx] = u; }
}

void launch_gate_bwd(const GateBwd& g, float* g_w1, float* g_b1, float* g_w2, float* g_b2, hipStream_t st) {
  const int C = g.Ca + g.Cs;
  hipLaunchKernelGGL(k_gate_bwd, dim3(g.B), dim3(kGateBlock), 0, st, g);
  if (g_w1) hipLaunchKernelGGL(k_gate_param_grad, dim3((unsigned)(((size_t)C*g.R + 255)/256)), dim3(256), 0, st, g.mean, g.hid, g.dz2, g.dz1, g_w1, g_b1, g_w2, g_b2,
                               g.B, C, g.R);
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
    float gv = fmaf(gt, up_pad_adj_at<false>(g, i, j, h, w, W), dm);
    if (av) gv *= glue_act_grad(a[(size_t)plane*h*w + idx] + bc, av);
    if (g_a) g_a[(size_t)plane*h*w + idx] = gv;
    bsum += gv;
  }
  if (bias_partial) block_store_sum<Waves::Sequential, kDecBlock/64>(bsum, red, bias_partial + blockIdx.x);
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
  const GatePartial pp = ucg_partial(s, false);
  const int C = s.Ca + s.Cs, hw = s.h*s.w;
  const unsigned blocks = pp.na + (unsigned)((size_t)s.B*s.Cs*pp.chs);
  double* partial = (double*)ws;
  double* mean64 = partial + ucg_partial_floats(s, false);
  double* hid64 = mean64 + (size_t)s.B*C;
  hipLaunchKernelGGL(k_ucg_pool, dim3(blocks), dim3(kDecBlock), 0, st, a, bias, skip, s.Ca, hw, s.act, pp, partial);
  hipLaunchKernelGGL(k_ucg_gate_fwd, dim3(s.B), dim3(kGateBlock), 0, st, partial, pp, w1, w2, gate, mean, hid, mean64, hid64, s.Ca, s.Cs, s.R, hw);
  const unsigned chunks = ceil_div((2*s.h + 2)*(2*s.w + 2), kDecChunk);
  hipLaunchKernelGGL(k_ucg_apply_fwd, dim3((unsigned)((size_t)s.B*C*chunks)), dim3(kDecBlock), 0, st, a, bias, skip, gate, out, s.Ca, s.Cs, s.h, s.w, s.act, chunks);
  return hipGetLastError();
}

hipError_t launch_up_cat_gate_pad_bwd(const UpCatGate& s, const float* a, const float* bias, const float* skip, const float* w1, const float* w2,
                                      const float* gate, const float* mean, const float* hid, const float* g_out, float* g_a, float* g_skip, float* g_bias,
                                      float* g_w1, float* g_w2, float* ws, hipStream_t st) {
  const GatePartial pp = ucg_partial(s, true);
  const int C = s.Ca + s.Cs;
  float* partial = ws;
  float* vec = partial + ucg_partial_floats(s, true);       // dz2 (B,C), dmean (B,C), dz1 (B,R)
  float* bias_partial = vec + ucg_vec_floats(s);
  float* dmean = vec + (size_t)s.B*C;
  const unsigned blocks = pp.na + (unsigned)((size_t)s.B*s.Cs*pp.chs);
  hipLaunchKernelGGL(k_ucg_reduce_bwd, dim3(blocks), dim3(kDecBlock), 0, st, a, bias, skip, g_out, s.Ca, s.Cs, s.h, s.w, s.act, pp, partial);
  launch_gate_bwd(GateBwd{partial, w1, w2, gate, mean, hid, vec, vec + (size_t)2*s.B*C, dmean, pp, s.B, s.Ca, s.Cs, s.R, s.h*s.w}, g_w1, nullptr, g_w2, nullptr, st);
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
