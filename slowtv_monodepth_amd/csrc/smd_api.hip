// smd_api.hip — the extern "C" boundary (include/smd_hotpath.h): argument validation, workspace carving, launches.
// No torch types, no allocation, no synchronisation; every launch goes to the caller's stream.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "smd_kernels.h"
#include "smd_smooth_dev.h"   // block counts of the smoothness sweep / adjoint (host-side inline helpers)

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(hipError_t e, const char* what) {
  if (e != hipSuccess) return fail(SMD_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return SMD_OK;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct StripPlan { int rh, nsx, nsy; };
constexpr int kBwdAccRows = 16;    // = smd::kAccRows of smd_recon_bwd.hip
constexpr int kBwdMaskRows = 24;   // tallest backward strip: its per-row liveness masks (rows r0-3 .. r1+3) must fit 32 bits
constexpr int kMinStripRows = 4;   // lower bound of the rows-per-strip override; the workspace is sized for it
int max_strips(int h, int w, int cols) { return smd::ceil_div(w, cols)*smd::ceil_div(h, kMinStripRows); }


// Launch-shape knobs (smd_set_knob; unset = the built-in heuristics).  They select between partitions / code paths that must give the same
// results — the parity tests pin them to prove exactly that (tapered vs. plain partition, shared ring vs. per-wave loads, the two row loops
// of the backward) — and are NOT read from the environment: nothing in the library calls getenv.
//   fwd_rh / bwd_rh rows per strip (>= 4); fwd_taper_b / bwd_taper_b samples at the end of the dispatch order that get short strips (0: none)
//   and fwd_taper_rh / bwd_taper_rh their height; fwd_ni supports per forward launch (1..4); fwd_share (default 1: with four scales a block
//   of the hot forward is the four scales of one strip and the target-side rows reach it through an LDS ring); bwd_skip (0 / 2: the
//   backward's row loop, overriding the SMD_BWD_SKIP_DEAD_ROWS flag of the call); bwd_wps (waves per strip of the backward);
//   bwd_guest_finalize; bwd_direct_level; loss_path_guests (0: the fused loss path launches its guest work as kernels of their own);
//   bwd_live (0: the backward ignores the forward's liveness table and runs every wave's row loop); bwd_scales_block (0: with one wave per strip a
//   block stays four strips of one scale instead of the four scales of one strip).
//   conv_two_tiles (1: the decoder's wide convolutions run two tiles of 32 output channels over one staged patch — eight waves per block — where the layer has
//   them; default 0: measured neutral, profiles/r06_conv_mfma_ablations.txt; same bits either way).
//   metrics_store_pred (default 1: smd_depth_metrics writes the resampled prediction to its workspace in the first pass and re-reads it; 0: every pass
//   recomputes the four taps at the valid pixels; same bits either way; 86 vs 104 us at b = 12, 375x1242, 5 % density: profiles/val_metrics_times.txt).
constexpr const char* kKnobs[] = {"fwd_rh", "bwd_rh", "fwd_taper_b", "bwd_taper_b", "fwd_taper_rh", "bwd_taper_rh", "fwd_ni", "fwd_share", "bwd_skip", "bwd_wps",
                                  "bwd_guest_finalize", "bwd_direct_level", "loss_path_guests", "bwd_live", "bwd_scales_block", "conv_two_tiles", "metrics_store_pred"};
constexpr int kNumKnobs = sizeof(kKnobs)/sizeof(kKnobs[0]);
constexpr int kKnobUnset = INT_MIN;
struct KnobTable {
  int v[kNumKnobs];
  KnobTable() { for (int i = 0; i < kNumKnobs; ++i) v[i] = kKnobUnset; }
};
KnobTable g_knobs;
int knob_index(const char* name) {
  for (int i = 0; i < kNumKnobs; ++i) if (strcmp(kKnobs[i], name) == 0) return i;
  return -1;
}
int knob(const char* name, int dflt) {
  const int i = knob_index(name);
  return (i >= 0 && g_knobs.v[i] != kKnobUnset) ? g_knobs.v[i] : dflt;
}

StripPlan plan(int b, int S, int h, int w, int cols) {
  StripPlan p;
  p.rh = smd::pick_rows_per_strip(b, S, h, w, cols, 0);
  const int ov = knob(cols == smd::kFwdCols ? "fwd_rh" : "bwd_rh", 0);
  if (ov >= 1) p.rh = ov < kMinStripRows ? kMinStripRows : ov;
  if (cols == smd::kFwdCols && p.rh > 58) p.rh = 58;   // the K0-fused forward keeps the strip's rh + 4 row-table entries one per lane
  p.nsx = smd::ceil_div(w, cols);
  p.nsy = smd::ceil_div(h, p.rh);
  return p;
}

// Tapered partition of the fused kernels (smd_kernels.h: ReconMainArgs::b1): the last `b2` samples of the dispatch order get
// strips of `rh2` = rh/2 rows.  A launch is two to three "generations" of waves on the 4096 wave slots of the chip and a wave
// lives 30-40 us, so with equal units the last ones dispatched run almost alone for tens of microseconds (wave traces:
// profiles/r04_fwd_wave_traces.txt; time-averaged occupancy 2.96 -> 3.19 waves per SIMD with the taper, forward 93 -> 87-89 us at
// cfg 2).  Default: a sixth of the batch, when the batch has at least four samples; the knobs *_taper_b / *_taper_rh override (b = 0: off).
void taper(int& b1, int& rh2, int& nsy2, int b, int h, const StripPlan& pl, const char* env_b, const char* env_rh) {
  int b2 = knob(env_b, -1), r2 = knob(env_rh, -1);
  if (b2 < 0) {
    b2 = (b >= 4) ? (b + 3)/6 : 0;
    // the taper buys the tail of a launch that is two or three generations of waves; a launch of five or more (384x640 at b = 12) pays for the short
    // strips' halo rows without needing it: half as many samples (backward 268 -> 262 us at cfg 4, 497 -> 485 at cfg 5; r04_fwd_shape_sweep.txt)
    if ((long)b*h*pl.nsx > 36000) b2 = (b2 + 1)/2;
  }
  if (b2 > b - 1) b2 = b - 1;
  if (r2 < kMinStripRows) r2 = pl.rh/2 < kMinStripRows ? kMinStripRows : pl.rh/2;
  b1 = b - b2; rh2 = r2; nsy2 = smd::ceil_div(h, r2);
}

// The forward's partition (shared with the backward, which reads the liveness table the forward indexed by ITS strips).
StripPlan fwd_partition(int b, int S, int h, int w, int& b1, int& rh2, int& nsy2) {
  const StripPlan pl = plan(b, S, h, w, smd::kFwdCols);
  taper(b1, rh2, nsy2, b, h, pl, "fwd_taper_b", "fwd_taper_rh");
  if (rh2 > 58) { rh2 = 58; nsy2 = smd::ceil_div(h, rh2); }   // as plan(): one row-table entry per lane
  return pl;
}

// ---- optional event-pair recording around the dominant kernels (bench.py roofline measurement) ----
struct ProfSlot { hipEvent_t* ev = nullptr; int cap = 0, used = 0; };
ProfSlot g_prof[5];   // SMD_PROF_*: dominant forward kernel, dominant backward kernel, whole forward entry point, whole backward entry point, prep launches

void prof_mark(int which, hipStream_t st, bool begin) {
  ProfSlot& p = g_prof[which];
  if (!p.ev || p.used >= p.cap) return;
  // a failed record only loses one timing sample (collect() reports the pairs that completed)
  if (begin) (void)hipEventRecord(p.ev[2*p.used], st);
  else { (void)hipEventRecord(p.ev[2*p.used + 1], st); ++p.used; }
}


// The K0-fused instantiations of k_recon_main exist for the SSIM loss and walk the low-resolution rows one at a time, which
// needs every pyramid level to be no taller than the image (always true for a decoder's outputs).
bool k0_fusable(const smd::ScaleSet& sc, int h, int flags) {
  if (flags & SMD_LOSS_L1) return false;
  for (int s = 0; s < sc.S; ++s) if (sc.hs[s] > h) return false;
  return true;
}

struct ReconWs { float* loss_partial; float* pose_partial; size_t bytes; };
// What the fused loss path adds to the reconstruction forward: the smoothness sweep (as guest blocks of the main launch, or launched behind
// it) and the in-launch weighted sum of the two losses.
struct LossPathFwd { smd::SmoothFwdJob job; smd::LossCombine comb; bool guests; };

ReconWs carve_recon(void* base, int b, int n, int S, int h, int w) {
  ReconWs r;
  size_t off = 0;
  char* p = (char*)base;
  r.loss_partial = (float*)(p + off); off += align256((size_t)S*b*max_strips(h, w, smd::kFwdCols)*sizeof(float));
  r.pose_partial = (float*)(p + off); off += align256((size_t)n*b*S*max_strips(h, w, smd::kBwdCols)*smd::kPoseSums*sizeof(float));
  r.bytes = off;
  return r;
}

unsigned* packed_live(float* packed, int b, int n, int h, int w) { return (unsigned*)(packed + smd::packed_live_offset_floats(b, n, h, w)); }
uint4* packed_rowtab(float* packed, int b, int n, int h, int w) { return (uint4*)(packed + smd::packed_rowtab_offset_floats(b, n, h, w)); }
unsigned* packed_arrive(float* packed, int b, int n, int h, int w) { return (unsigned*)(packed + smd::packed_arrive_offset_floats(b, n, h, w)); }

int check_dims(int b, int n, int S, int h, int w) {
  if (b < 1 || n < 1 || S < 1 || h < 2 || w < 2) return fail(SMD_E_INVALID, "invalid sizes b=%d n=%d S=%d h=%d w=%d (need h, w >= 2)", b, n, S, h, w);
  if (n > SMD_MAX_SUPPORTS) return fail(SMD_E_INVALID, "n=%d exceeds SMD_MAX_SUPPORTS=%d", n, SMD_MAX_SUPPORTS);
  if (S > 65535 || b > 65535) return fail(SMD_E_INVALID, "b or S exceeds the grid limit");
  if ((size_t)S*b*h*w >= ((size_t)1 << 32)) return fail(SMD_E_INVALID, "S*b*h*w must stay below 2^32");
  return SMD_OK;
}

int fill_scales(smd::ScaleSet& sc, const float* const* p, float* const* g, const int* hs, const int* ws, const int* keys, int S) {
  if (S < 1 || S > SMD_MAX_SCALES) return fail(SMD_E_INVALID, "S=%d outside [1, %d]", S, SMD_MAX_SCALES);
  if (!hs || !ws) return fail(SMD_E_INVALID, "null scale-size arrays");
  memset(&sc, 0, sizeof(sc));
  sc.S = S;
  for (int s = 0; s < S; ++s) {
    if (hs[s] < 1 || ws[s] < 1) return fail(SMD_E_INVALID, "scale %d has empty size %dx%d", s, hs[s], ws[s]);
    sc.p[s] = p ? p[s] : nullptr;
    sc.g[s] = g ? g[s] : nullptr;
    sc.hs[s] = hs[s]; sc.ws[s] = ws[s];
    sc.key[s] = keys ? keys[s] : s;
  }
  return SMD_OK;
}

}  // namespace

namespace smd {
char g_variant[2][128] = {"", ""};   // process-wide on purpose: autograd launches the backward from its own thread, the caller asks from another (a diagnostic label, last writer wins)
void note_variant(int which, const char* fmt, ...) {
  if (which < 0 || which > 1) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_variant[which], sizeof(g_variant[which]), fmt, ap);
  va_end(ap);
}
}  // namespace smd

extern "C" {

const char* smd_last_error(void) { return g_err; }
const char* smd_last_kernel_variant(int which) { return (which == 0 || which == 1) ? smd::g_variant[which] : ""; }
int smd_abi_version(void) { return SMD_ABI_VERSION; }

int smd_set_knob(const char* name, int value) {
  const int i = name ? knob_index(name) : -1;
  if (i < 0) return fail(SMD_E_INVALID, "unknown knob '%s'", name ? name : "(null)");
  g_knobs.v[i] = value;
  return SMD_OK;
}
void smd_reset_knobs(void) { for (int i = 0; i < kNumKnobs; ++i) g_knobs.v[i] = kKnobUnset; }

// ------------------------------------------------------------------------------------------------
int smd_disp_to_depth_fwd(const float* const* disp, const int* hs, const int* ws, int S, int b, int h, int w,
                          float min_depth, float max_depth, float* depth_up, float* disp_up, void* stream) {
  if (!disp || !depth_up) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes");
  if ((min_depth > 0.f || max_depth > 0.f) && !(min_depth > 0.f)) return fail(SMD_E_INVALID, "Min depth must be greater than 0. (%g)", min_depth);
  if (max_depth > 0.f && max_depth < min_depth) return fail(SMD_E_INVALID, "Max depth must be greater than min. (%g vs. %g)", max_depth, min_depth);
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, nullptr, hs, ws, nullptr, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s]) return fail(SMD_E_INVALID, "null disparity pointer for scale %d", s);
  return check_launch(smd::launch_disp_to_depth_fwd(sc, b, h, w, min_depth, max_depth, depth_up, disp_up, (hipStream_t)stream), "disp_to_depth_fwd");
}

size_t smd_disp_to_depth_workspace_bytes(const int* hs, const int* ws, int S, int b, int h, int w) {
  smd::ScaleSet sc;
  if (b < 1 || h < 1 || w < 1 || fill_scales(sc, nullptr, nullptr, hs, ws, nullptr, S)) return 0;
  return align256(smd::disp_to_depth_bwd_tmp_floats(sc, b, h, w, nullptr)*sizeof(float)) + 256;
}

int smd_disp_to_depth_bwd(const int* hs, const int* ws, int S, int b, int h, int w, float min_depth, float max_depth,
                          const float* depth_up, const float* g_depth_up, float* const* g_disp,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!depth_up || !g_depth_up || !g_disp || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, nullptr, g_disp, hs, ws, nullptr, S)) return rc;
  for (int s = 0; s < S; ++s) if (!g_disp[s]) return fail(SMD_E_INVALID, "null gradient pointer for scale %d", s);
  const size_t need = smd_disp_to_depth_workspace_bytes(hs, ws, S, b, h, w);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  return check_launch(smd::launch_disp_to_depth_bwd(sc, b, h, w, min_depth, max_depth, depth_up, g_depth_up, (float*)workspace, false,
                                                    (hipStream_t)stream), "disp_to_depth_bwd");
}

// ------------------------------------------------------------------------------------------------
size_t smd_image_recon_workspace_bytes(int b, int n, int S, int h, int w) {
  if (b < 1 || n < 1 || S < 1 || h < 2 || w < 2) return 0;
  return carve_recon(nullptr, b, n, S, h, w).bytes;
}

size_t smd_packed_supports_bytes(int b, int n, int h, int w) {
  if (b < 1 || n < 1 || h < 2 || w < 2) return 0;
  return smd::packed_total_floats(b, n, h, w)*sizeof(float);
}

// The input-only half of the forward (k_recon_prep): everything that depends on the frames alone.  `sc` != null and K0 fusable:
// also the vertical up-sampling table of the pyramid.  Zeroes the arrival counters in the tail of `packed`.
static int recon_prep_impl(const float* tgt, const float* supp, float* supp_packed, const smd::ScaleSet* sc, int b, int n, int S, int h, int w,
                           int flags, hipStream_t st) {
  int kMaxPerPass = knob("fwd_ni", 4);   // supports held in registers by one launch (1..4)
  if (kMaxPerPass < 1 || kMaxPerPass > 4) kMaxPerPass = 4;
  smd::ReconPrepArgs p;
  memset(&p, 0, sizeof(p));
  p.tgt = tgt; p.supp = supp; p.packed = supp_packed;
  p.b = b; p.n = n; p.h = h; p.w = w; p.flags = flags & (SMD_USE_MIN | SMD_LOSS_L1 | SMD_USE_AUTOMASK);
  const StripPlan ipl = plan(b, 1, h, w, smd::kFwdCols);  // one "scale" only: shorter strips keep the chip full
  p.rh = ipl.rh; p.nsx = ipl.nsx; p.nsy = ipl.nsy;
  const bool fuse_k0 = sc && k0_fusable(*sc, h, flags);
  prof_mark(SMD_PROF_RECON_PREP, st, true);
  for (int i0 = 0; i0 < n; i0 += kMaxPerPass) {
    p.i0 = i0; p.ni = (n - i0 < kMaxPerPass) ? n - i0 : kMaxPerPass;
    p.first_pass = (i0 == 0); p.last_pass = (i0 + p.ni >= n);
    p.rowtab = (fuse_k0 && i0 == 0) ? packed_rowtab(supp_packed, b, n, h, w) : nullptr;
    p.arrive = (i0 == 0) ? packed_arrive(supp_packed, b, n, h, w) : nullptr;
    if (p.rowtab) { p.sc_S = S; for (int s = 0; s < S; ++s) { p.sc_hs[s] = sc->hs[s]; p.sc_ws[s] = sc->ws[s]; } }
    if (int rc = check_launch(smd::launch_recon_prep(p, st), "recon prep")) return rc;
  }
  prof_mark(SMD_PROF_RECON_PREP, st, false);
  return SMD_OK;
}

// Shared body of the two forward entry points.  `sc` != null: K0 fused — the first launch computes the depth from the
// low-resolution disparity pyramid and writes it to `depth_out`; otherwise the depth is read from `depth`.
static int recon_fwd_impl(const float* depth, float* depth_out, const smd::ScaleSet* sc, float min_depth, float max_depth,
                          const float* tgt, const float* supp, const float* T, const float* K,
                          const float* K_inv, const float* noise, uint64_t seed, float* supp_packed, float* err, uint8_t* sel, float* loss,
                          float* warp0, void* workspace, size_t workspace_bytes,
                          int b, int n, int S, int h, int w, int flags, void* stream, const LossPathFwd* lp = nullptr) {
  if (int rc = check_dims(b, n, S, h, w)) return rc;
  if ((!depth && !sc) || !tgt || !supp || !T || !K || !K_inv || !supp_packed || !sel || !loss || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (smd_packed_supports_bytes(b, n, h, w) >= ((size_t)1 << 32)) return fail(SMD_E_INVALID, "the packed buffer (%zu bytes) must stay below 2^32", smd_packed_supports_bytes(b, n, h, w));
  if ((size_t)n*b*3*h*w*4 >= ((size_t)1 << 32)) return fail(SMD_E_INVALID, "n*b*3*h*w*4 must stay below 2^32");
  if ((size_t)(h + 1)*(size_t)(w + 1) >= ((size_t)1 << 24)) return fail(SMD_E_INVALID, "(h+1)*(w+1) must stay below 2^24");
  ReconWs ws = carve_recon(workspace, b, n, S, h, w);
  if (workspace_bytes < ws.bytes) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = (hipStream_t)stream;
  prof_mark(SMD_PROF_RECON_FWD_ALL, st, true);
  int kMaxPerPass = knob("fwd_ni", 4);   // supports held in registers by one launch (1..4)
  if (kMaxPerPass < 1 || kMaxPerPass > 4) kMaxPerPass = 4;
  if (!err && n > kMaxPerPass) return fail(SMD_E_INVALID, "err may be NULL only when all %d supports fit one pass (%d)", n, kMaxPerPass);

  if (!(flags & SMD_PACKED_READY)) {   // once per sample: texel repack, target window sums, identity error (scale independent)
    if (int rc = recon_prep_impl(tgt, supp, supp_packed, sc, b, n, S, h, w, flags, st)) return rc;
  }

  smd::ReconMainArgs a;
  memset(&a, 0, sizeof(a));
  if (sc && !k0_fusable(*sc, h, flags)) {   // see k0_fusable: run the K0 kernel, then the reconstruction on its output
    if (int rc = check_launch(smd::launch_disp_to_depth_fwd(*sc, b, h, w, min_depth, max_depth, depth_out, nullptr, st), "disp_to_depth_fwd")) return rc;
    depth = depth_out; sc = nullptr;
  }
  if (sc) {
    a.sc = *sc; a.depth_out = depth_out; a.rowtab = packed_rowtab(supp_packed, b, n, h, w);
    a.a_scale = 1.f; a.a_off = 0.f;
    if (min_depth > 0.f || max_depth > 0.f) {  // to_scaled: i_max = 1/min, i_min = 1/max (0 if unset)
      const float i_max = 1.f/min_depth, i_min = max_depth > 0.f ? 1.f/max_depth : 0.f;
      a.a_scale = i_max - i_min; a.a_off = i_min;
    }
  }
  a.depth = depth; a.packed = supp_packed; a.T = T; a.K = K; a.Kinv = K_inv;
  a.noise = noise; a.err = err; a.sel = sel; a.partial = ws.loss_partial; a.warp0 = warp0;
  a.arrive = packed_arrive(supp_packed, b, n, h, w); a.loss = loss; a.loss_scale = 1.0/((double)S*b*h*w);
  a.live = packed_live(supp_packed, b, n, h, w);
  a.b = b; a.n = n; a.S = S; a.h = h; a.w = w; a.flags = flags;
  a.wscale = (float)((double)w/(double)(w - 1)); a.hscale = (float)((double)h/(double)(h - 1));
  a.inv_n = (float)(1.0/(double)n);
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  const StripPlan pl = fwd_partition(b, S, h, w, a.b1, a.rh2, a.nsy2);
  a.rh = pl.rh; a.nsx = pl.nsx; a.nsy = pl.nsy;
  if (lp) {
    a.comb = lp->comb;
    if (lp->guests) { a.sm = lp->job; a.guest_blocks = smd::smooth_main_blocks(a.sc, b); }
  }
  a.share = (knob("fwd_share", 1) != 0 && a.S == 4 && a.rh % 4 == 0 && (a.b1 >= a.b || a.rh2 % 4 == 0)) ? 1 : 0;
  for (int i0 = 0; i0 < n; i0 += kMaxPerPass) {
    a.i0 = i0; a.ni = (n - i0 < kMaxPerPass) ? n - i0 : kMaxPerPass;
    a.first_pass = (i0 == 0); a.last_pass = (i0 + a.ni >= n);
    if (i0 == 0) prof_mark(SMD_PROF_RECON_FWD, st, true);
    if (int rc = check_launch(smd::launch_recon_main(a, st), "image_recon_fwd")) return rc;
    if (a.last_pass) prof_mark(SMD_PROF_RECON_FWD, st, false);
    if (a.depth_out) { a.depth = a.depth_out; a.depth_out = nullptr; }   // later passes (n > 4) read the depth the first one wrote
  }
  if (lp && !lp->guests) { if (int rc = check_launch(smd::launch_smooth_main(a.sc, b, lp->job, st), "loss_path smoothness sweep")) return rc; }
  prof_mark(SMD_PROF_RECON_FWD_ALL, st, false);   // the loss is reduced inside the last launch (recon_main_reduce)
  return SMD_OK;
}

int smd_image_recon_supports_per_pass(void) { const int k = knob("fwd_ni", 4); return (k < 1 || k > 4) ? 4 : k; }

int smd_image_recon_prep(const float* tgt, const float* supp, float* supp_packed, const int* hs, const int* ws, int S,
                         int b, int n, int h, int w, int flags, void* stream) {
  if (int rc = check_dims(b, n, S > 0 ? S : 1, h, w)) return rc;
  if (!tgt || !supp || !supp_packed) return fail(SMD_E_INVALID, "null pointer");
  if (smd_packed_supports_bytes(b, n, h, w) >= ((size_t)1 << 32)) return fail(SMD_E_INVALID, "the packed buffer (%zu bytes) must stay below 2^32", smd_packed_supports_bytes(b, n, h, w));
  if ((size_t)n*b*3*h*w*4 >= ((size_t)1 << 32)) return fail(SMD_E_INVALID, "n*b*3*h*w*4 must stay below 2^32");
  smd::ScaleSet sc;
  const bool pyramid = hs && ws && S > 0;
  if (pyramid) { if (int rc = fill_scales(sc, nullptr, nullptr, hs, ws, nullptr, S)) return rc; }
  return recon_prep_impl(tgt, supp, supp_packed, pyramid ? &sc : nullptr, b, n, S, h, w, flags, (hipStream_t)stream);
}

int smd_image_recon_fwd(const float* depth, const float* tgt, const float* supp, const float* T, const float* K,
                        const float* K_inv, const float* noise, uint64_t seed, float* supp_packed, float* err, uint8_t* sel, float* loss,
                        float* warp0, void* workspace, size_t workspace_bytes,
                        int b, int n, int S, int h, int w, int flags, void* stream) {
  return recon_fwd_impl(depth, nullptr, nullptr, 0.f, 0.f, tgt, supp, T, K, K_inv, noise, seed, supp_packed, err, sel, loss, warp0, workspace, workspace_bytes,
                        b, n, S, h, w, flags, stream);
}

int smd_image_recon_disp_fwd(const float* const* disp, const int* hs, const int* ws, int S, float min_depth, float max_depth,
                             const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                             const float* noise, uint64_t seed, float* supp_packed, float* depth_up, float* err, uint8_t* sel, float* loss,
                             float* warp0, void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream) {
  if (!disp || !depth_up) return fail(SMD_E_INVALID, "null pointer");
  if ((min_depth > 0.f || max_depth > 0.f) && !(min_depth > 0.f)) return fail(SMD_E_INVALID, "Min depth must be greater than 0. (%g)", min_depth);
  if (max_depth > 0.f && max_depth < min_depth) return fail(SMD_E_INVALID, "Max depth must be greater than min. (%g vs. %g)", max_depth, min_depth);
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, nullptr, hs, ws, nullptr, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s]) return fail(SMD_E_INVALID, "null disparity pointer for scale %d", s);
  return recon_fwd_impl(nullptr, depth_up, &sc, min_depth, max_depth, tgt, supp, T, K, K_inv, noise, seed, supp_packed, err, sel, loss, warp0,
                        workspace, workspace_bytes, b, n, S, h, w, flags, stream);
}

static int recon_bwd_impl(const float* depth, float* supp_packed, const float* T, const float* K,
                          const float* K_inv, const uint8_t* sel, const float* g_loss, const float* g_in, float k0_scale,
                          float* g_depth, float* g_T, float* g_K, float* g_Kinv, void* workspace, size_t workspace_bytes,
                          int b, int n, int S, int h, int w, int flags, void* stream, smd::PoseFinJob* guest = nullptr,
                          float* g_direct = nullptr, int direct_scale = -1, float g_scale = 1.f) {
  if (int rc = check_dims(b, n, S, h, w)) return rc;
  if (!depth || !supp_packed || !T || !K || !K_inv || !sel || !g_loss || !g_depth || !g_T || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if ((flags & SMD_NEED_K_GRAD) && (!g_K || !g_Kinv)) return fail(SMD_E_INVALID, "SMD_NEED_K_GRAD requires g_K and g_Kinv");
  if (n >= SMD_SEL_MASKED) return fail(SMD_E_INVALID, "too many supports");
  ReconWs ws = carve_recon(workspace, b, n, S, h, w);
  if (workspace_bytes < ws.bytes) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = (hipStream_t)stream;

  smd::ReconBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = depth; a.packed = supp_packed; a.T = T; a.K = K; a.Kinv = K_inv; a.sel = sel; a.g_loss = g_loss;
  a.g_depth = g_depth; a.pose_partial = ws.pose_partial;
  a.g_in = g_in; a.k0_scale = k0_scale; a.g_scale = g_scale;
  a.g_direct = g_direct; a.direct_scale = g_direct ? direct_scale : -1;
  a.arrive = packed_arrive(supp_packed, b, n, h, w) + 1;
  a.live = (n <= smd::kLiveSupports && knob("bwd_live", 1) != 0 && !(flags & SMD_BWD_NO_LIVE)) ? packed_live(supp_packed, b, n, h, w) : nullptr;   // (written by the forward on this buffer)
  { int fnsy2; const StripPlan fp = fwd_partition(b, S, h, w, a.fwd_b1, a.fwd_rh2, fnsy2); a.fwd_rh = fp.rh; }             // (same knobs as the forward call that filled it)
  a.g_T = g_T; a.g_K = (flags & SMD_NEED_K_GRAD) ? g_K : nullptr; a.g_Kinv = (flags & SMD_NEED_K_GRAD) ? g_Kinv : nullptr;
  a.b = b; a.n = n; a.S = S; a.h = h; a.w = w; a.flags = flags;
  a.wscale = (float)((double)w/(double)(w - 1)); a.hscale = (float)((double)h/(double)(h - 1));
  StripPlan pl = plan(b, S, h, w, smd::kBwdCols);
  if (pl.rh > kBwdMaskRows) { pl.rh = kBwdMaskRows; pl.nsy = smd::ceil_div(h, pl.rh); }            // a strip's row masks are 32-bit words (k_recon_bwd: rows r0-3 .. r1+3)
  if (n >= 2 && pl.rh > kBwdAccRows) { pl.rh = kBwdAccRows; pl.nsy = smd::ceil_div(h, pl.rh); }   // the supports' shares of dL/d depth are summed from LDS rows
  a.rh = pl.rh; a.nsx = pl.nsx; a.nsy = pl.nsy;
  taper(a.b1, a.rh2, a.nsy2, b, h, pl, "bwd_taper_b", "bwd_taper_rh");
  if (a.rh2 > kBwdMaskRows) { a.rh2 = kBwdMaskRows; a.nsy2 = smd::ceil_div(h, a.rh2); }
  if (n >= 2 && a.rh2 > kBwdAccRows) { a.rh2 = kBwdAccRows; a.nsy2 = smd::ceil_div(h, a.rh2); }
  a.pose_stride = S*pl.nsx*(a.nsy2 > pl.nsy ? a.nsy2 : pl.nsy);
  a.skip_level = knob("bwd_skip", (flags & SMD_BWD_SKIP_DEAD_ROWS) ? 2 : 0);
  // Waves per strip.  min(n, 4) (default): one support per wave — half as long work units (a launch is only ~2 generations of waves,
  // so its tail is a fraction of a unit) and the waves of a strip share the target-side rows through one L1; 1: a wave takes every
  // support of its strip in turn.  cfg 2, rocprofv3: 113 vs 115 us on coherent masks, 187 vs 212 us on incoherent inputs, 140 vs
  // 145 us in the bench (profiles/r03_ab_kernel_times.txt).
  // Round 5: ONE wave per strip, taking the supports in turn, once the launch has at least three generations of such waves (strips x scales x
  // samples >= 3 x 4096 slots: 384x640 at b = 12, 192x640 at b = 24).  With every support live the two shapes cost the same there (441.7 vs 445.5 us
  // at four supports, 243.2 vs 243.1 at two; 10 % in favour of one wave per support in launches half that size: r05_bwd_wps_sweep.txt); but a wave
  // that takes its supports in turn simply passes over the ones the liveness table calls dead, so its time follows the LIVE supports — whereas a
  // dead support's own wave frees an issue slot, not a place for another block (LDS-resident until the block's slowest wave ends).  cfg 5 on
  // the masks of a training run: 404 -> 362 us; three supports all live: 362 -> 346 (four waves' slots hold 4 strips instead of 1 1/3).
  const long units1 = (long)pl.nsx*pl.nsy*S*b;
  a.wps = knob("bwd_wps", (n >= 2 && units1 >= 3L*4096) ? 1 : (n < 4 ? n : 4));
  if (a.wps < 1) a.wps = 1;
  if (a.wps > 4) a.wps = 4;
  if (a.wps > n) a.wps = n;
  // four scales and two or four strips per block: blocks of the scales of a strip instead (k_recon_bwd) — every block must then have its strip
  const int spb = smd::kWavesPerBlock/a.wps;
  a.scales_block = (n > 1 && S == 4 && smd::kWavesPerBlock == 4 && (spb == 2 || spb == 4) && (pl.nsx*pl.nsy) % spb == 0
                    && (a.b1 >= b || (pl.nsx*a.nsy2) % spb == 0) && knob("bwd_scales_block", 1) != 0) ? 1 : 0;
  if (guest) {   // the caller's next launch finalises the pose sums: no in-launch hand-off (the kernel skips it when `arrive` is null)
    a.arrive = nullptr;
    const int spb = smd::kWavesPerBlock/a.wps;
    guest->a = a; guest->b1 = a.b1;   // (chain / sm of the job are the caller's: left as they are)
    guest->entries1 = S*smd::ceil_div(pl.nsx*pl.nsy, spb); guest->entries2 = S*smd::ceil_div(pl.nsx*a.nsy2, spb);
  }
  prof_mark(SMD_PROF_RECON_BWD_ALL, st, true);
  prof_mark(SMD_PROF_RECON_BWD, st, true);
  if (int rc = check_launch(smd::launch_recon_bwd(a, st), "image_recon_bwd")) return rc;
  prof_mark(SMD_PROF_RECON_BWD, st, false);
  prof_mark(SMD_PROF_RECON_BWD_ALL, st, false);   // g_T / g_K / g_Kinv come out of the same launch (pose_finalize_sample)
  return SMD_OK;
}

int smd_image_recon_bwd(const float* depth, const float* tgt, float* supp_packed, const float* T, const float* K,
                        const float* K_inv, const uint8_t* sel, const float* g_loss,
                        float* g_depth, float* g_T, float* g_K, float* g_Kinv, void* workspace, size_t workspace_bytes,
                        int b, int n, int S, int h, int w, int flags, void* stream) {
  (void)tgt;   // kept in the signature for ABI stability: the target is read from the packed buffer since ABI 3
  return recon_bwd_impl(depth, supp_packed, T, K, K_inv, sel, g_loss, nullptr, 0.f, g_depth, g_T, g_K, g_Kinv, workspace, workspace_bytes,
                        b, n, S, h, w, flags, stream);
}

size_t smd_image_recon_disp_workspace_bytes(const int* hs, const int* ws, int S, int b, int n, int h, int w) {
  const size_t base = smd_image_recon_workspace_bytes(b, n, S, h, w), k0 = smd_disp_to_depth_workspace_bytes(hs, ws, S, b, h, w);
  if (!base || !k0) return 0;
  return align256(base) + align256((size_t)S*b*h*w*sizeof(float)) + k0;
}

int smd_image_recon_disp_bwd(const int* hs, const int* ws, int S, float min_depth, float max_depth, const float* depth_up,
                             float* supp_packed, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                             const float* g_loss, const float* g_depth_up_in, float* const* g_disp, float* g_T, float* g_K, float* g_Kinv,
                             void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream) {
  if (!depth_up || !g_disp || !workspace) return fail(SMD_E_INVALID, "null pointer");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, nullptr, g_disp, hs, ws, nullptr, S)) return rc;
  for (int s = 0; s < S; ++s) if (!g_disp[s]) return fail(SMD_E_INVALID, "null gradient pointer for scale %d", s);
  const size_t need = smd_image_recon_disp_workspace_bytes(hs, ws, S, b, n, h, w);
  if (!need || workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  const size_t base = align256(smd_image_recon_workspace_bytes(b, n, S, h, w));
  float* g_depth = (float*)((char*)workspace + base);
  float* k0_tmp = (float*)((char*)workspace + base + align256((size_t)S*b*h*w*sizeof(float)));
  float a_scale = 1.f;
  if (min_depth > 0.f || max_depth > 0.f) a_scale = 1.f/min_depth - (max_depth > 0.f ? 1.f/max_depth : 0.f);
  // The fused backward applies d depth / d(scaled disparity) itself (it has the depth in a register), so the K0 adjoint is a
  // pure resampling adjoint of g_depth: it neither reads depth_up again (24 MB at cfg 2) nor multiplies.
  smd::PoseFinJob guest;
  memset(&guest, 0, sizeof(guest));
  const bool ride = knob("bwd_guest_finalize", 1) != 0;   // 0: the in-launch hand-off of smd_image_recon_bwd instead
  // A pyramid level that already has the image size (normally level 0) needs no resampling adjoint: the fused backward stores its rows
  // straight into that level's gradient tensor and the K0 adjoint launches no blocks for it (one (b,h,w) read + write less; needs another
  // level to carry the launch the pose epilogue rides in).
  int direct = -1;
  if (S > 1 && knob("bwd_direct_level", 1) != 0)
    for (int s = 0; s < S && direct < 0; ++s) if (hs[s] == h && ws[s] == w) direct = s;
  if (int rc = recon_bwd_impl(depth_up, supp_packed, T, K, K_inv, sel, g_loss, g_depth_up_in, a_scale,
                              g_depth, g_T, g_K, g_Kinv, workspace, base, b, n, S, h, w, flags, stream, ride ? &guest : nullptr,
                              direct >= 0 ? g_disp[direct] : nullptr, direct)) return rc;
  return check_launch(smd::launch_disp_to_depth_bwd(sc, b, h, w, min_depth, max_depth, depth_up, g_depth, k0_tmp, true, (hipStream_t)stream,
                                                    ride ? &guest : nullptr, direct), "disp_to_depth_bwd");
}

// ------------------------------------------------------------------------------------------------
// Fused loss path (round 5): `forward_loss` of the kbr configuration (src/core/trainer.py:383-392, 436-437, 462-464) as ONE operator.
// Forward = the K0-fused reconstruction launch carrying the smoothness sweep as guest blocks and forming the weighted sum in-launch;
// backward = the fused reconstruction backward, the K0 adjoint's first launch carrying the pose epilogue (now through to the pose network's
// outputs) and the smoothness adjoint as guests, and the K0 adjoint's second launch adding into what the smoothness adjoint wrote.
static const char* loss_path_unsupported(const smd::ScaleSet& sc, int n, int h, int w, int flags, int* direct) {
  if (flags & SMD_LOSS_L1) return "loss_name 'l1'";
  if ((flags & SMD_USE_LAPLACIAN) || !(flags & SMD_USE_EDGES)) return "a smoothness term other than SmoothReg(use_edges=True)";
  int per_pass = knob("fwd_ni", 4);
  if (per_pass < 1 || per_pass > 4) per_pass = 4;
  if (n > per_pass) return "more supports than one forward pass holds";
  if (!k0_fusable(sc, h, flags)) return "a pyramid level taller than the image";
  if (sc.S < 2) return "a single pyramid level";
  int ident = 0, d = -1;
  for (int s = 0; s < sc.S; ++s) if (sc.hs[s] == h && sc.ws[s] == w) { ++ident; if (d < 0) d = s; }
  if (ident > 1) return "two pyramid levels of the image's size";
  if (ident == 1 && knob("bwd_direct_level", 1) == 0) return "knob bwd_direct_level = 0";
  if (knob("bwd_guest_finalize", 1) == 0) return "knob bwd_guest_finalize = 0";
  *direct = d;
  return nullptr;
}

size_t smd_loss_path_workspace_bytes(const int* hs, const int* ws, int S, int b, int n, int h, int w) {
  const size_t fwd = align256(smd_image_recon_workspace_bytes(b, n, S, h, w)) + smd_disp_smooth_workspace_bytes(hs, ws, S, b);
  const size_t bwd = smd_image_recon_disp_workspace_bytes(hs, ws, S, b, n, h, w);
  if (!smd_image_recon_workspace_bytes(b, n, S, h, w) || !smd_disp_smooth_workspace_bytes(hs, ws, S, b) || !bwd) return 0;
  return fwd > bwd ? fwd : bwd;
}

int smd_loss_path_fwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, float min_depth, float max_depth,
                      const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv, uint64_t seed,
                      float* supp_packed, float* edge_weights, float* depth_up, uint8_t* sel, float* loss3, float* stats,
                      void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, float w_recon, float w_smooth, void* stream) {
  if (!disp || !depth_up || !edge_weights || !loss3 || !stats || !workspace || !tgt) return fail(SMD_E_INVALID, "null pointer");
  if ((min_depth > 0.f || max_depth > 0.f) && !(min_depth > 0.f)) return fail(SMD_E_INVALID, "Min depth must be greater than 0. (%g)", min_depth);
  if (max_depth > 0.f && max_depth < min_depth) return fail(SMD_E_INVALID, "Max depth must be greater than min. (%g vs. %g)", max_depth, min_depth);
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, nullptr, hs, ws, scale_keys, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s]) return fail(SMD_E_INVALID, "null disparity pointer for scale %d", s);
  int direct = -1;
  if (const char* why = loss_path_unsupported(sc, n, h, w, flags, &direct)) return fail(SMD_E_UNSUPPORTED, "the fused loss path does not serve %s", why);
  const size_t need = smd_loss_path_workspace_bytes(hs, ws, S, b, n, h, w);
  if (!need || workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (!(flags & SMD_EDGES_READY)) {   // frame-only half of the smoothness term inline (also zeroes the sweep's and the combination's counters)
    if (int rc = check_launch(smd::launch_smooth_edges(sc, b, tgt, h, w, edge_weights, st), "disp_smooth_prep")) return rc;
  }
  const size_t base = align256(smd_image_recon_workspace_bytes(b, n, S, h, w));
  LossPathFwd lp;
  smd::smooth_fwd_job(sc, b, loss3 + 2, stats, (float*)((char*)workspace + base), edge_weights, &lp.job);
  lp.comb.out3 = loss3; lp.comb.arrive = lp.job.arrive + (size_t)S*b + 1; lp.comb.w_rec = w_recon; lp.comb.w_sm = w_smooth;
  lp.job.comb = lp.comb;
  lp.guests = knob("loss_path_guests", 1) != 0;
  const int rflags = flags & (SMD_USE_MIN | SMD_USE_AUTOMASK | SMD_PACKED_READY);
  return recon_fwd_impl(nullptr, depth_up, &sc, min_depth, max_depth, tgt, supp, T, K, K_inv, nullptr, seed, supp_packed, nullptr, sel, loss3 + 1, nullptr,
                        workspace, base, b, n, S, h, w, rflags, stream, &lp);
}

int smd_loss_path_bwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, float min_depth, float max_depth,
                      const float* depth_up, float* supp_packed, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                      const float* stats, const float* edge_weights, const float* g_loss, float w_recon, float w_smooth,
                      const float* aa, const float* t, const uint8_t* invert, const float* fs, const float* cs,
                      float* const* g_disp, float* g_T, float* g_K, float* g_Kinv, float* g_aa, float* g_t, float* g_fs, float* g_cs,
                      void* workspace, size_t workspace_bytes, int b, int n, int h, int w, int flags, void* stream) {
  if (!disp || !depth_up || !g_disp || !stats || !edge_weights || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if ((aa != nullptr) != (t != nullptr) || (aa != nullptr) != (g_aa != nullptr) || (aa != nullptr) != (g_t != nullptr)) return fail(SMD_E_INVALID, "aa, t, g_aa, g_t go together");
  if ((fs != nullptr) != (cs != nullptr) || (fs != nullptr) != (g_fs != nullptr) || (fs != nullptr) != (g_cs != nullptr)) return fail(SMD_E_INVALID, "fs, cs, g_fs, g_cs go together");
  if (fs && (!aa || !(flags & SMD_NEED_K_GRAD))) return fail(SMD_E_INVALID, "the intrinsics' chain rule needs the pose chain and SMD_NEED_K_GRAD");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, g_disp, hs, ws, scale_keys, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s] || !g_disp[s]) return fail(SMD_E_INVALID, "null pointer for scale %d", s);
  int direct = -1;
  if (const char* why = loss_path_unsupported(sc, n, h, w, flags, &direct)) return fail(SMD_E_UNSUPPORTED, "the fused loss path does not serve %s", why);
  const size_t need = smd_loss_path_workspace_bytes(hs, ws, S, b, n, h, w);
  if (!need || workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  const size_t base = align256(smd_image_recon_workspace_bytes(b, n, S, h, w));
  float* g_depth = (float*)((char*)workspace + base);
  float* k0_tmp = (float*)((char*)workspace + base + align256((size_t)S*b*h*w*sizeof(float)));
  float a_scale = 1.f;
  if (min_depth > 0.f || max_depth > 0.f) a_scale = 1.f/min_depth - (max_depth > 0.f ? 1.f/max_depth : 0.f);
  const bool guests = knob("loss_path_guests", 1) != 0;
  smd::PoseFinJob job;
  memset(&job, 0, sizeof(job));
  job.chain.aa = aa; job.chain.t = t; job.chain.invert = invert; job.chain.g_aa = g_aa; job.chain.g_t = g_t;
  job.chain.fs = fs; job.chain.cs = cs; job.chain.g_fs = g_fs; job.chain.g_cs = g_cs; job.chain.h = h; job.chain.w = w;
  job.sm.stats = stats; job.sm.edge_w = edge_weights; job.sm.g_loss = g_loss; job.sm.g_scale = w_smooth; job.sm.accumulate_scale = direct;
  job.sm.blocks_per_sample = guests ? smd::smooth_bwd_blocks_per_sample(sc) : 0;
  const int rflags = flags & (SMD_USE_MIN | SMD_USE_AUTOMASK | SMD_NEED_K_GRAD | SMD_BWD_SKIP_DEAD_ROWS | SMD_BWD_NO_LIVE);
  if (int rc = recon_bwd_impl(depth_up, supp_packed, T, K, K_inv, sel, g_loss, nullptr, a_scale, g_depth, g_T, g_K, g_Kinv, workspace, base,
                              b, n, S, h, w, rflags, stream, &job, direct >= 0 ? g_disp[direct] : nullptr, direct, w_recon)) return rc;
  if (!guests) {   // the smoothness adjoint as a launch of its own, between the reconstruction backward (which wrote the direct level) and the K0 adjoint (which adds)
    if (int rc = check_launch(smd::launch_smooth_bwd(sc, b, nullptr, h, w, SMD_USE_EDGES, stats, g_loss, edge_weights, (hipStream_t)stream, w_smooth, direct), "loss_path smoothness adjoint")) return rc;
  }
  return check_launch(smd::launch_disp_to_depth_bwd(sc, b, h, w, min_depth, max_depth, depth_up, g_depth, k0_tmp, true, (hipStream_t)stream, &job, direct, true), "loss_path K0 adjoint");
}

// ------------------------------------------------------------------------------------------------
static int smooth_chunks(const int* hs, const int* ws, int S) {
  int mx = 1;
  for (int s = 0; s < S; ++s) {   // units of the streaming sweep, or blocks of 256 pixels of the second-order (laplacian) sweep
    const int u = smd::smooth_units_of(hs[s], ws[s]), p = smd::ceil_div(hs[s]*ws[s], 256);
    mx = (u > p ? u : p) > mx ? (u > p ? u : p) : mx;
  }
  return mx;
}

size_t smd_disp_smooth_workspace_bytes(const int* hs, const int* ws, int S, int b) {
  if (!hs || !ws || S < 1 || S > SMD_MAX_SCALES || b < 1) return 0;
  return align256((size_t)S*b*smooth_chunks(hs, ws, S)*2*sizeof(float) + (size_t)S*b*sizeof(double));   // per-unit partials + per-pair loss shares
}

size_t smd_disp_smooth_edge_weight_bytes(const int* hs, const int* ws, int S, int b) {
  smd::ScaleSet sc;
  if (b < 1 || fill_scales(sc, nullptr, nullptr, hs, ws, nullptr, S)) return 0;
  return smd::smooth_edge_bytes(sc, b);   // {wx, wy} per pixel of every level + the arrival counters of the sweep's in-launch second stage
}

int smd_gaussian_blur3x3(const float* x, float* out, int planes, int h, int w, int adjoint, void* stream) {
  if (!x || !out) return fail(SMD_E_INVALID, "null pointer");
  if (x == out) return fail(SMD_E_INVALID, "in-place blur is not supported");
  if (planes < 1) return fail(SMD_E_INVALID, "invalid sizes");
  if (h < 2 || w < 2) return fail(SMD_E_INVALID, "reflect padding by one needs at least 2 x 2 pixels (got %d x %d)", h, w);   // F.pad(mode='reflect') raises too
  return check_launch(smd::launch_blur3(x, out, planes, h, w, adjoint != 0, (hipStream_t)stream), "gaussian_blur3x3");
}

int smd_disp_smooth_prep(const float* img, const int* hs, const int* ws, int S, int b, int h, int w, int flags, float* edge_weights, void* stream) {
  if (!img || !edge_weights) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes");
  if (!(flags & SMD_USE_EDGES) || (flags & SMD_USE_LAPLACIAN)) return fail(SMD_E_INVALID, "smd_disp_smooth_prep serves SmoothReg(use_edges=True) without use_laplacian");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, nullptr, nullptr, hs, ws, nullptr, S)) return rc;
  return check_launch(smd::launch_smooth_edges(sc, b, img, h, w, edge_weights, (hipStream_t)stream), "disp_smooth_prep");
}

int smd_disp_smooth_fwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, int b,
                        const float* img, int h, int w, int flags, float* loss, float* stats, float* disp_grad, float* image_grad,
                        float* edge_weights, void* workspace, size_t workspace_bytes, void* stream) {
  if (!disp || !img || !loss || !stats || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, nullptr, hs, ws, scale_keys, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s]) return fail(SMD_E_INVALID, "null disparity pointer for scale %d", s);
  const size_t need = smd_disp_smooth_workspace_bytes(hs, ws, S, b);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  if ((flags & SMD_USE_EDGES) && !edge_weights) return fail(SMD_E_INVALID, "SMD_USE_EDGES needs the edge_weights buffer (smd_disp_smooth_edge_weight_bytes)");
  if ((flags & SMD_EDGES_READY) && (!(flags & SMD_USE_EDGES) || (flags & SMD_USE_LAPLACIAN))) return fail(SMD_E_INVALID, "SMD_EDGES_READY goes with SMD_USE_EDGES (first-order form)");
  return check_launch(smd::launch_smooth_fwd(sc, b, img, h, w, flags, loss, stats, disp_grad, image_grad, (float*)workspace,
                                             edge_weights, (flags & SMD_EDGES_READY) != 0, (hipStream_t)stream), "disp_smooth_fwd");
}

int smd_disp_smooth_bwd(const float* const* disp, const int* hs, const int* ws, const int* scale_keys, int S, int b,
                        const float* img, int h, int w, int flags, const float* stats, const float* edge_weights, const float* g_loss,
                        float* const* g_disp, void* stream) {
  if (!disp || !img || !stats || !g_loss || !g_disp) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes");
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, disp, g_disp, hs, ws, scale_keys, S)) return rc;
  for (int s = 0; s < S; ++s) if (!disp[s] || !g_disp[s]) return fail(SMD_E_INVALID, "null pointer for scale %d", s);
  if ((flags & SMD_USE_LAPLACIAN) && (flags & SMD_USE_EDGES) && !edge_weights) return fail(SMD_E_INVALID, "the second-order adjoint needs the edge weights the forward cached");
  return check_launch(smd::launch_smooth_bwd(sc, b, img, h, w, flags, stats, g_loss, edge_weights, (hipStream_t)stream), "disp_smooth_bwd");
}

// ------------------------------------------------------------------------------------------------
// Un-fused operators
size_t smd_view_synth_workspace_bytes(int B, int h, int w) {
  if (B < 1 || h < 2 || w < 2) return 0;
  return align256((size_t)B*smd::ceil_div(h*w, 256)*smd::kPoseSums*sizeof(float));
}

int smd_view_synth_fwd(const float* input, const float* depth, const float* T, const float* K, const float* K_inv,
                       float* warp, float* depth_warp, uint8_t* mask_valid, int B, int C, int h, int w, void* stream) {
  if (!input || !depth || !T || !K || !K_inv || !warp) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || B > 65535 || C < 1 || h < 2 || w < 2) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  return check_launch(smd::launch_view_synth_fwd(input, depth, T, K, K_inv, warp, depth_warp, mask_valid, B, C, h, w, (hipStream_t)stream), "view_synth_fwd");
}

int smd_view_synth_bwd(const float* input, const float* depth, const float* T, const float* K, const float* K_inv,
                       const float* g_warp, const float* g_depth_warp, float* g_input, float* g_depth, float* g_T, float* g_K, float* g_Kinv,
                       void* workspace, size_t workspace_bytes, int B, int C, int h, int w, void* stream) {
  if (!input || !depth || !T || !K || !K_inv || !g_warp || !g_depth || !g_T || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || B > 65535 || C < 1 || h < 2 || w < 2) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  if (workspace_bytes < smd_view_synth_workspace_bytes(B, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_view_synth_bwd(input, depth, T, K, K_inv, g_warp, g_depth_warp, g_input, g_depth, g_T, g_K, g_Kinv,
                                                 (float*)workspace, B, C, h, w, (hipStream_t)stream), "view_synth_bwd");
}

size_t smd_photo_error_workspace_bytes(int N, int C, int h, int w) {
  if (N < 1 || C < 1 || h < 2 || w < 2) return 0;
  return align256((size_t)N*3*C*h*w*sizeof(float));
}

int smd_photo_error_fwd(const float* pred, const float* target, float* err, int N, int C, int h, int w, int flags, float weight_ssim, void* stream) {
  if (!pred || !target || !err) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || N > 65535 || C < 1 || h < 2 || w < 2) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d h=%d w=%d", N, C, h, w);
  if (!(weight_ssim >= 0.f && weight_ssim <= 1.f)) return fail(SMD_E_INVALID, "Invalid SSIM weight. (%g vs. [0, 1])", weight_ssim);
  return check_launch(smd::launch_photo_error_fwd(pred, target, err, N, C, h, w, flags, weight_ssim, (hipStream_t)stream), "photo_error_fwd");
}

int smd_photo_error_bwd(const float* pred, const float* target, const float* g_err, float* g_pred, void* workspace, size_t workspace_bytes,
                        int N, int C, int h, int w, int flags, float weight_ssim, void* stream) {
  if (!pred || !target || !g_err || !g_pred || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || N > 65535 || C < 1 || h < 2 || w < 2) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d h=%d w=%d", N, C, h, w);
  if (workspace_bytes < smd_photo_error_workspace_bytes(N, C, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  if (!(weight_ssim >= 0.f && weight_ssim <= 1.f)) return fail(SMD_E_INVALID, "Invalid SSIM weight. (%g vs. [0, 1])", weight_ssim);
  return check_launch(smd::launch_photo_error_bwd(pred, target, g_err, g_pred, (float*)workspace, N, C, h, w, flags, weight_ssim, (hipStream_t)stream), "photo_error_bwd");
}

// ------------------------------------------------------------------------------------------------
// RegressionLoss
size_t smd_regression_workspace_bytes(size_t N) {
  if (N < 1) return 0;
  return align256((size_t)smd::regr_blocks(N)*3*sizeof(float));
}

int smd_regression_fwd(const float* pred, const float* target, const uint8_t* mask, size_t N, int flags, float* loss, float* err, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !target || !loss || !stats || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || N > ((size_t)1 << 40)) return fail(SMD_E_INVALID, "invalid size N=%zu", N);
  if (workspace_bytes < smd_regression_workspace_bytes(N)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_regression_fwd(pred, target, mask, N, flags, loss, err, stats, (float*)workspace, (hipStream_t)stream), "regression_fwd");
}

int smd_regression_bwd(const float* pred, const float* target, const uint8_t* mask, size_t N, int flags, float* stats, const float* g_loss,
                       float* g_pred, float* g_target, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !target || !stats || !g_loss || !workspace || (!g_pred && !g_target)) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || N > ((size_t)1 << 40)) return fail(SMD_E_INVALID, "invalid size N=%zu", N);
  if (workspace_bytes < smd_regression_workspace_bytes(N)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_regression_bwd(pred, target, mask, N, flags, stats, g_loss, g_pred, g_target, (float*)workspace, (hipStream_t)stream),
                      "regression_bwd");
}

// workspace of smd_depth_metrics: the radix histograms (zeroed by the call) | the blocks' fp64 partial sums | the resampled prediction
static size_t metrics_partial_bytes(int b, int H, int W) { return align256((size_t)b*smd::metrics_blocks_per_sample(b, H, W)*smd::kMetSums*sizeof(double)); }

size_t smd_depth_metrics_workspace_bytes(int b, int H, int W) {
  if (b < 1 || H < 1 || W < 1 || b > 65535 || (size_t)H*W >= ((size_t)1 << 31)) return 0;
  return align256(smd::metrics_hist_bytes(b)) + metrics_partial_bytes(b, H, W) + align256((size_t)b*H*W*sizeof(float));
}

int smd_depth_metrics(const float* pred, const float* target, int b, int h, int w, int H, int W, float min_depth, float max_depth, float* values,
                      float* medians, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !target || !values || !medians || !counts || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || H < 1 || W < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes b=%d h=%d w=%d H=%d W=%d", b, h, w, H, W);
  if ((size_t)H*W >= ((size_t)1 << 31) || (size_t)h*w >= ((size_t)1 << 31)) return fail(SMD_E_INVALID, "h*w and H*W must stay below 2^31");
  if (!(min_depth > 0.f)) return fail(SMD_E_INVALID, "Min depth must be greater than 0. (%g)", min_depth);
  if (!(max_depth > min_depth) || !(max_depth < INFINITY)) return fail(SMD_E_INVALID, "Max depth must be finite and greater than min. (%g vs. %g)", max_depth, min_depth);
  const size_t need = smd_depth_metrics_workspace_bytes(b, H, W);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  char* ws = (char*)workspace;
  unsigned* hist = (unsigned*)ws; ws += align256(smd::metrics_hist_bytes(b));
  double* partial = (double*)ws; ws += metrics_partial_bytes(b, H, W);
  return check_launch(smd::launch_depth_metrics(pred, target, b, h, w, H, W, min_depth, max_depth, values, medians, counts, hist, partial, (float*)ws,
                                                knob("metrics_store_pred", 1) != 0, (hipStream_t)stream), "depth_metrics");
}

// workspace of smd_eval_metrics: the radix histograms (zeroed by the call) | the blocks' alignment sums | their metric sums | (scale, shift) | the masked prediction
static size_t eval_partial_bytes(int b, int H, int W, int sums) { return align256((size_t)b*smd::eval_blocks_per_item(b, H, W)*sums*sizeof(double)); }

size_t smd_eval_metrics_workspace_bytes(int b, int H, int W) {
  if (b < 1 || H < 1 || W < 1 || b > 65535 || (size_t)H*W >= ((size_t)1 << 31)) return 0;
  return align256(smd::eval_hist_bytes(b)) + eval_partial_bytes(b, H, W, smd::kEvAlignSums) + eval_partial_bytes(b, H, W, smd::kEvSums) +
         align256((size_t)b*2*sizeof(double)) + align256((size_t)b*H*W*sizeof(float));
}

int smd_eval_metrics(const float* disp, const float* target, const uint8_t* mask, int b, int h, int w, int H, int W, int crop_y0, int crop_y1, int crop_x0,
                     int crop_x1, float min_depth, float max_depth, int align_mode, float factor, int flags, double* values, int* counts, int* status,
                     float* medians, float* depth, uint8_t* valid, float* resized, void* workspace, size_t workspace_bytes, void* stream) {
  if (!disp || !target || !values || !counts || !status || !medians || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || H < 1 || W < 1 || b > 65535) return fail(SMD_E_INVALID, "invalid sizes b=%d h=%d w=%d H=%d W=%d", b, h, w, H, W);
  if ((size_t)H*W >= ((size_t)1 << 31) || (size_t)h*w >= ((size_t)1 << 31)) return fail(SMD_E_INVALID, "h*w and H*W must stay below 2^31");
  if (!(min_depth >= 0.f) || !(min_depth < INFINITY)) return fail(SMD_E_INVALID, "min_depth must be finite and not negative (%g): the selection orders bit patterns", min_depth);
  if (!(max_depth >= 0.f) || (max_depth > 0.f && !(max_depth > min_depth))) return fail(SMD_E_INVALID, "max_depth must be 0 (none) or greater than min. (%g vs. %g)", max_depth, min_depth);
  if (align_mode < SMD_EVAL_ALIGN_FACTOR || align_mode > SMD_EVAL_ALIGN_LSQR) return fail(SMD_E_INVALID, "unknown align_mode %d", align_mode);
  if ((flags & ~(SMD_EVAL_EIGEN | SMD_EVAL_BENCHMARK | SMD_EVAL_NEAREST)) || !(flags & (SMD_EVAL_EIGEN | SMD_EVAL_BENCHMARK))) return fail(SMD_E_INVALID, "invalid flags 0x%x (at least one of SMD_EVAL_EIGEN, SMD_EVAL_BENCHMARK)", flags);
  if ((uintptr_t)workspace % 8 || (uintptr_t)values % 8) return fail(SMD_E_INVALID, "the workspace and values need 8-byte alignment");
  const size_t need = smd_eval_metrics_workspace_bytes(b, H, W);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  smd::EvalArgs a;
  memset(&a, 0, sizeof(a));
  a.disp = disp; a.target = target; a.mask = mask; a.b = b; a.h = h; a.w = w; a.H = H; a.W = W;
  a.y0 = crop_y0; a.y1 = crop_y1; a.x0 = crop_x0; a.x1 = crop_x1;
  a.lo = min_depth; a.hi = max_depth; a.has_hi = max_depth > 0.f; a.nearest = (flags & SMD_EVAL_NEAREST) != 0;
  a.mode = align_mode; a.groups = flags & (SMD_EVAL_EIGEN | SMD_EVAL_BENCHMARK); a.factor = factor;
  char* ws = (char*)workspace;
  a.hist = (unsigned*)ws; ws += align256(smd::eval_hist_bytes(b));
  a.partial0 = (double*)ws; ws += eval_partial_bytes(b, H, W, smd::kEvAlignSums);
  a.partial1 = (double*)ws; ws += eval_partial_bytes(b, H, W, smd::kEvSums);
  a.align = (double*)ws; ws += align256((size_t)b*2*sizeof(double));
  a.pred = (float*)ws;
  a.values = values; a.counts = counts; a.status = status; a.medians = medians; a.depth = depth; a.valid = valid; a.resized = resized;
  return check_launch(smd::launch_eval_metrics(a, (hipStream_t)stream), "eval_metrics");
}

// workspace of smd_eval_pointcloud: both clouds as x | y | z arrays of H*W slots | the smallest squared distance per query and direction
size_t smd_eval_pointcloud_workspace_bytes(int b, int H, int W) {
  if (b < 1 || H < 1 || W < 1 || (size_t)H*W >= ((size_t)1 << 30)) return 0;
  const size_t cap = (size_t)H*W;
  if ((size_t)b*smd::pc_splits((int)cap) > 65535) return 0;
  return align256(b*6*cap*sizeof(float)) + align256((size_t)b*2*((cap + 1)/2)*sizeof(unsigned));
}

int smd_eval_pointcloud(const float* depth, const float* target, const uint8_t* mask, const int* prefix, const float* K_inv, int b, int H, int W,
                        float* nn, double* stats, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (!depth || !target || !mask || !prefix || !K_inv || !nn || !stats || !counts || !workspace) return fail(SMD_E_INVALID, "null pointer");
  const size_t need = smd_eval_pointcloud_workspace_bytes(b, H, W);
  if (need == 0) return fail(SMD_E_INVALID, "sizes that are not served b=%d H=%d W=%d (H*W < 2^30, b*min(32, ceil(H*W/2048)) <= 65535)", b, H, W);
  if ((uintptr_t)workspace % 4 || (uintptr_t)stats % 8) return fail(SMD_E_INVALID, "the workspace needs 4-byte and stats 8-byte alignment");
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  smd::PcArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = depth; a.target = target; a.mask = mask; a.cs = prefix; a.Kinv = K_inv; a.b = b; a.W = W; a.cap = H*W; a.nqcap = (a.cap + 1)/2;
  a.pts = (float*)workspace; a.best = (unsigned*)((char*)workspace + align256((size_t)b*6*a.cap*sizeof(float)));
  a.nn = nn; a.stats = stats; a.counts = counts;
  return check_launch(smd::launch_eval_pointcloud(a, (hipStream_t)stream), "eval_pointcloud");
}

// workspace of smd_viz_disp: the radix histograms (zeroed by the call)
size_t smd_viz_disp_workspace_bytes(int b, int h, int w) {
  if (b < 1 || h < 1 || w < 1 || b > 65535 || (size_t)h*w >= ((size_t)1 << 31)) return 0;
  return align256(smd::viz_hist_bytes(b));
}

int smd_viz_disp(const float* disp, int b, int h, int w, int invert, int select, float vmin, float den0, const float* lut, int N, float* rgb, float* vmax,
                 float* den, void* workspace, size_t workspace_bytes, void* stream) {
  if (!disp || !lut || !rgb || !vmax || !den || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1 || b > 65535 || (size_t)h*w >= ((size_t)1 << 31)) return fail(SMD_E_INVALID, "invalid sizes b=%d h=%d w=%d", b, h, w);
  if (N < 1 || N > smd::kVzMaxLut) return fail(SMD_E_INVALID, "the table has %d entries (1 .. %d)", N, smd::kVzMaxLut);
  if ((uintptr_t)workspace % 4) return fail(SMD_E_INVALID, "the workspace needs 4-byte alignment");
  const size_t need = smd_viz_disp_workspace_bytes(b, h, w);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  smd::VizDispArgs a;
  memset(&a, 0, sizeof(a));
  a.disp = disp; a.b = b; a.hw = h*w; a.invert = invert != 0; a.select = select != 0; a.vmin = vmin; a.den0 = den0; a.lut = lut; a.N = N;
  a.rgb = rgb; a.vmax = vmax; a.den = den; a.hist = (unsigned*)workspace;
  return check_launch(smd::launch_viz_disp(a, (hipStream_t)stream), "viz_disp");
}

// workspace of smd_viz_feat_*: the mean's block sums | the fp32 means | the blocks' tiles | the projection's block extrema | the six extrema
static bool viz_feat_args(smd::VizFeatArgs& a, int b, int C, int h, int w) {
  if (b < 1 || C < 3 || C > smd::kVzMaxC || h < 1 || w < 1 || (size_t)b*h*w >= ((size_t)1 << 31) || (size_t)b*h*w < 3) return false;
  memset(&a, 0, sizeof(a));
  a.b = b; a.C = C; a.hw = h*w;
  smd::viz_feat_plan(a);
  return a.nchunk <= 65535;
}
static size_t viz_feat_carve(smd::VizFeatArgs& a, void* workspace) {
  // offsets first (the size query passes no workspace), pointers only where there is one
  size_t off = 0;
  const size_t o_mean_part = off; off += align256((size_t)a.C*a.nsplit*sizeof(double));
  const size_t o_meanf = off; off += align256((size_t)a.C*sizeof(float));
  const size_t o_tile = off; off += align256((size_t)a.npairs*a.nchunk*smd::kVzTileElems*sizeof(float));
  const size_t o_ext_part = off; off += align256((size_t)a.nblk*6*sizeof(float));
  const size_t o_ext = off; off += 256;
  if (workspace) {
    char* ws = (char*)workspace;
    a.mean_part = (double*)(ws + o_mean_part); a.meanf = (float*)(ws + o_meanf); a.tile_part = (float*)(ws + o_tile);
    a.ext_part = (float*)(ws + o_ext_part); a.ext = (float*)(ws + o_ext);
  }
  return off;
}

size_t smd_viz_feat_workspace_bytes(int b, int C, int h, int w) {
  smd::VizFeatArgs a;
  if (!viz_feat_args(a, b, C, h, w)) return 0;
  return viz_feat_carve(a, nullptr);
}

int smd_viz_feat_moments(const float* feat, int b, int C, int h, int w, double* mean, double* cov, void* workspace, size_t workspace_bytes, void* stream) {
  if (!feat || !mean || !cov || !workspace) return fail(SMD_E_INVALID, "null pointer");
  smd::VizFeatArgs a;
  if (!viz_feat_args(a, b, C, h, w)) return fail(SMD_E_INVALID, "sizes that are not served b=%d C=%d h=%d w=%d (3 <= C <= %d, 3 <= b*h*w < 2^31)", b, C, h, w, smd::kVzMaxC);
  if ((uintptr_t)workspace % 8 || (uintptr_t)mean % 8 || (uintptr_t)cov % 8) return fail(SMD_E_INVALID, "the workspace, mean and cov need 8-byte alignment");
  const size_t need = viz_feat_carve(a, workspace);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  a.feat = feat; a.mean = mean; a.cov = cov;
  return check_launch(smd::launch_viz_feat_moments(a, (hipStream_t)stream), "viz_feat_moments");
}

int smd_viz_feat_project(const float* feat, const double* mean, const float* V, int b, int C, int h, int w, float* rgb, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!feat || !mean || !V || !rgb || !workspace) return fail(SMD_E_INVALID, "null pointer");
  smd::VizFeatArgs a;
  if (!viz_feat_args(a, b, C, h, w)) return fail(SMD_E_INVALID, "sizes that are not served b=%d C=%d h=%d w=%d (3 <= C <= %d, 3 <= b*h*w < 2^31)", b, C, h, w, smd::kVzMaxC);
  if ((uintptr_t)workspace % 8 || (uintptr_t)mean % 8) return fail(SMD_E_INVALID, "the workspace and mean need 8-byte alignment");
  const size_t need = viz_feat_carve(a, workspace);
  if (workspace_bytes < need) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  a.feat = feat; a.mean = (double*)mean; a.V = V; a.rgb = rgb;
  return check_launch(smd::launch_viz_feat_project(a, (hipStream_t)stream), "viz_feat_project");
}

// workspace of smd_make_grid: the extrema of the blocks of the normalize pass
size_t smd_make_grid_workspace_bytes(void) { return align256((size_t)smd::kVzGridParts*2*sizeof(float)); }

int smd_make_grid(const void* x, int is_u8, int b, int c, int h, int w, int n_imgs, int nrow, int padding, float pad_value, int normalize, float* grid,
                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !grid || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || (c != 1 && c != 3) || h < 1 || w < 1) return fail(SMD_E_INVALID, "invalid sizes b=%d c=%d h=%d w=%d (c is 1 or 3)", b, c, h, w);
  if (n_imgs < 1 || nrow < 1 || padding < 0) return fail(SMD_E_INVALID, "invalid grid n_imgs=%d nrow=%d padding=%d", n_imgs, nrow, padding);
  if ((uintptr_t)workspace % 4) return fail(SMD_E_INVALID, "the workspace needs 4-byte alignment");
  if (workspace_bytes < smd_make_grid_workspace_bytes()) return fail(SMD_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, smd_make_grid_workspace_bytes());
  smd::GridArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.u8 = is_u8 != 0; a.c = c; a.h = h; a.w = w; a.n = std::min(b, n_imgs);
  a.xmaps = std::min(nrow, a.n); a.ymaps = smd::ceil_div(a.n, a.xmaps);
  a.pad = a.n == 1 ? 0 : padding;                  // a single image is returned as it is (torchvision: `tensor.squeeze(0)`)
  const size_t Hg = (size_t)(h + a.pad)*a.ymaps + a.pad, Wg = (size_t)(w + a.pad)*a.xmaps + a.pad;
  if (3*Hg*Wg >= ((size_t)1 << 31) || (size_t)a.n*c*h*w >= ((size_t)1 << 31)) return fail(SMD_E_INVALID, "the grid and the images must stay below 2^31 elements");
  a.Hg = (int)Hg; a.Wg = (int)Wg; a.pad_value = pad_value; a.normalize = normalize != 0; a.grid = grid; a.ext_part = (float*)workspace;
  return check_launch(smd::launch_make_grid(a, (hipStream_t)stream), "make_grid");
}

size_t smd_recon_reduce_workspace_bytes(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1) return 0;
  return align256((size_t)smd::ceil_div(B*h*w, 256)*sizeof(float));
}

int smd_recon_reduce_fwd(const float* err_warp, const float* err_static, const float* mask, const float* noise, uint64_t seed, float* err, uint8_t* sel,
                         float* loss, void* workspace, size_t workspace_bytes, int n, int B, int h, int w, int flags, void* stream) {
  if (!err_warp || !err || !sel || !loss || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if ((flags & (SMD_MASK_EXPLAINABILITY | SMD_MASK_UNCERTAINTY)) && !mask) return fail(SMD_E_INVALID, "Must provide a 'mask' when masking...");
  if ((flags & SMD_USE_AUTOMASK) && !err_static) return fail(SMD_E_INVALID, "Must provide the original 'source' images when automasking...");
  if (n < 1 || n >= SMD_SEL_MASKED || B < 1 || h < 1 || w < 1) return fail(SMD_E_INVALID, "invalid sizes");
  if (workspace_bytes < smd_recon_reduce_workspace_bytes(B, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_recon_reduce_fwd(err_warp, err_static, mask, noise, seed, err, sel, loss, (float*)workspace, n, B, h, w, flags,
                                                   (hipStream_t)stream), "recon_reduce_fwd");
}

int smd_recon_reduce_bwd(const uint8_t* sel, const float* g_loss, float* g_err_warp, const float* err_warp, const float* err_static,
                         const float* mask, float* g_mask, int n, int B, int h, int w, int flags, void* stream) {
  if (!sel || !g_loss || !g_err_warp) return fail(SMD_E_INVALID, "null pointer");
  if (n < 1 || B < 1 || h < 1 || w < 1) return fail(SMD_E_INVALID, "invalid sizes");
  if (mask && (!g_mask || !err_warp || ((flags & SMD_USE_AUTOMASK) && !err_static))) return fail(SMD_E_INVALID, "a masked reduction needs err_warp, err_static (with automask) and g_mask");
  return check_launch(smd::launch_recon_reduce_bwd(sel, g_loss, g_err_warp, err_warp, err_static, mask, g_mask, n, B, h, w, flags, (hipStream_t)stream), "recon_reduce_bwd");
}

// ------------------------------------------------------------------------------------------------
// Monodepth decoder glue
static bool dec_sizes_ok(long long planes, int h, int w) {
  return planes >= 1 && h >= 2 && w >= 2 && (long long)(h + 2)*(w + 2) < (1ll << 30) && planes*(((long long)(h + 2)*(w + 2) + 255)/256) < (1ll << 31);
}
size_t smd_decoder_glue_workspace_bytes(int B, int C, int h, int w) {
  if (B < 1 || C < 1 || h < 1 || w < 1) return 0;
  return align256(smd::decoder_bias_partials(B, C, h, w)*sizeof(float));
}
int smd_elu_pad_fwd(const void* x, const float* bias, void* out, int B, int C, int h, int w, int apply_elu, int dtypes, void* stream) {
  if (!x || !out) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || C < 1 || !dec_sizes_ok((long long)B*C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  return check_launch(smd::launch_elu_pad_fwd(x, bias, out, B, C, h, w, apply_elu, dtypes, (hipStream_t)stream), "elu_pad_fwd");
}
int smd_elu_pad_bwd(const void* x, const float* bias, const void* g_out, void* g_x, float* g_bias, void* workspace, size_t workspace_bytes,
                    int B, int C, int h, int w, int apply_elu, int dtypes, void* stream) {
  if (!x || !g_out || !g_x || (g_bias && !workspace)) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || C < 1 || !dec_sizes_ok((long long)B*C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  if (g_bias && workspace_bytes < smd_decoder_glue_workspace_bytes(B, C, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_elu_pad_bwd(x, bias, g_out, g_x, g_bias, (float*)workspace, B, C, h, w, apply_elu, dtypes, (hipStream_t)stream), "elu_pad_bwd");
}
static bool head_sizes_ok(int B, int C, int h, int w) {
  return B >= 1 && C >= 1 && C < 65535 && dec_sizes_ok((long long)B*C, h, w) && (long long)B*((h + 47)/48) < 65536 && h < 65536 && (long long)B*C*(h + 2)*(w + 2) < (1ll << 40);
}
size_t smd_conv3x3_head_workspace_bytes(int B, int C, int h, int w) {
  if (!head_sizes_ok(B, C, h, w)) return 0;
  return align256(smd::conv_head_partials(B, C, 1, h, w)*sizeof(float));
}
int smd_conv3x3_head_fwd(const void* xp, const float* weight, const float* bias, float* y, int B, int C, int h, int w, int act, void* stream) {
  if (!xp || !weight || !y) return fail(SMD_E_INVALID, "null pointer");
  if (!head_sizes_ok(B, C, h, w) || (act & ~(1 | SMD_HEAD_X_BF16))) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d act=%d", B, C, h, w, act);
  return check_launch(smd::launch_conv_head_fwd(xp, (act & SMD_HEAD_X_BF16) != 0, weight, bias, y, B, C, 1, h, w, act & 1, (hipStream_t)stream), "conv3x3_head_fwd");
}
int smd_conv3x3_head_bwd(const void* xp, const float* weight, const float* y, const float* g_y, void* g_xp, float* g_weight, float* g_bias,
                         void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int act, void* stream) {
  if (!weight || !y || !g_y || (!g_xp && !g_weight) || (g_weight && (!xp || !workspace)) || (g_bias && !g_weight)) return fail(SMD_E_INVALID, "null pointer");
  if (!head_sizes_ok(B, C, h, w) || (act & ~(1 | SMD_HEAD_X_BF16))) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d act=%d", B, C, h, w, act);
  if (g_weight && workspace_bytes < smd_conv3x3_head_workspace_bytes(B, C, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_conv_head_bwd(xp, (act & SMD_HEAD_X_BF16) != 0, weight, y, g_y, g_xp, g_weight, g_bias, (float*)workspace, B, C, 1, h, w, act & 1, (hipStream_t)stream), "conv3x3_head_bwd");
}
static bool headn_args_ok(int B, int C, int n, int h, int w, int act) {
  const int a = act & 3;
  return n >= 1 && n <= 4 && head_sizes_ok(B, C, h, w) && (act & ~(3 | SMD_HEADN_X_BF16)) == 0 && a != 3 && dec_sizes_ok((long long)B*n, h, w);
}
size_t smd_conv3x3_headn_workspace_bytes(int B, int C, int n, int h, int w) {
  if (!headn_args_ok(B, C, n, h, w, 0)) return 0;
  return align256(smd::conv_head_partials(B, C, n, h, w)*sizeof(float));
}
int smd_conv3x3_headn_fwd(const void* xp, const float* weight, const float* bias, float* y, int B, int C, int n, int h, int w, int act, void* stream) {
  if (!xp || !weight || !y) return fail(SMD_E_INVALID, "null pointer");
  if (!headn_args_ok(B, C, n, h, w, act)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d n=%d h=%d w=%d act=%d (1 <= n <= 4)", B, C, n, h, w, act);
  return check_launch(smd::launch_conv_head_fwd(xp, (act & SMD_HEADN_X_BF16) != 0, weight, bias, y, B, C, n, h, w, act & 3, (hipStream_t)stream), "conv3x3_headn_fwd");
}
int smd_conv3x3_headn_bwd_data(const float* weight, const float* y, const float* g_y, void* g_xp, int B, int C, int n, int h, int w, int act, void* stream) {
  if (!weight || !y || !g_y || !g_xp) return fail(SMD_E_INVALID, "null pointer");
  if (!headn_args_ok(B, C, n, h, w, act)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d n=%d h=%d w=%d act=%d (1 <= n <= 4)", B, C, n, h, w, act);
  return check_launch(smd::launch_conv_head_bwd(nullptr, (act & SMD_HEADN_X_BF16) != 0, weight, y, g_y, g_xp, nullptr, nullptr, nullptr, B, C, n, h, w, act & 3,
                                                (hipStream_t)stream), "conv3x3_headn_bwd_data");
}
int smd_conv3x3_headn_bwd_wgt(const void* xp, const float* y, const float* g_y, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                              int B, int C, int n, int h, int w, int act, void* stream) {
  if (!xp || !y || !g_y || !g_weight || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!headn_args_ok(B, C, n, h, w, act)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d n=%d h=%d w=%d act=%d (1 <= n <= 4)", B, C, n, h, w, act);
  if (workspace_bytes < smd_conv3x3_headn_workspace_bytes(B, C, n, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_conv_head_bwd(xp, (act & SMD_HEADN_X_BF16) != 0, nullptr, y, g_y, nullptr, g_weight, g_bias, (float*)workspace, B, C, n, h, w, act & 3,
                                                (hipStream_t)stream), "conv3x3_headn_bwd_wgt");
}

// Predictive-mask post-process and regularisers (smd_masks.hip)
static int up_stack_check(int S, int b, int n, int h, int w) {
  if (b < 1 || n < 1 || h < 1 || w < 1 || (long long)b*n > 65535 || (long long)h*w >= (1ll << 30)) return fail(SMD_E_INVALID, "invalid sizes b=%d n=%d h=%d w=%d (b*n <= 65535)", b, n, h, w);
  if ((long long)S*b*n*h*w >= (1ll << 40)) return fail(SMD_E_INVALID, "output too large");
  return SMD_OK;
}
int smd_upsample_stack_fwd(const float* const* x, const int* hs, const int* ws, int S, int b, int n, int h, int w, float* out, void* stream) {
  if (!x || !out) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = up_stack_check(S, b, n, h, w)) return rc;
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, x, nullptr, hs, ws, nullptr, S)) return rc;
  for (int s = 0; s < S; ++s) {
    if (!x[s]) return fail(SMD_E_INVALID, "null input pointer for scale %d", s);
    if ((long long)hs[s]*ws[s] >= (1ll << 30)) return fail(SMD_E_INVALID, "scale %d too large", s);
  }
  return check_launch(smd::launch_upsample_stack_fwd(sc, b*n, h, w, out, (hipStream_t)stream), "upsample_stack_fwd");
}
int smd_upsample_stack_bwd(const int* hs, const int* ws, int S, int b, int n, int h, int w, const float* g_out, float* const* g_x, void* stream) {
  if (!g_out || !g_x) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = up_stack_check(S, b, n, h, w)) return rc;
  smd::ScaleSet sc;
  if (int rc = fill_scales(sc, nullptr, g_x, hs, ws, nullptr, S)) return rc;
  long long blocks = 0;
  for (int s = 0; s < S; ++s) {
    if (!g_x[s]) return fail(SMD_E_INVALID, "null gradient pointer for scale %d", s);
    if ((long long)hs[s]*ws[s] >= (1ll << 30)) return fail(SMD_E_INVALID, "scale %d too large", s);
    blocks += ((long long)hs[s]*ws[s] + 255)/256;
  }
  if (blocks >= (1ll << 31)) return fail(SMD_E_INVALID, "too many source pixels");
  return check_launch(smd::launch_upsample_stack_bwd(sc, b*n, h, w, g_out, (hipStream_t)stream), "upsample_stack_bwd");
}
static int fill_means(smd::MeanSet& ms, const float* const* x, float* const* g, const long long* numel, int S, int mode) {
  if (S < 1 || S > SMD_MAX_SCALES) return fail(SMD_E_INVALID, "S=%d outside [1, %d]", S, SMD_MAX_SCALES);
  if (!numel) return fail(SMD_E_INVALID, "null size array");
  if (mode < SMD_MEAN_BCE_ONES || mode > SMD_MEAN_NEGATE) return fail(SMD_E_INVALID, "invalid mode %d", mode);
  memset(&ms, 0, sizeof(ms));
  ms.S = S;
  for (int s = 0; s < S; ++s) {
    if (numel[s] < 1) return fail(SMD_E_INVALID, "scale %d is empty", s);
    ms.p[s] = x ? x[s] : nullptr; ms.g[s] = g ? g[s] : nullptr; ms.n[s] = numel[s];
  }
  if (smd::scale_mean_blocks(ms) < 1) return fail(SMD_E_INVALID, "too many elements");
  return SMD_OK;
}
size_t smd_scale_mean_workspace_bytes(const long long* numel, int S) {
  smd::MeanSet ms;
  if (fill_means(ms, nullptr, nullptr, numel, S, 0)) return 0;
  return 256 + align256((size_t)ms.first_block[SMD_MAX_SCALES]*sizeof(float));
}
int smd_scale_mean_fwd(const float* const* x, const long long* numel, int S, int mode, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !loss || !workspace) return fail(SMD_E_INVALID, "null pointer");
  smd::MeanSet ms;
  if (int rc = fill_means(ms, x, nullptr, numel, S, mode)) return rc;
  for (int s = 0; s < S; ++s) if (!x[s]) return fail(SMD_E_INVALID, "null input pointer for scale %d", s);
  if (workspace_bytes < smd_scale_mean_workspace_bytes(numel, S)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_scale_mean_fwd(ms, mode, (float*)((char*)workspace + 256), (unsigned*)workspace, loss, (hipStream_t)stream), "scale_mean_fwd");
}
int smd_scale_mean_bwd(const float* const* x, const long long* numel, int S, int mode, const float* g_loss, float* const* g_x, void* stream) {
  if (!g_loss || !g_x || (mode == SMD_MEAN_BCE_ONES && !x)) return fail(SMD_E_INVALID, "null pointer");
  smd::MeanSet ms;
  if (int rc = fill_means(ms, x, g_x, numel, S, mode)) return rc;
  for (int s = 0; s < S; ++s) if (!g_x[s] || (mode == SMD_MEAN_BCE_ONES && !x[s])) return fail(SMD_E_INVALID, "null pointer for scale %d", s);
  return check_launch(smd::launch_scale_mean_bwd(ms, mode, g_loss, (hipStream_t)stream), "scale_mean_bwd");
}
static bool thin_sizes_ok(int B, int C, int h, int w) { return (C == 16 || C == 32) && head_sizes_ok(B, C, h, w) && dec_sizes_ok((long long)B*16, h, w) && B < 65536 && h + 2 < 4*65536; }
size_t smd_conv3x3_thin_workspace_bytes(int B, int C, int h, int w) {
  if (!thin_sizes_ok(B, C, h, w)) return 0;
  return align256(smd::conv_thin_partials(B, C, h, w)*sizeof(float));
}
int smd_conv3x3_thin_bwd(const float* xp, const float* weight, const float* g_y, float* g_xp, float* g_weight, void* workspace, size_t workspace_bytes,
                         int B, int C, int h, int w, void* stream) {
  if (!g_y || (!g_xp && !g_weight) || (g_xp && !weight) || (g_weight && (!xp || !workspace))) return fail(SMD_E_INVALID, "null pointer");
  if (C != 16 && C != 32 && C >= 1) return fail(SMD_E_UNSUPPORTED, "the thin convolution serves 16 or 32 input channels, not %d", C);
  if (!thin_sizes_ok(B, C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  if (g_weight && workspace_bytes < smd_conv3x3_thin_workspace_bytes(B, C, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (g_xp) { if (int rc = check_launch(smd::launch_conv_thin_bwd_data(g_y, weight, g_xp, B, C, h, w, st), "conv3x3_thin_bwd (data)")) return rc; }
  if (g_weight) { if (int rc = check_launch(smd::launch_conv_thin_bwd_wgt(xp, g_y, g_weight, (float*)workspace, B, C, h, w, st), "conv3x3_thin_bwd (weights)")) return rc; }
  return SMD_OK;
}
int smd_conv3x3_thin_fwd(const float* xp, const float* weight, float* y, int B, int C, int h, int w, void* stream) {
  if (!xp || !weight || !y) return fail(SMD_E_INVALID, "null pointer");
  if (C != 16 && C != 32 && C >= 1) return fail(SMD_E_UNSUPPORTED, "the thin convolution serves 16 or 32 input channels, not %d", C);
  if (!thin_sizes_ok(B, C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  return check_launch(smd::launch_conv_thin_fwd(xp, weight, y, B, C, h, w, (hipStream_t)stream), "conv3x3_thin_fwd");
}
static bool mfma_sizes_ok(int B, int C, int CO, int h, int w) {   // grid dimensions below 65536, element counts that int arithmetic inside a plane can hold,
  // one sample's activation and gradient under 2 GiB each (the weight gradient's LDS-DMA pieces carry 32-bit byte offsets from the sample's first element)
  return B >= 1 && C >= 1 && CO >= 1 && C <= 4096 && CO <= 4096 && h >= 1 && w >= 1 && h < 32768 && w < 32768 && (long long)(h + 2)*(w + 2) < (1ll << 30) &&
         (long long)B*((C + 31)/32)*((CO + 31)/32) < 65536 && (long long)C*(h + 2)*(w + 2) < (1ll << 29) && (long long)CO*h*w < (1ll << 29);
}
using smd::ConvOp;
static bool conv_two_tiles() { return knob("conv_two_tiles", 0) != 0; }   // read ONCE per entry point: its size check and its launch get the same value
size_t smd_conv3x3_mfma_packed_bytes(int C, int CO, int pieces) {
  if (C < 1 || CO < 1 || pieces < 1 || pieces > 3) return 0;
  return align256(smd::conv_mfma_packed_elems((C + 31) & ~31, CO, pieces)*2);   // (the data-gradient image: whole tiles of 32 input channels)
}
static size_t mfma_workspace_bytes(bool zpad, int B, int C, int CO, int h, int w, bool two_tiles) {   // one size for the three operators
  if (!mfma_sizes_ok(B, C, CO, h, w)) return 0;
  size_t n = std::max({(size_t)64, smd::conv_mfma_split_elems(ConvOp::Fwd, zpad, B, C, CO, h, w, two_tiles), smd::conv_mfma_split_elems(ConvOp::Data, zpad, B, C, CO, h, w, two_tiles)});
  if (smd::conv_mfma_served(ConvOp::Wgt, zpad, C, CO)) n = std::max(n, smd::conv_mfma_wgrad_partials(zpad, B, C, CO, h, w));
  return align256(n*sizeof(float));
}
size_t smd_conv3x3_mfma_workspace_bytes(int B, int C, int CO, int h, int w) { return mfma_workspace_bytes(false, B, C, CO, h, w, conv_two_tiles()); }
size_t smd_conv3x3z_mfma_workspace_bytes(int B, int C, int CO, int h, int w) { return mfma_workspace_bytes(true, B, C, CO, h, w, conv_two_tiles()); }
static int mfma_unserved(ConvOp op, bool zpad, int C, int CO) {   // (what IS served: smd::conv_mfma_served, include/smd_hotpath.h)
  const char* name[] = {"forward", "data gradient", "weight gradient"};
  return fail(SMD_E_UNSUPPORTED, "the %s%s does not serve C=%d CO=%d", zpad ? "zero-padded " : "", name[(int)op], C, CO);
}
// What the six launches check after their pointers, in this order: pieces, sizes (SMD_E_INVALID), channels (SMD_E_UNSUPPORTED), workspace (SMD_E_WORKSPACE).
static int mfma_check(ConvOp op, bool zpad, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, bool two_tiles) {
  if (zpad && pieces != 2 && pieces != 3) return fail(SMD_E_UNSUPPORTED, "the zero-padded forms take float tensors: pieces 2 or 3, not %d", pieces);
  if (pieces < 1 || pieces > 3) return fail(SMD_E_UNSUPPORTED, "pieces must be 1 (bfloat16 tensors), 2 or 3 (float tensors), not %d", pieces);
  if (!mfma_sizes_ok(B, C, CO, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d CO=%d h=%d w=%d", B, C, CO, h, w);
  if (!smd::conv_mfma_served(op, zpad, C, CO)) return mfma_unserved(op, zpad, C, CO);
  if (workspace_bytes < mfma_workspace_bytes(zpad, B, C, CO, h, w, two_tiles)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return SMD_OK;
}
int smd_conv3x3_mfma_pack(const float* weight, void* wp_fwd, void* wp_bwd, int C, int CO, int pieces, void* stream) {
  if (!weight || (!wp_fwd && !wp_bwd)) return fail(SMD_E_INVALID, "null pointer");
  if (pieces < 1 || pieces > 3) return fail(SMD_E_UNSUPPORTED, "pieces must be 1 (bfloat16 tensors), 2 or 3 (float tensors), not %d", pieces);
  if (C < 1 || CO < 1 || C > 4096 || CO > 4096) return fail(SMD_E_INVALID, "invalid sizes C=%d CO=%d", C, CO);
  if (wp_fwd && !smd::conv_mfma_served(ConvOp::Fwd, false, C, CO)) return mfma_unserved(ConvOp::Fwd, false, C, CO);
  if (wp_bwd && !smd::conv_mfma_served(ConvOp::Data, false, C, CO) && !(pieces == 3 && smd::conv_s2_served(C, CO))) return mfma_unserved(ConvOp::Data, false, C, CO);   // (or the stride-2 data gradient's channel counts)
  return check_launch(smd::launch_conv_mfma_pack(weight, wp_fwd, wp_bwd, C, CO, pieces, (hipStream_t)stream), "conv3x3_mfma_pack");
}
// One body for the padded (smd_conv3x3_mfma_*) and zero-padded (smd_conv3x3z_mfma_*: unpadded x / g_x, fp32 only) forward (x -> y) and data gradient (g_y -> g_x)
static int mfma_form(ConvOp op, bool zpad, const void* in, const void* wp, void* out, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream, const char* what) {
  if (!in || !wp || !out || !workspace) return fail(SMD_E_INVALID, "null pointer");
  const bool two_tiles = conv_two_tiles();
  if (int rc = mfma_check(op, zpad, workspace_bytes, B, C, CO, h, w, pieces, two_tiles)) return rc;
  const auto launch = op == ConvOp::Fwd ? smd::launch_conv_mfma_fwd : smd::launch_conv_mfma_bwd_data;
  return check_launch(launch(in, wp, out, (float*)workspace, zpad, B, C, CO, h, w, pieces, two_tiles, (hipStream_t)stream), what);
}
static int mfma_bwd_weight(bool zpad, const void* x, const void* g_y, float* g_weight, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  if (!x || !g_y || !g_weight || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = mfma_check(ConvOp::Wgt, zpad, workspace_bytes, B, C, CO, h, w, pieces, conv_two_tiles())) return rc;
  return check_launch(smd::launch_conv_mfma_bwd_wgt(x, g_y, g_weight, (float*)workspace, zpad, B, C, CO, h, w, pieces, (hipStream_t)stream), zpad ? "conv3x3z_mfma_bwd_weight" : "conv3x3_mfma_bwd_weight");
}
int smd_conv3x3_mfma_fwd(const void* xp, const void* wp_fwd, void* y, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_form(ConvOp::Fwd, false, xp, wp_fwd, y, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream, "conv3x3_mfma_fwd");
}
int smd_conv3x3_mfma_bwd_data(const void* g_y, const void* wp_bwd, void* g_xp, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_form(ConvOp::Data, false, g_y, wp_bwd, g_xp, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream, "conv3x3_mfma_bwd_data");
}
int smd_conv3x3_mfma_bwd_weight(const void* xp, const void* g_y, float* g_weight, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_bwd_weight(false, xp, g_y, g_weight, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream);
}
int smd_conv3x3z_mfma_fwd(const float* x, const void* wp_fwd, float* y, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_form(ConvOp::Fwd, true, x, wp_fwd, y, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream, "conv3x3z_mfma_fwd");
}
int smd_conv3x3z_mfma_bwd_data(const float* g_y, const void* wp_bwd, float* g_x, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_form(ConvOp::Data, true, g_y, wp_bwd, g_x, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream, "conv3x3z_mfma_bwd_data");
}
int smd_conv3x3z_mfma_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes, int B, int C, int CO, int h, int w, int pieces, void* stream) {
  return mfma_bwd_weight(true, x, g_y, g_weight, workspace, workspace_bytes, B, C, CO, h, w, pieces, stream);
}
// the ResNet stem: conv2d(x (B,C,H,W), weight (64,C,7,7), stride 2, padding 3), C = 3 | 6 (smd_conv_stem.hip)
static bool stem_sizes_ok(int B, int C, int H, int W) {
  if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1) return false;
  const long long ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  return (long long)C*H*W < (1ll << 31) && 64*ho*wo < (1ll << 31) && (ho + 3)/4 <= 65535;
}
size_t smd_conv7x7s2_packed_bytes(int C, int CO) { return smd::conv_stem_served(C, CO) ? smd::conv_stem_packed_bytes(C) : 0; }
size_t smd_conv7x7s2_workspace_bytes(int B, int C, int CO, int H, int W) {
  if (!smd::conv_stem_served(C, CO) || !stem_sizes_ok(B, C, H, W)) return 0;
  return align256(smd::conv_stem_wgrad_floats(B, C, H, W)*sizeof(float));
}
int smd_conv7x7s2_pack(const float* weight, void* wp, int C, int CO, void* stream) {
  if (!weight || !wp) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::conv_stem_served(C, CO)) return fail(SMD_E_UNSUPPORTED, "the stem kernels serve CO == 64 with C == 3 | 6, not C=%d CO=%d", C, CO);
  return check_launch(smd::launch_conv_stem_pack(weight, wp, C, (hipStream_t)stream), "conv7x7s2_pack");
}
int smd_conv7x7s2_fwd(const float* x, const void* wp, float* y, int B, int C, int CO, int H, int W, void* stream) {
  if (!x || !wp || !y) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::conv_stem_served(C, CO)) return fail(SMD_E_UNSUPPORTED, "the stem kernels serve CO == 64 with C == 3 | 6, not C=%d CO=%d", C, CO);
  if (!stem_sizes_ok(B, C, H, W)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d H=%d W=%d", B, C, H, W);
  return check_launch(smd::launch_conv_stem_fwd(x, wp, y, B, C, H, W, (hipStream_t)stream), "conv7x7s2_fwd");
}
int smd_conv7x7s2_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes,
                             int B, int C, int CO, int H, int W, void* stream) {
  if (!x || !g_y || !g_weight || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::conv_stem_served(C, CO)) return fail(SMD_E_UNSUPPORTED, "the stem kernels serve CO == 64 with C == 3 | 6, not C=%d CO=%d", C, CO);
  if (!stem_sizes_ok(B, C, H, W)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d H=%d W=%d", B, C, H, W);
  if (workspace_bytes < smd_conv7x7s2_workspace_bytes(B, C, CO, H, W)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_conv_stem_bwd_wgt(x, g_y, g_weight, (float*)workspace, B, C, H, W, (hipStream_t)stream), "conv7x7s2_bwd_weight");
}
// the encoders' transition convolutions: conv2d(x (B,C,H,W), weight (CO,C,3,3), stride 2, padding 1) (smd_conv_s2.hip)
static bool s2_sizes_ok(int B, int C, int CO, int H, int W) {     // grid dimensions below 65536; one sample's x and y under 2 GiB each, a plane's offsets in an int
  if (B < 1 || B > 65535 || C < 1 || CO < 1 || C > 4096 || CO > 4096 || H < 1 || W < 1) return false;
  const long long ho = (H - 1)/2 + 1, wo = (W - 1)/2 + 1;
  return (long long)C*H*W < (1ll << 29) && (long long)CO*ho*wo < (1ll << 29) && ho <= 65535 && (long long)B*((C + 63)/64)*((CO + 63)/64) < 65536;
}
size_t smd_conv3x3s2_mfma_workspace_bytes(int B, int C, int CO, int H, int W) {
  if (!smd::conv_s2_served(C, CO) || !s2_sizes_ok(B, C, CO, H, W)) return 0;
  return align256(smd::conv_s2_workspace_floats(B, C, CO, H, W)*sizeof(float));
}
static int s2_check(size_t workspace_bytes, int B, int C, int CO, int H, int W) {
  if (!smd::conv_s2_served(C, CO)) return fail(SMD_E_UNSUPPORTED, "the stride-2 kernels serve C %% 16 == 0 with CO %% 32 == 0, not C=%d CO=%d", C, CO);
  if (!s2_sizes_ok(B, C, CO, H, W)) return fail(SMD_E_UNSUPPORTED, "the stride-2 kernels do not serve B=%d C=%d CO=%d H=%d W=%d", B, C, CO, H, W);
  if (workspace_bytes < smd_conv3x3s2_mfma_workspace_bytes(B, C, CO, H, W)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return SMD_OK;
}
int smd_conv3x3s2_mfma_fwd(const float* x, const void* wp_fwd, float* y, void* workspace, size_t workspace_bytes, int B, int C, int CO, int H, int W, void* stream) {
  if (!x || !wp_fwd || !y || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = s2_check(workspace_bytes, B, C, CO, H, W)) return rc;
  return check_launch(smd::launch_conv_s2_fwd(x, wp_fwd, y, (float*)workspace, B, C, CO, H, W, (hipStream_t)stream), "conv3x3s2_mfma_fwd");
}
int smd_conv3x3s2_mfma_bwd_weight(const float* x, const float* g_y, float* g_weight, void* workspace, size_t workspace_bytes, int B, int C, int CO, int H, int W, void* stream) {
  if (!x || !g_y || !g_weight || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = s2_check(workspace_bytes, B, C, CO, H, W)) return rc;
  return check_launch(smd::launch_conv_s2_bwd_wgt(x, g_y, g_weight, (float*)workspace, B, C, CO, H, W, (hipStream_t)stream), "conv3x3s2_mfma_bwd_weight");
}
// their data gradient: the same channel counts and sizes, and a grid that 32 bits hold
static bool s2d_sizes_ok(int B, int C, int CO, int H, int W) { return s2_sizes_ok(B, C, CO, H, W) && smd::conv_s2d_blocks(B, C, CO, H, W) < (1ll << 31); }
size_t smd_conv3x3s2d_mfma_workspace_bytes(int B, int C, int CO, int H, int W) {
  if (!smd::conv_s2_served(C, CO) || !s2d_sizes_ok(B, C, CO, H, W)) return 0;
  return align256(smd::conv_s2d_workspace_floats(B, C, CO, H, W)*sizeof(float));
}
int smd_conv3x3s2d_mfma_bwd_data(const float* g_y, const void* wp_bwd, float* g_x, void* workspace, size_t workspace_bytes, int B, int C, int CO, int H, int W, void* stream) {
  if (!g_y || !wp_bwd || !g_x || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::conv_s2_served(C, CO)) return fail(SMD_E_UNSUPPORTED, "the stride-2 kernels serve C %% 16 == 0 with CO %% 32 == 0, not C=%d CO=%d", C, CO);
  if (!s2d_sizes_ok(B, C, CO, H, W)) return fail(SMD_E_UNSUPPORTED, "the stride-2 kernels do not serve B=%d C=%d CO=%d H=%d W=%d", B, C, CO, H, W);
  if (workspace_bytes < smd_conv3x3s2d_mfma_workspace_bytes(B, C, CO, H, W)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_conv_s2_bwd_data(g_y, wp_bwd, g_x, (float*)workspace, B, C, CO, H, W, (hipStream_t)stream), "conv3x3s2d_mfma_bwd_data");
}
int smd_elu_up_cat_pad_fwd(const void* a, const float* bias, const void* skip, void* out, int B, int Ca, int Cs, int h, int w, int dtypes, void* stream) {
  if (!a || !out || (Cs > 0 && !skip)) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || Ca < 1 || Cs < 0 || h < 1 || w < 1 || !dec_sizes_ok((long long)B*(Ca + Cs), 2*h, 2*w))
    return fail(SMD_E_INVALID, "invalid sizes B=%d Ca=%d Cs=%d h=%d w=%d", B, Ca, Cs, h, w);
  return check_launch(smd::launch_elu_up_cat_pad_fwd(a, bias, skip, out, B, Ca, Cs, h, w, dtypes, (hipStream_t)stream), "elu_up_cat_pad_fwd");
}
int smd_elu_up_cat_pad_bwd(const void* a, const float* bias, const void* g_out, void* g_a, void* g_skip, float* g_bias,
                           void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int dtypes, void* stream) {
  if (!a || !g_out || (!g_a && !g_skip) || (g_bias && (!workspace || !g_a))) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || Ca < 1 || Cs < 0 || h < 1 || w < 1 || !dec_sizes_ok((long long)B*(Ca + Cs), 2*h, 2*w))
    return fail(SMD_E_INVALID, "invalid sizes B=%d Ca=%d Cs=%d h=%d w=%d", B, Ca, Cs, h, w);
  if (g_bias && workspace_bytes < smd_decoder_glue_workspace_bytes(B, Ca, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_elu_up_cat_pad_bwd(a, bias, g_out, g_a, g_skip, g_bias, (float*)workspace, B, Ca, Cs, h, w, dtypes, (hipStream_t)stream),
                      "elu_up_cat_pad_bwd");
}

// ------------------------------------------------------------------------------------------------
// BatchNorm (+ residual, + ReLU)
size_t smd_bn_workspace_bytes(int N, int C, int HW) {
  if (N < 1 || C < 1 || HW < 1) return 0;
  return align256(((size_t)C*smd::bn_chunks(N, HW)*3 + (size_t)C*3)*sizeof(float));   // forward: 3 floats per chunk (k_bn_stats); backward: 2
}
int smd_bn_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* running_mean, float* running_var,
               float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
               int N, int C, int HW, void* stream) {
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || C > 65535 || HW < 1 || (long long)N*HW < 2) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d HW=%d", N, C, HW);
  if (workspace_bytes < smd_bn_workspace_bytes(N, C, HW)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_bn_fwd(x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, y, save_mean, save_invstd,
                                         (float*)workspace, N, C, HW, (hipStream_t)stream), "bn_fwd");
}
int smd_bn_bwd(const float* x, const float* y, const float* g_y, const float* gamma, const float* save_mean, const float* save_invstd, int relu,
               float* g_x, float* g_residual, float* g_gamma, float* g_beta, void* workspace, size_t workspace_bytes, int N, int C, int HW,
               void* stream) {
  if (!x || !g_y || !gamma || !save_mean || !save_invstd || !g_x || !g_gamma || !g_beta || !workspace || (relu && !y))
    return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || C > 65535 || HW < 1) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d HW=%d", N, C, HW);
  if (workspace_bytes < smd_bn_workspace_bytes(N, C, HW)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_bn_bwd(x, y, g_y, gamma, save_mean, save_invstd, relu, g_x, g_residual, g_gamma, g_beta, (float*)workspace,
                                         N, C, HW, (hipStream_t)stream), "bn_bwd");
}

int smd_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int C, int H, int W, void* stream) {
  if (!x || !y || !idx) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long long)N*C*(((long long)H*W + 1023)/1024) >= (1ll << 31)) return fail(SMD_E_INVALID, "invalid sizes");
  return check_launch(smd::launch_maxpool_fwd(x, y, idx, (size_t)N*C, H, W, (hipStream_t)stream), "maxpool_fwd");
}
int smd_maxpool3x3s2_bwd(const float* g_y, const uint8_t* idx, float* g_x, int N, int C, int H, int W, void* stream) {
  if (!g_y || !idx || !g_x) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long long)N*C*(((long long)H*W + 1023)/1024) >= (1ll << 31)) return fail(SMD_E_INVALID, "invalid sizes");
  return check_launch(smd::launch_maxpool_bwd(g_y, idx, g_x, (size_t)N*C, H, W, (hipStream_t)stream), "maxpool_bwd");
}

// ------------------------------------------------------------------------------------------------
// CADepth attention blocks (smd_attention.hip)
static bool ca_sizes_ok(int B, int C, int n) {
  return B >= 1 && B < 65536 && C >= 1 && n >= 1 && (n + 63)/64 < 65536 && (long long)B*C*std::max(C, n) < (1ll << 40);
}
size_t smd_channel_attention_workspace_bytes(int B, int C, int n, int backward) {
  if (!ca_sizes_ok(B, C, n)) return 0;
  return align256((size_t)B*C*C*sizeof(float)*(backward ? 2 : 1));
}
int smd_channel_attention_fwd(const float* x, float* out, float* stats, void* workspace, size_t workspace_bytes, int B, int C, int n, void* stream) {
  if (!x || !out || !stats || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!ca_sizes_ok(B, C, n)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d n=%d", B, C, n);
  if (workspace_bytes < smd_channel_attention_workspace_bytes(B, C, n, 0)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_channel_attention_fwd(x, out, stats, (float*)workspace, B, C, n, (hipStream_t)stream), "channel_attention_fwd");
}
int smd_channel_attention_bwd(const float* x, const float* stats, const float* g, float* g_x, void* workspace, size_t workspace_bytes,
                              int B, int C, int n, void* stream) {
  if (!x || !stats || !g || !g_x || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!ca_sizes_ok(B, C, n)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d n=%d", B, C, n);
  if (workspace_bytes < smd_channel_attention_workspace_bytes(B, C, n, 1)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_channel_attention_bwd(x, stats, g, g_x, (float*)workspace, B, C, n, (hipStream_t)stream), "channel_attention_bwd");
}

static bool se_sizes_ok(int B, int C, int HW) {
  return B >= 1 && C >= 1 && HW >= 1 && (long long)B*C*smd::se_chunks(HW) < (1ll << 31) && (long long)C*C < (1ll << 39);
}
size_t smd_se_gate_workspace_bytes(int B, int C, int HW) {
  if (!se_sizes_ok(B, C, HW)) return 0;
  return align256(((((size_t)B*C*smd::se_chunks(HW) + 3) & ~(size_t)3) + (size_t)3*B*C)*sizeof(float));
}
int smd_se_gate_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* save,
                    void* workspace, size_t workspace_bytes, int B, int C, int HW, void* stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !y || !save || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!se_sizes_ok(B, C, HW)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d HW=%d", B, C, HW);
  if (workspace_bytes < smd_se_gate_workspace_bytes(B, C, HW)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_se_gate_fwd(x, w1, b1, w2, b2, y, save, (float*)workspace, B, C, HW, (hipStream_t)stream), "se_gate_fwd");
}
int smd_se_gate_bwd(const float* x, const float* g_y, const float* w1, const float* w2, const float* save, float* g_x, float* g_w1, float* g_b1,
                    float* g_w2, float* g_b2, void* workspace, size_t workspace_bytes, int B, int C, int HW, void* stream) {
  if (!x || !g_y || !w1 || !w2 || !save || !workspace) return fail(SMD_E_INVALID, "null pointer");
  const int np = (g_w1 != nullptr) + (g_b1 != nullptr) + (g_w2 != nullptr) + (g_b2 != nullptr);
  if (np != 0 && np != 4) return fail(SMD_E_INVALID, "the parameter gradients come all four or not at all");
  if (!g_x && np == 0) return fail(SMD_E_INVALID, "nothing to compute");
  if (!se_sizes_ok(B, C, HW)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d HW=%d", B, C, HW);
  if (workspace_bytes < smd_se_gate_workspace_bytes(B, C, HW)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_se_gate_bwd(x, g_y, w1, w2, save, g_x, g_w1, g_b1, g_w2, g_b2, (float*)workspace, B, C, HW, (hipStream_t)stream), "se_gate_bwd");
}

// ------------------------------------------------------------------------------------------------
// The DDVNet output head (smd_ddv.hip): conv3x3 to 128 bins per group + softmax + expectation, the logit volume never written
size_t smd_ddv_head_workspace_bytes(int B, int C, int G, int h, int w) {
  if (!smd::ddv_head_sizes_ok(B, C, G, h, w)) return 0;
  return align256(smd::ddv_head_bias_partials(B, G)*sizeof(float));
}
int smd_ddv_head_fwd(const float* xp, const void* wp_fwd, const float* bias, float* disp, float* stats, int B, int C, int G, int h, int w, void* stream) {
  if (!xp || !wp_fwd || !bias || !disp || !stats) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::ddv_head_sizes_ok(B, C, G, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d G=%d h=%d w=%d (C a multiple of 16, G in 1..4)", B, C, G, h, w);
  return check_launch(smd::launch_ddv_head_fwd(xp, wp_fwd, bias, disp, stats, B, C, G, h, w, (hipStream_t)stream), "ddv_head_fwd");
}
int smd_ddv_head_bwd_logits(const float* xp, const void* wp_fwd, const float* bias, const float* disp, const float* stats, const float* g_disp,
                            float* g_logits, float* g_bias, void* workspace, size_t workspace_bytes, int B, int C, int G, int h, int w, void* stream) {
  if (!xp || !wp_fwd || !bias || !disp || !stats || !g_disp || !g_logits || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!smd::ddv_head_sizes_ok(B, C, G, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d G=%d h=%d w=%d (C a multiple of 16, G in 1..4)", B, C, G, h, w);
  if (workspace_bytes < smd_ddv_head_workspace_bytes(B, C, G, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_ddv_head_bwd_logits(xp, wp_fwd, bias, disp, stats, g_disp, g_logits, g_bias, (float*)workspace, B, C, G, h, w, (hipStream_t)stream),
                      "ddv_head_bwd_logits");
}

// ------------------------------------------------------------------------------------------------
// The DiffNet attention stage in front of its convolution (smd_decoder.hip): up-sample + cat + channel gate + pad, and the ReLU form of the pad glue
size_t smd_up_cat_gate_pad_workspace_bytes(int B, int Ca, int Cs, int h, int w, int R) {
  const smd::UpCatGate s{B, Ca, Cs, h, w, R, 0};
  if (!smd::up_cat_gate_sizes_ok(s)) return 0;
  return align256(smd::up_cat_gate_workspace_floats(s)*sizeof(float));
}
int smd_up_cat_gate_pad_fwd(const float* a, const float* bias_a, const float* skip, const float* w1, const float* w2, float* out, float* gate, float* mean,
                            float* hid, void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int R, int act, void* stream) {
  if (!a || !skip || !w1 || !w2 || !out || !gate || !mean || !hid || !workspace) return fail(SMD_E_INVALID, "null pointer");
  const smd::UpCatGate s{B, Ca, Cs, h, w, R, act};
  if (!smd::up_cat_gate_sizes_ok(s)) return fail(SMD_E_INVALID, "invalid sizes B=%d Ca=%d Cs=%d h=%d w=%d R=%d act=%d", B, Ca, Cs, h, w, R, act);
  if (workspace_bytes < smd_up_cat_gate_pad_workspace_bytes(B, Ca, Cs, h, w, R)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_up_cat_gate_pad_fwd(s, a, bias_a, skip, w1, w2, out, gate, mean, hid, (float*)workspace, (hipStream_t)stream), "up_cat_gate_pad_fwd");
}
int smd_up_cat_gate_pad_bwd(const float* a, const float* bias_a, const float* skip, const float* w1, const float* w2, const float* gate, const float* mean,
                            const float* hid, const float* g_out, float* g_a, float* g_skip, float* g_bias_a, float* g_w1, float* g_w2,
                            void* workspace, size_t workspace_bytes, int B, int Ca, int Cs, int h, int w, int R, int act, void* stream) {
  if (!a || !skip || !w1 || !w2 || !gate || !mean || !hid || !g_out || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if ((g_w1 != nullptr) != (g_w2 != nullptr)) return fail(SMD_E_INVALID, "the gradients of w1 and w2 come both or not at all");
  if (!g_a && !g_skip && !g_bias_a && !g_w1) return fail(SMD_E_INVALID, "nothing to compute");
  const smd::UpCatGate s{B, Ca, Cs, h, w, R, act};
  if (!smd::up_cat_gate_sizes_ok(s)) return fail(SMD_E_INVALID, "invalid sizes B=%d Ca=%d Cs=%d h=%d w=%d R=%d act=%d", B, Ca, Cs, h, w, R, act);
  if (workspace_bytes < smd_up_cat_gate_pad_workspace_bytes(B, Ca, Cs, h, w, R)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_up_cat_gate_pad_bwd(s, a, bias_a, skip, w1, w2, gate, mean, hid, g_out, g_a, g_skip, g_bias_a, g_w1, g_w2, (float*)workspace,
                                                      (hipStream_t)stream), "up_cat_gate_pad_bwd");
}
int smd_relu_pad_fwd(const float* x, const float* bias, float* out, int B, int C, int h, int w, void* stream) {
  if (!x || !out) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || C < 1 || !dec_sizes_ok((long long)B*C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  return check_launch(smd::launch_relu_pad_fwd(x, bias, out, B, C, h, w, (hipStream_t)stream), "relu_pad_fwd");
}
int smd_relu_pad_bwd(const float* x, const float* bias, const float* g_out, float* g_x, float* g_bias, void* workspace, size_t workspace_bytes,
                     int B, int C, int h, int w, void* stream) {
  if (!x || !g_out || !g_x || (g_bias && !workspace)) return fail(SMD_E_INVALID, "null pointer");
  if (B < 1 || C < 1 || !dec_sizes_ok((long long)B*C, h, w)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d h=%d w=%d", B, C, h, w);
  if (g_bias && workspace_bytes < smd_decoder_glue_workspace_bytes(B, C, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_relu_pad_bwd(x, bias, g_out, g_x, g_bias, (float*)workspace, B, C, h, w, (hipStream_t)stream), "relu_pad_bwd");
}

// ------------------------------------------------------------------------------------------------
// The SuperDepth decoder's sub-pixel convolution (smd_subpixel.hip): pre-activation + depth-wise 3x3 to r^2 channels + pixel shuffle + activation [+ cat + pad]
size_t smd_subpixel_workspace_bytes(int B, int C, int Cs, int h, int w, int r, int pad) {
  const smd::SubPixel s{B, C, Cs, h, w, r, 0, 0, pad};
  if (!smd::subpixel_sizes_ok(s)) return 0;
  return align256(smd::subpixel_workspace_floats(s)*sizeof(float));
}
int smd_subpixel_fwd(const float* x, const float* pre_bias, const float* weight, const float* bias, const float* skip, float* out,
                     int B, int C, int Cs, int h, int w, int r, int pre_act, int act, int pad, void* stream) {
  if (!x || !weight || !bias || !out || (Cs > 0 && !skip)) return fail(SMD_E_INVALID, "null pointer");
  const smd::SubPixel s{B, C, Cs, h, w, r, pre_act, act, pad};
  if (!smd::subpixel_sizes_ok(s)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d Cs=%d h=%d w=%d r=%d pre_act=%d act=%d pad=%d", B, C, Cs, h, w, r, pre_act, act, pad);
  return check_launch(smd::launch_subpixel_fwd(s, x, pre_bias, weight, bias, skip, out, (hipStream_t)stream), "subpixel_fwd");
}
int smd_subpixel_bwd(const float* x, const float* pre_bias, const float* weight, const float* out, const float* g_out, float* g_x, float* g_pre_bias,
                     float* g_weight, float* g_bias, float* g_skip, void* workspace, size_t workspace_bytes,
                     int B, int C, int Cs, int h, int w, int r, int pre_act, int act, int pad, void* stream) {
  if (!x || !weight || !g_out || !workspace || (act != 0 && !out) || (g_pre_bias && !pre_bias)) return fail(SMD_E_INVALID, "null pointer");
  if (!g_x && !g_pre_bias && !g_weight && !g_bias && !g_skip) return fail(SMD_E_INVALID, "nothing to compute");
  const smd::SubPixel s{B, C, Cs, h, w, r, pre_act, act, pad};
  if (!smd::subpixel_sizes_ok(s)) return fail(SMD_E_INVALID, "invalid sizes B=%d C=%d Cs=%d h=%d w=%d r=%d pre_act=%d act=%d pad=%d", B, C, Cs, h, w, r, pre_act, act, pad);
  if (g_skip && Cs == 0) return fail(SMD_E_INVALID, "invalid sizes: a skip gradient without skip channels");
  if (workspace_bytes < smd_subpixel_workspace_bytes(B, C, Cs, h, w, r, pad)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_subpixel_bwd(s, x, pre_bias, weight, out, g_out, g_x, g_pre_bias, g_weight, g_bias, g_skip, (float*)workspace,
                                               (hipStream_t)stream), "subpixel_bwd");
}

// ------------------------------------------------------------------------------------------------
// Monodepth's flip-and-blend post-process (smd_blend.hip): every level of a pyramid in one launch
static int blend_fill(smd::BlendSet& bs, const float* const* ramp, const int* hs, const int* ws, int S, int planes, int flags) {
  if (S < 1 || S > SMD_MAX_SCALES) return fail(SMD_E_INVALID, "S=%d outside [1, %d]", S, SMD_MAX_SCALES);
  if (!ramp || !hs || !ws) return fail(SMD_E_INVALID, "null pointer");
  if (planes < 1 || (flags & ~(SMD_BLEND_MIRROR | SMD_BLEND_SCALE))) return fail(SMD_E_INVALID, "invalid sizes planes=%d flags=0x%x", planes, flags);
  for (int s = 0; s < S; ++s) {
    if (hs[s] < 1 || ws[s] < 1) return fail(SMD_E_INVALID, "invalid sizes: level %d is %dx%d", s, hs[s], ws[s]);
    if (!ramp[s]) return fail(SMD_E_INVALID, "null ramp pointer for level %d", s);
  }
  memset(&bs, 0, sizeof(bs));
  if (smd::blend_plan(bs, hs, ws, S, planes) < 1) return fail(SMD_E_INVALID, "invalid sizes: a level of 2^31 elements or more");
  for (int s = 0; s < S; ++s) bs.ramp[s] = ramp[s];
  return SMD_OK;
}
int smd_flip_blend_fwd(const float* const* l, const float* const* r, const float* const* ramp, float* const* out, const int* hs, const int* ws,
                       int S, int planes, int flags, float scale, float offset, void* stream) {
  if (!l || !r || !out) return fail(SMD_E_INVALID, "null pointer");
  smd::BlendSet bs;
  if (int rc = blend_fill(bs, ramp, hs, ws, S, planes, flags)) return rc;
  for (int s = 0; s < S; ++s) {
    if (!l[s] || !r[s] || !out[s]) return fail(SMD_E_INVALID, "null pointer for level %d", s);
    bs.a[s] = l[s]; bs.b[s] = r[s]; bs.o0[s] = out[s];
  }
  return check_launch(smd::launch_flip_blend_fwd(bs, flags, scale, offset, (hipStream_t)stream), "flip_blend_fwd");
}
int smd_flip_blend_bwd(const float* const* g_out, const float* const* ramp, float* const* g_l, float* const* g_r, const int* hs, const int* ws,
                       int S, int planes, int flags, float scale, void* stream) {
  if (!g_out) return fail(SMD_E_INVALID, "null pointer");
  smd::BlendSet bs;
  if (int rc = blend_fill(bs, ramp, hs, ws, S, planes, flags)) return rc;
  bool any = false;
  for (int s = 0; s < S; ++s) {
    if (!g_out[s]) return fail(SMD_E_INVALID, "null pointer for level %d", s);
    bs.a[s] = g_out[s]; bs.o0[s] = g_l ? g_l[s] : nullptr; bs.o1[s] = g_r ? g_r[s] : nullptr;
    any = any || bs.o0[s] || bs.o1[s];
  }
  if (!any) return fail(SMD_E_INVALID, "nothing to compute");
  return check_launch(smd::launch_flip_blend_bwd(bs, flags, scale, (hipStream_t)stream), "flip_blend_bwd");
}

// ------------------------------------------------------------------------------------------------
// FeatDepth's feature regularisers (smd_featreg.hip): every level of a feature pyramid in one launch
static int feat_regs_fill(smd::FeatRegSet& fs, const float* const* feat, const float* const* img, const int* Cs, const int* hs, const int* ws, int S, int B, int flags) {
  if (S < 1 || S > SMD_MAX_SCALES) return fail(SMD_E_INVALID, "S=%d outside [1, %d]", S, SMD_MAX_SCALES);
  if (!feat || !img || !Cs || !hs || !ws) return fail(SMD_E_INVALID, "null pointer");
  const int all = SMD_FEATREG_PEAKY_EDGES | SMD_FEATREG_SMOOTH_EDGES | SMD_FEATREG_PEAKY | SMD_FEATREG_SMOOTH;
  if (B < 1 || (flags & ~all) || !(flags & (SMD_FEATREG_PEAKY | SMD_FEATREG_SMOOTH))) return fail(SMD_E_INVALID, "invalid sizes B=%d flags=0x%x", B, flags);
  for (int s = 0; s < S; ++s) {
    if (Cs[s] < 1 || hs[s] < 1 || ws[s] < 1) return fail(SMD_E_INVALID, "invalid sizes: level %d is %dx%dx%d", s, Cs[s], hs[s], ws[s]);
    if (!feat[s] || !img[s]) return fail(SMD_E_INVALID, "null pointer for level %d", s);
  }
  memset(&fs, 0, sizeof(fs));
  if (smd::feat_regs_plan(fs, Cs, hs, ws, S, B) < 1) return fail(SMD_E_INVALID, "invalid sizes: a level of 2^31 elements or more");
  for (int s = 0; s < S; ++s) {
    fs.L[s].x = feat[s]; fs.L[s].img = img[s];
    fs.L[s].vec_x = ws[s] % 4 == 0 && (uintptr_t)feat[s] % 16 == 0;
    fs.L[s].vec_img = ws[s] % 4 == 0 && (uintptr_t)img[s] % 16 == 0;
  }
  return SMD_OK;
}
size_t smd_feat_regs_workspace_bytes(const int* Cs, const int* hs, const int* ws, int S, int B) {
  if (!Cs || !hs || !ws || S < 1 || S > SMD_MAX_SCALES || B < 1) return 0;
  for (int s = 0; s < S; ++s) if (Cs[s] < 1 || hs[s] < 1 || ws[s] < 1) return 0;
  smd::FeatRegSet fs;
  memset(&fs, 0, sizeof(fs));
  const long units = smd::feat_regs_plan(fs, Cs, hs, ws, S, B);
  return units < 1 ? 0 : align256((size_t)units*2*sizeof(double));
}
int smd_feat_regs_fwd(const float* const* feat, const float* const* img, const int* Cs, const int* hs, const int* ws, int S, int B, int flags,
                      float* out_peaky, float* out_smooth, void* workspace, size_t workspace_bytes, void* stream) {
  if (!out_peaky || !out_smooth || !workspace) return fail(SMD_E_INVALID, "null pointer");
  smd::FeatRegSet fs;
  if (int rc = feat_regs_fill(fs, feat, img, Cs, hs, ws, S, B, flags)) return rc;
  if (workspace_bytes < (size_t)fs.units*2*sizeof(double)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_feat_regs_fwd(fs, flags, (double*)workspace, out_peaky, out_smooth, (hipStream_t)stream), "feat_regs_fwd");
}
int smd_feat_regs_bwd(const float* const* feat, const float* const* img, const float* g_peaky, const float* g_smooth, float* const* g_feat,
                      const int* Cs, const int* hs, const int* ws, int S, int B, int flags, void* stream) {
  if (!g_feat) return fail(SMD_E_INVALID, "null pointer");
  if (!g_peaky && !g_smooth) return fail(SMD_E_INVALID, "nothing to compute");
  if ((g_peaky && !(flags & SMD_FEATREG_PEAKY)) || (g_smooth && !(flags & SMD_FEATREG_SMOOTH))) return fail(SMD_E_INVALID, "a gradient for a loss that was not computed (flags=0x%x)", flags);
  smd::FeatRegSet fs;
  if (int rc = feat_regs_fill(fs, feat, img, Cs, hs, ws, S, B, flags)) return rc;
  for (int s = 0; s < S; ++s) {
    if (!g_feat[s]) return fail(SMD_E_INVALID, "null g_feat pointer for level %d", s);
    fs.L[s].gx = g_feat[s];
    fs.L[s].vec_gx = ws[s] % 4 == 0 && (uintptr_t)g_feat[s] % 16 == 0;
  }
  return check_launch(smd::launch_feat_regs_bwd(fs, flags, g_peaky, g_smooth, (hipStream_t)stream), "feat_regs_bwd");
}

// ------------------------------------------------------------------------------------------------
// Depth-Hints regression over all scales (smd_hints.hip)
static const int kHintsFlags = SMD_REGR_LOG_L1 | SMD_REGR_BERHU | SMD_REGR_INVERT | SMD_REGR_AUTOMASK;
static bool hints_sizes_ok(int S, int b, int h, int w) {
  return S >= 1 && S <= SMD_MAX_SCALES && b >= 1 && h >= 1 && w >= 1 && (size_t)b*h*w < ((size_t)1 << 31);
}
size_t smd_hints_regr_workspace_bytes(int S, int b, int h, int w) {
  if (!hints_sizes_ok(S, b, h, w)) return 0;
  return align256((size_t)smd::hints_blocks((size_t)b*h*w)*4*sizeof(double));
}
int smd_hints_regr_fwd(const float* depth, const float* hints, const float* err, int S, int b, int h, int w, int flags, float* loss, uint8_t* mask0,
                       uint32_t* bits, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!depth || !hints || !loss || !mask0 || !bits || !stats || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!hints_sizes_ok(S, b, h, w)) return fail(SMD_E_INVALID, "invalid sizes S=%d b=%d h=%d w=%d", S, b, h, w);
  if ((flags & ~kHintsFlags) || ((flags & SMD_REGR_LOG_L1) && (flags & SMD_REGR_BERHU))) return fail(SMD_E_INVALID, "invalid flags 0x%x", flags);
  if (((flags & SMD_REGR_AUTOMASK) != 0) != (err != nullptr)) return fail(SMD_E_INVALID, "err goes with SMD_REGR_AUTOMASK (flags=0x%x, err %s)", flags, err ? "given" : "NULL");
  if ((uintptr_t)bits % 4 || (uintptr_t)workspace % 8) return fail(SMD_E_INVALID, "bits needs 4-byte, the workspace 8-byte alignment");
  if (workspace_bytes < smd_hints_regr_workspace_bytes(S, b, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  const size_t P = (size_t)b*h*w;
  const int vec = P % 4 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)hints % 16 == 0 && (uintptr_t)err % 16 == 0 && (uintptr_t)mask0 % 4 == 0;
  return check_launch(smd::launch_hints_regr_fwd(depth, hints, err, S, P, flags, vec, loss, mask0, bits, stats, (double*)workspace, (hipStream_t)stream), "hints_regr_fwd");
}
int smd_hints_regr_bwd(const float* depth, const float* hints, const uint32_t* bits, const float* stats, const float* g_loss, float* g_depth,
                       int S, int b, int h, int w, int flags, void* stream) {
  if (!depth || !hints || !bits || !stats || !g_loss || !g_depth) return fail(SMD_E_INVALID, "null pointer");
  if (!hints_sizes_ok(S, b, h, w)) return fail(SMD_E_INVALID, "invalid sizes S=%d b=%d h=%d w=%d", S, b, h, w);
  if ((flags & ~kHintsFlags) || ((flags & SMD_REGR_LOG_L1) && (flags & SMD_REGR_BERHU))) return fail(SMD_E_INVALID, "invalid flags 0x%x", flags);
  if ((uintptr_t)bits % 4) return fail(SMD_E_INVALID, "bits needs 4-byte alignment");
  const size_t P = (size_t)b*h*w;
  const int vec = P % 4 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)hints % 16 == 0 && (uintptr_t)g_depth % 16 == 0;
  return check_launch(smd::launch_hints_regr_bwd(depth, hints, bits, S, P, flags, vec, stats, g_loss, g_depth, (hipStream_t)stream), "hints_regr_bwd");
}

// ------------------------------------------------------------------------------------------------
// Feature-metric reconstruction loss from the low-resolution features (smd_featrecon.hip).  Workspace: one double per block | the pose sums, 16-byte aligned
// inside it whatever the base (the finalize reads them as 16-byte vectors).
static const int kFeatReconFlags = SMD_LOSS_L1 | SMD_LOSS_L2 | SMD_USE_MIN | SMD_USE_AUTOMASK;
static size_t feat_recon_part_bytes(int b, int H, int W) { return align256((size_t)smd::feat_recon_blocks(b, H, W)*sizeof(double)); }
static float* feat_recon_pose_partial(void* workspace, int b, int H, int W) {
  return (float*)(((uintptr_t)workspace + feat_recon_part_bytes(b, H, W) + 15) & ~(uintptr_t)15);
}
static int feat_recon_check(int b, int n, int C, int H, int W, int hf, int wf, int flags, const void* workspace, size_t workspace_bytes) {
  if (b < 1 || n < 1 || C < 1 || H < 2 || W < 2 || hf < 1 || wf < 1) return fail(SMD_E_INVALID, "invalid sizes b=%d n=%d C=%d H=%d W=%d hf=%d wf=%d (need H, W >= 2)", b, n, C, H, W, hf, wf);
  if (hf > H || wf > W) return fail(SMD_E_INVALID, "features larger than the depth map (%dx%d vs. %dx%d): the operator up-samples", hf, wf, H, W);
  if ((size_t)b*H*W >= ((size_t)1 << 31)) return fail(SMD_E_INVALID, "b*H*W must stay below 2^31");
  if (!smd::feat_recon_sizes_ok(b, n, C, H, W, hf, wf)) return fail(SMD_E_INVALID, "sizes that are not served b=%d n=%d C=%d H=%d W=%d hf=%d wf=%d (n <= %d, H, W <= 2048, n*b*C*hf*wf*4 < 2^32)", b, n, C, H, W, hf, wf, SMD_MAX_SUPPORTS);
  if ((flags & ~kFeatReconFlags) || ((flags & SMD_LOSS_L1) != 0) == ((flags & SMD_LOSS_L2) != 0)) return fail(SMD_E_INVALID, "invalid flags 0x%x (one of SMD_LOSS_L1, SMD_LOSS_L2)", flags);
  if ((uintptr_t)workspace % 8) return fail(SMD_E_INVALID, "the workspace needs 8-byte alignment");
  if (workspace_bytes < smd_feat_recon_workspace_bytes(b, n, C, H, W, hf, wf)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return SMD_OK;
}
size_t smd_feat_recon_workspace_bytes(int b, int n, int C, int H, int W, int hf, int wf) {
  if (!smd::feat_recon_sizes_ok(b, n, C, H, W, hf, wf)) return 0;
  return feat_recon_part_bytes(b, H, W) + align256((size_t)n*smd::feat_recon_blocks(b, H, W)*smd::kPoseSums*sizeof(float)) + 16;
}
int smd_feat_recon_fwd(const float* depth, const float* feat, const float* supp_feat, const float* T, const float* K, const float* K_inv, const float* noise,
                       uint64_t seed, float* loss, uint8_t* sel, float* warp, void* workspace, size_t workspace_bytes, int b, int n, int C, int H, int W,
                       int hf, int wf, int flags, void* stream) {
  if (!depth || !feat || !supp_feat || !T || !K || !K_inv || !loss || !sel || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = feat_recon_check(b, n, C, H, W, hf, wf, flags, workspace, workspace_bytes)) return rc;
  return check_launch(smd::launch_feat_recon_fwd(depth, feat, supp_feat, T, K, K_inv, noise, seed, loss, sel, warp, (double*)workspace, b, n, C, H, W, hf, wf, flags,
                                                 (hipStream_t)stream), "feat_recon_fwd");
}
int smd_feat_recon_bwd(const float* depth, const float* feat, const float* supp_feat, const float* T, const float* K, const float* K_inv, const uint8_t* sel,
                       const float* g_loss, float* g_depth, float* g_T, void* workspace, size_t workspace_bytes, int b, int n, int C, int H, int W, int hf, int wf,
                       int flags, void* stream) {
  if (!depth || !feat || !supp_feat || !T || !K || !K_inv || !sel || !g_loss || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!g_depth && !g_T) return fail(SMD_E_INVALID, "nothing to compute: neither g_depth nor g_T is asked for");
  if (int rc = feat_recon_check(b, n, C, H, W, hf, wf, flags, workspace, workspace_bytes)) return rc;
  return check_launch(smd::launch_feat_recon_bwd(depth, feat, supp_feat, T, K, K_inv, sel, g_loss, g_depth, g_T, feat_recon_pose_partial(workspace, b, H, W), b, n, C, H, W,
                                                 hf, wf, flags, (hipStream_t)stream), "feat_recon_bwd");
}

// ------------------------------------------------------------------------------------------------
// Image reconstruction loss with a predictive weighting mask (smd_maskrecon.hip).  Workspace: one double per block | the pose sums, 16-byte aligned inside it
// whatever the base (the finalize reads them as 16-byte vectors).
static const int kMaskReconFlags = SMD_LOSS_L1 | SMD_USE_MIN | SMD_USE_AUTOMASK | SMD_MASK_EXPLAINABILITY | SMD_MASK_UNCERTAINTY;
static size_t mask_recon_part_bytes(int S, int b, int h, int w) { return align256((size_t)smd::mask_recon_tiles(h, w)*S*b*sizeof(double)); }
static float* mask_recon_pose_partial(void* workspace, int S, int b, int h, int w) {
  return (float*)(((uintptr_t)workspace + mask_recon_part_bytes(S, b, h, w) + 15) & ~(uintptr_t)15);
}
static int mask_recon_check(int S, int b, int n, int h, int w, int flags, const void* workspace, size_t workspace_bytes) {
  if (!smd::mask_recon_sizes_ok(S, b, n, h, w))
    return fail(SMD_E_UNSUPPORTED, "the masked reconstruction does not serve S=%d b=%d n=%d h=%d w=%d (S <= %d, n <= %d, 2 <= h, w <= 2048, S*b*h*w < 2^31)", S, b, n, h, w,
                SMD_MAX_SCALES, SMD_MAX_SUPPORTS);
  if ((flags & ~kMaskReconFlags) || ((flags & SMD_MASK_EXPLAINABILITY) != 0) == ((flags & SMD_MASK_UNCERTAINTY) != 0))
    return fail(SMD_E_UNSUPPORTED, "the masked reconstruction does not serve flags 0x%x (exactly one of SMD_MASK_EXPLAINABILITY, SMD_MASK_UNCERTAINTY)", flags);
  if ((uintptr_t)workspace % 8) return fail(SMD_E_INVALID, "the workspace needs 8-byte alignment");
  if (workspace_bytes < smd_mask_recon_workspace_bytes(S, b, n, h, w)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return SMD_OK;
}
size_t smd_mask_recon_workspace_bytes(int S, int b, int n, int h, int w) {
  if (!smd::mask_recon_sizes_ok(S, b, n, h, w)) return 0;
  return mask_recon_part_bytes(S, b, h, w) + align256((size_t)n*b*S*smd::mask_recon_tiles(h, w)*smd::kPoseSums*sizeof(float)) + 16;
}
int smd_mask_recon_fwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                       const float* noise, uint64_t seed, float* loss, uint8_t* sel, uint8_t* stat, float* warp0, void* workspace, size_t workspace_bytes,
                       int S, int b, int n, int h, int w, int flags, void* stream) {
  if (!depth || !mask || !tgt || !supp || !T || !K || !K_inv || !loss || !sel || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (int rc = mask_recon_check(S, b, n, h, w, flags, workspace, workspace_bytes)) return rc;
  if ((flags & SMD_USE_MIN) && (flags & SMD_USE_AUTOMASK) && !stat) return fail(SMD_E_INVALID, "min + automask: `stat` (the static winner) is an output");
  return check_launch(smd::launch_mask_recon_fwd(depth, mask, tgt, supp, T, K, K_inv, noise, seed, loss, sel, stat, warp0, (double*)workspace, S, b, n, h, w, flags,
                                                 (hipStream_t)stream), "mask_recon_fwd");
}
int smd_mask_recon_bwd(const float* depth, const float* mask, const float* tgt, const float* supp, const float* T, const float* K, const float* K_inv,
                       const uint8_t* sel, const uint8_t* stat, const float* g_loss, float* g_depth, float* g_mask, float* g_T, void* workspace,
                       size_t workspace_bytes, int S, int b, int n, int h, int w, int flags, void* stream) {
  if (!depth || !mask || !tgt || !supp || !T || !K || !K_inv || !sel || !g_loss || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!g_depth && !g_mask && !g_T) return fail(SMD_E_INVALID, "nothing to compute: none of g_depth, g_mask, g_T is asked for");
  if (int rc = mask_recon_check(S, b, n, h, w, flags, workspace, workspace_bytes)) return rc;
  if ((flags & SMD_USE_MIN) && (flags & SMD_USE_AUTOMASK) && !stat) return fail(SMD_E_INVALID, "min + automask: `stat` (the static winner) is an input");
  return check_launch(smd::launch_mask_recon_bwd(depth, mask, tgt, supp, T, K, K_inv, sel, stat, g_loss, g_depth, g_mask, g_T,
                                                 mask_recon_pose_partial(workspace, S, b, h, w), S, b, n, h, w, flags, (hipStream_t)stream), "mask_recon_bwd");
}

// ------------------------------------------------------------------------------------------------
// Depthwise 7x7 convolution (ConvNeXt)
static bool dw_sizes_ok(int N, int C, int H, int W) {
  return N >= 1 && C >= 1 && H >= 1 && W >= 1 && (long long)N*C*smd::dwconv_tiles(H, W) < (1ll << 31) && (long long)H*W < (1ll << 30);
}
size_t smd_dwconv7x7_workspace_bytes(int C, int H, int W) {
  if (C < 1 || H < 1 || W < 1) return 0;
  return align256((size_t)C*smd::dwconv_tiles(H, W)*50*sizeof(float));
}
int smd_dwconv7x7_fwd(const float* x, const float* weight, const float* bias, float* y, int N, int C, int H, int W, int flip, void* stream) {
  if (!x || !weight || !y) return fail(SMD_E_INVALID, "null pointer");
  if (!dw_sizes_ok(N, C, H, W)) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d H=%d W=%d", N, C, H, W);
  return check_launch(smd::launch_dwconv7(x, weight, bias, y, N, C, H, W, flip, (hipStream_t)stream), "dwconv7x7_fwd");
}
int smd_dwconv7x7_wrw(const float* x, const float* g_y, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, void* stream) {
  if (!x || !g_y || !g_weight || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (!dw_sizes_ok(N, C, H, W)) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d H=%d W=%d", N, C, H, W);
  if (workspace_bytes < smd_dwconv7x7_workspace_bytes(C, H, W)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_dwconv7_wrw(x, g_y, g_weight, g_bias, (float*)workspace, N, C, H, W, (hipStream_t)stream), "dwconv7x7_wrw");
}

// ------------------------------------------------------------------------------------------------
// Channel LayerNorm on NCHW (ConvNeXt)
size_t smd_layernorm_cf_workspace_bytes(int N, int C, int HW) {
  if (N < 1 || C < 1 || HW < 1) return 0;
  return align256((size_t)smd::ln_cf_chunks((size_t)N*HW)*C*2*sizeof(float));
}
int smd_layernorm_cf_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_is_bf16, float* mean, float* rstd, int N, int C, int HW,
                         float eps, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !rstd) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || HW < 1 || (long long)N*HW >= (1ll << 38)) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d HW=%d", N, C, HW);
  return check_launch(smd::launch_ln_cf_fwd(x, gamma, beta, y, y_is_bf16, mean, rstd, N, C, HW, eps, (hipStream_t)stream), "layernorm_cf_fwd");
}
int smd_layernorm_cf_bwd(const float* x, const void* g_y, int g_y_is_bf16, const float* gamma, const float* mean, const float* rstd, float* g_x, float* g_gamma,
                         float* g_beta, void* workspace, size_t workspace_bytes, int N, int C, int HW, void* stream) {
  if (!x || !g_y || !gamma || !mean || !rstd || !g_x || !g_gamma || !g_beta || !workspace) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1 || C < 1 || C > 32767 || HW < 1) return fail(SMD_E_INVALID, "invalid sizes N=%d C=%d HW=%d", N, C, HW);
  if (workspace_bytes < smd_layernorm_cf_workspace_bytes(N, C, HW)) return fail(SMD_E_WORKSPACE, "workspace too small");
  return check_launch(smd::launch_ln_cf_bwd(x, g_y, g_y_is_bf16, gamma, mean, rstd, g_x, g_gamma, g_beta, (float*)workspace, N, C, HW, (hipStream_t)stream),
                      "layernorm_cf_bwd");
}

// ------------------------------------------------------------------------------------------------
// Pose / intrinsics prologue
int smd_pose_fwd(const float* aa, const float* t, const uint8_t* invert, int N, float* T, void* stream) {
  if (!aa || !t || !T) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1) return fail(SMD_E_INVALID, "invalid size N=%d", N);
  return check_launch(smd::launch_pose_fwd(aa, t, invert, N, T, (hipStream_t)stream), "pose_fwd");
}
int smd_pose_bwd(const float* aa, const float* t, const uint8_t* invert, int N, const float* g_T, float* g_aa, float* g_t, void* stream) {
  if (!aa || !t || !g_T || !g_aa || !g_t) return fail(SMD_E_INVALID, "null pointer");
  if (N < 1) return fail(SMD_E_INVALID, "invalid size N=%d", N);
  return check_launch(smd::launch_pose_bwd(aa, t, invert, N, g_T, g_aa, g_t, (hipStream_t)stream), "pose_bwd");
}
int smd_intrinsics_fwd(const float* fs, const float* cs, const float* K_in, int b, int h, int w, float* K, float* K_inv, void* stream) {
  if (!K_inv || (fs && (!cs || !K)) || (!fs && !K_in)) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1) return fail(SMD_E_INVALID, "invalid sizes");
  return check_launch(smd::launch_intrinsics_fwd(fs, cs, K_in, b, h, w, K, K_inv, (hipStream_t)stream), "intrinsics_fwd");
}
int smd_intrinsics_bwd(const float* fs, const float* cs, int b, int h, int w, const float* g_K, const float* g_Kinv,
                       float* g_fs, float* g_cs, void* stream) {
  if (!fs || !cs || !g_K || !g_Kinv || !g_fs || !g_cs) return fail(SMD_E_INVALID, "null pointer");
  if (b < 1 || h < 1 || w < 1) return fail(SMD_E_INVALID, "invalid sizes");
  return check_launch(smd::launch_intrinsics_bwd(fs, cs, b, h, w, g_K, g_Kinv, g_fs, g_cs, (hipStream_t)stream), "intrinsics_bwd");
}

// ------------------------------------------------------------------------------------------------
// Aspect-ratio augmentation
int smd_crop_resize(const float* const* src, float* const* dst, const int* planes, int nseg, int H, int W, int crop_h, int crop_w,
                    int out_h, int out_w, const float* K_in, float* K_out, int nK, void* stream) {
  if (!src || !dst || !planes) return fail(SMD_E_INVALID, "null pointer");
  if (nseg < 1 || nseg > smd::SMD_MAX_AR_SEGMENTS) return fail(SMD_E_INVALID, "nseg=%d outside [1, %d]", nseg, smd::SMD_MAX_AR_SEGMENTS);
  if (H < 2 || W < 2 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W || out_h < 1 || out_w < 1)
    return fail(SMD_E_INVALID, "invalid sizes: input %dx%d, crop %dx%d, output %dx%d", H, W, crop_h, crop_w, out_h, out_w);
  if ((K_in != nullptr) != (K_out != nullptr) || (K_in && nK < 1)) return fail(SMD_E_INVALID, "K_in / K_out / nK must be given together");
  smd::CropResizeArgs a;
  memset(&a, 0, sizeof(a));
  long long total = 0;
  for (int k = 0; k < nseg; ++k) {
    if (!src[k] || !dst[k] || planes[k] < 1) return fail(SMD_E_INVALID, "segment %d: null pointer or no planes", k);
    a.src[k] = src[k]; a.dst[k] = dst[k]; a.planes[k] = planes[k]; a.first_plane[k] = (int)total;
    total += planes[k];
  }
  if (total + 1 > 65535) return fail(SMD_E_INVALID, "too many image planes for one launch (%lld)", total);
  a.nseg = nseg; a.H = H; a.W = W; a.ch = crop_h; a.cw = crop_w; a.oh = out_h; a.ow = out_w;
  // kornia.geometry.transform.center_crop: start = int(src/2 - dst/2) (truncation); the window is then RESAMPLED (smd_aspect.hip), unless
  // it is the whole frame — the augmentation's resize-only branch (src/core/aspect_ratio.py:60)
  a.y0 = (int)((double)H/2.0 - (double)crop_h/2.0); a.x0 = (int)((double)W/2.0 - (double)crop_w/2.0);
  a.resample = (crop_h != H || crop_w != W) ? 1 : 0;
  a.K_in = K_in; a.K_out = K_out; a.nK = nK;
  return check_launch(smd::launch_crop_resize(a, (hipStream_t)stream), "crop_resize");
}

int smd_profile_enable(int which, int capacity) {
  if (which < 0 || which > 4 || capacity < 0) return fail(SMD_E_INVALID, "bad profile slot");
  ProfSlot& p = g_prof[which];
  for (int i = 0; i < 2*p.cap; ++i) (void)hipEventDestroy(p.ev[i]);
  delete[] p.ev;
  p = ProfSlot();
  if (capacity == 0) return SMD_OK;
  p.ev = new hipEvent_t[2*capacity];
  for (int i = 0; i < 2*capacity; ++i)
    if (hipEventCreate(&p.ev[i]) != hipSuccess) return fail(SMD_E_LAUNCH, "hipEventCreate failed");
  p.cap = capacity;
  return SMD_OK;
}

int smd_profile_collect(int which, float* ms_out, int max_out, int* n_out) {
  if (which < 0 || which > 4 || !ms_out || !n_out) return fail(SMD_E_INVALID, "bad profile arguments");
  ProfSlot& p = g_prof[which];
  int n = 0;
  for (int i = 0; i < p.used && n < max_out; ++i) {
    if (hipEventSynchronize(p.ev[2*i + 1]) != hipSuccess) return fail(SMD_E_LAUNCH, "hipEventSynchronize failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.ev[2*i], p.ev[2*i + 1]) != hipSuccess) return fail(SMD_E_LAUNCH, "hipEventElapsedTime failed");
    ms_out[n++] = ms;
  }
  p.used = 0;
  *n_out = n;
  return SMD_OK;
}

int smd_debug_stream_copy(const void* src, void* dst, size_t nbytes, int mode, void* stream) {
  if (!src || !dst) return fail(SMD_E_INVALID, "null pointer");
  if (nbytes < 16 || (nbytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return fail(SMD_E_INVALID, "size and pointers must be multiples of 16");
  return check_launch(smd::launch_stream_copy(src, dst, nbytes, mode, (hipStream_t)stream), "stream_copy");
}

int smd_debug_lane_shift(float* out_left, float* out_right, void* stream) {
  if (!out_left || !out_right) return fail(SMD_E_INVALID, "null pointer");
  return check_launch(smd::launch_debug_lane_shift(out_left, out_right, (hipStream_t)stream), "debug_lane_shift");
}

}  // extern "C"
