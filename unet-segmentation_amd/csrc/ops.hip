// Per-op C-ABI entry points (include/unet_hip.h): single reference ops on
// caller buffers, built from the same kernels the network plan schedules.
// They exist for op-level parity tests and for callers that compose their own
// graph; the training path uses unet_plan_*.
#include <algorithm>
#include <cerrno>
#include <string>

#include "../../include/unet_hip.h"
#include "unet_internal.h"

using namespace unet;

namespace unet {
extern int g_tune_igemm, g_tune_wgrad, g_autotune, g_force_split, g_force_tile, g_concurrent, g_wino_max,
    g_wino_dgrad_max, g_wino_wgrad_max, g_bf16_norm, g_bn_fold, g_wino4_fwd_min_cg, g_wino4_fwd_small_cg,
    g_maxpool_vec8, g_wgrad_fwd_u, g_ctc_chunk_frames, g_ctc_dense_cells, g_region_lds_objects, g_link_lds_objects;
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s);
hipError_t launch_pair_sum(const double* st, int g, int c, float* out, hipStream_t s);
}  // namespace unet

namespace {
thread_local std::string g_op_err;
inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
// unet_set_tuning("op_precision", UNET_PREC_*): GEMM arithmetic of the per-op
// entry points (the plan has its own, unet_plan_create_ex)
int g_op_prec = UNET_PREC_FP32;
// unet_set_tuning("op_a16", 1): with op_precision UNET_PREC_BF16 the 3x3
// conv entry points store their A operand in bf16 first, as a bf16 plan does
// (raw conv outputs and padded dY are bf16 there): the conv forward rounds x to
// bf16 before its BN+ReLU transform, the input gradient stores the padded dY
// bf16.  Lets op-level tests and tools run the plan's exact GEMM configuration.
int g_op_a16 = 0;
// unet_set_tuning("op_strict", 1): a forced tile ("igemm_variant" > 0, or a
// unet_gemm_site descriptor's tile / split) that does not apply to a per-op
// call is -EINVAL before anything is launched, instead of the built-in tile
// running in its place (tests: the only way to know which tile ran)
int g_op_strict = 0;

// the K-chunk quantum launch_igemm holds a call with forced tile t to
int op_quantum(const IgemmTile* t) { return t && t->family == IgemmFamily::WinoFused && t->wino_m == 2 ? 8 : 16; }
// a as the GEMM will see it: packed B in op_precision's planes (pointers only)
IgemmArgs op_as_launched(IgemmArgs a) {
  if (g_op_prec != UNET_PREC_FP32 && a.b) {
    a.bh = reinterpret_cast<const uint16_t*>(a.b);
    a.bl = g_op_prec == UNET_PREC_BF16X3 ? a.bh : nullptr;
    a.b = nullptr;
  }
  return a;
}
// tile `id` applies to the call: its fits() and launch_igemm's channel quantum
bool op_tile_applies(const IgemmArgs& a0, int id) {
  const IgemmArgs a = op_as_launched(a0);
  const int q = op_quantum(igemm_tile(id));
  return igemm_tile_fits(a, id) && a.K % q == 0 && a.a.Cg % q == 0 && a.a.c_split % q == 0;
}
// op_strict: false when "igemm_variant" forces a tile that does not apply to a
bool op_forced_ok(const IgemmArgs& a) { return !g_op_strict || g_tune_igemm <= 0 || op_tile_applies(a, g_tune_igemm); }

// bf16 / split per-op GEMMs: round the packed fp32 B (n elements) into
// `scratch` (4n bytes: hi plane, then the lo plane of split operands) and point
// the GEMM at it
hipError_t op_b_to_bf16(IgemmArgs& a, size_t n, void* scratch, hipStream_t s) {
  if (g_op_prec == UNET_PREC_FP32) return hipSuccess;
  uint16_t* bh = reinterpret_cast<uint16_t*>(scratch);
  uint16_t* bl = g_op_prec == UNET_PREC_BF16X3 ? bh + n : nullptr;
  hipError_t e = launch_f2bf(a.b, bh, n, s, bl);
  a.bh = bh;
  a.bl = bl;
  a.b = nullptr;
  return e;
}
}  // namespace

namespace {
// dz = dy where the (ReLU) output y > 0, else 0 (torch's threshold_backward on
// the output, nn.ReLU(inplace=True) of models/unet_model.py:13, 17)
__global__ void k_relu_mask(const float* __restrict__ dy, const float* __restrict__ y, long long n4,
                            float* __restrict__ dz) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 g = reinterpret_cast<const float4*>(dy)[i], v = reinterpret_cast<const float4*>(y)[i];
    reinterpret_cast<float4*>(dz)[i] =
        make_float4(v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f);
  }
}

// eval-mode BatchNorm statistics: the running ones (invstd as k_bn_eval_prepare)
__global__ void k_bn_eval_stats(int C, const float* rm, const float* rv, float eps, float* mean, float* invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = rm[c];
  invstd[c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
}
}  // namespace

#define OPCK(x)                                                           \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) return e_ == hipErrorInvalidValue ? -EINVAL : -EIO; \
  } while (0)

extern "C" {

// transformed weights of the fused Winograd tiles (72, 73, 75, 76) for forced
// per-op GEMMs (tests: unet_set_tuning("igemm_variant", t)); the built-in
// choice of the per-op entry points never takes a Winograd tile
// (+ 256 B: the claim counters of the persistent forms, behind V)
static size_t op_wino_bytes(int ci, int co) { return al256(sizeof(float) * 36 * (size_t)ci * co) + 256; }
static size_t op_wgrad_wino_bytes(int n, int h, int w, int ci, int co);
static size_t op_wgrad_extra_bytes(int n, int h, int w, int ci, int co);
// A forced unfused Winograd tile (70, 71: U, M and V in HBM) borrows the scratch
// unet_conv_ws_bytes reserves for a forced Winograd weight gradient instead: it
// holds the larger of F(2x2) / F(4x4) / F(6x6) over the n x h x w grid, which
// covers the forward's (h - 2) x (w - 2) and the input gradient's h x w tiles
// (the size is symmetric in Cg and N).
static void op_set_wino(IgemmArgs& a, void* ws, int n, int h, int w, int ci, int co) {
  const size_t ws_bytes = unet_conv_ws_bytes(n, h, w, ci, co);
  const IgemmTile* forced = igemm_tile(g_tune_igemm);
  if (forced && forced->family == IgemmFamily::Wino && op_wgrad_extra_bytes(n, h, w, ci, co)) {
    a.wino_ws = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + ws_bytes - op_wino_bytes(ci, co) -
                                         op_wgrad_extra_bytes(n, h, w, ci, co));
    a.wino_ws_bytes = op_wgrad_wino_bytes(n, h, w, ci, co);
    return;
  }
  a.wino_ws = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + ws_bytes - op_wino_bytes(ci, co));
  a.wino_ws_bytes = op_wino_bytes(ci, co);
}

// Scratch of a forced Winograd weight gradient in unet_conv3x3_wgrad (tests:
// wgrad_variant 71 / 74, 1071 / 1074; the built-in choice never takes one):
// U, Vd and Mw of the larger of F(4x4) / F(6x6), then the point GEMMs' split
// partials (slab forms: one split per 256 tiles at most, wgrad_splits).  Small
// grids only -- 0 past 256 MB, where the forced tile then does not apply.
static size_t op_wgrad_wino_bytes(int n, int h, int w, int ci, int co) {
  return al256(wino_ws_bytes_grid(n, h, w, ci, co));
}
static size_t op_wgrad_slab_bytes(int n, int h, int w, int ci, int co) {
  const long long t4 = (long long)n * ((h + 3) / 4) * ((w + 3) / 4);
  return al256(sizeof(float) * 64 * (size_t)std::min<long long>(64, (t4 + 255) / 256) * ci * co);
}
static size_t op_wgrad_extra_bytes(int n, int h, int w, int ci, int co) {
  const size_t b = op_wgrad_wino_bytes(n, h, w, ci, co) + op_wgrad_slab_bytes(n, h, w, ci, co);
  return b <= ((size_t)256 << 20) ? b : 0;
}

size_t unet_conv_ws_bytes(int n, int h, int w, int ci, int co) {
  const size_t wb = al256(sizeof(float) * 9 * (size_t)ci * co);
  const size_t pad = al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co);  // (h-2+4)
  const size_t misc = al256(sizeof(float) * 4 * co) + al256(sizeof(double) * kStatGroups * 2 * co);
  const size_t x16 = al256(sizeof(uint16_t) * (size_t)n * h * w * ci);  // op_a16: bf16 copy of x
  return 2 * wb + pad + misc + x16 + op_wgrad_extra_bytes(n, h, w, ci, co) + op_wino_bytes(ci, co);
}

int unet_conv3x3_fwd(const float* x, int n, int h, int w, int ci, const float* wt, const float* bias, int co,
                     const float* xs, const float* xb, float* y, void* ws, unet_stream_t st) {
  // ci % 16; 8 more channels only for a forced fp32 tile that takes them (the
  // fused F(2x2) tiles' single-chunk case, tests)
  if (ci % 8 || co % 64 || h < 3 || w < 3) return -EINVAL;
  if (ci % 16 && (g_op_prec != UNET_PREC_FP32 || g_tune_igemm <= 0)) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  float* wf = reinterpret_cast<float*>(ws);
  IgemmArgs a;
  Src x0;
  x0.ptr = x;
  x0.H = h;
  x0.W = w;
  x0.C = ci;
  x0.scale = xs;
  x0.shift = xb;
  uint16_t* x16 = nullptr;
  if (g_op_prec == UNET_PREC_BF16 && g_op_a16) {
    const size_t wb = al256(sizeof(float) * 9 * (size_t)ci * co);
    const size_t off = 2 * wb + al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co) +
                       al256(sizeof(float) * 4 * co) + al256(sizeof(double) * kStatGroups * 2 * co);
    x16 = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(ws) + off);
    x0.ptr = reinterpret_cast<const float*>(x16);
    x0.h16 = 1;
  }
  a.a.s[0] = a.a.s[1] = x0;
  a.a.Cg = a.a.c_split = ci;
  a.a.taps_h = a.a.taps_w = 3;
  a.a.Hg = h - 2;
  a.a.Wg = w - 2;
  a.a.nimg = n;
  a.b = wf;
  a.M = n * (h - 2) * (w - 2);
  a.N = co;
  a.K = 9 * ci;
  a.e.bias = bias;
  a.e.d[0] = Dst{y, h - 2, w - 2, co, 0, 0};
  op_set_wino(a, ws, n, h, w, ci, co);
  if (ci % 16 && resolve_forced_igemm(a, g_tune_igemm).tile < 0) return -EINVAL;
  if (!op_forced_ok(a)) return -EINVAL;
  OPCK(launch_pack_conv(wt, co, ci, 3, 3, wf, nullptr, s));
  if (x16) OPCK(launch_f2bf(x, x16, (size_t)n * h * w * ci, s));
  OPCK(op_b_to_bf16(a, 9 * (size_t)ci * co, reinterpret_cast<char*>(ws) + al256(sizeof(float) * 9 * (size_t)ci * co),
                    s));
  OPCK(launch_igemm(a, s));
  return 0;
}

int unet_conv3x3_dgrad(const float* dy, int n, int h, int w, int ci, const float* wt, int co, float* dx, void* ws,
                       unet_stream_t st) {
  if (ci % 64 || co % 8 || h < 3 || w < 3) return -EINVAL;  // co % 16, or 8 more as unet_conv3x3_fwd's ci
  if (co % 16 && (g_op_prec != UNET_PREC_FP32 || g_tune_igemm <= 0)) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  const size_t wb = al256(sizeof(float) * 9 * (size_t)ci * co);
  float* wf = reinterpret_cast<float*>(p);
  float* wd = reinterpret_cast<float*>(p + wb);
  float* dyp = reinterpret_cast<float*>(p + 2 * wb);
  float* coef = reinterpret_cast<float*>(p + 2 * wb + al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co));
  const int dy16 = g_op_prec == UNET_PREC_BF16 && g_op_a16;
  IgemmArgs a;
  Src d;
  d.ptr = dyp;
  d.h16 = dy16;
  d.H = h + 2;
  d.W = w + 2;
  d.C = co;
  a.a.s[0] = a.a.s[1] = d;
  a.a.Cg = a.a.c_split = co;
  a.a.taps_h = a.a.taps_w = 3;
  a.a.Hg = h;
  a.a.Wg = w;
  a.a.nimg = n;
  a.b = wd;
  a.M = n * h * w;
  a.N = ci;
  a.K = 9 * co;
  a.e.d[0] = Dst{dx, h, w, ci, 0, 0};
  op_set_wino(a, ws, n, h, w, ci, co);
  if (co % 16 && resolve_forced_igemm(a, g_tune_igemm).tile < 0) return -EINVAL;
  if (!op_forced_ok(a)) return -EINVAL;
  OPCK(launch_pack_conv(wt, co, ci, 3, 3, wf, wd, s));
  // zero-bordered copy of dy: dYpad = 1*dy + 0*(y-0) + 0
  OPCK(launch_fill(coef, co, 1.f, s));
  OPCK(launch_fill(coef + co, 3 * (size_t)co, 0.f, s));
  OPCK(launch_bnb_apply(dy, dy, coef, n, h - 2, w - 2, co, dyp, 2, s, dy16, 0));
  OPCK(op_b_to_bf16(a, 9 * (size_t)ci * co, wf, s));
  OPCK(launch_igemm(a, s));
  return 0;
}

int unet_conv3x3_wgrad(const float* x, const float* dy, int n, int h, int w, int ci, int co, float* dw, float* db,
                       void* ws, unet_stream_t st) {
  if (ci % 64 || co % 64 || h < 3 || w < 3) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  const size_t wb = al256(sizeof(float) * 9 * (size_t)ci * co);
  float* dwp = reinterpret_cast<float*>(p);
  double* st2 = reinterpret_cast<double*>(p + 2 * wb + al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co) +
                                          al256(sizeof(float) * 4 * co));
  OPCK(hipMemsetAsync(dwp, 0, sizeof(float) * 9 * (size_t)ci * co, s));
  WgradArgs a;
  Src d;
  d.ptr = dy;
  d.H = h - 2;
  d.W = w - 2;
  d.C = co;
  a.ga.s[0] = a.ga.s[1] = d;
  a.ga.Cg = a.ga.c_split = co;
  a.ga.Hg = h - 2;
  a.ga.Wg = w - 2;
  a.ga.nimg = n;
  Src xs;
  xs.ptr = x;
  xs.H = h;
  xs.W = w;
  xs.C = ci;
  a.gb.s[0] = a.gb.s[1] = xs;
  a.gb.Cg = a.gb.c_split = ci;
  a.gb.taps_h = a.gb.taps_w = 3;
  a.gb.Hg = h - 2;
  a.gb.Wg = w - 2;
  a.gb.nimg = n;
  a.Mo = co;
  a.No = 9 * ci;
  a.P = n * (h - 2) * (w - 2);
  a.out = dwp;
  a.bf16 = g_op_prec != UNET_PREC_FP32;
  a.split = g_op_prec == UNET_PREC_BF16X3;
  if (g_op_prec == UNET_PREC_BF16 && g_op_a16) {  // bf16-stored dY and X, as in a bf16 plan
    // dY as the plan keeps it: a zero-bordered padded bf16 copy (border 2),
    // written by the BN-backward apply with identity coefficients
    uint16_t* dy16 = reinterpret_cast<uint16_t*>(p + 2 * wb);
    float* coef = reinterpret_cast<float*>(p + 2 * wb + al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co));
    uint16_t* x16 = reinterpret_cast<uint16_t*>(p + 2 * wb + al256(sizeof(float) * (size_t)n * (h + 2) * (w + 2) * co) +
                                                al256(sizeof(float) * 4 * co) +
                                                al256(sizeof(double) * kStatGroups * 2 * co));
    OPCK(launch_fill(coef, co, 1.f, s));
    OPCK(launch_fill(coef + co, 3 * (size_t)co, 0.f, s));
    OPCK(launch_bnb_apply(dy, dy, coef, n, h - 2, w - 2, co, reinterpret_cast<float*>(dy16), 2, s, 1, 0));
    OPCK(launch_f2bf(x, x16, (size_t)n * h * w * ci, s));
    a.ga.s[0].ptr = a.ga.s[1].ptr = reinterpret_cast<const float*>(dy16);
    a.ga.s[0].H = a.ga.s[1].H = h + 2;
    a.ga.s[0].W = a.ga.s[1].W = w + 2;
    a.ga.s[0].oy = a.ga.s[1].oy = a.ga.s[0].ox = a.ga.s[1].ox = 2;
    a.ga.s[0].h16 = a.ga.s[1].h16 = 1;
    a.gb.s[0].ptr = a.gb.s[1].ptr = reinterpret_cast<const float*>(x16);
    a.gb.s[0].h16 = a.gb.s[1].h16 = 1;
  }
  const WgradTile* forced = wgrad_tile(g_tune_wgrad >= 1000 ? g_tune_wgrad - 1000 : g_tune_wgrad);
  if (forced && forced->family == WgradFamily::Wino && !a.bf16 && op_wgrad_extra_bytes(n, h, w, ci, co)) {
    char* e = p + unet_conv_ws_bytes(n, h, w, ci, co) - op_wino_bytes(ci, co) - op_wgrad_extra_bytes(n, h, w, ci, co);
    a.wino_ws = reinterpret_cast<float*>(e);
    a.wino_ws_bytes = op_wgrad_wino_bytes(n, h, w, ci, co);
    a.slab = reinterpret_cast<float*>(e + a.wino_ws_bytes);
    a.slab_bytes = op_wgrad_slab_bytes(n, h, w, ci, co);
  }
  OPCK(launch_wgrad(a, s));
  OPCK(launch_permute_last2(dwp, co, 9, ci, dw, s));
  if (db) {
    OPCK(hipMemsetAsync(st2, 0, sizeof(double) * kStatGroups * 2 * co, s));
    OPCK(launch_channel_stats(dy, (size_t)n * (h - 2) * (w - 2), co, st2, s));
    OPCK(launch_pair_sum(st2, kStatGroups, co, db, s));
  }
  return 0;
}

int unet_convT2_fwd(const float* x, int n, int h, int w, int ci, const float* wt, const float* bias, int co, float* y,
                    void* ws, unet_stream_t st) {
  if (ci % 16 || co % 16) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  float* wf = reinterpret_cast<float*>(p);
  float* wd = reinterpret_cast<float*>(p + al256(sizeof(float) * 4 * (size_t)ci * co));
  IgemmArgs a;
  Src x0;
  x0.ptr = x;
  x0.H = h;
  x0.W = w;
  x0.C = ci;
  a.a.s[0] = a.a.s[1] = x0;
  a.a.Cg = a.a.c_split = ci;
  a.a.Hg = h;
  a.a.Wg = w;
  a.a.nimg = n;
  a.b = wf;
  a.M = n * h * w;
  a.N = 4 * co;
  a.K = ci;
  a.e.bias = bias;
  a.e.shuffle_co = co;
  a.e.d[0] = Dst{y, 2 * h, 2 * w, co, 0, 0};
  if (!op_forced_ok(a)) return -EINVAL;
  OPCK(launch_pack_convT(wt, ci, co, wf, wd, s));
  OPCK(op_b_to_bf16(a, 4 * (size_t)ci * co, p + 2 * al256(sizeof(float) * 4 * (size_t)ci * co), s));
  OPCK(launch_igemm(a, s));
  return 0;
}

int unet_convT2_bwd(const float* x, const float* dy, int n, int h, int w, int ci, const float* wt, int co, float* dx,
                    float* dw, float* db, void* ws, unet_stream_t st) {
  if (ci % 64 || co % 64) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  const size_t wb = al256(sizeof(float) * 4 * (size_t)ci * co);
  float* wf = reinterpret_cast<float*>(p);
  float* wd = reinterpret_cast<float*>(p + wb);
  float* dwp = reinterpret_cast<float*>(p + 2 * wb);
  double* st2 = reinterpret_cast<double*>(p + 3 * wb);
  Src d;
  d.ptr = dy;
  d.H = 2 * h;
  d.W = 2 * w;
  d.C = co;
  IgemmArgs a;
  a.a.s[0] = a.a.s[1] = d;
  a.a.Cg = a.a.c_split = co;
  a.a.taps_h = a.a.taps_w = 2;
  a.a.stride = 2;
  a.a.Hg = h;
  a.a.Wg = w;
  a.a.nimg = n;
  a.b = wd;
  a.M = n * h * w;
  a.N = ci;
  a.K = 4 * co;
  a.e.d[0] = Dst{dx, h, w, ci, 0, 0};
  if (!op_forced_ok(a)) return -EINVAL;
  OPCK(launch_pack_convT(wt, ci, co, wf, wd, s));
  OPCK(op_b_to_bf16(a, 4 * (size_t)ci * co, wf, s));  // wf (4n bytes) is not read again
  OPCK(launch_igemm(a, s));
  OPCK(hipMemsetAsync(dwp, 0, sizeof(float) * 4 * (size_t)ci * co, s));
  WgradArgs g;
  Src x0;
  x0.ptr = x;
  x0.H = h;
  x0.W = w;
  x0.C = ci;
  g.ga.s[0] = g.ga.s[1] = x0;
  g.ga.Cg = g.ga.c_split = ci;
  g.ga.Hg = h;
  g.ga.Wg = w;
  g.ga.nimg = n;
  g.gb.s[0] = g.gb.s[1] = d;
  g.gb.Cg = g.gb.c_split = co;
  g.gb.taps_h = g.gb.taps_w = 2;
  g.gb.stride = 2;
  g.gb.Hg = h;
  g.gb.Wg = w;
  g.gb.nimg = n;
  g.Mo = ci;
  g.No = 4 * co;
  g.P = n * h * w;
  g.out = dwp;
  g.bf16 = g_op_prec != UNET_PREC_FP32;
  g.split = g_op_prec == UNET_PREC_BF16X3;
  OPCK(launch_wgrad(g, s));
  OPCK(launch_permute_last2(dwp, ci, 4, co, dw, s));
  OPCK(hipMemsetAsync(st2, 0, sizeof(double) * kStatGroups * 2 * co, s));
  OPCK(launch_channel_stats(dy, (size_t)n * 4 * h * w, co, st2, s));
  OPCK(launch_pair_sum(st2, kStatGroups, co, db, s));
  return 0;
}

int unet_maxpool2_fwd(const float* x, int n, int h, int w, int c, float* y, uint8_t* arg, unet_stream_t st) {
  Src s0;
  s0.ptr = x;
  s0.H = h;
  s0.W = w;
  s0.C = c;
  OPCK(launch_maxpool_fwd(s0, n, h, w, y, arg, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_maxpool2_bwd(const float* dy, const uint8_t* arg, int n, int h, int w, int c, float* dx, unet_stream_t st) {
  OPCK(launch_maxpool_bwd_fused(dy, arg, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, n, h, w, c,
                                dx, nullptr, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

size_t unet_bn_ws_bytes(int c) { return al256(sizeof(double) * kStatGroups * 2 * c) + 8 * al256(sizeof(float) * c); }

int unet_bn_train_fwd(const float* x, int n, int h, int w, int c, const float* gamma, const float* beta, float* rm,
                      float* rv, float* y, float* save_mean, float* save_invstd, void* ws, unet_stream_t st) {
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  double* stats = reinterpret_cast<double*>(p);
  float* scale = reinterpret_cast<float*>(p + al256(sizeof(double) * kStatGroups * 2 * c));
  float* shift = scale + al256(sizeof(float) * c) / 4;
  const size_t pix = (size_t)n * h * w;
  OPCK(hipMemsetAsync(stats, 0, sizeof(double) * kStatGroups * 2 * c, s));
  OPCK(launch_channel_stats(x, pix, c, stats, s));
  OPCK(launch_bn_finalize(stats, c, (double)pix, gamma, beta, rm, rv, nullptr, save_mean, save_invstd, scale, shift,
                          0.1f, 1e-5f, s));
  OPCK(launch_affine_relu(x, pix, c, scale, shift, 0, y, s));
  return 0;
}

int unet_bn_train_bwd(const float* x, const float* dy, int n, int h, int w, int c, const float* gamma,
                      const float* mean, const float* invstd, float* dx, float* dgamma, float* dbeta, void* ws,
                      unet_stream_t st) {
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  double* stats = reinterpret_cast<double*>(p);
  float* coef = reinterpret_cast<float*>(p + al256(sizeof(double) * kStatGroups * 2 * c));
  const size_t pix = (size_t)n * h * w;
  OPCK(hipMemsetAsync(stats, 0, sizeof(double) * kStatGroups * 2 * c, s));
  OPCK(launch_bn_bwd_stats(dy, x, mean, invstd, pix, c, stats, s));
  OPCK(launch_bnb_finalize(stats, c, (double)pix, gamma, mean, invstd, dgamma, dbeta, nullptr, coef, s));
  OPCK(launch_bnb_apply(dy, x, coef, n, h, w, c, dx, 0, s));
  return 0;
}

size_t unet_bn_relu_ws_bytes(int n, int h, int w, int c) {
  return unet_bn_ws_bytes(c) + al256(sizeof(float) * (size_t)n * h * w * c);
}

int unet_bn_relu_fwd(const float* x, int n, int h, int w, int c, const float* gamma, const float* beta, float* rm,
                     float* rv, int64_t* nbt, float momentum, float eps, int training, int relu, float* y,
                     float* save_mean, float* save_invstd, void* ws, unet_stream_t st) {
  if (!x || !y || !gamma || !beta || !save_mean || !save_invstd || c < 4 || c % 4 || 256 % (c / 4) || n < 1) return -EINVAL;
  if (!training && (!rm || !rv)) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  double* stats = reinterpret_cast<double*>(p);
  float* scale = reinterpret_cast<float*>(p + al256(sizeof(double) * kStatGroups * 2 * c));
  float* shift = scale + al256(sizeof(float) * c) / 4;
  const size_t pix = (size_t)n * h * w;
  if (training) {
    OPCK(hipMemsetAsync(stats, 0, sizeof(double) * kStatGroups * 2 * c, s));
    OPCK(launch_channel_stats(x, pix, c, stats, s));
    OPCK(launch_bn_finalize(stats, c, (double)pix, gamma, beta, rm, rv, nbt, save_mean, save_invstd, scale, shift,
                            momentum, eps, s));
  } else {
    OPCK(launch_bn_eval_prepare(c, gamma, beta, rm, rv, scale, shift, eps, s));
    hipLaunchKernelGGL(k_bn_eval_stats, dim3((c + 255) / 256), dim3(256), 0, s, c, rm, rv, eps, save_mean,
                       save_invstd);
    OPCK(hipGetLastError());
  }
  OPCK(launch_affine_relu(x, pix, c, scale, shift, relu, y, s));
  return 0;
}

int unet_bn_relu_bwd(const float* x, const float* y, const float* dy, int n, int h, int w, int c, const float* gamma,
                     const float* save_mean, const float* save_invstd, int training, int relu, float* dx,
                     float* dgamma, float* dbeta, void* ws, unet_stream_t st) {
  if (!x || !dy || !dx || !gamma || c < 4 || c % 4 || 256 % (c / 4) || n < 1 || (relu && !y)) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  double* stats = reinterpret_cast<double*>(p);
  float* coef = reinterpret_cast<float*>(p + al256(sizeof(double) * kStatGroups * 2 * c));
  float* dz = reinterpret_cast<float*>(p + unet_bn_ws_bytes(c));
  const size_t pix = (size_t)n * h * w;
  const float* g = dy;
  if (relu) {
    const long long n4 = (long long)(pix * c / 4);
    hipLaunchKernelGGL(k_relu_mask, dim3((unsigned)std::min<long long>((n4 + 255) / 256, 8192)), dim3(256), 0, s, dy,
                       y, n4, dz);
    OPCK(hipGetLastError());
    g = dz;
  }
  OPCK(hipMemsetAsync(stats, 0, sizeof(double) * kStatGroups * 2 * c, s));
  OPCK(launch_bn_bwd_stats(g, x, save_mean, save_invstd, pix, c, stats, s));
  OPCK(launch_bnb_finalize(stats, c, (double)pix, gamma, save_mean, save_invstd, dgamma, dbeta, nullptr, coef, s,
                           training ? 0 : 1));
  OPCK(launch_bnb_apply(g, x, coef, n, h, w, c, dx, 0, s));
  return 0;
}

size_t unet_conv_first_ws_bytes(int n, int ci, int h, int w) {
  (void)n; (void)h; (void)w;
  return conv_first_wgrad_ws_bytes(ci) + al256(sizeof(double) * kStatGroups * 2 * 64);
}

int unet_conv_first_fwd(const float* x, int n, int ci, int h, int w, const float* wt, const float* bias, float* y,
                        unet_stream_t st) {
  if (!x || !wt || !bias || !y || n < 1 || ci < 1 || h < 3 || w < 3) return -EINVAL;
  OPCK(launch_conv_first_fwd(x, n, ci, h, w, wt, bias, 64, y, nullptr, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_conv_first_bwd(const float* x, const float* dy, int n, int ci, int h, int w, const float* wt, float* dx,
                        float* dw, float* db, void* ws, unet_stream_t st) {
  if (!x || !dy || !wt || !dw || !db || !ws || n < 1 || ci < 1 || h < 3 || w < 3) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  char* p = reinterpret_cast<char*>(ws);
  float* slabs = reinterpret_cast<float*>(p);
  double* st2 = reinterpret_cast<double*>(p + conv_first_wgrad_ws_bytes(ci));
  Src d;
  d.ptr = dy;
  d.H = h - 2;
  d.W = w - 2;
  d.C = 64;
  OPCK(launch_conv_first_wgrad(x, n, ci, h, w, d, 64, dw, slabs, s));
  OPCK(hipMemsetAsync(st2, 0, sizeof(double) * kStatGroups * 2 * 64, s));
  OPCK(launch_channel_stats(dy, (size_t)n * (h - 2) * (w - 2), 64, st2, s));
  OPCK(launch_pair_sum(st2, kStatGroups, 64, db, s));
  if (dx) OPCK(launch_conv_first_dgrad(dy, n, ci, h, w, wt, dx, s));
  return 0;
}

size_t unet_conv1x1_ws_bytes(int k) { return al256(sizeof(double) * ((size_t)k * 64 + k)); }

int unet_conv1x1_fwd(const float* x, int n, int h, int w, int c, const float* wt, const float* bias, int k,
                     float* logits, unet_stream_t st) {
  if (!x || !wt || !bias || !logits || c != 64 || k < 1 || n < 1) return -EINVAL;
  Src s0;
  s0.ptr = x;
  s0.H = h;
  s0.W = w;
  s0.C = 64;
  OPCK(launch_head_fwd(s0, n, h, w, 64, wt, bias, k, logits, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_conv1x1_bwd(const float* x, const float* dl, int n, int h, int w, int c, const float* wt, int k, float* dx,
                     float* dw, float* db, void* ws, unet_stream_t st) {
  if (!x || !dl || !wt || !dw || !db || !ws || c != 64 || k < 1 || n < 1) return -EINVAL;
  OPCK(launch_head_bwd_plain(x, dl, n, h, w, wt, k, dx, dw, db, reinterpret_cast<double*>(ws),
                             reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_wce_fwd_bwd(const float* logits, const int64_t* t, const float* wm, int n, int k, int h, int w,
                     const int64_t* ts, const int64_t* wsd, float* loss, float* dl, float gscale, void* ws,
                     unet_stream_t st) {
  if (!ts || !wsd || k < 1) return -EINVAL;
  OPCK(launch_wce(logits, t, wm, n, k, h, w, ts, wsd, loss, dl, gscale, reinterpret_cast<double*>(ws),
                  reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_scale_by_device_scalar(float* x, size_t n, const float* g, unet_stream_t st) {
  OPCK(launch_scale_by_dev(x, x, n, g, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_scale_by_device_scalar_out(const float* x, float* y, size_t n, const float* g, unet_stream_t st) {
  OPCK(launch_scale_by_dev(x, y, n, g, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_sgd_momentum(float* p, const float* g, float* buf, size_t n, float lr, float mom, float gscale, int first,
                      unet_stream_t st) {
  OPCK(launch_sgd(p, g, buf, n, lr, mom, gscale, first, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_iou_counts(const uint8_t* a, const uint8_t* b, size_t n, unsigned long long* out, unet_stream_t st) {
  OPCK(launch_iou(a, b, n, out, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_set_tuning(const char* key, int value) {
  if (!key) return -EINVAL;
  const std::string k(key);
  if (k == "igemm_variant") g_tune_igemm = value;
  else if (k == "wgrad_variant") g_tune_wgrad = value;
  else if (k == "autotune") g_autotune = value;
  else if (k == "force_split") g_force_split = value;
  else if (k == "force_tile") g_force_tile = value;
  else if (k == "concurrent") g_concurrent = value;
  else if (k == "wino_max") g_wino_max = value;
  else if (k == "bf16_norm") g_bf16_norm = value;
  else if (k == "bn_fold") g_bn_fold = value != 0;
  else if (k == "wino_dgrad_max") g_wino_dgrad_max = value;
  else if (k == "wino_wgrad_max") g_wino_wgrad_max = value;
  else if (k == "wino4_fwd_min_cg") g_wino4_fwd_min_cg = value;
  else if (k == "wino4_fwd_small_cg") g_wino4_fwd_small_cg = value;
  else if (k == "op_a16") g_op_a16 = value != 0;
  else if (k == "op_strict") g_op_strict = value != 0;
  else if (k == "maxpool_vec8") g_maxpool_vec8 = value;
  else if (k == "bnb_fuse") g_bnb_fuse = value;
  else if (k == "wgrad_early_u") g_wgrad_early_u = value;
  else if (k == "wgrad_fwd_u") g_wgrad_fwd_u = value;
  else if (k == "wgrad_plane") g_wgrad_plane = value;
  else if (k == "wgrad_oihw") g_wgrad_oihw = value;
  else if (k == "igemm_plane") g_igemm_plane = value;
  else if (k == "wino_persist") g_wino_persist = value;
  else if (k == "wino_persist_wgs") g_wino_persist_wgs = value;
  else if (k == "wino_point_tile") g_wino_point_tile = value;
  else if (k == "ctc_chunk_frames" || k == "ctc_dense_cells") {  // ctc.hip clamps them to what it supports
    if (value < -1 || (value == 0 && k == "ctc_chunk_frames")) return -EINVAL;  // -1 = the default
    (k == "ctc_chunk_frames" ? g_ctc_chunk_frames : g_ctc_dense_cells) = value;
  }
  else if (k == "region_lds_objects") {  // region.hip clamps it to its table; -1 = the default
    if (value < -1) return -EINVAL;
    g_region_lds_objects = value;
  }
  else if (k == "link_lds_objects") {  // link.hip clamps it to what a CU's LDS holds; -1 = the default
    if (value < -1) return -EINVAL;
    g_link_lds_objects = value;
  }
  else if (k == "split_threads") {  // split.hip: the growth workgroup's size, -1 = the default
    if (value != -1 && (value < 64 || value > 1024 || value % 64)) return -EINVAL;
    g_split_threads = value;
  }
  else if (k == "deterministic") g_deterministic = value != 0;  // 0: bf16 plans pool with the 4-channel kernel (A/B tests)
  else if (k == "op_precision") {
    if (value != UNET_PREC_FP32 && value != UNET_PREC_BF16 && value != UNET_PREC_BF16X3) return -EINVAL;
    g_op_prec = value;
  } else return -EINVAL;
  return 0;
}

int unet_tile_gather(const float* image, int c, int h, int w, int tile_in, int tile_out, int top, int left, int nx,
                     int first, int stride, int ntiles, float* tiles, unet_stream_t st) {
  if (!image || !tiles) return -EINVAL;
  OPCK(launch_tile_gather(image, c, h, w, tile_in, tile_out, top, left, nx, first, stride, ntiles, tiles,
                          reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_tile_scatter(const float* tile_logits, int k, int tile_out, int nx, int first, int stride, int ntiles, int h,
                      int w, float* logits, uint8_t* mask, unet_stream_t st) {
  if (!tile_logits) return -EINVAL;
  OPCK(launch_tile_scatter(tile_logits, k, tile_out, nx, first, stride, ntiles, h, w, logits, mask,
                           reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_seq_tile_gather(const void* frames, int frames_u8, int nframes, int c, int h, int w, int tile_in,
                         int tile_out, int top, int left, int nx, const int32_t* work, int ngroups,
                         const int32_t* codes, int ns, float* tiles, unet_stream_t st) {
  if (!frames || !work || !codes || !tiles) return -EINVAL;
  OPCK(launch_seq_tile_gather(frames, frames_u8, nframes, c, h, w, tile_in, tile_out, top, left, nx, work, ngroups,
                              codes, ns, tiles, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_seq_tile_reduce(const float* tile_logits, int k, int tile_out, int nx, const int32_t* work, int ngroups,
                         const int32_t* codes, int ns, int nframes, int h, int w, float threshold, float* prob,
                         uint8_t* mask, float* logits, unet_stream_t st) {
  if (!tile_logits || !work || !codes) return -EINVAL;
  OPCK(launch_seq_tile_reduce(tile_logits, k, tile_out, nx, work, ngroups, codes, ns, nframes, h, w, threshold, prob,
                              mask, logits, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

size_t unet_instance_masks_ws_bytes(int n, int h, int w) {
  return n > 0 && h > 0 && w > 0 ? instance_masks_ws_bytes(n, h, w) : 0;
}

int unet_instance_masks(const uint8_t* mask, int n, int h, int w, int min_size, uint16_t* labels, void* ws,
                        unet_stream_t st) {
  if (!mask || !labels || !ws) return -EINVAL;
  OPCK(launch_instance_masks(mask, n, h, w, min_size, labels, ws, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

size_t unet_rand_index_ws_bytes(int h, int w) { return h > 0 && w > 0 ? rand_index_ws_bytes(h, w) : 0; }

int unet_rand_index(const uint16_t* gt, const uint16_t* pred, int h, int w, double* out, void* ws,
                    unet_stream_t st) {
  if (!gt || !pred || !out || !ws) return -EINVAL;
  OPCK(launch_rand_index(gt, pred, h, w, out, ws, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

size_t unet_weight_map_ws_bytes(int n) { return n > 0 ? weight_map_ws_bytes(n) : 0; }

int unet_weight_map(const uint16_t* labels, int n, int h, int w, double w0, double sigma, float* weights,
                    double* weights64, void* ws, unet_stream_t st) {
  if (!labels || !weights || !ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return -EINVAL;
  OPCK(launch_weight_map(labels, n, h, w, w0, sigma, weights, weights64, ws, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

size_t unet_weight_map_border_ws_bytes(int n, int h, int w) { return weight_map_border_ws_bytes(n, h, w); }

int unet_weight_map_border(const uint16_t* labels, int n, int h, int w, double w0, double sigma, float* weights,
                           double* weights64, int32_t* d1sq, int32_t* d2sq, void* ws, unet_stream_t st) {
  if (n < 1 || h < 1 || w < 1 || h > 16384 || w > 16384) {
    set_last_error("unet_weight_map_border: need n, h, w >= 1 and h, w <= 16384 (h^2 + w^2 must fit int32)");
    return -EINVAL;
  }
  if (!labels || !weights || !ws || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_last_error("unet_weight_map_border: null labels / weights / ws, or ws not 16-byte aligned");
    return -EINVAL;
  }
  const hipError_t e = launch_weight_map_border(labels, n, h, w, w0, sigma, weights, weights64, d1sq, d2sq, ws,
                                                reinterpret_cast<hipStream_t>(st));
  if (e != hipSuccess) {
    set_last_error(std::string("unet_weight_map_border: ") + hipGetErrorString(e));
    return e == hipErrorInvalidValue ? -EINVAL : -EIO;
  }
  return 0;
}

size_t unet_elastic_ws_bytes(int n, int h, int w) { return n > 0 && h > 0 && w > 0 ? elastic_ws_bytes(n, h, w) : 0; }

int unet_elastic_deform_ex(const uint8_t* image, const uint16_t* labels, int n, int h, int w, const double* noise,
                           double alpha, double sigma, float* x_out, uint8_t* target_out, uint8_t* image_out,
                           uint16_t* ids_out, void* ws, unet_stream_t st) {
  if (!image || !labels || !noise || !x_out || !target_out || !ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return -EINVAL;
  OPCK(launch_elastic(image, labels, n, h, w, noise, alpha, sigma, x_out, target_out, image_out, ids_out, ws,
                      reinterpret_cast<hipStream_t>(st)));
  return 0;
}

int unet_elastic_deform(const uint8_t* image, const uint16_t* labels, int n, int h, int w, const double* noise,
                        double alpha, double sigma, float* x_out, uint8_t* target_out, uint8_t* image_out, void* ws,
                        unet_stream_t st) {
  return unet_elastic_deform_ex(image, labels, n, h, w, noise, alpha, sigma, x_out, target_out, image_out, nullptr, ws,
                                st);
}

size_t unet_tile_warp_ws_bytes(int n, int th, int tw) {
  return n > 0 && th > 0 && tw > 0 ? elastic_ws_bytes(n, th, tw) : 0;
}

int unet_tile_warp(const uint8_t* frames, const uint16_t* labels, const float* weights, int nframes, int h, int w,
                   const int32_t* frame_idx, const double* params, int n, int th, int tw, int extend,
                   const double* noise, double alpha, double sigma, float* x_out, uint8_t* target_out,
                   uint8_t* image_out, uint16_t* ids_out, float* weight_out, void* ws, unet_stream_t st) {
  // every check runs on the host, before the first device call
  if (!tile_warp_check(nframes, h, w, n, th, tw, extend, noise != nullptr, sigma)) {
    set_last_error("unet_tile_warp: need nframes, h, w, n, th, tw >= 1, extend 0 (reflect) or 1 (mirror) and, with an "
                   "elastic field, sigma > 0 with radius int(4 sigma + 0.5) <= 128");
    return -EINVAL;
  }
  if (!frames || !labels || !frame_idx || !params || !x_out || !target_out) {
    set_last_error("unet_tile_warp: null frames / labels / frame_idx / params / x_out / target_out");
    return -EINVAL;
  }
  if (weight_out && !weights) {
    set_last_error("unet_tile_warp: weight_out needs the weights planes");
    return -EINVAL;
  }
  if (noise && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7))) {
    set_last_error("unet_tile_warp: the elastic field needs an 8-byte aligned ws of unet_tile_warp_ws_bytes");
    return -EINVAL;
  }
  const hipError_t e = launch_tile_warp(frames, labels, weights, nframes, h, w, frame_idx, params, n, th, tw, extend,
                                        noise, alpha, sigma, x_out, target_out, image_out, ids_out, weight_out, ws,
                                        reinterpret_cast<hipStream_t>(st));
  if (e != hipSuccess) {
    set_last_error(std::string("unet_tile_warp: ") + hipGetErrorString(e));
    return e == hipErrorInvalidValue ? -EINVAL : -EIO;
  }
  return 0;
}

int unet_mask_from_logits(const float* logits, uint8_t* mask, int n, int h, int w, unet_stream_t st) {
  OPCK(launch_mask(logits, mask, n, h, w, reinterpret_cast<hipStream_t>(st)));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// unet_gemm_site: one forward / input-gradient GEMM with the arguments the plan
// builds at that launch site (plan.hip run_forward / run_backward), on caller
// buffers.  Layout of ws (256-B aligned pieces): packed B (forward form, then
// the input-gradient form), its bf16 planes, the bf16 copies of the sources and
// of yref (op_a16), the split-K / stream-K slab, the Winograd scratch.
// ---------------------------------------------------------------------------
namespace {
struct SiteBuild {
  IgemmArgs a;
  GemmChoice c;          // tile < 0: the built-in choice
  float *wf, *wd;        // packed B of the forward / the input-gradient GEMM
  uint16_t* b16;         // bf16 planes of the GEMM's B (nullptr: fp32)
  size_t nw;             // weight elements
  uint16_t *s16[2], *y16;  // bf16 copies (nullptr: none)
  size_t ns[2], ny;      // their element counts
  size_t bytes;
  int nstat, ncs;        // columns of stats / bstats and of colsum1
};

bool site_is_fwd(int s) { return s == UNET_SITE_F_PLAIN || s == UNET_SITE_F_CAT || s == UNET_SITE_F_EVAL; }
bool site_is_dgrad(int s) { return s == UNET_SITE_D_POOL || s == UNET_SITE_D_MASK || s == UNET_SITE_D_SPLIT; }
bool site_masks(int s) { return s == UNET_SITE_D_MASK || s == UNET_SITE_T_MASK; }

// the built-in choice, whatever "igemm_variant" says
int site_builtin_tile(const IgemmArgs& a) {
  const int knob = g_tune_igemm;
  g_tune_igemm = -1;
  const int t = igemm_heuristic_tile(a);
  g_tune_igemm = knob;
  return t;
}

// the K slices launch_igemm_v makes of a request for `split` with tile t
int site_slices(const IgemmArgs& a, const IgemmTile& t, int split) {
  const int nk = a.K / t.bk;
  int ks = split < 1 || t.wino_m ? 1 : (split > nk ? nk : split);
  if (ks > 1) {
    const int per = (nk + ks - 1) / ks;
    ks = (nk + per - 1) / per;
  }
  return ks;
}

// Validates d and lays the GEMM out over ws (pointers only, nothing is
// launched; ws may be any non-null address when only the layout is wanted).
// 0, or -EINVAL with the reason in unet_last_error().
int site_build(const unet_gemm_site* dp, char* ws, SiteBuild& b) {
  auto bad = [](const char* why) {
    set_last_error(std::string("unet_gemm_site: ") + why);
    return -EINVAL;
  };
  if (!dp) return bad("null descriptor");
  const unet_gemm_site& d = *dp;
  if (d.site < UNET_SITE_F_PLAIN || d.site > UNET_SITE_T_MASK) return bad("unknown site");
  if (d.n < 1 || d.h < 1 || d.w < 1 || d.ci < 8 || d.co < 8) return bad("need n, h, w >= 1 and ci, co >= 8");
  if ((long long)d.n * (d.h + 2) * (d.w + 2) * 4 > 0x7fffffffLL) return bad("grid too large");
  const bool fwd = site_is_fwd(d.site), dgrad = site_is_dgrad(d.site), cat = d.site == UNET_SITE_F_CAT;
  const bool tfwd = d.site == UNET_SITE_T_FWD, tmask = d.site == UNET_SITE_T_MASK, split2 = d.site == UNET_SITE_D_SPLIT;
  const int Cg = fwd || tfwd ? d.ci : d.co;                // channels per tap
  const int N = fwd ? d.co : tfwd ? 4 * d.co : d.ci;       // GEMM columns
  if (Cg % 8 || N % 32) return bad("channels per tap must be a multiple of 8, columns a multiple of 32");
  if (tfwd && d.co % 8) return bad("convT co must be a multiple of 8");
  if (cat && (d.c_split < 8 || d.c_split >= d.ci || d.c_split % 8)) return bad("c_split must be a multiple of 8 in (0, ci)");
  if (cat && (d.oy < 0 || d.ox < 0 || d.oy + d.h + 2 > d.skip_h || d.ox + d.w + 2 > d.skip_w))
    return bad("the cropped window leaves the stored skip grid");
  if (split2 && (d.n_split < 32 || d.n_split >= N || d.n_split % 32)) return bad("n_split must be a multiple of 32 in (0, ci)");
  if (!d.src0 || !d.wt || !d.dst0) return bad("null src0 / wt / dst0");
  if (cat && !d.src1) return bad("F_CAT needs src1");
  if ((d.scale0 == nullptr) != (d.shift0 == nullptr) || (d.scale1 == nullptr) != (d.shift1 == nullptr))
    return bad("scale and shift come in pairs");
  if ((dgrad || tmask) && (d.scale0 || d.scale1)) return bad("input-gradient sources take no transform");
  if (site_masks(d.site) && (!d.yref || !d.bn_scale || !d.bn_shift || !d.bn_mean || !d.bn_invstd || !d.bstats))
    return bad("mask sites need yref, bn_scale / shift / mean / invstd and bstats");
  if (split2 && (!d.dst1 || !d.colsum1)) return bad("D_SPLIT needs dst1 and colsum1");
  if ((d.site == UNET_SITE_F_PLAIN || cat) && !d.stats) return bad("F_PLAIN / F_CAT need stats");
  if ((fwd || tfwd) && !d.bias) return bad("forward sites need bias");

  const int h16 = g_op_prec == UNET_PREC_BF16 && g_op_a16;
  b = SiteBuild{};
  const bool conv = fwd || dgrad;
  b.nw = (size_t)(conv ? 9 : 4) * d.ci * d.co;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = ws + off;
    off += al256(bytes);
    return p;
  };
  b.wf = reinterpret_cast<float*>(take(sizeof(float) * b.nw));
  b.wd = reinterpret_cast<float*>(take(sizeof(float) * b.nw));
  b.b16 = g_op_prec != UNET_PREC_FP32 ? reinterpret_cast<uint16_t*>(take(sizeof(float) * b.nw)) : nullptr;

  IgemmArgs& a = b.a;
  Gather& g = a.a;
  g.Cg = g.c_split = Cg;
  g.Hg = d.h;
  g.Wg = d.w;
  g.nimg = d.n;
  Src s0;
  s0.ptr = d.src0;
  s0.C = Cg;
  s0.scale = d.scale0;
  s0.shift = d.shift0;
  if (conv) {
    g.taps_h = g.taps_w = 3;
    s0.H = d.h + 2;
    s0.W = d.w + 2;
  } else if (tmask) {
    g.taps_h = g.taps_w = 2;
    g.stride = 2;
    s0.H = 2 * d.h;
    s0.W = 2 * d.w;
  } else {
    s0.H = d.h;
    s0.W = d.w;
  }
  g.s[0] = g.s[1] = s0;
  if (cat) {  // input_gather, l >= 10: cat([crop(skip), up], 1) without a copy
    g.s[0].H = d.skip_h;
    g.s[0].W = d.skip_w;
    g.s[0].C = d.c_split;
    g.s[0].oy = d.oy;
    g.s[0].ox = d.ox;
    g.s[1].ptr = d.src1;
    g.s[1].C = d.ci - d.c_split;
    g.s[1].scale = d.scale1;
    g.s[1].shift = d.shift1;
    g.c_split = d.c_split;
  }
  for (int k = 0; k < (cat ? 2 : 1); ++k) {
    b.ns[k] = (size_t)d.n * g.s[k].H * g.s[k].W * g.s[k].C;
    if (h16) {
      b.s16[k] = reinterpret_cast<uint16_t*>(take(sizeof(uint16_t) * b.ns[k]));
      g.s[k].ptr = reinterpret_cast<const float*>(b.s16[k]);
      g.s[k].h16 = 1;
    }
  }
  if (!cat) g.s[1] = g.s[0];
  a.M = d.n * d.h * d.w;
  a.N = N;
  a.K = g.taps_h * g.taps_w * Cg;
  a.b = fwd || tfwd ? b.wf : b.wd;
  a.fwd = fwd;
  Epilogue& e = a.e;
  e.bias = fwd || tfwd ? d.bias : nullptr;
  e.d[0] = Dst{reinterpret_cast<float*>(d.dst0), d.h, d.w, N, 0, 0, h16};
  if (tfwd) {
    e.shuffle_co = d.co;
    e.d[0] = Dst{reinterpret_cast<float*>(d.dst0), 2 * d.h, 2 * d.w, d.co, 0, 0, h16};
  }
  b.nstat = N;
  if (split2) {
    e.n_split = d.n_split;
    e.d[0].C = d.n_split;
    e.d[1] = Dst{reinterpret_cast<float*>(d.dst1), d.h, d.w, N - d.n_split, 0, 0, h16};
    e.colsum1 = d.colsum1;
    b.ncs = N - d.n_split;
  }
  if (d.site == UNET_SITE_F_PLAIN || cat) e.stats = d.stats;
  if (d.site == UNET_SITE_F_EVAL) e.relu = 1;
  if (site_masks(d.site)) {
    e.yref = d.yref;
    b.ny = (size_t)a.M * N;
    if (h16) {
      b.y16 = reinterpret_cast<uint16_t*>(take(sizeof(uint16_t) * b.ny));
      e.yref = reinterpret_cast<const float*>(b.y16);
      e.yref_h16 = 1;
    }
    e.bn_scale = d.bn_scale;
    e.bn_shift = d.bn_shift;
    e.bn_mean = d.bn_mean;
    e.bn_invstd = d.bn_invstd;
    e.bstats = d.bstats;
  }
  if (b.b16) {
    a.bh = b.b16;
    a.bl = g_op_prec == UNET_PREC_BF16X3 ? b.b16 + b.nw : nullptr;
    a.b = nullptr;
  }

  // the variant: the descriptor's tile, else the knob's, else the built-in one
  const int want = d.tile > 0 ? d.tile : (d.tile == -1 && g_tune_igemm > 0 ? g_tune_igemm : -1);
  const IgemmTile* t = want > 0 ? igemm_tile(want) : nullptr;
  if (want > 0 && !t && g_op_strict) return bad("no such tile");
  // the scratch a Winograd tile works in (sized like the plan's: the unfused
  // tiles' U / M / V, or the fused tiles' transformed weights + claim counters)
  if (t && t->wino_m && conv) {
    a.wino_ws_bytes = std::max(al256(wino_ws_bytes_grid(d.n, d.h, d.w, Cg, N)), al256(sizeof(float) * 36 * (size_t)Cg * N) + 256);
    a.wino_ws = reinterpret_cast<float*>(ws + off);  // taken below, after the slab
  }
  if (d.split > 1 || (t && t->slab_bytes)) a.slab = reinterpret_cast<float*>(ws + off);  // taken below, if used
  const int q = op_quantum(t);
  const bool chunks_ok = a.K % q == 0 && Cg % q == 0 && g.c_split % q == 0;
  if (t && !(chunks_ok && igemm_tile_fits(a, t->id))) {
    if (g_op_strict) return bad("the forced tile does not apply to this site (its fits() refuses the arguments)");
    t = nullptr;  // the built-in tile in its place
  }
  int ks = 1;
  if (d.split > 1) {  // of the forced tile, else of the built-in one
    const IgemmTile* st = t ? t : igemm_tile(chunks_ok ? site_builtin_tile(a) : -1);
    if (st && st->ksplit && N % 64 == 0 && a.K % st->bk == 0) ks = site_slices(a, *st, d.split);
    if (g_op_strict && ks != d.split)
      return bad("the K split does not apply to the tile (no split-K form, or its K chunks do not divide that way)");
    if (ks > 1) t = st;
  }
  if (!t && (!chunks_ok || site_builtin_tile(a) < 0)) return bad("no built-in tile takes these channel counts");
  b.c = t ? GemmChoice{t->id, ks} : GemmChoice{};
  size_t slab = ks > 1 ? igemm_slab_bytes(a, ks) : 0;
  if (t && t->slab_bytes && ks == 1) slab = t->slab_bytes(a);
  if (slab == ~(size_t)0) slab = 0;
  a.slab = slab ? reinterpret_cast<float*>(take(slab)) : nullptr;
  if (a.wino_ws) {
    a.wino_ws = reinterpret_cast<float*>(ws + off);
    take(a.wino_ws_bytes);
  }
  // a tile that wants its slab or scratch sees them only now
  if (t && !igemm_tile_fits(a, t->id)) {
    if (g_op_strict) return bad("the forced tile does not apply to this site (its fits() refuses the arguments)");
    b.c = GemmChoice{};
  }
  b.bytes = off;
  return 0;
}
}  // namespace

extern "C" {

int unet_gemm_site_check(const unet_gemm_site* d, int* tile) {
  SiteBuild b;
  const int r = site_build(d, reinterpret_cast<char*>(uintptr_t{4096}), b);
  if (r) return r;
  if (tile) *tile = b.c.tile > 0 ? b.c.tile : site_builtin_tile(b.a);
  return 0;
}

size_t unet_gemm_site_ws_bytes(const unet_gemm_site* d) {
  SiteBuild b;
  return site_build(d, reinterpret_cast<char*>(uintptr_t{4096}), b) ? 0 : b.bytes;
}

int unet_gemm_site_run(const unet_gemm_site* d, void* ws, unet_stream_t st) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    set_last_error("unet_gemm_site_run: ws must be 256-byte aligned and hold unet_gemm_site_ws_bytes");
    return -EINVAL;
  }
  SiteBuild b;
  if (const int r = site_build(d, reinterpret_cast<char*>(ws), b)) return r;
  hipStream_t s = reinterpret_cast<hipStream_t>(st);
  const bool conv = site_is_fwd(d->site) || site_is_dgrad(d->site);
  if (conv) OPCK(launch_pack_conv(d->wt, d->co, d->ci, 3, 3, b.wf, b.wd, s));
  else OPCK(launch_pack_convT(d->wt, d->ci, d->co, b.wf, b.wd, s));
  if (b.b16)  // the planes of this GEMM's packed B
    OPCK(launch_f2bf(site_is_fwd(d->site) || d->site == UNET_SITE_T_FWD ? b.wf : b.wd, b.b16, b.nw, s,
                     const_cast<uint16_t*>(b.a.bl)));
  const float* srcs[2] = {d->src0, d->src1};
  for (int k = 0; k < 2; ++k)
    if (b.s16[k]) OPCK(launch_f2bf(srcs[k], b.s16[k], b.ns[k], s));
  if (b.y16) OPCK(launch_f2bf(d->yref, b.y16, b.ny, s));
  if (b.a.e.stats) OPCK(hipMemsetAsync(b.a.e.stats, 0, sizeof(double) * kStatGroups * 2 * b.nstat, s));
  if (b.a.e.bstats)
    OPCK(hipMemsetAsync(b.a.e.bstats, 0, sizeof(double) * kStatGroups * 2 * std::min(b.a.e.n_split, b.a.N), s));
  if (b.a.e.colsum1) OPCK(hipMemsetAsync(b.a.e.colsum1, 0, sizeof(double) * kStatGroups * b.ncs, s));
  if (b.c.tile > 0 && b.c.split <= 1) {
    // through launch_igemm, as the other per-op entry points run a forced tile
    // (it alone admits the 8-channel chunks of the fused F(2x2) tiles)
    const int knob = g_tune_igemm;
    g_tune_igemm = b.c.tile;
    const hipError_t e = launch_igemm(b.a, s);
    g_tune_igemm = knob;
    OPCK(e);
    return 0;
  }
  if (b.c.tile > 0) {
    OPCK(launch_igemm_v(b.a, s, b.c));
    return 0;
  }
  const int knob = g_tune_igemm;
  g_tune_igemm = -1;  // a knob that does not apply was dropped above
  const hipError_t e = launch_igemm(b.a, s);
  g_tune_igemm = knob;
  OPCK(e);
  return 0;
}

int unet_igemm_tile_table(int* out, int cap) {
  const std::vector<IgemmTile>& v = igemm_tiles();
  for (int i = 0; out && i < cap && i < (int)v.size(); ++i) {
    const IgemmTile& t = v[i];
    const int row[6] = {t.id, (int)t.family, t.bf16, t.x3, t.ksplit, t.wino_m};
    std::copy(row, row + 6, out + 6 * i);
  }
  return (int)v.size();
}

}  // extern "C"
