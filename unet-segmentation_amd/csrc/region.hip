// Per-object measurements of a whole label stack (the reference's
// get_mask_properties, scripts/track.py:39-70, is an np.argwhere per label and
// frame): one all-integer record per object per frame -- area, index sums and
// their products, extent, boundary / edge / contact counts and intensity sums --
// ordered by frame, then by ascending label (np.unique's order).
//
// Index phase, per call:
//   k_rg_mark     label presence bitmaps (65536 bits per frame), set in LDS
//                 first, one global atomicOr per non-zero word and block
//   k_rg_rank     popcount prefix of each bitmap: label -> compact index, and
//                 the object count of each frame
//   k_rg_scan     exclusive scan of the counts into frame_offsets (n + 1)
//   (one host synchronisation: the object total, frame_offsets[n])
// Accumulate phase (only when the total fits the caller's records):
//   k_rg_init     every record's frame, label and the neutral values of its
//                 sums and extremes
//   k_rg_accum    one launch for the stack, grid = frames x bands of kPiece-
//                 sized pieces of the flattened frame.  A thread walks 16
//                 consecutive pixels, merges the runs of equal labels within a
//                 row in registers (a run of r pixels from column x0 adds the
//                 closed forms of sum x and sum x^2), and adds each run into a
//                 table of records in LDS, flushed with one set of global
//                 integer atomics per non-empty entry and block.  A frame with
//                 more objects than the table holds ("region_lds_objects")
//                 sends its runs to global atomics directly.  The rows above
//                 and below come through L2.
// Every field is an integer, so the records do not depend on the order of the
// atomics.  unet_region_props_host is the same in plain C++ loops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/unet_hip.h"
#include "unet_internal.h"

static_assert(sizeof(unet_region_record) == 128, "unet_region_record is 128 bytes");

namespace unet {
// unet_set_tuning("region_lds_objects", n): most objects of a frame that
// k_rg_accum collects in its LDS table (0 = every frame goes straight to
// global atomics; at most kLdsMax; -1 = the default, kLdsMax)
int g_region_lds_objects = -1;
}  // namespace unet

namespace {

constexpr int kWords = 2048;  // 65536 label bits
constexpr int kThreads = 256;
constexpr int kPix = 16;  // consecutive pixels per thread
constexpr int kPiece = kThreads * kPix;
constexpr int kLdsMax = 512;         // entries of the LDS table (96 bytes each)
constexpr unsigned kOut = 0x10000u;  // a neighbour outside the frame: equals no label
constexpr int kMaxDim = 32768;
constexpr long long kMaxPixels = 1ll << 30;

// s32 / s64 rows of the LDS table
enum { A_AREA, A_BOUNDARY, A_EDGE, A_CONTACT, A_MIN_Y, A_MIN_X, A_MAX_Y, A_MAX_X, A_MIN_V, A_MAX_V, A_N32 };
enum { S_Y, S_X, S_YY, S_XX, S_XY, S_V, S_VV, S_N64 };

std::atomic<long long> g_region_launches{0};

int lds_objects() {
  return unet::g_region_lds_objects < 0 ? kLdsMax : std::min(unet::g_region_lds_objects, kLdsMax);
}

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

void errf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  unet::set_last_error(buf);
}

// ------------------------------- GPU part ------------------------------------
__device__ __forceinline__ void rg_unpack(const unsigned* w, unsigned (&v)[kPix]) {
#pragma unroll
  for (int k = 0; k < kPix / 2; ++k) {
    v[2 * k] = w[k] & 0xffffu;
    v[2 * k + 1] = w[k] >> 16;
  }
}

// the kPix labels from flattened index q0 on (q0 may be negative, q0 + kPix may
// pass the frame's end: such elements read as kOut): the widest loads the
// address allows -- a frame of odd size starts 2-byte aligned, the rows above
// and below a 16-byte aligned piece are as aligned as the row pitch
__device__ __forceinline__ void rg_load(const uint16_t* __restrict__ img, long long q0, long long hw,
                                        unsigned (&v)[kPix]) {
  if (q0 >= 0 && q0 + kPix <= hw) {
    const uint16_t* p = img + q0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    unsigned w[kPix / 2];
    if ((a & 15) == 0) {
      const uint4 x = reinterpret_cast<const uint4*>(p)[0], y = reinterpret_cast<const uint4*>(p)[1];
      w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w, w[4] = y.x, w[5] = y.y, w[6] = y.z, w[7] = y.w;
      rg_unpack(w, v);
    } else if ((a & 7) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint2 x = reinterpret_cast<const uint2*>(p)[k];
        w[2 * k] = x.x, w[2 * k + 1] = x.y;
      }
      rg_unpack(w, v);
    } else if ((a & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = reinterpret_cast<const unsigned*>(p)[k];
      rg_unpack(w, v);
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k) v[k] = p[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const long long q = q0 + k;
      v[k] = q >= 0 && q < hw ? (unsigned)img[q] : kOut;
    }
  }
}

// the kPix intensities from p0 on (0 past the frame's end; never read there)
__device__ __forceinline__ void rg_load_u8(const uint8_t* __restrict__ img, long long p0, long long hw,
                                           unsigned (&v)[kPix]) {
  const uint8_t* p = img + p0;
  if (p0 + kPix <= hw && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const uint4 x = reinterpret_cast<const uint4*>(p)[0];
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = p0 + k < hw ? (unsigned)p[k] : 0u;
  }
}

// grid: frames x bx; block b of frame f walks pieces b, b + bx, ...
__global__ __launch_bounds__(kThreads) void k_rg_mark(const uint16_t* __restrict__ lab, long long hw, unsigned bx,
                                                       unsigned* __restrict__ bits) {
  __shared__ unsigned sb[kWords];
  for (int i = threadIdx.x; i < kWords; i += kThreads) sb[i] = 0;
  __syncthreads();
  const size_t f = blockIdx.x / bx;
  const unsigned b = blockIdx.x % bx;
  const uint16_t* g = lab + f * (size_t)hw;
  for (long long base = (long long)b * kPiece; base < hw; base += (long long)bx * kPiece) {
    const long long p0 = base + threadIdx.x * (long long)kPix;
    if (p0 >= hw) continue;
    unsigned a[kPix];
    rg_load(g, p0, hw, a);
    unsigned prev = 0;  // background needs no bit
#pragma unroll
    for (int k = 0; k < kPix; ++k) {  // one LDS atomic per run of equal labels
      const unsigned l = a[k];
      if (l != prev && l != 0 && l != kOut) atomicOr(&sb[l >> 5], 1u << (l & 31));
      prev = l;
    }
  }
  __syncthreads();
  unsigned* out = bits + f * kWords;
  for (int i = threadIdx.x; i < kWords; i += kThreads) {
    const unsigned v = sb[i];
    if (v) atomicOr(out + i, v);
  }
}

// one block per frame: the number of set bits before each word, and the total
__global__ __launch_bounds__(kThreads) void k_rg_rank(const unsigned* __restrict__ bits, int* __restrict__ prefix,
                                                       int* __restrict__ counts) {
  __shared__ int sh[kThreads];
  constexpr int per = kWords / kThreads;
  const unsigned* b = bits + (size_t)blockIdx.x * kWords;
  int* pre = prefix + (size_t)blockIdx.x * kWords;
  unsigned w[per];
  int sum = 0;
  for (int k = 0; k < per; ++k) {
    w[k] = b[threadIdx.x * per + k];
    sum += __popc(w[k]);
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const int v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int run = sh[threadIdx.x] - sum;
  for (int k = 0; k < per; ++k) {
    pre[threadIdx.x * per + k] = run;
    run += __popc(w[k]);
  }
  if (threadIdx.x == kThreads - 1) counts[blockIdx.x] = sh[threadIdx.x];
}

// one block: offsets[f] = the objects of the frames before f, offsets[n] = all
__global__ __launch_bounds__(kThreads) void k_rg_scan(const int* __restrict__ counts, int n,
                                                       int* __restrict__ offsets) {
  __shared__ int sh[kThreads];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + threadIdx.x;
    const int c = i < n ? counts[i] : 0;
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
      const int v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
      __syncthreads();
      sh[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < n) offsets[i] = carry + sh[threadIdx.x] - c;
    __syncthreads();
    if (threadIdx.x == kThreads - 1) carry += sh[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[n] = carry;
}

// a thread per bitmap word: the records of its labels
__global__ __launch_bounds__(kThreads) void k_rg_init(const unsigned* __restrict__ bits,
                                                       const int* __restrict__ prefix,
                                                       const int* __restrict__ offsets, long long nwords, int has_image,
                                                       unet_region_record* __restrict__ rec) {
  const long long i = blockIdx.x * (long long)kThreads + threadIdx.x;
  if (i >= nwords) return;
  const int f = (int)(i / kWords), wd = (int)(i % kWords);
  unsigned v = bits[i];
  unet_region_record* r = rec + offsets[f] + prefix[i];
  for (; v; v &= v - 1, ++r) {
    unet_region_record o;
    memset(&o, 0, sizeof o);
    o.frame = f;
    o.label = wd * 32 + __builtin_ctz(v);
    o.min_y = o.min_x = INT_MAX;
    o.max_y = o.max_x = -1;
    o.min_v = has_image ? 255 : 0;
    *r = o;
  }
}

// compact index of a label that occurs in the frame: 0.. in ascending label order
__device__ __forceinline__ unsigned rg_rank(const unsigned* __restrict__ bits, const int* __restrict__ pre,
                                            unsigned l) {
  return (unsigned)pre[l >> 5] + __popc(bits[l >> 5] & ((1u << (l & 31)) - 1u));
}

struct Run {
  unsigned label, y, x0, r, boundary, edge, contact, sv, minv, maxv;
  unsigned long long svv;
};

__device__ __forceinline__ void rg_add_global(unet_region_record* __restrict__ q, unsigned area, unsigned boundary,
                                              unsigned edge, unsigned long long contact, int min_y, int min_x,
                                              int max_y, int max_x, unsigned long long sy, unsigned long long sx,
                                              unsigned long long syy, unsigned long long sxx, unsigned long long sxy,
                                              bool img, int min_v, int max_v, unsigned long long sv,
                                              unsigned long long svv) {
  typedef unsigned long long u64;
  atomicAdd(reinterpret_cast<unsigned*>(&q->area), area);
  if (boundary) atomicAdd(reinterpret_cast<unsigned*>(&q->boundary), boundary);
  if (edge) atomicAdd(reinterpret_cast<unsigned*>(&q->edge), edge);
  if (contact) atomicAdd(reinterpret_cast<u64*>(&q->contact), contact);
  atomicMin(&q->min_y, min_y);
  atomicMin(&q->min_x, min_x);
  atomicMax(&q->max_y, max_y);
  atomicMax(&q->max_x, max_x);
  if (sy) atomicAdd(reinterpret_cast<u64*>(&q->sum_y), sy);
  if (sx) atomicAdd(reinterpret_cast<u64*>(&q->sum_x), sx);
  if (syy) atomicAdd(reinterpret_cast<u64*>(&q->sum_yy), syy);
  if (sxx) atomicAdd(reinterpret_cast<u64*>(&q->sum_xx), sxx);
  if (sxy) atomicAdd(reinterpret_cast<u64*>(&q->sum_xy), sxy);
  if (img) {
    atomicMin(&q->min_v, min_v);
    atomicMax(&q->max_v, max_v);
    if (sv) atomicAdd(reinterpret_cast<u64*>(&q->sum_v), sv);
    if (svv) atomicAdd(reinterpret_cast<u64*>(&q->sum_vv), svv);
  }
}

// grid: frames x bands; a band is ppb consecutive pieces of the flattened frame
template <bool IMG>
__global__ __launch_bounds__(kThreads) void k_rg_accum(const uint16_t* __restrict__ lab,
                                                        const uint8_t* __restrict__ image, int h, int w,
                                                        unsigned bands, unsigned ppb, int lds_max,
                                                        const unsigned* __restrict__ bits,
                                                        const int* __restrict__ prefix, const int* __restrict__ offsets,
                                                        unet_region_record* __restrict__ rec) {
  typedef unsigned long long u64;
  __shared__ u64 s64[S_N64][kLdsMax];
  __shared__ unsigned s32[A_N32][kLdsMax];
  const long long hw = (long long)h * w;
  const int f = (int)(blockIdx.x / bands);
  const unsigned band = blockIdx.x % bands;
  const int off = offsets[f];
  const int nobj = offsets[f + 1] - off;
  if (nobj == 0) return;  // (the whole block)
  const bool lds = nobj <= lds_max;
  if (lds) {
    for (int i = threadIdx.x; i < nobj; i += kThreads) {
#pragma unroll
      for (int k = 0; k < S_N64; ++k) s64[k][i] = 0;
#pragma unroll
      for (int k = 0; k < A_N32; ++k) s32[k][i] = (k == A_MIN_Y || k == A_MIN_X || k == A_MIN_V) ? 0x7fffffffu : 0u;
    }
    __syncthreads();
  }
  const uint16_t* g = lab + (size_t)f * hw;
  const uint8_t* im = IMG ? image + (size_t)f * hw : nullptr;
  const unsigned* fb = bits + (size_t)f * kWords;
  const int* fp = prefix + (size_t)f * kWords;
  unet_region_record* frec = rec + off;

  auto flush = [&](const Run& t) {
    const unsigned i = rg_rank(fb, fp, t.label);
    if (i >= (unsigned)nobj) return;  // cannot happen: the bitmaps come from the same labels
    const u64 r = t.r, x0 = t.x0, y = t.y;
    const u64 tri = r * (r - 1) / 2;                      // sum of 0..r-1
    const u64 sx = r * x0 + tri;                          // sum of x0..x0+r-1
    const u64 sq = (r - 1) * r * (2 * r - 1) / 6;         // sum of squares of 0..r-1
    const u64 sxx = r * x0 * x0 + 2 * x0 * tri + sq;      // sum of (x0 + i)^2
    const u64 sy = r * y, syy = sy * y, sxy = y * sx;
    const unsigned x1 = t.x0 + t.r - 1;
    if (lds) {
      atomicAdd(&s32[A_AREA][i], t.r);
      if (t.boundary) atomicAdd(&s32[A_BOUNDARY][i], t.boundary);
      if (t.edge) atomicAdd(&s32[A_EDGE][i], t.edge);
      if (t.contact) atomicAdd(&s32[A_CONTACT][i], t.contact);
      atomicMin(&s32[A_MIN_Y][i], t.y);
      atomicMax(&s32[A_MAX_Y][i], t.y);
      atomicMin(&s32[A_MIN_X][i], t.x0);
      atomicMax(&s32[A_MAX_X][i], x1);
      if (sy) atomicAdd(&s64[S_Y][i], sy);
      if (sx) atomicAdd(&s64[S_X][i], sx);
      if (syy) atomicAdd(&s64[S_YY][i], syy);
      if (sxx) atomicAdd(&s64[S_XX][i], sxx);
      if (sxy) atomicAdd(&s64[S_XY][i], sxy);
      if (IMG) {
        atomicMin(&s32[A_MIN_V][i], t.minv);
        atomicMax(&s32[A_MAX_V][i], t.maxv);
        if (t.sv) atomicAdd(&s64[S_V][i], (u64)t.sv);
        if (t.svv) atomicAdd(&s64[S_VV][i], t.svv);
      }
    } else {
      rg_add_global(frec + i, t.r, t.boundary, t.edge, t.contact, (int)t.y, (int)t.x0, (int)t.y, (int)x1, sy, sx, syy,
                    sxx, sxy, IMG, (int)t.minv, (int)t.maxv, t.sv, t.svv);
    }
  };

  const long long band0 = (long long)band * ppb * kPiece;
  for (unsigned piece = 0; piece < ppb; ++piece) {
    const long long p0 = band0 + (long long)piece * kPiece + threadIdx.x * (long long)kPix;
    if (p0 >= hw) break;
    const int n = hw - p0 < kPix ? (int)(hw - p0) : kPix;
    unsigned c[kPix], up[kPix], dn[kPix], iv[kPix];
    rg_load(g, p0, hw, c);
    rg_load(g, p0 - w, hw, up);
    rg_load(g, p0 + w, hw, dn);
    if (IMG) rg_load_u8(im, p0, hw, iv);
    const unsigned lft = p0 > 0 ? (unsigned)g[p0 - 1] : kOut;
    const unsigned rgt = p0 + kPix < hw ? (unsigned)g[p0 + kPix] : kOut;
    unsigned y = (unsigned)(p0 / w), x = (unsigned)(p0 % w);
    Run t;
    t.r = 0;
    t.label = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const unsigned l = k < n ? c[k] : 0u;  // past the frame's end: background, which ends the run
      if (t.r && (l != t.label || x == 0)) {  // a run ends with its label or its row
        flush(t);
        t.r = 0;
      }
      if (l) {
        if (!t.r) {
          t.label = l;
          t.y = y;
          t.x0 = x;
          t.boundary = t.edge = t.contact = t.sv = 0;
          t.svv = 0;
          t.minv = 255;
          t.maxv = 0;
        }
        ++t.r;
        const unsigned a = up[k], b = dn[k];
        const unsigned le = x == 0 ? kOut : (k == 0 ? lft : c[k > 0 ? k - 1 : 0]);
        const unsigned ri = x == (unsigned)w - 1 ? kOut : (k == kPix - 1 ? rgt : c[k < kPix - 1 ? k + 1 : k]);
        t.boundary += (a != l) | (b != l) | (le != l) | (ri != l);
        t.edge += (y == 0) | (y == (unsigned)h - 1) | (x == 0) | (x == (unsigned)w - 1);
        // a neighbour in another object: a label 1..65535 other than l
        t.contact += (unsigned)(a != l && a - 1u < 0xffffu) + (unsigned)(b != l && b - 1u < 0xffffu) +
                     (unsigned)(le != l && le - 1u < 0xffffu) + (unsigned)(ri != l && ri - 1u < 0xffffu);
        if (IMG) {
          const unsigned v = iv[k];
          t.sv += v;
          t.svv += v * v;
          t.minv = min(t.minv, v);
          t.maxv = max(t.maxv, v);
        }
      }
      if (++x == (unsigned)w) {
        x = 0;
        ++y;
      }
    }
    if (t.r) flush(t);
  }
  if (!lds) return;
  __syncthreads();
  for (int i = threadIdx.x; i < nobj; i += kThreads) {
    const unsigned area = s32[A_AREA][i];
    if (!area) continue;
    rg_add_global(frec + i, area, s32[A_BOUNDARY][i], s32[A_EDGE][i], s32[A_CONTACT][i], (int)s32[A_MIN_Y][i],
                  (int)s32[A_MIN_X][i], (int)s32[A_MAX_Y][i], (int)s32[A_MAX_X][i], s64[S_Y][i], s64[S_X][i],
                  s64[S_YY][i], s64[S_XX][i], s64[S_XY][i], IMG, (int)s32[A_MIN_V][i], (int)s32[A_MAX_V][i],
                  s64[S_V][i], s64[S_VV][i]);
  }
}

// workspace (unet_region_props_ws_bytes): bitmaps n x 8 KB, prefix n x 8 KB,
// counts n x 4 B, each part rounded up to 256 bytes
struct RegionWs {
  unsigned* bits;
  int* prefix;
  int* counts;
  size_t total;
};

RegionWs region_ws(void* ws, int n) {
  const size_t c = (size_t)std::max(n, 1);
  RegionWs o{};
  const size_t bits = 0, prefix = bits + al256(c * kWords * 4), counts = prefix + al256(c * kWords * 4);
  o.total = counts + al256(c * 4);
  if (char* p = reinterpret_cast<char*>(ws)) {
    o.bits = reinterpret_cast<unsigned*>(p + bits);
    o.prefix = reinterpret_cast<int*>(p + prefix);
    o.counts = reinterpret_cast<int*>(p + counts);
  }
  return o;
}

// 0 = fine; the limits inside which no sum passes 63 bits and every count and
// offset fits its field
int region_args(const char* who, int n, int h, int w, long long cap) {
  if (n < 0 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim || (long long)h * w > kMaxPixels || cap < 0 ||
      (long long)n * std::min<long long>(65535, (long long)h * w) > INT_MAX) {
    errf("%s: need n >= 0, 1 <= h, w <= 32768, h w <= 2^30, cap >= 0 and at most 2^31 - 1 objects in all "
         "(n %d, h %d, w %d, cap %lld)", who, n, h, w, cap);
    return -EINVAL;
  }
  return 0;
}

}  // namespace

extern "C" {

size_t unet_region_props_ws_bytes(int n, int h, int w) {
  if (region_args("unet_region_props_ws_bytes", n, h, w, 0)) return 0;
  return region_ws(nullptr, n).total;
}

int unet_region_props(const uint16_t* labels, const uint8_t* image, int n, int h, int w, int32_t* frame_offsets,
                      unet_region_record* records, long long cap, long long* host_total, void* ws,
                      unet_stream_t stream) {
  if (host_total) *host_total = 0;
  if (const int rc = region_args("unet_region_props", n, h, w, cap)) return rc;
  const long long hw = (long long)h * w;
  const long long pieces = (hw + kPiece - 1) / kPiece;
  // bands of a frame: enough blocks to fill the device, few enough that the
  // table's set-up and flush stay small beside a block's pixels
  const long long ppb = std::max<long long>(1, std::min<long long>(8, (long long)n * pieces / 1024));
  const long long bands = (pieces + ppb - 1) / ppb;
  const long long bx = std::min<long long>(pieces, 64);
  if (!frame_offsets || !host_total || (n > 0 && (!labels || !ws || (reinterpret_cast<uintptr_t>(ws) & 255))) ||
      (cap > 0 && !records) || (reinterpret_cast<uintptr_t>(labels) & 1) ||
      (reinterpret_cast<uintptr_t>(records) & 15) || (reinterpret_cast<uintptr_t>(frame_offsets) & 3) ||
      (long long)n * bands > INT_MAX || (long long)n * bx > INT_MAX) {
    errf("unet_region_props: null labels / frame_offsets / host_total / ws (or records with cap > 0), a misaligned "
         "pointer (labels 2, frame_offsets 4, records 16, ws 256 bytes), or a stack of more than 2^31 - 1 workgroups");
    return -EINVAL;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e;
#define RG_HIP(x)                                                       \
  if ((e = (x)) != hipSuccess) {                                        \
    errf("unet_region_props: %s (%s)", hipGetErrorString(e), #x);       \
    return -EIO;                                                        \
  }
  if (n == 0) {
    RG_HIP(hipMemsetAsync(frame_offsets, 0, 4, s));
    return 0;
  }
  const RegionWs W = region_ws(ws, n);
  RG_HIP(hipMemsetAsync(W.bits, 0, (size_t)n * kWords * 4, s));
  hipLaunchKernelGGL(k_rg_mark, dim3((unsigned)(n * bx)), dim3(kThreads), 0, s, labels, hw, (unsigned)bx, W.bits);
  hipLaunchKernelGGL(k_rg_rank, dim3((unsigned)n), dim3(kThreads), 0, s, W.bits, W.prefix, W.counts);
  hipLaunchKernelGGL(k_rg_scan, dim3(1), dim3(kThreads), 0, s, W.counts, n, frame_offsets);
  RG_HIP(hipGetLastError());
  int32_t total = 0;
  RG_HIP(hipMemcpyAsync(&total, frame_offsets + n, 4, hipMemcpyDeviceToHost, s));
  RG_HIP(hipStreamSynchronize(s));
  *host_total = total;
  if (total > cap) {
    errf("unet_region_props: the stack holds %d objects, the records buffer %lld", (int)total, cap);
    return -ENOSPC;
  }
  if (total == 0) return 0;
  const long long nwords = (long long)n * kWords;
  hipLaunchKernelGGL(k_rg_init, dim3((unsigned)((nwords + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, W.bits,
                     W.prefix, frame_offsets, nwords, image ? 1 : 0, records);
  const dim3 grid((unsigned)(n * bands));
  if (image)
    hipLaunchKernelGGL(k_rg_accum<true>, grid, dim3(kThreads), 0, s, labels, image, h, w, (unsigned)bands,
                       (unsigned)ppb, lds_objects(), W.bits, W.prefix, frame_offsets, records);
  else
    hipLaunchKernelGGL(k_rg_accum<false>, grid, dim3(kThreads), 0, s, labels, image, h, w, (unsigned)bands,
                       (unsigned)ppb, lds_objects(), W.bits, W.prefix, frame_offsets, records);
  g_region_launches.fetch_add(1);
  RG_HIP(hipGetLastError());
#undef RG_HIP
  return 0;
}

int unet_region_props_host(const uint16_t* labels, const uint8_t* image, int n, int h, int w, int32_t* frame_offsets,
                           unet_region_record* records, long long cap, long long* host_total) {
  if (host_total) *host_total = 0;
  if (const int rc = region_args("unet_region_props_host", n, h, w, cap)) return rc;
  if (!frame_offsets || !host_total || (n > 0 && !labels) || (cap > 0 && !records)) {
    errf("unet_region_props_host: null labels / frame_offsets / host_total (or records with cap > 0)");
    return -EINVAL;
  }
  const size_t hw = (size_t)h * w;
  // index phase: which labels each frame holds
  std::vector<char> seen(65536);
  std::vector<int32_t> index(65536);
  long long total = 0;
  frame_offsets[0] = 0;
  for (int f = 0; f < n; ++f) {
    std::fill(seen.begin(), seen.end(), 0);
    const uint16_t* g = labels + (size_t)f * hw;
    for (size_t p = 0; p < hw; ++p) seen[g[p]] = 1;
    for (int l = 1; l < 65536; ++l) total += seen[l];
    frame_offsets[f + 1] = (int32_t)total;
  }
  *host_total = total;
  if (total > cap) {
    errf("unet_region_props_host: the stack holds %lld objects, the records buffer %lld", total, cap);
    return -ENOSPC;
  }
  for (int f = 0; f < n; ++f) {
    const uint16_t* g = labels + (size_t)f * hw;
    const uint8_t* im = image ? image + (size_t)f * hw : nullptr;
    std::fill(seen.begin(), seen.end(), 0);
    for (size_t p = 0; p < hw; ++p) seen[g[p]] = 1;
    unet_region_record* rec = records + frame_offsets[f];
    int k = 0;
    for (int l = 1; l < 65536; ++l)
      if (seen[l]) {
        unet_region_record& o = rec[k];
        std::memset(&o, 0, sizeof o);
        o.frame = f;
        o.label = l;
        o.min_y = o.min_x = INT_MAX;
        o.max_y = o.max_x = -1;
        o.min_v = im ? 255 : 0;
        index[l] = k++;
      }
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t p = (size_t)y * w + x;
        const unsigned l = g[p];
        if (!l) continue;
        unet_region_record& o = rec[index[l]];
        o.area += 1;
        o.sum_y += y;
        o.sum_x += x;
        o.sum_yy += (int64_t)y * y;
        o.sum_xx += (int64_t)x * x;
        o.sum_xy += (int64_t)y * x;
        o.min_y = std::min(o.min_y, y);
        o.min_x = std::min(o.min_x, x);
        o.max_y = std::max(o.max_y, y);
        o.max_x = std::max(o.max_x, x);
        const unsigned nb[4] = {y > 0 ? g[p - w] : kOut, y < h - 1 ? g[p + w] : kOut, x > 0 ? g[p - 1] : kOut,
                                x < w - 1 ? g[p + 1] : kOut};
        bool boundary = false;
        for (unsigned q : nb) {
          boundary |= q != l;
          o.contact += q != l && q != 0 && q != kOut;
        }
        o.boundary += boundary;
        o.edge += y == 0 || y == h - 1 || x == 0 || x == w - 1;
        if (im) {
          const int v = im[p];
          o.sum_v += v;
          o.sum_vv += (int64_t)v * v;
          o.min_v = std::min(o.min_v, v);
          o.max_v = std::max(o.max_v, v);
        }
      }
  }
  return 0;
}

long long unet_region_props_launches(int reset) {
  return reset ? g_region_launches.exchange(0) : g_region_launches.load();
}

}  // extern "C"
