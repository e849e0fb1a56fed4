// Warping error and pixel error (Jain et al., "Boundary learning by
// optimization with topological constraints", CVPR 2010; the measures the
// U-Net paper ranks by).  The reference's utils/metrics.py ends in a
// commented-out calculate_warping_error placeholder; include/unet_hip.h states
// the definition this file computes (G0, the simple-point table, the mask M
// and the four-sub-field schedule).
//
// One workgroup per frame does everything in one launch.  The frame lives in
// four bit planes of (h + 2) rows of ceil(w / 32) + 2 words: bit b of word c
// of a row is pixel x = 32 c + b, and a zero guard row and guard word all
// round (and zero bits past w in a row's last word) let every neighbour fetch
// go without a bounds test.  The planes are in LDS where 4 of them fit its 160
// KB (512 x 512: 148,032 bytes) and in the caller's workspace otherwise; the
// kernel is the same, a template on the storage.
//   1. G0 -> plane L: one pixel per lane, a wave64 ballot is two words.
//   2. M: G0 and its in-frame complement dilated `radius` times by 3 x 3
//      (word shifts + row neighbours), ping-pong between two planes, one
//      barrier per step; M = the AND of the two, in place.
//   3. T -> the plane the dilation left free; the pixel error is counted here.
//   4. sweeps: per sub-step a thread walks the words it owns in the rows of
//      the sub-field's parity; candidates = M & (L ^ T) & 0x55555555 or
//      0xAAAAAAAA.  A zero word costs its three loads; for a set bit the 3 x 3
//      neighbourhood bits index a 512-entry table (16 words of LDS, the
//      256-entry simple-point table with the centre bit ignored, built on
//      the host and passed with the arguments).  The owner
//      flips its word at once: another thread may fetch that word while it
//      changes, but the bits it reads from it are 8-neighbours of a candidate
//      of this sub-step, which are never candidates of the same sub-step, so
//      they do not change, and a word has one writer.  One barrier per
//      sub-step; the fourth is the workgroup-wide OR of "flipped something".
//   5. popcount of L ^ T, counts, and the warped plane as bytes if asked.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/unet_hip.h"
#include "unet_internal.h"

namespace {

constexpr int kMaxThreads = 1024;
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kStaticLds = 1024;  // the table, the counters and the workgroup reduction's word, with room

// ---- the simple-point table, from the definition --------------------------
// neighbour k of N, NE, E, SE, S, SW, W, NW as (dy, dx)
constexpr int kDy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
constexpr int kDx[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// components of the neighbours whose bit equals `value`, two neighbours joined
// when |dy| + |dx| <= reach (1 = 4-adjacent) or max(|dy|, |dx|) <= 1 (reach 2 =
// 8-adjacent); only components holding a neighbour with need4 satisfied count
// (need4: it is 4-adjacent to the centre, i.e. k even)
constexpr int nb_components(unsigned cfg, unsigned value, int reach, bool need4) {
  int label[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 8; ++k) label[k] = ((cfg >> k) & 1u) == value ? k + 1 : 0;
  for (int pass = 0; pass < 8; ++pass)  // propagate the smallest label (8 nodes: 8 passes suffice)
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b) {
        if (!label[a] || !label[b]) continue;
        const int dy = kDy[a] - kDy[b], dx = kDx[a] - kDx[b];
        const int ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
        const bool adj = reach == 1 ? ay + ax <= 1 : (ay <= 1 && ax <= 1);
        if (adj && label[b] < label[a]) label[a] = label[b];
      }
  int n = 0;
  for (int root = 1; root <= 8; ++root) {
    bool found = false;
    for (int k = 0; k < 8; ++k)
      if (label[k] == root && (!need4 || (k & 1) == 0)) found = true;
    n += found;
  }
  return n;
}

constexpr bool simple_cfg(unsigned cfg) {
  return nb_components(cfg, 1u, 2, false) == 1 && nb_components(cfg, 0u, 1, true) == 1;
}

// the table the kernel indexes: bit i of 512, i = up | mid << 3 | down << 6,
// each a row's three bits (x - 1, x, x + 1); the centre (bit 4) is ignored
struct Tab9 {
  unsigned v[16];
};
Tab9 make_tab9() {
  Tab9 t{};
  for (unsigned i = 0; i < 512; ++i) {
    const unsigned cfg = ((i >> 1) & 1u) | ((i >> 2) & 1u) << 1 | ((i >> 5) & 1u) << 2 | ((i >> 8) & 1u) << 3 |
                         ((i >> 7) & 1u) << 4 | ((i >> 6) & 1u) << 5 | ((i >> 3) & 1u) << 6 | (i & 1u) << 7;
    if (simple_cfg(cfg)) t.v[i >> 5] |= 1u << (i & 31);
  }
  return t;
}

// ---- the kernel -------------------------------------------------------------
struct WarpArgs {
  const uint16_t* gt;
  const uint8_t* pred;
  uint8_t* warped;
  long long* counts;
  unsigned* ws;
  int h, w, wd, stride;  // wd = ceil(w / 32) words of a row, stride = wd + 2
  int radius, separate, max_sweeps;
  unsigned last_mask;    // the valid bits of a row's last word
  size_t plane_words;    // (h + 2) * stride
  Tab9 tab;
};

// f(r, c) for the words j = tid, tid + nt, ... < nrows * wd of a thread, as
// row r = j / wd and word c = j % wd, without a division per word
template <class F>
__device__ __forceinline__ void for_words(unsigned tid, unsigned nt, unsigned nrows, unsigned wd, F&& f) {
  unsigned r = tid / wd, c = tid % wd;
  const unsigned dr = nt / wd, dc = nt % wd;
  while (r < nrows) {
    f(r, c);
    r += dr;
    c += dc;
    if (c >= wd) {
      c -= wd;
      ++r;
    }
  }
}

// bits x - 1 .. x + 32 of a row around word o, at bits 0 .. 33
template <class P, class I>
__device__ __forceinline__ unsigned long long row34(const P* p, I o) {
  return (unsigned long long)(p[o - 1] >> 31) | (unsigned long long)p[o] << 1 |
         (unsigned long long)(p[o + 1] & 1u) << 33;
}

// a word of the 3 x 3 dilation of plane p
template <class I>
__device__ __forceinline__ unsigned dilate_word(const unsigned* p, I o, I stride) {
  unsigned out = 0;
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    const I q = d < 0 ? o - stride : d > 0 ? o + stride : o;
    const unsigned m = p[q];
    out |= m | m << 1 | m >> 1 | p[q - 1] >> 31 | p[q + 1] << 31;
  }
  return out;
}

template <bool LDS>
__global__ __launch_bounds__(kMaxThreads) void k_warp(const WarpArgs a) {
  extern __shared__ unsigned smem[];
  __shared__ unsigned s_tab[16];
  __shared__ unsigned s_cnt[3];  // pixel error, warping error, flips
  using I = std::conditional_t<LDS, unsigned, size_t>;
  const unsigned tid = threadIdx.x, nt = blockDim.x;
  const unsigned h = (unsigned)a.h, w = (unsigned)a.w, wd = (unsigned)a.wd;
  const I S = (I)a.stride, pw = (I)a.plane_words;
  unsigned* base = LDS ? smem : a.ws + (size_t)blockIdx.x * 4 * a.plane_words;
  unsigned* L = base;
  unsigned* pa = base + pw;
  unsigned* pb = base + 2 * pw;
  unsigned* px = base + 3 * pw;
  const size_t frame = (size_t)blockIdx.x * h * w;
  const uint16_t* gt = a.gt + frame;
  const uint8_t* pred = a.pred + frame;

  for (I i = tid; i < 4 * pw; i += nt) base[i] = 0;
  if (tid < 16) s_tab[tid] = a.tab.v[tid];
  if (tid < 3) s_cnt[tid] = 0;
  __syncthreads();

  // a wave packs 64 consecutive pixels of a row per step
  const unsigned lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
  const unsigned cw = (w + 63) / 64;
  auto pack = [&](unsigned* plane, auto&& fg_of) {
    unsigned y = wave / cw, ch = wave % cw;
    const unsigned dy = nwaves / cw, dch = nwaves % cw;
    while (y < h) {
      const unsigned x = ch * 64 + lane;
      const bool fg = x < w && fg_of(y, x);
      const unsigned long long bits = __ballot(fg);
      if (lane == 0) {
        const I o = (I)(y + 1) * S + 1 + 2 * ch;
        plane[o] = (unsigned)bits;
        if (2 * ch + 1 < wd) plane[o + 1] = (unsigned)(bits >> 32);
      }
      y += dy;
      ch += dch;
      if (ch >= cw) {
        ch -= cw;
        ++y;
      }
    }
  };

  // 1. G0
  const bool separate = a.separate != 0;
  pack(L, [&](unsigned y, unsigned x) {
    const unsigned id = gt[(size_t)y * w + x];
    if (id == 0) return false;
    if (!separate) return true;
    const unsigned y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < h ? y + 1 : h - 1;
    const unsigned x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < w ? x + 1 : w - 1;
    bool ok = true;
    for (unsigned yy = y0; yy <= y1; ++yy)
      for (unsigned xx = x0; xx <= x1; ++xx) {
        const unsigned v = gt[(size_t)yy * w + xx];
        ok = ok && (v == 0 || v == id);
      }
    return ok;
  });
  __syncthreads();

  // 2. M (ends in pa)
  const unsigned last_mask = a.last_mask;
  if (a.radius < 0) {
    for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
      pa[(I)(r + 1) * S + c + 1] = c + 1 == wd ? last_mask : 0xffffffffu;
    });
  } else if (a.radius > 0) {
    for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
      const I o = (I)(r + 1) * S + c + 1;
      const unsigned l = L[o];
      pa[o] = l;
      pb[o] = ~l & (c + 1 == wd ? last_mask : 0xffffffffu);
    });
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
      unsigned* src = pass ? pb : pa;  // the other of pa / pb is not touched in this pass
      unsigned* dst = px;
      for (int k = 0; k < a.radius; ++k) {
        for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
          const I o = (I)(r + 1) * S + c + 1;
          dst[o] = dilate_word<I>(src, o, S) & (c + 1 == wd ? last_mask : 0xffffffffu);
        });
        __syncthreads();
        unsigned* t = src;
        src = dst;
        dst = t;
      }
      // the result is in src, the free plane is dst
      if (pass)
        pb = src;
      else
        pa = src;
      px = dst;
    }
    for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
      const I o = (I)(r + 1) * S + c + 1;
      pa[o] &= pb[o];
    });
  }
  const unsigned* M = pa;

  // 3. T into the free plane (px: every word inside the frame is written, and
  // its guards were never written); the pixel error
  unsigned* T = px;
  pack(T, [&](unsigned y, unsigned x) { return pred[(size_t)y * w + x] > 0; });
  __syncthreads();
  unsigned n_pix = 0, n_flip = 0, n_warp = 0;
  for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
    const I o = (I)(r + 1) * S + c + 1;
    n_pix += __popc(L[o] ^ T[o]);
  });

  // 4. sweeps
  auto substep = [&](int s) {
    const unsigned par = (s & 1) ? 0xAAAAAAAAu : 0x55555555u;
    const unsigned p = (unsigned)s >> 1;
    for_words(tid, nt, (h - p + 1) / 2, wd, [&](unsigned r, unsigned c) {
      const I o = (I)(2 * r + p + 1) * S + c + 1;
      const unsigned l = L[o];
      unsigned cand = M[o] & (l ^ T[o]) & par;
      if (!cand) return;
      const unsigned long long up = row34(L, o - S), mid = row34(L, o), dn = row34(L, o + S);
      unsigned flip = 0;
      while (cand) {
        const int b = __ffs(cand) - 1;
        cand &= cand - 1;
        const unsigned i9 =
            ((unsigned)(up >> b) & 7u) | ((unsigned)(mid >> b) & 7u) << 3 | ((unsigned)(dn >> b) & 7u) << 6;
        flip |= ((s_tab[i9 >> 5] >> (i9 & 31)) & 1u) << b;
      }
      if (flip) {
        L[o] = l ^ flip;
        n_flip += __popc(flip);
      }
    });
  };
  unsigned sweeps = 0;
  int converged = 0;
  for (;;) {
    const unsigned before = n_flip;
    for (int s = 0; s < 3; ++s) {
      substep(s);
      __syncthreads();
    }
    substep(3);
    const int any = __syncthreads_or(n_flip != before);
    ++sweeps;
    if (!any) {
      converged = 1;
      break;
    }
    if (a.max_sweeps > 0 && sweeps >= (unsigned)a.max_sweeps) break;
  }

  // 5. counts and the warped plane
  for_words(tid, nt, h, wd, [&](unsigned r, unsigned c) {
    const I o = (I)(r + 1) * S + c + 1;
    n_warp += __popc(L[o] ^ T[o]);
  });
  if (n_pix) atomicAdd(&s_cnt[0], n_pix);
  if (n_warp) atomicAdd(&s_cnt[1], n_warp);
  if (n_flip) atomicAdd(&s_cnt[2], n_flip);
  if (a.warped) {
    uint8_t* out = a.warped + frame;
    // x, y of pixel tid, tid + nt, ... without a division per pixel
    unsigned y = tid / w, x = tid % w;
    const unsigned dy = nt / w, dx = nt % w;
    while (y < h) {
      out[(size_t)y * w + x] = (uint8_t)((L[(I)(y + 1) * S + 1 + (x >> 5)] >> (x & 31)) & 1u);
      y += dy;
      x += dx;
      if (x >= w) {
        x -= w;
        ++y;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    long long* o = a.counts + (size_t)blockIdx.x * 5;
    o[0] = s_cnt[0];
    o[1] = s_cnt[1];
    o[2] = s_cnt[2];
    o[3] = sweeps;
    o[4] = converged;
  }
}

struct Geometry {
  int wd, stride;
  size_t plane_words, frame_bytes;  // frame_bytes: the four planes of one frame
};

bool warp_shape_ok(int n, int h, int w) {
  return n >= 1 && h >= 1 && w >= 1 && (long long)n * h * w < (1ll << 31);
}

Geometry geometry(int h, int w) {
  Geometry g{};
  g.wd = (w + 31) / 32;
  g.stride = g.wd + 2;
  g.plane_words = ((size_t)h + 2) * (size_t)g.stride;
  g.frame_bytes = 4 * g.plane_words * sizeof(unsigned);
  return g;
}

}  // namespace

extern "C" {

void unet_simple_point_table(uint8_t out[256]) {
  for (unsigned c = 0; c < 256; ++c) out[c] = simple_cfg(c) ? 1 : 0;
}

size_t unet_warping_error_ws_bytes(int n, int h, int w) {
  if (!warp_shape_ok(n, h, w)) return 0;
  const size_t b = (size_t)n * geometry(h, w).frame_bytes;
  return (b + 255) / 256 * 256;
}

int unet_warping_error(const uint16_t* gt, const uint8_t* pred, int n, int h, int w, int radius, int separate,
                       int max_sweeps, int flags, uint8_t* warped, int64_t* counts, void* ws, unet_stream_t stream) {
  if (!warp_shape_ok(n, h, w) || radius < -1 || radius > 255 || max_sweeps < 0) {
    char buf[256];
    std::snprintf(buf, sizeof buf,
                  "unet_warping_error: need n, h, w >= 1, n h w < 2^31, -1 <= radius <= 255, max_sweeps >= 0 "
                  "(n %d, h %d, w %d, radius %d, max_sweeps %d)", n, h, w, radius, max_sweeps);
    unet::set_last_error(buf);
    return -EINVAL;
  }
  if (!gt || !pred || !counts) {
    unet::set_last_error("unet_warping_error: null gt / pred / counts");
    return -EINVAL;
  }
  const Geometry g = geometry(h, w);
  const bool lds = !(flags & UNET_WARP_FORCE_WS) && g.frame_bytes + kStaticLds <= kLdsBytes;
  if (!lds && (!ws || (reinterpret_cast<uintptr_t>(ws) & 255))) {
    unet::set_last_error("unet_warping_error: the planes need the workspace: null ws, or ws not 256-byte aligned");
    return -EINVAL;
  }
  WarpArgs a{};
  a.gt = gt;
  a.pred = pred;
  a.warped = warped;
  a.counts = reinterpret_cast<long long*>(counts);
  a.ws = reinterpret_cast<unsigned*>(ws);
  a.h = h;
  a.w = w;
  a.wd = g.wd;
  a.stride = g.stride;
  a.radius = radius;
  a.separate = separate;
  a.max_sweeps = max_sweeps;
  a.last_mask = (w & 31) ? (1u << (w & 31)) - 1u : 0xffffffffu;
  a.plane_words = g.plane_words;
  static const Tab9 tab = make_tab9();
  a.tab = tab;
  // a thread per word, whole waves, at most 1024
  const size_t words = (size_t)h * g.wd;
  const unsigned threads = (unsigned)std::min<size_t>(kMaxThreads, (words + 63) / 64 * 64);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (lds) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_warp<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(kLdsBytes - kStaticLds));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_warp<true>, dim3(n), dim3(threads), g.frame_bytes, s, a);
      e = hipGetLastError();
    }
  } else {
    hipLaunchKernelGGL(k_warp<false>, dim3(n), dim3(threads), 0, s, a);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    unet::set_last_error(std::string("unet_warping_error: ") + hipGetErrorString(e));
    return -EIO;
  }
  return 0;
}

}  // extern "C"
