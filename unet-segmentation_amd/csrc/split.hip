// Marker-seeded instance masks (unet_split_instances, include/unet_hip.h):
// unet_instance_masks with touching cells separated.  The reference labels
// plain 8-connected components (get_instance_masks, utils/metrics.py:42-72) and
// leaves the separation to a post-processing it does not have.
//
// 1. d2: exact squared distance to the nearest in-frame background pixel, the
//    one-nearest case of weightmap.hip's border mode.  k_sp_cols (a thread per
//    column) scans down and up for the vertically nearest background row and
//    stores its squared distance; k_sp_rows (a thread per pixel) completes
//    min over x' of (x - x')^2 + g(x') from the row staged in LDS, sweeping
//    outwards and stopping once the columns still to come cannot lower any
//    lane's minimum -- or, when d2 itself is not asked for, once the
//    comparison with core_d2 is decided.
// 2. Markers: fg & (d2 >= core_d2), or the caller's; their components are
//    numbered by postproc.hip's union-find and scan (cc_union_mask, cc_number).
// 3. Growth (k_sp_grow): one workgroup per frame, 64-bit keys
//    dist << 32 | label in the workspace (1 MiB for a 512 x 512 frame: L2
//    resident, too large for LDS), relaxed in place by directional sweeps --
//    down and up over rows (threads across x, predecessors the three pixels of
//    the previous row), right and left over columns -- with one barrier per
//    line, until a round of four sweeps changes nothing.  The least fixed point
//    is unique, so neither the sweep order nor the workgroup size shows in the
//    result.  A sweep carries a label along any path monotone in its
//    direction, so the number of rounds follows the turns of the geodesic
//    paths, not their length, where level-by-level steps need one barrier
//    round over the whole frame per unit of distance.
// 4. Numbering: union-find again, joining foreground neighbours of equal
//    label (unreached pixels carry label 0: a component without a marker stays
//    one segment); roots are first pixels, so the scan of the root flags is the
//    raster numbering; min_size as k_cc_label.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <string>

#include "unet_hip.h"
#include "unet_internal.h"

namespace unet {

int g_split_threads = -1;

namespace {

typedef unsigned long long u64;

constexpr int kSpChunk = 512;     // columns per LDS stage of k_sp_rows
constexpr int kSpNone = 1 << 30;  // no background in the column; > any h^2 + w^2 (h, w <= 16384)
constexpr int kSpMaxDim = 16384;
// keys: dist << 32 | label.  dist < h w < 2^31 - 1, so neither constant is a key, and adding kStep to either does
// not wrap
constexpr u64 kBg = 0xFFFFFFFE00000000ull;         // background: never relaxed, never a useful predecessor
constexpr u64 kUnreached = 0x7FFFFFFF00000000ull;  // foreground no marker has reached (label field 0)
constexpr u64 kStep = 1ull << 32;

// g[y][x] = squared distance from row y to the nearest background row of column x (0 on background, kSpNone
// where the column has none)
__global__ __launch_bounds__(64) void k_sp_cols(const uint8_t* __restrict__ mask, int h, int w, int* __restrict__ g) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  const size_t off = (size_t)blockIdx.y * h * w + x;
  const uint8_t* m = mask + off;
  int* c = g + off;
  int last = -1;
#pragma unroll 8
  for (int y = 0; y < h; ++y) {
    if (!m[(size_t)y * w]) last = y;
    c[(size_t)y * w] = last < 0 ? kSpNone : (y - last) * (y - last);
  }
  last = -1;
#pragma unroll 8
  for (int y = h - 1; y >= 0; --y) {
    if (!m[(size_t)y * w]) last = y;
    if (last >= 0) c[(size_t)y * w] = min(c[(size_t)y * w], (last - y) * (last - y));
  }
}

// d2 = min over x' of (x - x')^2 + g[y][x'] (k_wb_rows's sweep with one candidate per column); exact == 0: only
// mk = fg & (d2 >= core_d2) is needed, so a wave also stops once every lane is decided
__global__ __launch_bounds__(256) void k_sp_rows(const uint8_t* __restrict__ mask, const int* __restrict__ g, int w,
                                                 int tiles, int core_d2, int exact, int* __restrict__ d2o,
                                                 uint8_t* __restrict__ mk) {
  __shared__ int sh[kSpChunk];
  const int tile = blockIdx.x % tiles;
  const size_t row = blockIdx.x / tiles;  // frame * h + y
  const int* gr = g + row * w;
  const int x = tile * 256 + threadIdx.x;
  const int wx0 = __builtin_amdgcn_readfirstlane(tile * 256 + (int)(threadIdx.x & ~63u));
  const int nchunk = (w + kSpChunk - 1) / kSpChunk, home = min(tile * 256 + 128, w - 1) / kSpChunk;
  int b = kSpNone;
  for (int cc = 0; cc < nchunk; ++cc) {  // the workgroup's own chunk first
    const int c0 = (home + cc) % nchunk * kSpChunk;
    const int len = min(kSpChunk, w - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += 256) sh[i] = gr[c0 + i];
    __syncthreads();
    if (wx0 >= w) continue;  // a wave past the row's end (wave-uniform; it still meets the barriers)
    const int pc = min(max(min(wx0 + 32, w - 1) - c0, 0), len - 1);
    for (int k = 0; pc + k < len || pc - 1 - k >= 0; ++k) {
      // the columns still to come are at least gap away from every lane's column
      const int ir = pc + k, il = pc - 1 - k;
      const int gapr = ir < len ? max(c0 + ir - (wx0 + 63), 0) : 0x7fff, gapl = il >= 0 ? max(wx0 - (c0 + il), 0) : 0x7fff;
      const int gap = min(gapr, gapl), g2 = gap * gap;
      if (__all(g2 >= b || (!exact && (g2 >= core_d2 || b < core_d2)))) break;
      if (ir < len) {
        const int dx = x - (c0 + ir);
        b = min(b, dx * dx + sh[ir]);
      }
      if (il >= 0) {
        const int dx = x - (c0 + il);
        b = min(b, dx * dx + sh[il]);
      }
    }
  }
  if (x >= w) return;
  const size_t i = row * w + x;
  if (d2o) d2o[i] = b;
  if (mk) mk[i] = mask[i] && b >= core_d2;
}

// marker set without a distance: fg, or the caller's markers within fg
__global__ void k_sp_mark(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ markers, size_t total,
                          uint8_t* __restrict__ mk) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < total) mk[i] = mask[i] && (!markers || markers[i]);
}

// one line of a sweep: pixel t of the line at `line`, predecessors t - 1, t, t + 1 of the line at `prev`
__device__ __forceinline__ bool relax_line(u64* k, size_t line, size_t prev, size_t st, int len) {
  bool changed = false;
  for (int t = threadIdx.x; t < len; t += blockDim.x) {
    const u64 own = k[line + t * st];
    if (own == kBg) continue;
    u64 m = k[prev + t * st];
    if (t > 0) m = min(m, k[prev + (t - 1) * st]);
    if (t + 1 < len) m = min(m, k[prev + (t + 1) * st]);
    m += kStep;
    if (m < own) {
      k[line + t * st] = m;
      changed = true;
    }
  }
  return changed;
}

// parent / is_root / rank: the numbered forest of the marker components (cc_number)
__global__ __launch_bounds__(1024) void k_sp_grow(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ mk,
                                                  const int* __restrict__ parent, const int* __restrict__ is_root,
                                                  const int* __restrict__ rank, int n, int h, int w, u64* keys,
                                                  int* __restrict__ info) {
  __shared__ int sh_max;
  const int f = blockIdx.x;
  const size_t hw = (size_t)h * w, base = f * hw, total = n * hw;
  const int r0 = rank[base];
  const int nm = (f + 1 < n ? rank[base + hw] : rank[total - 1] + is_root[total - 1]) - r0;
  u64* k = keys + base;
  for (size_t i = threadIdx.x; i < hw; i += blockDim.x) {
    const size_t gi = base + i;
    k[i] = !mask[gi] ? kBg : mk[gi] ? (u64)(rank[parent[gi]] - r0 + 1) : kUnreached;
  }
  if (threadIdx.x == 0) sh_max = 0;
  __syncthreads();
  bool more = nm > 0;  // uniform over the workgroup
  while (more) {
    bool ch = false;
    for (int y = 1; y < h; ++y) {
      ch |= relax_line(k, (size_t)y * w, (size_t)(y - 1) * w, 1, w);
      __syncthreads();
    }
    for (int y = h - 2; y >= 0; --y) {
      ch |= relax_line(k, (size_t)y * w, (size_t)(y + 1) * w, 1, w);
      __syncthreads();
    }
    for (int x = 1; x < w; ++x) {
      ch |= relax_line(k, x, x - 1, w, h);
      __syncthreads();
    }
    for (int x = w - 2; x >= 0; --x) {
      ch |= relax_line(k, x, x + 1, w, h);
      __syncthreads();
    }
    more = __syncthreads_or(ch);
  }
  int mx = 0;
  for (size_t i = threadIdx.x; i < hw; i += blockDim.x) {
    const u64 v = k[i];
    if (v < kUnreached) mx = max(mx, (int)(v >> 32));
  }
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) atomicMax(&sh_max, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    info[4 * f + 0] = nm;
    info[4 * f + 2] = sh_max;
    info[4 * f + 3] = nm > 65535;
  }
}

// segments: foreground neighbours of equal label (unreached = 0) are one
__global__ void k_sp_seg_init(const u64* __restrict__ keys, size_t total, int* __restrict__ parent) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < total) parent[i] = keys[i] == kBg ? -1 : (int)i;
}

__global__ void k_sp_seg_union(const u64* __restrict__ keys, int n, int h, int w, int* __restrict__ parent) {
  const size_t hw = (size_t)h * w;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)n * hw || keys[i] == kBg) return;
  const unsigned lab = (unsigned)keys[i];
  const int p = (int)(i % hw);
  const int y = p / w, x = p - (p / w) * w;
  auto same = [&](size_t j) { return keys[j] != kBg && (unsigned)keys[j] == lab; };
  if (x > 0 && same(i - 1)) uf_union(parent, (int)i, (int)i - 1);
  if (y > 0) {
    if (x > 0 && same(i - w - 1)) uf_union(parent, (int)i, (int)(i - w - 1));
    if (same(i - w)) uf_union(parent, (int)i, (int)(i - w));
    if (x + 1 < w && same(i - w + 1)) uf_union(parent, (int)i, (int)(i - w + 1));
  }
}

// k_cc_label's numbering; a frame's first pixel also writes its segment count and overflow
__global__ void k_sp_label(size_t total, size_t hw, const int* __restrict__ parent, const int* __restrict__ is_root,
                           const int* __restrict__ rank, const unsigned* __restrict__ size, int min_size,
                           uint16_t* __restrict__ out, int* __restrict__ info) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t f = i / hw, first = f * hw;
  if (i == first) {
    const int segs = (first + hw < total ? rank[first + hw] : rank[total - 1] + is_root[total - 1]) - rank[first];
    info[4 * f + 1] = segs;
    if (segs > 65535) info[4 * f + 3] = 1;
  }
  const int r = parent[i];  // flattened by cc_number
  out[i] = r < 0 || (int)size[r] < min_size ? 0 : (uint16_t)(rank[r] - rank[first] + 1);
}

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

char* carve(char*& p, size_t bytes) {
  char* r = p;
  p += al256(bytes);
  return r;
}

bool split_shape_ok(int n, int h, int w) {
  return n >= 1 && h >= 1 && w >= 1 && h <= kSpMaxDim && w <= kSpMaxDim && n <= 65535 &&
         (size_t)n * h * w < ((size_t)1 << 31);
}

}  // namespace

// keys (8 B per pixel; the column distances live there before the keys do), parent, is_root, rank, size (4 B
// each), the marker plane (1 B), the scan's scratch
size_t split_instances_ws_bytes(int n, int h, int w) {
  if (!split_shape_ok(n, h, w)) return 0;
  const size_t total = (size_t)n * h * w, scan = cc_scan_bytes(total);
  return scan ? al256(total * 8) + 4 * al256(total * 4) + al256(total) + al256(scan) : 0;
}

hipError_t launch_split_instances(const uint8_t* mask, const uint8_t* markers, int n, int h, int w, int core_d2,
                                  int min_size, uint16_t* labels, int32_t* d2, int32_t* info, void* ws, hipStream_t s) {
  if (!split_shape_ok(n, h, w)) return hipErrorInvalidValue;
  const size_t total = (size_t)n * h * w, hw = (size_t)h * w, scan = cc_scan_bytes(total);
  if (!scan) return hipErrorInvalidValue;
  char* p = reinterpret_cast<char*>(ws);
  u64* keys = reinterpret_cast<u64*>(carve(p, total * 8));
  int* parent = reinterpret_cast<int*>(carve(p, total * 4));
  int* is_root = reinterpret_cast<int*>(carve(p, total * 4));
  int* rank = reinterpret_cast<int*>(carve(p, total * 4));
  unsigned* size = reinterpret_cast<unsigned*>(carve(p, total * 4));
  uint8_t* mk = reinterpret_cast<uint8_t*>(carve(p, total));
  void* tmp = carve(p, scan);
  const unsigned g = (unsigned)((total + 255) / 256);
  const bool dist = d2 || (!markers && core_d2 > 0);
  if (dist) {
    int* gcol = reinterpret_cast<int*>(keys);
    const int tiles = (w + 255) / 256;
    hipLaunchKernelGGL(k_sp_cols, dim3((w + 63) / 64, n), dim3(64), 0, s, mask, h, w, gcol);
    hipLaunchKernelGGL(k_sp_rows, dim3((unsigned)((size_t)n * h * tiles)), dim3(256), 0, s, mask, gcol, w, tiles,
                       core_d2, d2 ? 1 : 0, d2, markers ? nullptr : mk);
  }
  if (markers || !dist) hipLaunchKernelGGL(k_sp_mark, dim3(g), dim3(256), 0, s, mask, markers, total, mk);
  cc_union_mask(mk, n, h, w, parent, s);
  hipError_t e = cc_number(total, parent, is_root, rank, size, tmp, scan, s);
  if (e != hipSuccess) return e;
  const int threads = g_split_threads > 0 ? g_split_threads : 1024;
  hipLaunchKernelGGL(k_sp_grow, dim3(n), dim3(threads), 0, s, mask, mk, parent, is_root, rank, n, h, w, keys, info);
  hipLaunchKernelGGL(k_sp_seg_init, dim3(g), dim3(256), 0, s, keys, total, parent);
  hipLaunchKernelGGL(k_sp_seg_union, dim3(g), dim3(256), 0, s, keys, n, h, w, parent);
  e = cc_number(total, parent, is_root, rank, size, tmp, scan, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sp_label, dim3(g), dim3(256), 0, s, total, hw, parent, is_root, rank, size, min_size, labels,
                     info);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

size_t unet_split_instances_ws_bytes(int n, int h, int w) { return unet::split_instances_ws_bytes(n, h, w); }

int unet_split_instances(const uint8_t* mask, const uint8_t* markers, int n, int h, int w, int core_d2, int min_size,
                         uint16_t* labels, int32_t* d2, int32_t* info, void* ws, unet_stream_t stream) {
  if (!unet::split_shape_ok(n, h, w) || min_size < 0 ||
      (!markers && (core_d2 < 0 || core_d2 > (1 << 30)))) {
    char buf[256];
    std::snprintf(buf, sizeof buf,
                  "unet_split_instances: need 1 <= h, w <= 16384, 1 <= n <= 65535, n h w < 2^31, 0 <= core_d2 <= 2^30, "
                  "min_size >= 0 (n %d, h %d, w %d, core_d2 %d, min_size %d)", n, h, w, core_d2, min_size);
    unet::set_last_error(buf);
    return -EINVAL;
  }
  if (!mask || !labels || !info || !ws || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    unet::set_last_error("unet_split_instances: null mask / labels / info / ws, or ws not 256-byte aligned");
    return -EINVAL;
  }
  const hipError_t e = unet::launch_split_instances(mask, markers, n, h, w, core_d2, min_size, labels, d2, info, ws,
                                                    reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) {
    unet::set_last_error(std::string("unet_split_instances: ") + hipGetErrorString(e));
    return e == hipErrorInvalidValue ? -EINVAL : -EIO;
  }
  return 0;
}

}  // extern "C"
