// Distance-based linker ("Distance-based linker"): the objects of
// frame f are assigned to the objects of frame f + 1 by the squared distance of
// their quantised centroids, inside a gate, with a private "no successor" column
// per previous object.  Unlike the IoU tracker the assignment of a frame pair
// reads those two frames only, so every pair of a sequence is solved in one
// launch, one workgroup per pair.
//
//   k_link   prologue: the quantised centroids of the pair's P previous and C
//            current objects from the region records.
//            Per row (previous object, ascending): a Dijkstra search for the
//            shortest augmenting path.  One iteration relaxes the unscanned
//            columns in parallel (a thread owns columns tid, tid + 256, ...; the
//            cost d(i, j) is computed from the centroids in registers, the
//            matrix is never stored), then two workgroup reductions pick the
//            next column: the least distance first, then the least
//            (assigned flag, column index) among the lanes that hold it.  Two
//            barriers per iteration, two more per row (dual update, augment).
//            Epilogue: prev / dist of every current object, the pair's total,
//            and the mother of every birth.
//   The arrays (centroids, duals, shortest, path, col4row, row4col, scanned
//   flags: 33 bytes per object + 12 per previous object) sit in LDS where the
//   pair's P + C fits ("link_lds_objects"), in the workspace otherwise; the code
//   is the same.  The kernel is bound by barrier latency: a search iteration is
//   a few LDS reads per column between two barriers.
//
// unet_link_frames_host is the explicit algorithm in plain loops (the matrix is
// stored, the P private columns are real columns); unet_link_assemble chains
// the links into tracks on the host.  All arithmetic is integer.
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

namespace unet {
// unet_set_tuning("link_lds_objects", n): most objects P + C of a frame pair
// that k_link serves from LDS (0 = every pair from the workspace; at most
// kLdsMaxObjects; -1 = the default, kLdsMaxObjects)
int g_link_lds_objects = -1;
}  // namespace unet

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kInf = LLONG_MAX;
constexpr int kLdsBytes = 160 * 1024;     // a CU's LDS, all of it for one workgroup
constexpr int kScratch = 128;             // reduction scratch at the head of the LDS block
constexpr int kPerObject = 45;            // bytes of the arrays per object when every object is a row too
constexpr int kLdsMaxObjects = 3600;      // kScratch + 45 x 3600 + alignment slack < 160 KB
constexpr long long kMaxTotal = (1ll << 30) - 1;  // 2 x total indexes the per-column arrays
static_assert(kScratch + kPerObject * kLdsMaxObjects + 64 <= kLdsBytes, "the LDS arrays fit a CU");

std::atomic<long long> g_link_launches{0};

int lds_objects() {
  return unet::g_link_lds_objects < 0 ? kLdsMaxObjects : std::min(unet::g_link_lds_objects, kLdsMaxObjects);
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

// quantised centroid coordinate in 1/16 pixel: floor((32 sum + area) / (2 area))
__host__ __device__ inline int quant(long long sum, long long area) {
  return area > 0 ? (int)((32 * sum + area) / (2 * area)) : 0;
}

__host__ __device__ inline long long dist2(int ay, int ax, int by, int bx) {
  const long long dy = (long long)ay - by, dx = (long long)ax - bx;
  return dy * dy + dx * dx;
}

// ------------------------------- GPU part ------------------------------------
// the arrays of one frame pair with M = P + C objects; objects 0..P-1 are the
// previous frame's, P..M-1 the current frame's; columns 0..C-1 are the current
// objects, column C + i is row i's private one
struct Arr {
  long long *v, *sh, *u;              // column duals, shortest[], row duals
  int *path, *r4c, *c4r, *qy, *qx;    // path[], row4col, col4row, centroids
  unsigned char* sc;                  // scanned flags of the columns
};

// workspace (unet_link_ws_bytes), T = total: per-column arrays hold 2 T
// elements (pair f starts at offsets[f] + offsets[f + 1] and has
// offsets[f + 2] - offsets[f] columns: the pairs tile [0, 2 T) without
// overlap), per-row arrays T (pair f starts at offsets[f])
struct LinkWs {
  size_t v, sh, u, path, r4c, c4r, qy, qx, sc, total;
};

LinkWs link_ws(long long T) {
  LinkWs o{};
  const size_t t = (size_t)T;
  size_t at = 0;
  auto part = [&](size_t bytes) {
    const size_t r = at;
    at += al256(bytes);
    return r;
  };
  o.v = part(16 * t);
  o.sh = part(16 * t);
  o.u = part(8 * t);
  o.path = part(8 * t);
  o.r4c = part(8 * t);
  o.c4r = part(4 * t);
  o.qy = part(8 * t);
  o.qx = part(8 * t);
  o.sc = part(2 * t);
  o.total = at;
  return o;
}

template <class T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
  for (int m = 32; m; m >>= 1) {
    const T y = __shfl_xor(x, m);
    x = y < x ? y : x;
  }
  return x;
}

__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
  for (int m = 32; m; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

__device__ __forceinline__ void link_pair(const Arr a, const int P, const int C, const long long g2,
                                          const long long gd2, const unet_region_record* __restrict__ rec,
                                          const int o0, const int o1, int32_t* __restrict__ prev,
                                          int64_t* __restrict__ dist, int32_t* __restrict__ mother,
                                          int64_t* __restrict__ pair_total, long long* wmin, unsigned* wkey) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = P + C;
  // prologue: centroids (the records of the two frames are consecutive) and
  // the neutral state
  for (int k = tid; k < M; k += kThreads) {
    const unet_region_record& r = rec[o0 + k];
    a.qy[k] = quant(r.sum_y, r.area);
    a.qx[k] = quant(r.sum_x, r.area);
    a.v[k] = 0;
    a.sh[k] = kInf;
    a.sc[k] = 0;
    a.r4c[k] = -1;
    a.path[k] = -1;
    if (k < P) {
      a.u[k] = 0;
      a.c4r[k] = -1;
    }
  }
  __syncthreads();
  for (int cur = 0; cur < P; ++cur) {
    long long minval = 0;
    int i = cur, sink = -1;
    for (int it = 0; it <= M; ++it) {  // a search scans a column per iteration: at most M
      const long long ui = a.u[i];
      const int iy = a.qy[i], ix = a.qx[i];
      long long lv = kInf;
      unsigned lk = ~0u;
      for (int j = tid; j < M; j += kThreads) {
        if (a.sc[j]) continue;
        long long s = a.sh[j];
        long long c = -1;  // absent
        if (j < C) {
          const long long d = dist2(iy, ix, a.qy[P + j], a.qx[P + j]);
          if (d <= g2) c = d;
        } else if (j - C == i) {
          c = g2;
        }
        if (c >= 0) {
          const long long r = minval + c - ui - a.v[j];
          if (r < s) {
            s = r;
            a.sh[j] = r;
            a.path[j] = i;
          }
        }
        if (s != kInf) {
          const unsigned key = (a.r4c[j] >= 0 ? 0x80000000u : 0u) | (unsigned)j;
          if (s < lv || (s == lv && key < lk)) {
            lv = s;
            lk = key;
          }
        }
      }
      // the least distance, then the least (assigned, index) among its holders
      const long long wv = wave_min(lv);
      if (lane == 0) wmin[wave] = wv;
      __syncthreads();
      long long gmin = wmin[0];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) gmin = wmin[k] < gmin ? wmin[k] : gmin;
      if (gmin == kInf) break;  // (infeasible: cannot happen, row i's private column is always there)
      const unsigned wk = wave_min(lv == gmin ? lk : ~0u);
      if (lane == 0) wkey[wave] = wk;
      __syncthreads();
      unsigned gk = wkey[0];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) gk = wkey[k] < gk ? wkey[k] : gk;
      const int j = (int)(gk & 0x7fffffffu);
      minval = gmin;
      if (j % kThreads == tid) a.sc[j] = 1;
      if (!(gk >> 31)) {
        sink = j;
        break;
      }
      i = a.r4c[j];
    }
    // duals: a scanned column j gives minval - shortest[j] to v[j] and, where
    // it is assigned, to the dual of its row (the rows the search visited)
    for (int j = tid; j < M; j += kThreads) {
      if (a.sc[j]) {
        const long long delta = minval - a.sh[j];
        a.v[j] -= delta;
        const int r = a.r4c[j];
        if (r >= 0) a.u[r] += delta;
        a.sc[j] = 0;
      }
      a.sh[j] = kInf;
    }
    if (tid == 0) a.u[cur] += minval;
    __syncthreads();
    if (tid == 0 && sink >= 0) {
      int j = sink;
      for (int guard = 0; guard <= P; ++guard) {
        const int r = a.path[j];
        a.r4c[j] = r;
        const int t = a.c4r[r];
        a.c4r[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  // epilogue
  long long sum = 0;
  for (int r = tid; r < P; r += kThreads) {
    const int j = a.c4r[r];
    sum += (j >= 0 && j < C) ? dist2(a.qy[r], a.qx[r], a.qy[P + j], a.qx[P + j]) : g2;
  }
  sum = wave_sum(sum);
  if (lane == 0) wmin[wave] = sum;
  for (int j = tid; j < C; j += kThreads) {
    const int r = a.r4c[j];
    const int jy = a.qy[P + j], jx = a.qx[P + j];
    int m = -1;
    if (r < 0 && gd2 > 0) {
      long long best = kInf;
      for (int q = 0; q < P; ++q) {
        const int cq = a.c4r[q];
        if (cq < 0 || cq >= C) continue;  // no linked successor
        const long long d = dist2(a.qy[q], a.qx[q], jy, jx);
        if (d <= gd2 && d < best) {
          best = d;
          m = q;
        }
      }
    }
    prev[o1 + j] = r >= 0 ? o0 + r : -1;
    dist[o1 + j] = r >= 0 ? dist2(a.qy[r], a.qx[r], jy, jx) : -1;
    mother[o1 + j] = m >= 0 ? o0 + m : -1;
  }
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
    for (int k = 0; k < kWaves; ++k) t += wmin[k];
    *pair_total = t;
  }
}

// grid: max(n - 1, 1) workgroups; workgroup f serves the pair (f, f + 1), and
// workgroup 0 also gives frame 0 its -1s
__global__ __launch_bounds__(kThreads) void k_link(const unet_region_record* __restrict__ rec,
                                                    const int32_t* __restrict__ offsets, int n, int total,
                                                    long long g2, long long gd2, int lds_cap,
                                                    int32_t* __restrict__ prev, int64_t* __restrict__ dist,
                                                    int32_t* __restrict__ mother, int64_t* __restrict__ pair_total,
                                                    char* __restrict__ ws, LinkWs W) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int f = blockIdx.x;
  const int o0 = offsets[f], o1 = offsets[f + 1];
  // offsets that do not ascend inside [0, total] would index outside the
  // buffers: such a workgroup writes nothing
  if (o0 < 0 || o1 < o0 || o1 > total) return;
  if (f == 0)
    for (int k = threadIdx.x; k < o1; k += kThreads) {
      prev[k] = -1;
      dist[k] = -1;
      mother[k] = -1;
    }
  if (f + 1 >= n) return;
  const int o2 = offsets[f + 2];
  if (o2 < o1 || o2 > total) return;
  const int P = o1 - o0, C = o2 - o1, M = P + C;
  long long* wmin = reinterpret_cast<long long*>(smem);
  unsigned* wkey = reinterpret_cast<unsigned*>(smem + 64);
  Arr a;
  if (M <= lds_cap) {
    const size_t L = (size_t)lds_cap;
    char* p = smem + kScratch;
    a.v = reinterpret_cast<long long*>(p);
    a.sh = a.v + L;
    a.u = a.sh + L;
    a.path = reinterpret_cast<int*>(a.u + L);
    a.r4c = a.path + L;
    a.c4r = a.r4c + L;
    a.qy = a.c4r + L;
    a.qx = a.qy + L;
    a.sc = reinterpret_cast<unsigned char*>(a.qx + L);
    link_pair(a, P, C, g2, gd2, rec, o0, o1, prev, dist, mother, pair_total + f, wmin, wkey);
  } else {
    const size_t cb = (size_t)o0 + (size_t)o1;  // the pair's first column element
    a.v = reinterpret_cast<long long*>(ws + W.v) + cb;
    a.sh = reinterpret_cast<long long*>(ws + W.sh) + cb;
    a.u = reinterpret_cast<long long*>(ws + W.u) + o0;
    a.path = reinterpret_cast<int*>(ws + W.path) + cb;
    a.r4c = reinterpret_cast<int*>(ws + W.r4c) + cb;
    a.c4r = reinterpret_cast<int*>(ws + W.c4r) + o0;
    a.qy = reinterpret_cast<int*>(ws + W.qy) + cb;
    a.qx = reinterpret_cast<int*>(ws + W.qx) + cb;
    a.sc = reinterpret_cast<unsigned char*>(ws + W.sc) + cb;
    link_pair(a, P, C, g2, gd2, rec, o0, o1, prev, dist, mother, pair_total + f, wmin, wkey);
  }
}

size_t lds_bytes(int cap) { return (size_t)kScratch + ((size_t)kPerObject * cap + 15) / 16 * 16; }

// 0 = fine
int link_args(const char* who, int n, long long total, int gate_q, int division_gate_q) {
  if (n < 0 || total < 0 || total > kMaxTotal || gate_q < 1 || gate_q > 65535 || division_gate_q < 0 ||
      division_gate_q > 65535) {
    errf("%s: need n >= 0, 0 <= total < 2^30, 1 <= gate_q <= 65535 and 0 <= division_gate_q <= 65535 "
         "(n %d, total %lld, gate_q %d, division_gate_q %d)", who, n, total, gate_q, division_gate_q);
    return -EINVAL;
  }
  return 0;
}

bool bad_ptr(const void* p, bool needed, unsigned align) {
  return (needed && !p) || (reinterpret_cast<uintptr_t>(p) & (align - 1));
}

// ------------------------------- host twin ------------------------------------
// the explicit P x (C + P) matrix (-1 = absent) of one pair and the algorithm
// of DESIGN.md word for word
struct HostPair {
  std::vector<long long> cost, u, v, sh;
  std::vector<int> path, c4r, r4c;
  std::vector<char> sr, sc;
};

long long solve_pair(HostPair& h, const int* qy, const int* qx, int P, int C, long long g2) {
  const int N = C + P;
  h.cost.assign((size_t)P * N, -1);
  for (int i = 0; i < P; ++i) {
    for (int j = 0; j < C; ++j) {
      const long long d = dist2(qy[i], qx[i], qy[P + j], qx[P + j]);
      if (d <= g2) h.cost[(size_t)i * N + j] = d;
    }
    h.cost[(size_t)i * N + C + i] = g2;
  }
  h.u.assign(P, 0);
  h.v.assign(N, 0);
  h.sh.assign(N, kInf);
  h.path.assign(N, -1);
  h.c4r.assign(P, -1);
  h.r4c.assign(N, -1);
  h.sr.assign(P, 0);
  h.sc.assign(N, 0);
  for (int cur = 0; cur < P; ++cur) {
    std::fill(h.sr.begin(), h.sr.end(), 0);
    std::fill(h.sc.begin(), h.sc.end(), 0);
    std::fill(h.sh.begin(), h.sh.end(), kInf);
    long long minval = 0;
    int i = cur, sink = -1;
    while (sink < 0) {
      h.sr[i] = 1;
      int best = -1;
      long long lowest = kInf;
      for (int j = 0; j < N; ++j) {
        if (h.sc[j]) continue;
        const long long c = h.cost[(size_t)i * N + j];
        if (c >= 0) {
          const long long r = minval + c - h.u[i] - h.v[j];
          if (r < h.sh[j]) {
            h.sh[j] = r;
            h.path[j] = i;
          }
        }
        // (a) an unassigned column before an assigned one, (b) the lowest index
        if (h.sh[j] < lowest || (h.sh[j] == lowest && best >= 0 && h.r4c[j] < 0 && h.r4c[best] >= 0)) {
          lowest = h.sh[j];
          best = j;
        }
      }
      if (best < 0) return -1;  // infeasible: cannot happen
      minval = lowest;
      h.sc[best] = 1;
      if (h.r4c[best] < 0)
        sink = best;
      else
        i = h.r4c[best];
    }
    h.u[cur] += minval;
    for (int r = 0; r < P; ++r)
      if (h.sr[r] && r != cur) h.u[r] += minval - h.sh[h.c4r[r]];
    for (int j = 0; j < N; ++j)
      if (h.sc[j]) h.v[j] -= minval - h.sh[j];
    int j = sink;
    while (true) {
      const int r = h.path[j];
      h.r4c[j] = r;
      std::swap(h.c4r[r], j);
      if (r == cur) break;
    }
  }
  long long total = 0;
  for (int i = 0; i < P; ++i) total += h.cost[(size_t)i * N + h.c4r[i]];
  return total;
}

}  // namespace

extern "C" {

size_t unet_link_ws_bytes(int n, long long total) {
  if (n < 2 || total <= 0 || total > kMaxTotal) return 0;
  return link_ws(total).total;
}

int unet_link_frames(const unet_region_record* records, const int32_t* frame_offsets, int n, long long total,
                     int gate_q, int division_gate_q, int32_t* prev, int64_t* dist, int32_t* mother,
                     int64_t* pair_total, void* ws, unet_stream_t stream) {
  if (const int rc = link_args("unet_link_frames", n, total, gate_q, division_gate_q)) return rc;
  const bool any = n > 0 && total > 0;
  if (bad_ptr(frame_offsets, n > 0, 4) || bad_ptr(records, any, 16) || bad_ptr(prev, any, 4) ||
      bad_ptr(dist, any, 8) || bad_ptr(mother, any, 4) || bad_ptr(pair_total, n > 1, 8) ||
      bad_ptr(ws, unet_link_ws_bytes(n, total) > 0, 256)) {
    errf("unet_link_frames: a null or misaligned pointer (frame_offsets, prev, mother 4 bytes, dist, pair_total 8, "
         "records 16, ws 256)");
    return -EINVAL;
  }
  if (n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int cap = (int)std::min<long long>(lds_objects(), total);
  const size_t smem = lds_bytes(cap);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_link), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes(kLdsMaxObjects));
  if (e == hipSuccess) {
    const long long g2 = (long long)gate_q * gate_q, gd2 = (long long)division_gate_q * division_gate_q;
    hipLaunchKernelGGL(k_link, dim3((unsigned)std::max(n - 1, 1)), dim3(kThreads), smem, s, records, frame_offsets, n,
                       (int)total, g2, gd2, cap, prev, dist, mother, pair_total, reinterpret_cast<char*>(ws),
                       link_ws(std::max<long long>(total, 1)));
    g_link_launches.fetch_add(1);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    errf("unet_link_frames: %s", hipGetErrorString(e));
    return -EIO;
  }
  return 0;
}

int unet_link_frames_host(const unet_region_record* records, const int32_t* frame_offsets, int n, long long total,
                          int gate_q, int division_gate_q, int32_t* prev, int64_t* dist, int32_t* mother,
                          int64_t* pair_total) {
  if (const int rc = link_args("unet_link_frames_host", n, total, gate_q, division_gate_q)) return rc;
  const bool any = n > 0 && total > 0;
  if ((n > 0 && !frame_offsets) || (any && (!records || !prev || !dist || !mother)) || (n > 1 && !pair_total)) {
    errf("unet_link_frames_host: a null pointer");
    return -EINVAL;
  }
  if (n == 0) return 0;
  for (int f = 0; f < n; ++f)
    if (frame_offsets[f] < 0 || frame_offsets[f + 1] < frame_offsets[f] || frame_offsets[f + 1] > total) {
      errf("unet_link_frames_host: frame_offsets must ascend inside [0, total]");
      return -EINVAL;
    }
  const long long g2 = (long long)gate_q * gate_q, gd2 = (long long)division_gate_q * division_gate_q;
  for (int k = 0; k < frame_offsets[1]; ++k) {
    prev[k] = -1;
    dist[k] = -1;
    mother[k] = -1;
  }
  HostPair h;
  std::vector<int> qy, qx;
  for (int f = 0; f + 1 < n; ++f) {
    const int o0 = frame_offsets[f], o1 = frame_offsets[f + 1], o2 = frame_offsets[f + 2];
    const int P = o1 - o0, C = o2 - o1;
    qy.resize((size_t)P + C);
    qx.resize((size_t)P + C);
    for (int k = 0; k < P + C; ++k) {
      qy[k] = quant(records[o0 + k].sum_y, records[o0 + k].area);
      qx[k] = quant(records[o0 + k].sum_x, records[o0 + k].area);
    }
    const long long t = solve_pair(h, qy.data(), qx.data(), P, C, g2);
    if (t < 0) {
      errf("unet_link_frames_host: pair %d has no assignment", f);
      return -EINVAL;
    }
    pair_total[f] = t;
    for (int j = 0; j < C; ++j) {
      const int r = h.r4c[j];
      int m = -1;
      if (r < 0 && gd2 > 0) {
        long long best = kInf;
        for (int q = 0; q < P; ++q) {
          if (h.c4r[q] >= C) continue;  // no linked successor
          const long long d = dist2(qy[q], qx[q], qy[P + j], qx[P + j]);
          if (d <= gd2 && d < best) {
            best = d;
            m = q;
          }
        }
      }
      prev[o1 + j] = r >= 0 ? o0 + r : -1;
      dist[o1 + j] = r >= 0 ? dist2(qy[r], qx[r], qy[P + j], qx[P + j]) : -1;
      mother[o1 + j] = m >= 0 ? o0 + m : -1;
    }
  }
  return 0;
}

long long unet_link_launches(int reset) { return reset ? g_link_launches.exchange(0) : g_link_launches.load(); }

int unet_link_assemble(const unet_region_record* records, const int32_t* frame_offsets, int n,
                       const int32_t* frames, const int32_t* prev, const int64_t* dist, const int32_t* mother,
                       double division_min_ratio, int max_children, int32_t* rows, int rows_cap, int32_t* ids) {
  if (n < 0 || rows_cap < 0 || (n > 0 && (!frame_offsets || !frames))) {
    errf("unet_link_assemble: n or rows_cap < 0, or null frame_offsets / frames");
    return -EINVAL;
  }
  if (n == 0) return 0;
  for (int f = 0; f < n; ++f)
    if (frame_offsets[f] < 0 || frame_offsets[f + 1] < frame_offsets[f] || (f > 0 && frames[f] <= frames[f - 1])) {
      errf("unet_link_assemble: frame_offsets must ascend and frame numbers ascend strictly");
      return -EINVAL;
    }
  const int total = frame_offsets[n];
  if (total > 0 && (!records || !prev || !dist || !mother || !ids || (rows_cap > 0 && !rows))) {
    errf("unet_link_assemble: a null pointer");
    return -EINVAL;
  }
  struct Row {
    int start, end, parent;
  };
  std::vector<Row> tr;
  struct Claim {
    long long d;
    int rec;
  };
  std::vector<int> succ;            // per previous object: its linked successor's record, -1 = none
  std::vector<int> parent_of;       // per current object: the dividing predecessor's record, -1 = none
  std::vector<std::vector<Claim>> claims;
  for (int f = 0; f < n; ++f) {
    const int o1 = frame_offsets[f], o2 = frame_offsets[f + 1];
    const int o0 = f > 0 ? frame_offsets[f - 1] : o1;
    const int P = o1 - o0, C = o2 - o1;
    parent_of.assign(C, -1);
    if (f > 0) {
      succ.assign(P, -1);
      claims.assign(P, {});
      for (int j = 0; j < C; ++j) {
        const int p = prev[o1 + j], m = mother[o1 + j];
        if ((p >= 0 && (p < o0 || p >= o1)) || (m >= 0 && (m < o0 || m >= o1 || p >= 0))) {
          errf("unet_link_assemble: record %d names a predecessor or mother outside the frame before it", o1 + j);
          return -EINVAL;
        }
        if (p >= 0) {
          if (succ[p - o0] >= 0) {
            errf("unet_link_assemble: record %d has two successors", p);
            return -EINVAL;
          }
          succ[p - o0] = o1 + j;
        }
      }
      for (int j = 0; j < C; ++j) {
        const int m = mother[o1 + j];
        if (m < 0 || succ[m - o0] < 0) continue;
        const unet_region_record &a = records[m], &b = records[o1 + j];
        claims[m - o0].push_back({dist2(quant(a.sum_y, a.area), quant(a.sum_x, a.area), quant(b.sum_y, b.area),
                                        quant(b.sum_x, b.area)), o1 + j});
      }
      for (int i = 0; i < P && max_children >= 2; ++i) {
        if (claims[i].empty()) continue;
        const int k = succ[i];
        const double ak = (double)records[k].area;
        std::vector<Claim> pass;
        for (const Claim& c : claims[i]) {
          const double aj = (double)records[c.rec].area;
          if (std::min(ak, aj) / std::max(ak, aj) >= division_min_ratio) pass.push_back(c);
        }
        if (pass.empty()) continue;
        // nearest first, ties to the lowest label (= the lowest record)
        std::stable_sort(pass.begin(), pass.end(), [](const Claim& x, const Claim& y) { return x.d < y.d; });
        if ((int)pass.size() > max_children - 1) pass.resize((size_t)max_children - 1);
        parent_of[k - o1] = o0 + i;
        for (const Claim& c : pass) parent_of[c.rec - o1] = o0 + i;
      }
    }
    for (int j = 0; j < C; ++j) {
      const int r = o1 + j;
      const int p = f > 0 ? prev[r] : -1;
      if (parent_of[j] >= 0) {
        tr.push_back({frames[f], frames[f], ids[parent_of[j]]});
        ids[r] = (int)tr.size();
      } else if (p >= 0) {
        ids[r] = ids[p];
        tr[(size_t)ids[r] - 1].end = frames[f];
      } else {
        tr.push_back({frames[f], frames[f], -1});
        ids[r] = (int)tr.size();
      }
    }
  }
  const int k = std::min(rows_cap, (int)tr.size());
  for (int q = 0; q < k; ++q) {
    rows[4 * q + 0] = q + 1;
    rows[4 * q + 1] = tr[q].start;
    rows[4 * q + 2] = tr[q].end;
    rows[4 * q + 3] = tr[q].parent;
  }
  return (int)tr.size();
}

}  // extern "C"
