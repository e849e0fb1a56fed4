// Cell Tracking Challenge measures SEG / DET / TRA (the reference's README
// step 8, EvaluationSoftware/*/{SEG,DET,TRA}Measure; Matula et al., "Cell
// tracking accuracy measurement based on comparison of acyclic oriented
// graphs", PLoS ONE 2015; Ulman et al., Nature Methods 2017).
//
// Like track.hip: the GPU turns label images into overlap tables, plain C++ on
// the host runs the graph logic, and a host-only twin entry point
// (unet_ctc_add_frame_host) feeds the same logic without a device.
//
// Device part: the sparse overlap records of T frame pairs from two (T, h, w)
// uint16 stacks.  Per chunk of at most "ctc_chunk_frames" frames:
//   k_ctc_mark    label presence bitmaps (65536 bits per frame and side), set
//                 in LDS first, one global atomicOr per non-zero word and block
//   k_ctc_rank    popcount prefix of each bitmap: label -> compact index, and
//                 the object count of each frame and side
//                 (k_ctc_mark also counts each frame's runs of equal non-
//                 background keys: no more distinct pairs can exist)
//   (one host synchronisation: the counts and bitmaps; the host derives the
//    ascending label lists from the bitmaps and lays the tables out, charging
//    a frame min(cells, runs, pixels) records and a table for that many)
// then per round -- one round per chunk while the chunk's tables fit the
// table region and its charges the record buffer, which both grow with the
// chunk; more rounds only where they do not:
//   k_ctc_count   a frame with (n_gt + 1) x (n_res + 1) <= "ctc_dense_cells"
//                 cells counts in a dense LDS table per block, flushed with one
//                 global atomicAdd per non-zero cell and block; a frame with
//                 more cells counts into an open-addressing hash table in
//                 global memory keyed by (gt label, res label), behind a
//                 direct-mapped (key, count) cache in LDS that merges the
//                 block's equal keys first.  Every thread walks 16 consecutive
//                 pixels and merges the run of equal (gt, res) keys in
//                 registers before it touches a counter.
//   k_ctc_compact the non-zero cells / used slots -> (frame, key, count)
//                 records, one global atomic per block for their positions
//   (one host synchronisation: the record count arrives in the same copy as
//    the first 65,536 records; a round with more takes a second copy)
// So a chunk costs 2 + 2 R launches and 1 + R synchronisations for R rounds
// (+1 per round with more than 65,536 records), R = 1 unless the frames'
// charges exceed the regions (see ctc_ws).
// Counts are integers, so the records do not depend on the order of the
// atomics.  Areas are the row / column sums of a frame's records, background
// pairs included; the (background, background) cell is never read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/unet_hip.h"
#include "unet_internal.h"

namespace unet {
// unet_set_tuning("ctc_chunk_frames", n): frames per chunk (1..1024; -1 = the
// default, kDefaultChunk)
int g_ctc_chunk_frames = -1;
// unet_set_tuning("ctc_dense_cells", n): largest dense LDS table in cells
// (0 = every frame takes the hash fallback; at most kDenseMax; -1 = the
// default, kDefaultDense)
int g_ctc_dense_cells = -1;
}  // namespace unet

namespace {

constexpr int kWords = 2048;      // 65536 label bits
constexpr int kThreads = 256;
constexpr int kPix = 16;          // consecutive pixels per thread
constexpr int kPiece = kThreads * kPix;
constexpr int kDenseMax = 8192;   // cells of the LDS table (32 KB)
constexpr int kCacheBits = 11;    // hashed frames: entries of a block's LDS merge cache
constexpr int kCache = 1 << kCacheBits;
constexpr int kMaxChunk = 1024;
constexpr int kDefaultChunk = 32;
constexpr int kDefaultDense = 4096;
constexpr size_t kFirstCopy = 65536;        // records read back with the record count
constexpr size_t kFrameTable = 256 << 10;   // table bytes and records the regions hold per chunk frame
constexpr size_t kFrameRecords = 16384;

int chunk_frames() {
  return unet::g_ctc_chunk_frames < 1 ? kDefaultChunk : std::min(unet::g_ctc_chunk_frames, kMaxChunk);
}
size_t dense_cells() {
  return (size_t)(unet::g_ctc_dense_cells < 0 ? kDefaultDense : std::min(unet::g_ctc_dense_cells, kDenseMax));
}

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
// offset of the next part of a workspace laid out from `at`
size_t carve(size_t& at, size_t bytes) {
  const size_t r = at;
  at += al256(bytes);
  return r;
}

struct FrameDesc {
  int f;                        // frame within the chunk
  int dense;                    // 1 = dense table of ncells uint32, 0 = hash of mask + 1 uint64 slots
  unsigned ncol;                // dense: n_res + 1
  unsigned ncells;              // dense: (n_gt + 1) * (n_res + 1)
  unsigned mask;                // hash: slots - 1 (slots a power of two)
  unsigned pad;
  unsigned long long off;       // byte offset of the table in the table region
};

// ------------------------------- GPU part ------------------------------------
// a thread's kPix consecutive pixels from p0 on: two 16-byte loads where the
// address allows (a frame of odd size starts 2-byte aligned), else pixel by
// pixel up to the frame's end; returns how many there are
__device__ __forceinline__ int ctc_load(const uint16_t* __restrict__ img, size_t p0, size_t hw,
                                        unsigned (&v)[kPix]) {
  if (p0 >= hw) return 0;
  const int n = hw - p0 < (size_t)kPix ? (int)(hw - p0) : kPix;
  const uint16_t* p = img + p0;
  if (n == kPix && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[2 * k] = w[k] & 0xffffu;
      v[2 * k + 1] = w[k] >> 16;
    }
  } else {
    for (int k = 0; k < n; ++k) v[k] = p[k];
  }
  return n;
}

__global__ __launch_bounds__(kThreads) void k_ctc_mark(const uint16_t* __restrict__ gt,
                                                        const uint16_t* __restrict__ res, size_t hw,
                                                        unsigned* __restrict__ bits,
                                                        unsigned* __restrict__ runs) {
  __shared__ unsigned sb[2 * kWords];
  __shared__ unsigned s_runs;
  for (int i = threadIdx.x; i < 2 * kWords; i += kThreads) sb[i] = 0;
  if (threadIdx.x == 0) s_runs = 0;
  __syncthreads();
  unsigned mine = 0;  // runs of equal non-background keys, cut as k_ctc_count cuts them
  const size_t f = blockIdx.y;
  const uint16_t* g = gt + f * hw;
  const uint16_t* r = res + f * hw;
  for (size_t base = blockIdx.x * (size_t)kPiece; base < hw; base += gridDim.x * (size_t)kPiece) {
    const size_t p0 = base + threadIdx.x * (size_t)kPix;
    unsigned a[kPix], b[kPix];
    const int n = ctc_load(g, p0, hw, a);
    ctc_load(r, p0, hw, b);
#pragma unroll
    for (int k = 0; k < kPix; ++k) {  // one LDS atomic per run of equal labels
      if (k >= n) break;
      if (k == 0 || a[k] != a[k - 1]) atomicOr(&sb[a[k] >> 5], 1u << (a[k] & 31));
      if (k == 0 || b[k] != b[k - 1]) atomicOr(&sb[kWords + (b[k] >> 5)], 1u << (b[k] & 31));
      mine += (a[k] | b[k]) != 0 && (k == 0 || a[k] != a[k - 1] || b[k] != b[k - 1]);
    }
  }
  if (mine) atomicAdd(&s_runs, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_runs) atomicAdd(runs + f, s_runs);
  unsigned* out = bits + f * 2 * kWords;
  for (int i = threadIdx.x; i < 2 * kWords; i += kThreads) {
    const unsigned v = sb[i];
    if (v) atomicOr(out + i, v);
  }
}

// one block per (frame, side): clears the background bit, writes the number of
// set bits before each word and the total
__global__ __launch_bounds__(kThreads) void k_ctc_rank(unsigned* __restrict__ bits, int* __restrict__ prefix,
                                                        int* __restrict__ counts) {
  __shared__ int sh[kThreads];
  constexpr int per = kWords / kThreads;
  unsigned* b = bits + (size_t)blockIdx.x * kWords;
  int* pre = prefix + (size_t)blockIdx.x * kWords;
  unsigned w[per];
  int sum = 0;
  for (int k = 0; k < per; ++k) {
    w[k] = b[threadIdx.x * per + k];
    if (threadIdx.x == 0 && k == 0) {
      w[0] &= ~1u;
      b[0] = w[0];
    }
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

// compact index of a label: 0 = background, 1.. in ascending label order
__device__ __forceinline__ unsigned ctc_rank(const unsigned* __restrict__ bits, const int* __restrict__ pre,
                                             unsigned l) {
  if (l == 0) return 0;
  return (unsigned)pre[l >> 5] + __popc(bits[l >> 5] & ((1u << (l & 31)) - 1u)) + 1u;
}

// slot = key << 32 | count; key 0 (background, background) is never added, so
// an empty slot is 0.  count <= h w < 2^31 cannot carry into the key.
__device__ __forceinline__ void ctc_hash_add(unsigned long long* __restrict__ slots, unsigned mask, unsigned key,
                                             unsigned cnt) {
  unsigned h = key * 2654435761u;
  h ^= h >> 15;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    unsigned long long* s = slots + ((h + probe) & mask);
    unsigned long long cur = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      cur = atomicCAS(s, 0ull, (unsigned long long)key << 32);
      if (cur == 0) cur = (unsigned long long)key << 32;
    }
    if ((unsigned)(cur >> 32) == key) {
      atomicAdd(s, (unsigned long long)cnt);
      return;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ctc_count(const uint16_t* __restrict__ gt,
                                                         const uint16_t* __restrict__ res, size_t hw,
                                                         const FrameDesc* __restrict__ desc,
                                                         const unsigned* __restrict__ bits,
                                                         const int* __restrict__ prefix, char* __restrict__ tables) {
  // dense frame: the table; hashed frame: a direct-mapped cache of kCache
  // (key, count) entries that merges the block's equal keys before they reach
  // the global table (keys in tab[0, kCache), counts behind them)
  __shared__ unsigned tab[kDenseMax];
  const FrameDesc d = desc[blockIdx.y];
  const unsigned ncells = d.ncells < (unsigned)kDenseMax ? d.ncells : (unsigned)kDenseMax;
  const unsigned nlds = d.dense ? ncells : 2u * kCache;
  for (unsigned i = threadIdx.x; i < nlds; i += kThreads) tab[i] = 0;
  __syncthreads();
  const uint16_t* g = gt + (size_t)d.f * hw;
  const uint16_t* r = res + (size_t)d.f * hw;
  const unsigned* bg = bits + (size_t)d.f * 2 * kWords;
  const unsigned* br = bg + kWords;
  const int* pg = prefix + (size_t)d.f * 2 * kWords;
  const int* pr = pg + kWords;
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(tables + d.off);
  auto flush = [&](unsigned key, unsigned cnt) {
    if (d.dense) {
      const unsigned cell = ctc_rank(bg, pg, key >> 16) * d.ncol + ctc_rank(br, pr, key & 0xffffu);
      if (cell < ncells) atomicAdd(&tab[cell], cnt);
    } else if (key) {
      const unsigned c = (key * 2654435761u) >> (32 - kCacheBits);
      const unsigned old = atomicCAS(&tab[c], 0u, key);
      if (old == 0 || old == key)
        atomicAdd(&tab[kCache + c], cnt);
      else  // the entry belongs to another key
        ctc_hash_add(slots, d.mask, key, cnt);
    }
  };
  for (size_t base = blockIdx.x * (size_t)kPiece; base < hw; base += gridDim.x * (size_t)kPiece) {
    const size_t p0 = base + threadIdx.x * (size_t)kPix;
    unsigned a[kPix], b[kPix];
    const int n = ctc_load(g, p0, hw, a);
    ctc_load(r, p0, hw, b);
    unsigned key = 0, cnt = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {  // runs of equal keys merge in registers
      const unsigned q = k < n ? a[k] << 16 | b[k] : key;  // past the frame's end: the run goes on, uncounted
      if (q != key && cnt) {
        flush(key, cnt);
        cnt = 0;
      }
      key = q;
      cnt += k < n;
    }
    if (cnt) flush(key, cnt);
  }
  __syncthreads();
  if (d.dense) {
    unsigned* out = reinterpret_cast<unsigned*>(tables + d.off);
    for (unsigned i = threadIdx.x; i < ncells; i += kThreads) {
      const unsigned v = tab[i];
      if (v) atomicAdd(out + i, v);
    }
  } else {
    for (unsigned i = threadIdx.x; i < (unsigned)kCache; i += kThreads)
      if (tab[i]) ctc_hash_add(slots, d.mask, tab[i], tab[kCache + i]);
  }
}

// records: (frame within the chunk, key, count, 0); key = gt << 16 | res, in
// compact indices for a dense frame and in labels for a hashed one
__global__ __launch_bounds__(kThreads) void k_ctc_compact(const FrameDesc* __restrict__ desc,
                                                           const char* __restrict__ tables, uint4* __restrict__ rec,
                                                           unsigned cap) {
  unsigned* nrec = &rec[0].x;  // rec[0] is the header: the record count; records follow
  __shared__ unsigned s_cnt, s_base;
  const FrameDesc d = desc[blockIdx.y];
  const unsigned n = d.dense ? d.ncells : d.mask + 1u;
  const unsigned* cells = reinterpret_cast<const unsigned*>(tables + d.off);
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(tables + d.off);
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  unsigned mine = 0;
  // cell 0 of a dense table is (background, background)
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads)
    mine += d.dense ? (i != 0 && cells[i] != 0) : (slots[i] != 0);
  unsigned at = mine ? atomicAdd(&s_cnt, mine) : 0;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(nrec, s_cnt) : 0;
  __syncthreads();
  at += s_base;
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n && mine; i += gridDim.x * kThreads) {
    unsigned key, cnt;
    if (d.dense) {
      cnt = i ? cells[i] : 0;
      key = (i / d.ncol) << 16 | (i % d.ncol);
    } else {
      const unsigned long long v = slots[i];
      cnt = (unsigned)v;
      key = (unsigned)(v >> 32);
      if (v == 0) cnt = 0;
    }
    if (cnt) {
      if (at < cap) rec[1 + at] = make_uint4((unsigned)d.f, key, cnt, 0u);
      ++at;
      --mine;
    }
  }
}

size_t pow2ceil(size_t v) {
  size_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// workspace layout (unet_ctc_ws_bytes): with c = min(t, kMaxChunk) frames, k =
// min(t, "ctc_chunk_frames") frames per chunk and P = h w pixels per frame
//   runs      c x 4 B           bitmaps c x 2 x 8 KB     prefix  c x 2 x 8 KB
//   counts    c x 2 x 4 B       descs   c x 32 B
//   tables    max(8 B x pow2ceil(2 P), k x 256 KB)
//   records   16 B x (1 + max(P, 4096, k x 16384))
// The first terms of the last two are one frame's worst case (P distinct pairs
// in a hash at load <= 1/2), so any frame fits alone; the second let a chunk
// of frames with up to 16,384 key runs each pass in one round.
struct CtcWs {
  unsigned* runs;
  unsigned* bits;
  int* prefix;
  int* counts;
  FrameDesc* desc;
  char* tables;
  uint4* rec;
  size_t table_bytes, rec_cap, total;
};

CtcWs ctc_ws(void* ws, int t, int h, int w) {
  const size_t c = (size_t)std::min(std::max(t, 1), kMaxChunk), hw = (size_t)h * w;
  const size_t k = std::min(c, (size_t)chunk_frames());
  CtcWs o{};
  size_t at = 0;
  const size_t runs = carve(at, c * 4);  // directly before the bitmaps: one memset clears both
  const size_t bits = carve(at, c * 2 * kWords * 4), prefix = carve(at, c * 2 * kWords * 4);
  const size_t counts = carve(at, c * 2 * 4), desc = carve(at, c * sizeof(FrameDesc));
  o.table_bytes = std::max(std::max<size_t>(8 * pow2ceil(2 * hw), (size_t)kDenseMax * 4), k * kFrameTable);
  const size_t tables = carve(at, o.table_bytes);
  o.rec_cap = std::max(std::max<size_t>(hw, 4096), k * kFrameRecords);
  const size_t rec = carve(at, (o.rec_cap + 1) * 16);
  o.total = at;
  if (char* p = reinterpret_cast<char*>(ws)) {  // null: the sizes only (unet_ctc_ws_bytes)
    o.runs = reinterpret_cast<unsigned*>(p + runs);
    o.bits = reinterpret_cast<unsigned*>(p + bits);
    o.prefix = reinterpret_cast<int*>(p + prefix);
    o.counts = reinterpret_cast<int*>(p + counts);
    o.desc = reinterpret_cast<FrameDesc*>(p + desc);
    o.tables = p + tables;
    o.rec = reinterpret_cast<uint4*>(p + rec);
  }
  return o;
}

struct Pair {
  int g, r;
  long long n;
};

struct Frame {
  int frame = 0;
  std::vector<int> gl, rl;          // ascending labels, no background
  std::vector<long long> ga, ra;    // their areas
  std::vector<Pair> pairs;          // overlapping (gt label, res label) pairs, sorted
};

void errf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  unet::set_last_error(buf);
}

void appendf(std::string& o, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  o += buf;
}

struct Edge {
  int u, v, kind;  // vertex indices; kind 0 = track link, 1 = parent link
};

struct Row {
  int l, b, e, p;
};

// the acyclic oriented graph of one side
struct Graph {
  std::vector<int> vframe, vlabel;                 // per vertex, ordered by frame, then label
  std::vector<size_t> first;                       // per TRA frame: its first vertex
  std::vector<Edge> edges;                         // construction order
  std::unordered_map<unsigned long long, int> ek;  // (u, v) -> kind
  int find(int u, int v) const {
    auto it = ek.find((unsigned long long)(unsigned)u << 32 | (unsigned)v);
    return it == ek.end() ? -1 : it->second;
  }
};

}  // namespace

struct unet_ctc {
  std::vector<Frame> frames[2];  // by kind
  std::vector<Row> tracks[2];    // by side
  bool has_tracks[2] = {false, false};
  int h = 0, w = 0;
  long long stats[6] = {0, 0, 0, 0, 0, 0};  // chunks, launches, host syncs, dense frames, hashed frames, records
  // results (valid while !dirty)
  bool dirty = true;
  int rc = 0;
  std::string err, log;
  double out[3] = {0, 0, 0};
  long long counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  int add(int kind, Frame&& f) {
    for (const Frame& o : frames[kind])
      if (o.frame == f.frame) {
        errf("unet_ctc: %s frame %d was added twice", kind == UNET_CTC_SEG ? "SEG" : "TRA", f.frame);
        return -EEXIST;
      }
    frames[kind].push_back(std::move(f));
    dirty = true;
    return 0;
  }

  int build_graph(int side, const std::vector<Frame>& fr, Graph& g) {
    const char* sn = side == UNET_CTC_GT ? "GT" : "RES";
    g.first.assign(fr.size() + 1, 0);
    for (size_t i = 0; i < fr.size(); ++i) {
      const std::vector<int>& ls = side == UNET_CTC_GT ? fr[i].gl : fr[i].rl;
      g.first[i] = g.vframe.size();
      for (int l : ls) {
        g.vframe.push_back(fr[i].frame);
        g.vlabel.push_back(l);
      }
    }
    g.first[fr.size()] = g.vframe.size();
    if (!has_tracks[side]) return 0;
    std::vector<int> row_of(65536, -1);
    const std::vector<Row>& rows = tracks[side];
    for (size_t k = 0; k < rows.size(); ++k) row_of[rows[k].l] = (int)k;
    // the present vertices of each row, inside [B, E], ascending
    std::vector<std::vector<int>> present(rows.size());
    for (size_t v = 0; v < g.vframe.size(); ++v) {
      const int k = row_of[g.vlabel[v]];
      if (k < 0) {
        errf("unet_ctc: %s label %d occurs in frame %d but has no track row", sn, g.vlabel[v], g.vframe[v]);
        return -ENOENT;
      }
      if (g.vframe[v] >= rows[k].b && g.vframe[v] <= rows[k].e) present[k].push_back((int)v);
    }
    auto add_edge = [&](int u, int v, int kind) {
      if (g.ek.emplace((unsigned long long)(unsigned)u << 32 | (unsigned)v, kind).second) g.edges.push_back({u, v, kind});
    };
    for (size_t k = 0; k < rows.size(); ++k) {
      if (rows[k].p != 0) {
        const int pk = rows[k].p > 0 && rows[k].p < 65536 ? row_of[rows[k].p] : -1;
        if (pk < 0) {
          errf("unet_ctc: %s label %d (frame %d) names parent %d, which has no track row", sn, rows[k].l, rows[k].b,
               rows[k].p);
          return -ESRCH;
        }
        if (!present[pk].empty() && !present[k].empty()) add_edge(present[pk].back(), present[k].front(), 1);
      }
      for (size_t q = 1; q < present[k].size(); ++q) add_edge(present[k][q - 1], present[k][q], 0);
    }
    return 0;
  }

  // the S with 2 |R and S| > |R| for every R of a frame (-1 = none): index into f.rl
  static void match(const Frame& f, std::vector<int>& m, std::vector<long long>& inter) {
    m.assign(f.gl.size(), -1);
    inter.assign(f.gl.size(), 0);
    for (const Pair& p : f.pairs) {
      const size_t gi = std::lower_bound(f.gl.begin(), f.gl.end(), p.g) - f.gl.begin();
      if (2 * p.n > f.ga[gi]) {
        m[gi] = (int)(std::lower_bound(f.rl.begin(), f.rl.end(), p.r) - f.rl.begin());
        inter[gi] = p.n;
      }
    }
  }

  int evaluate() {
    if (!dirty) {
      if (rc) unet::set_last_error(err);
      return rc;
    }
    rc = compute();
    if (rc) err = unet_last_error();
    dirty = false;
    return rc;
  }

  int compute() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out[0] = out[1] = out[2] = nan;
    std::fill(counts, counts + 8, 0);
    log.clear();
    for (int k = 0; k < 2; ++k)
      std::sort(frames[k].begin(), frames[k].end(), [](const Frame& a, const Frame& b) { return a.frame < b.frame; });
    std::vector<int> m;
    std::vector<long long> inter;
    // SEG: mean Jaccard index of the reference objects with their matches
    {
      double sum = 0;
      long long n = 0;
      for (const Frame& f : frames[UNET_CTC_SEG]) {
        match(f, m, inter);
        for (size_t i = 0; i < f.gl.size(); ++i, ++n)
          if (m[i] >= 0) sum += (double)inter[i] / (double)(f.ga[i] + f.ra[m[i]] - inter[i]);
      }
      if (n) out[0] = sum / (double)n;
    }
    const std::vector<Frame>& fr = frames[UNET_CTC_TRA];
    if (fr.empty()) return 0;
    Graph G, R;
    int e = build_graph(UNET_CTC_GT, fr, G);
    if (e) return e;
    if ((e = build_graph(UNET_CTC_RES, fr, R))) return e;
    // vertex matching
    std::vector<int> g2r(G.vframe.size(), -1), nmatch(R.vframe.size(), 0), r2g(R.vframe.size(), -1);
    for (size_t i = 0; i < fr.size(); ++i) {
      match(fr[i], m, inter);
      for (size_t k = 0; k < m.size(); ++k)
        if (m[k] >= 0) {
          const size_t gv = G.first[i] + k, rv = R.first[i] + (size_t)m[k];
          g2r[gv] = (int)rv;
          ++nmatch[rv];
          r2g[rv] = (int)gv;
        }
    }
    long long ns = 0, fn = 0, fp = 0, ed = 0, ea = 0, ec = 0;
    log += "----------Splitting Operations (Penalty=5)----------\n";
    for (size_t v = 0; v < R.vframe.size(); ++v)
      for (int k = 1; k < nmatch[v]; ++k, ++ns) appendf(log, "T=%d Label=%d\n", R.vframe[v], R.vlabel[v]);
    log += "----------False Negative Vertices (Penalty=10)----------\n";
    for (size_t v = 0; v < G.vframe.size(); ++v)
      if (g2r[v] < 0) {
        ++fn;
        appendf(log, "T=%d GT_label=%d\n", G.vframe[v], G.vlabel[v]);
      }
    log += "----------False Positive Vertices (Penalty=1)----------\n";
    for (size_t v = 0; v < R.vframe.size(); ++v)
      if (nmatch[v] == 0) {
        ++fp;
        appendf(log, "T=%d Label=%d\n", R.vframe[v], R.vlabel[v]);
      }
    const bool graphs = has_tracks[0] && has_tracks[1];
    std::string wrong;
    log += "----------Redundant Edges To Be Deleted (Penalty=1)----------\n";
    for (const Edge& x : R.edges) {
      if (nmatch[x.u] != 1 || nmatch[x.v] != 1) continue;
      const int k = G.find(r2g[x.u], r2g[x.v]);
      if (k < 0) {
        ++ed;
        appendf(log, "[T=%d Label=%d] -> [T=%d Label=%d]\n", R.vframe[x.u], R.vlabel[x.u], R.vframe[x.v],
                R.vlabel[x.v]);
      } else if (k != x.kind) {
        ++ec;
        appendf(wrong, "[T=%d Label=%d] -> [T=%d Label=%d]\n", R.vframe[x.u], R.vlabel[x.u], R.vframe[x.v],
                R.vlabel[x.v]);
      }
    }
    log += "----------Edges To Be Added (Penalty=1.5)----------\n";
    for (const Edge& x : G.edges) {
      const int a = g2r[x.u], b = g2r[x.v];
      if (a >= 0 && b >= 0 && nmatch[a] == 1 && nmatch[b] == 1 && R.find(a, b) >= 0) continue;
      ++ea;
      appendf(log, "[T=%d GT_label=%d] -> [T=%d GT_label=%d]\n", G.vframe[x.u], G.vlabel[x.u], G.vframe[x.v],
              G.vlabel[x.v]);
    }
    log += "----------Edges with Wrong Semantics (Penalty=1)----------\n";
    log += wrong;
    const long long vg = (long long)G.vframe.size(), eg = (long long)G.edges.size();
    const long long c[8] = {ns, fn, fp, ed, ea, ec, vg, eg};
    std::copy(c, c + 8, counts);
    if (vg > 0) {
      const double d0 = 10.0 * (double)vg, d = 5.0 * (double)ns + 10.0 * (double)fn + (double)fp;
      out[1] = 1.0 - std::min(d, d0) / d0;
      if (graphs) {
        const double a0 = d0 + 1.5 * (double)eg, a = d + (double)ed + 1.5 * (double)ea + (double)ec;
        out[2] = 1.0 - std::min(a, a0) / a0;
      }
    }
    log += std::string(81, '=') + "\n";
    appendf(log, "TRA measure: %.6f\n", out[2]);
    return 0;
  }
};

namespace {

bool ascending_labels(const int32_t* l, int n) {
  for (int k = 0; k < n; ++k)
    if (l[k] <= 0 || l[k] >= 65536 || (k > 0 && l[k] <= l[k - 1])) return false;
  return true;
}

// one chunk of frames [f0, f0 + tc) of the stacks
int ctc_chunk(unet_ctc* c, int kind, const uint16_t* gt, const uint16_t* res, const int32_t* frames, int f0, int tc,
              int h, int w, const CtcWs& W, hipStream_t s, std::vector<Frame>& done) {
  const size_t hw = (size_t)h * w;
  const uint16_t* g = gt + (size_t)f0 * hw;
  const uint16_t* r = res + (size_t)f0 * hw;
  hipError_t e;
#define CTC_HIP(x)                                                          \
  if ((e = (x)) != hipSuccess) {                                            \
    errf("unet_ctc_add_frames: %s (%s)", hipGetErrorString(e), #x);         \
    return -EIO;                                                            \
  }
  const unsigned bx = (unsigned)std::min<size_t>((hw + kPiece - 1) / kPiece, 64);
  CTC_HIP(hipMemsetAsync(W.runs, 0, (size_t)((char*)W.bits - (char*)W.runs) + (size_t)tc * 2 * kWords * 4, s));
  hipLaunchKernelGGL(k_ctc_mark, dim3(bx, tc), dim3(kThreads), 0, s, g, r, hw, W.bits, W.runs);
  hipLaunchKernelGGL(k_ctc_rank, dim3(2 * tc), dim3(kThreads), 0, s, W.bits, W.prefix, W.counts);
  CTC_HIP(hipGetLastError());
  std::vector<int> cnt((size_t)tc * 2);
  std::vector<unsigned> bits((size_t)tc * 2 * kWords), runs(tc);
  CTC_HIP(hipMemcpyAsync(runs.data(), W.runs, runs.size() * 4, hipMemcpyDeviceToHost, s));
  CTC_HIP(hipMemcpyAsync(cnt.data(), W.counts, cnt.size() * 4, hipMemcpyDeviceToHost, s));
  CTC_HIP(hipMemcpyAsync(bits.data(), W.bits, bits.size() * 4, hipMemcpyDeviceToHost, s));
  CTC_HIP(hipStreamSynchronize(s));
  c->stats[0] += 1;
  c->stats[1] += 2;
  c->stats[2] += 1;
  std::vector<Frame> out(tc);
  for (int f = 0; f < tc; ++f) {
    out[f].frame = frames[f0 + f];
    for (int side = 0; side < 2; ++side) {
      std::vector<int>& l = side ? out[f].rl : out[f].gl;
      const unsigned* b = bits.data() + ((size_t)f * 2 + side) * kWords;
      for (int wd = 0; wd < kWords; ++wd)
        for (unsigned v = b[wd]; v; v &= v - 1) l.push_back(wd * 32 + __builtin_ctz(v));
      if ((int)l.size() != cnt[(size_t)f * 2 + side]) {
        errf("unet_ctc_add_frames: frame %d: label count %d differs from the bitmap's %zu", out[f].frame,
             cnt[(size_t)f * 2 + side], l.size());
        return -EIO;
      }
    }
    out[f].ga.assign(out[f].gl.size(), 0);
    out[f].ra.assign(out[f].rl.size(), 0);
  }
  const size_t dense_max = dense_cells();
  std::vector<FrameDesc> desc;
  std::vector<uint4> rec;
  for (int f = 0; f < tc;) {
    // a round: as many frames as fit the table region and the record buffer
    // (all of the chunk's, unless their charges exceed what ctc_ws provides)
    desc.clear();
    size_t off = 0, recs = 0;
    for (; f < tc; ++f) {
      const size_t ng = out[f].gl.size(), nr = out[f].rl.size(), cells = (ng + 1) * (nr + 1);
      // no more records than cells, than runs of equal keys, than pixels
      const size_t worst = std::max<size_t>(std::min(std::min(cells, (size_t)runs[f]), hw), 1);
      FrameDesc d{};
      d.f = f;
      d.off = off;
      size_t bytes;
      if (cells <= dense_max) {
        d.dense = 1;
        d.ncol = (unsigned)(nr + 1);
        d.ncells = (unsigned)cells;
        bytes = cells * 4;
      } else {
        const size_t slots = pow2ceil(2 * worst);
        d.mask = (unsigned)(slots - 1);
        bytes = slots * 8;
      }
      if (!desc.empty() && (off + al256(bytes) > W.table_bytes || recs + worst > W.rec_cap)) break;
      if (off + bytes > W.table_bytes || recs + worst > W.rec_cap) {
        errf("unet_ctc_add_frames: frame %d does not fit the workspace", out[f].frame);
        return -ENOMEM;
      }
      off += al256(bytes);
      recs += worst;
      desc.push_back(d);
      c->stats[d.dense ? 3 : 4] += 1;
    }
    const unsigned nf = (unsigned)desc.size();
    CTC_HIP(hipMemsetAsync(W.tables, 0, off, s));
    CTC_HIP(hipMemsetAsync(W.rec, 0, 16, s));
    CTC_HIP(hipMemcpyAsync(W.desc, desc.data(), nf * sizeof(FrameDesc), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ctc_count, dim3(bx, nf), dim3(kThreads), 0, s, g, r, hw, W.desc, W.bits, W.prefix, W.tables);
    hipLaunchKernelGGL(k_ctc_compact, dim3(32, nf), dim3(kThreads), 0, s, W.desc, W.tables, W.rec,
                       (unsigned)W.rec_cap);
    CTC_HIP(hipGetLastError());
    // the header (record count) and the first records in one copy
    const size_t first = std::min(recs, kFirstCopy);
    rec.resize(1 + first);
    CTC_HIP(hipMemcpyAsync(rec.data(), W.rec, (1 + first) * 16, hipMemcpyDeviceToHost, s));
    CTC_HIP(hipStreamSynchronize(s));
    const size_t nrec = rec[0].x;
    if (nrec > recs) {
      errf("unet_ctc_add_frames: %zu overlap records where at most %zu can exist", nrec, recs);
      return -EIO;
    }
    rec.resize(1 + nrec);
    c->stats[1] += 2;
    c->stats[2] += 1;
    if (nrec > first) {
      CTC_HIP(hipMemcpyAsync(rec.data() + 1 + first, W.rec + 1 + first, (nrec - first) * 16, hipMemcpyDeviceToHost, s));
      CTC_HIP(hipStreamSynchronize(s));
      c->stats[2] += 1;
    }
    c->stats[5] += (long long)nrec;
    std::vector<char> is_dense(tc, 0);
    for (const FrameDesc& d : desc) is_dense[d.f] = (char)d.dense;
    auto bad = [&](const uint4& q) {
      errf("unet_ctc_add_frames: overlap record (frame %u of the chunk, key 0x%08x, %u pixels) names no object of "
           "its frame", q.x, q.y, q.z);
      return -EIO;
    };
    for (size_t k = 1; k < rec.size(); ++k) {
      const uint4& q = rec[k];
      if ((int)q.x >= tc) return bad(q);
      Frame& F = out[q.x];
      unsigned a = q.y >> 16, b = q.y & 0xffffu;
      if (is_dense[q.x]) {  // compact indices -> labels
        if (a > F.gl.size() || b > F.rl.size()) return bad(q);
        a = a ? (unsigned)F.gl[a - 1] : 0;
        b = b ? (unsigned)F.rl[b - 1] : 0;
      }
      if (a) {
        const size_t i = std::lower_bound(F.gl.begin(), F.gl.end(), (int)a) - F.gl.begin();
        if (i == F.gl.size() || F.gl[i] != (int)a) return bad(q);
        F.ga[i] += q.z;
      }
      if (b) {
        const size_t i = std::lower_bound(F.rl.begin(), F.rl.end(), (int)b) - F.rl.begin();
        if (i == F.rl.size() || F.rl[i] != (int)b) return bad(q);
        F.ra[i] += q.z;
      }
      if (a && b) F.pairs.push_back({(int)a, (int)b, (long long)q.z});
    }
  }
#undef CTC_HIP
  for (Frame& F : out) {
    std::sort(F.pairs.begin(), F.pairs.end(), [](const Pair& x, const Pair& y) { return x.g != y.g ? x.g < y.g : x.r < y.r; });
    done.push_back(std::move(F));
  }
  return 0;
}

}  // namespace

extern "C" {

unet_ctc* unet_ctc_create(void) { return new unet_ctc(); }

void unet_ctc_destroy(unet_ctc* c) { delete c; }

size_t unet_ctc_ws_bytes(int t, int h, int w) {
  if (t < 1 || h < 1 || w < 1 || (long long)h * w >= (1ll << 31)) return 0;
  return ctc_ws(nullptr, t, h, w).total;
}

int unet_ctc_add_frames(unet_ctc* c, int kind, const uint16_t* gt, const uint16_t* res, const int32_t* host_frames,
                        int t, int h, int w, void* ws, unet_stream_t stream) {
  if (!c || (kind != UNET_CTC_SEG && kind != UNET_CTC_TRA) || t < 0 || h < 1 || w < 1 ||
      (long long)h * w >= (1ll << 31)) {
    errf("unet_ctc_add_frames: bad arguments (kind %d, t %d, h %d, w %d)", kind, t, h, w);
    return -EINVAL;
  }
  if (c->h && (c->h != h || c->w != w)) {
    errf("unet_ctc_add_frames: frame %d: the stacks' sizes differ, %d x %d after %d x %d",
         t > 0 && host_frames ? host_frames[0] : -1, h, w, c->h, c->w);
    return -EINVAL;
  }
  c->h = h;
  c->w = w;
  if (t == 0) return 0;
  if (!gt || !res || !host_frames || !ws || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    errf("unet_ctc_add_frames: null stack, frame numbers or workspace, or a workspace not 256-byte aligned");
    return -EINVAL;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const CtcWs W = ctc_ws(ws, t, h, w);
  const int chunk = std::min(chunk_frames(), t);
  // the evaluator takes the frames once every chunk has succeeded: all or none
  std::vector<Frame> done;
  for (int f0 = 0; f0 < t; f0 += chunk) {
    const int rc = ctc_chunk(c, kind, gt, res, host_frames, f0, std::min(chunk, t - f0), h, w, W, s, done);
    if (rc) return rc;
  }
  std::vector<int> nums;
  for (const Frame& f : c->frames[kind]) nums.push_back(f.frame);
  for (const Frame& f : done) nums.push_back(f.frame);
  std::sort(nums.begin(), nums.end());
  const auto dup = std::adjacent_find(nums.begin(), nums.end());
  if (dup != nums.end()) {
    errf("unet_ctc: %s frame %d was added twice", kind == UNET_CTC_SEG ? "SEG" : "TRA", *dup);
    return -EEXIST;
  }
  for (Frame& f : done) c->add(kind, std::move(f));
  return 0;
}

int unet_ctc_add_frame_host(unet_ctc* c, int kind, int frame, int n_gt, const int32_t* gt_labels,
                            const int64_t* gt_areas, int n_res, const int32_t* res_labels, const int64_t* res_areas,
                            int n_pairs, const int64_t* pairs) {
  if (!c || (kind != UNET_CTC_SEG && kind != UNET_CTC_TRA) || n_gt < 0 || n_pairs < 0 ||
      (n_gt > 0 && (!gt_labels || !gt_areas)) || (n_res > 0 && (!res_labels || !res_areas)) ||
      (n_pairs > 0 && !pairs)) {
    errf("unet_ctc_add_frame_host: frame %d: bad arguments", frame);
    return -EINVAL;
  }
  if (n_res < 0) {
    errf("unet_ctc: GT %s frame %d has no RES frame", kind == UNET_CTC_SEG ? "SEG" : "TRA", frame);
    return -ENODATA;
  }
  if (!ascending_labels(gt_labels, n_gt) || !ascending_labels(res_labels, n_res)) {
    errf("unet_ctc_add_frame_host: frame %d: labels must ascend within 1..65535", frame);
    return -EINVAL;
  }
  Frame f;
  f.frame = frame;
  f.gl.assign(gt_labels, gt_labels + n_gt);
  f.rl.assign(res_labels, res_labels + n_res);
  f.ga.assign(gt_areas, gt_areas + n_gt);
  f.ra.assign(res_areas, res_areas + n_res);
  for (int k = 0; k < n_pairs; ++k) {
    const int64_t g = pairs[3 * k], r = pairs[3 * k + 1], n = pairs[3 * k + 2];
    const auto gi = std::lower_bound(f.gl.begin(), f.gl.end(), g), ri = std::lower_bound(f.rl.begin(), f.rl.end(), r);
    if (gi == f.gl.end() || *gi != g || ri == f.rl.end() || *ri != r || n < 1 || n > f.ga[gi - f.gl.begin()] ||
        n > f.ra[ri - f.rl.begin()]) {
      errf("unet_ctc_add_frame_host: frame %d: pair %d (gt %lld, res %lld, %lld pixels) fits no listed object", frame,
           k, (long long)g, (long long)r, (long long)n);
      return -EINVAL;
    }
    f.pairs.push_back({(int)g, (int)r, (long long)n});
  }
  std::sort(f.pairs.begin(), f.pairs.end(), [](const Pair& x, const Pair& y) { return x.g != y.g ? x.g < y.g : x.r < y.r; });
  for (size_t k = 1; k < f.pairs.size(); ++k)
    if (f.pairs[k].g == f.pairs[k - 1].g && f.pairs[k].r == f.pairs[k - 1].r) {
      errf("unet_ctc_add_frame_host: frame %d: pair (gt %d, res %d) listed twice", frame, f.pairs[k].g, f.pairs[k].r);
      return -EINVAL;
    }
  return c->add(kind, std::move(f));
}

int unet_ctc_set_tracks(unet_ctc* c, int side, const int32_t* rows, int n) {
  if (!c || (side != UNET_CTC_GT && side != UNET_CTC_RES) || n < 0 || (n > 0 && !rows)) {
    errf("unet_ctc_set_tracks: bad arguments");
    return -EINVAL;
  }
  std::vector<Row> t;
  std::vector<char> seen(65536, 0);
  for (int k = 0; k < n; ++k) {
    const Row r{rows[4 * k], rows[4 * k + 1], rows[4 * k + 2], rows[4 * k + 3]};
    if (r.l <= 0 || r.l >= 65536 || r.e < r.b || r.p < 0 || seen[r.l]) {
      errf("unet_ctc_set_tracks: row %d (%d %d %d %d): label outside 1..65535, listed twice, end before begin or "
           "negative parent", k, r.l, r.b, r.e, r.p);
      return -EINVAL;
    }
    seen[r.l] = 1;
    t.push_back(r);
  }
  c->tracks[side] = std::move(t);
  c->has_tracks[side] = true;
  c->dirty = true;
  return 0;
}

int unet_ctc_measures(unet_ctc* c, double* out, int64_t* counts) {
  if (!c || !out) return -EINVAL;
  const int rc = c->evaluate();
  if (rc) return rc;
  std::copy(c->out, c->out + 3, out);
  if (counts) std::copy(c->counts, c->counts + 8, counts);
  return 0;
}

long long unet_ctc_log(unet_ctc* c, char* buf, size_t cap) {
  if (!c || (cap > 0 && !buf)) return -EINVAL;
  const int rc = c->evaluate();
  if (rc) return rc;
  if (cap > 0) {
    const size_t n = std::min(cap - 1, c->log.size());
    std::memcpy(buf, c->log.data(), n);
    buf[n] = 0;
  }
  return (long long)c->log.size() + 1;
}

int unet_ctc_num_frames(const unet_ctc* c, int kind) {
  if (!c || (kind != UNET_CTC_SEG && kind != UNET_CTC_TRA)) return -EINVAL;
  return (int)c->frames[kind].size();
}

int unet_ctc_frame_sizes(const unet_ctc* c, int kind, int index, int32_t* out) {
  if (!c || !out || (kind != UNET_CTC_SEG && kind != UNET_CTC_TRA) || index < 0 ||
      index >= (int)c->frames[kind].size())
    return -EINVAL;
  const Frame& f = c->frames[kind][index];
  out[0] = f.frame;
  out[1] = (int32_t)f.gl.size();
  out[2] = (int32_t)f.rl.size();
  out[3] = (int32_t)f.pairs.size();
  return 0;
}

int unet_ctc_frame_tables(const unet_ctc* c, int kind, int index, int32_t* gt_labels, int64_t* gt_areas,
                          int32_t* res_labels, int64_t* res_areas, int64_t* pairs) {
  if (!c || (kind != UNET_CTC_SEG && kind != UNET_CTC_TRA) || index < 0 || index >= (int)c->frames[kind].size())
    return -EINVAL;
  const Frame& f = c->frames[kind][index];
  if (gt_labels) std::copy(f.gl.begin(), f.gl.end(), gt_labels);
  if (gt_areas) std::copy(f.ga.begin(), f.ga.end(), gt_areas);
  if (res_labels) std::copy(f.rl.begin(), f.rl.end(), res_labels);
  if (res_areas) std::copy(f.ra.begin(), f.ra.end(), res_areas);
  if (pairs)
    for (size_t k = 0; k < f.pairs.size(); ++k) {
      pairs[3 * k] = f.pairs[k].g;
      pairs[3 * k + 1] = f.pairs[k].r;
      pairs[3 * k + 2] = f.pairs[k].n;
    }
  return 0;
}

int unet_ctc_stats(const unet_ctc* c, int64_t* out) {
  if (!c || !out) return -EINVAL;
  std::copy(c->stats, c->stats + 6, out);
  return 0;
}

}  // extern "C"
