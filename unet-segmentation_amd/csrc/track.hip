// Cell tracking (SURVEY.md §8f rank 4 remainder): scripts/track.py:103-275.
//
// Per frame the reference builds, for every (previous object, current object)
// pair, two full-frame boolean masks and counts their intersection and union
// (calculate_mask_iou, :73-100) -- O(objects^2 * pixels) host work.  Here one
// pass over the frame pair on the GPU gives the whole overlap table:
//   * label presence flags of both frames -> exclusive scans -> compact indices
//     (background forced to index 0, so objects are 1..n in ascending label
//     order = np.unique's order, get_mask_properties :52-54);
//   * a dense (n_prev + 1) x (n_curr + 1) histogram of (prev, curr) index
//     pairs: cell (i, j) = |prev object i AND curr object j|, row / column sums
//     = the object areas, so IoU = inter / (area_p + area_c - inter) exactly as
//     np.sum(and) / np.sum(or).
// The table (a few 10 KB) goes back to the host, where the tracker -- plain
// C++ below, a statement of track_sequence's control flow including its
// dictionary semantics -- runs the linear sum assignment and the division /
// new-object rules.  The assignment is a restatement of scipy's
// linear_sum_assignment (scipy 1.15.3, scipy/optimize/_lsap: Crouse's
// shortest augmenting path, "Implementing the 2-D rectangular assignment
// problem", IEEE TAES 2016) with the same tie-breaking, because the reference
// calls it on matrices full of equal 1000 entries.
//
// The augmenting_path / lsap functions below transcribe scipy's
// scipy/optimize/rectangular_lsap/rectangular_lsap.cpp, distributed under
// scipy's BSD 3-clause licence:
//
//   Copyright (c) 2001-2002 Enthought, Inc. 2003-2024, SciPy Developers.
//   All rights reserved.
//
//   Redistribution and use in source and binary forms, with or without
//   modification, are permitted provided that the following conditions are
//   met:
//   1. Redistributions of source code must retain the above copyright notice,
//      this list of conditions and the following disclaimer.
//   2. Redistributions in binary form must reproduce the above copyright
//      notice, this list of conditions and the following disclaimer in the
//      documentation and/or other materials provided with the distribution.
//   3. Neither the name of the copyright holder nor the names of its
//      contributors may be used to endorse or promote products derived from
//      this software without specific prior written permission.
//
//   THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS
//   IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT LIMITED TO,
//   THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR
//   PURPOSE ARE DISCLAIMED. IN NO EVENT SHALL THE COPYRIGHT HOLDER OR
//   CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL,
//   EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT LIMITED TO,
//   PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR
//   PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF
//   LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING
//   NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS
//   SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/unet_hip.h"
#include "unet_internal.h"

namespace {

constexpr int kLabels = 65536;
constexpr long long kMaxCells = 1ll << 24;

thread_local std::string g_track_err;

char* carve(char*& p, size_t bytes) {
  char* r = p;
  p += (bytes + 255) / 256 * 256;
  return r;
}

// ------------------------------- GPU part ------------------------------------
__global__ void k_tr_mark(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b, size_t n,
                          int* __restrict__ fa, int* __restrict__ fb) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i == 0) {  // background keeps compact index 0 whether or not it occurs
    fa[0] = 1;
    fb[0] = 1;
  }
  if (i >= n) return;
  if (a) fa[a[i]] = 1;
  fb[b[i]] = 1;
}

// compact index -> label value
__global__ void k_tr_list(const int* __restrict__ flag, const int* __restrict__ idx, int* __restrict__ list) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < kLabels && flag[l]) list[idx[l]] = l;
}

// table[(ia * nb) + ib] += 1 per pixel; a == nullptr: every pixel in row 0
__global__ void k_tr_hist(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b, size_t n,
                          const int* __restrict__ ia, const int* __restrict__ ib, int nb, unsigned* __restrict__ table) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = a ? ia[a[i]] : 0;
  atomicAdd(table + (size_t)r * nb + ib[b[i]], 1u);
}

size_t overlap_ws_bytes(int h, int w) {
  size_t scan = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (const int*)nullptr, (int*)nullptr, kLabels + 1) != hipSuccess)
    return 0;
  return 4 * ((size_t)(kLabels + 1) * 4 + 256) + 2 * ((size_t)kLabels * 4 + 256) + (size_t)kMaxCells * 4 + 256 +
         scan + 256 + (size_t)h * w * 2 + 256;
}

// Overlap table of frames (a, b) (a may be null = no previous frame).  Host
// outputs: label lists (without background) and the (na+1) x (nb+1) table.
hipError_t overlap(const uint16_t* a, const uint16_t* b, int h, int w, void* ws, hipStream_t s,
                   std::vector<int>& la, std::vector<int>& lb, std::vector<unsigned>& table) {
  const size_t n = (size_t)h * w;
  char* c = reinterpret_cast<char*>(ws);
  int* fa = reinterpret_cast<int*>(carve(c, (kLabels + 1) * 4));
  int* fb = reinterpret_cast<int*>(carve(c, (kLabels + 1) * 4));
  int* ia = reinterpret_cast<int*>(carve(c, (kLabels + 1) * 4));
  int* ib = reinterpret_cast<int*>(carve(c, (kLabels + 1) * 4));
  int* lista = reinterpret_cast<int*>(carve(c, kLabels * 4));
  int* listb = reinterpret_cast<int*>(carve(c, kLabels * 4));
  unsigned* tab = reinterpret_cast<unsigned*>(carve(c, (size_t)kMaxCells * 4));
  size_t scan = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan, fa, ia, kLabels + 1, s);
  if (e != hipSuccess) return e;
  void* tmp = carve(c, scan);
  if ((e = hipMemsetAsync(fa, 0, (kLabels + 1) * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(fb, 0, (kLabels + 1) * 4, s)) != hipSuccess) return e;
  const unsigned g = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_tr_mark, dim3(g), dim3(256), 0, s, a, b, n, fa, fb);
  if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, scan, fa, ia, kLabels + 1, s)) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, scan, fb, ib, kLabels + 1, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_tr_list, dim3(kLabels / 256), dim3(256), 0, s, fa, ia, lista);
  hipLaunchKernelGGL(k_tr_list, dim3(kLabels / 256), dim3(256), 0, s, fb, ib, listb);
  int cnt[2];
  if ((e = hipMemcpyAsync(&cnt[0], ia + kLabels, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&cnt[1], ib + kLabels, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  const long long cells = (long long)cnt[0] * cnt[1];
  if (cells > kMaxCells) return hipErrorInvalidValue;
  if ((e = hipMemsetAsync(tab, 0, (size_t)cells * 4, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_tr_hist, dim3(g), dim3(256), 0, s, a, b, n, ia, ib, cnt[1], tab);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  table.resize((size_t)cells);
  std::vector<int> l0(cnt[0]), l1(cnt[1]);
  if ((e = hipMemcpyAsync(table.data(), tab, (size_t)cells * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(l0.data(), lista, (size_t)cnt[0] * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(l1.data(), listb, (size_t)cnt[1] * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  la.assign(l0.begin() + 1, l0.end());
  lb.assign(l1.begin() + 1, l1.end());
  return hipSuccess;
}

// ------------------------- track-labelled result masks -----------------------
// out[f][p] = lut[f][labels[f][p]]: a pure stream, 2 bytes in and 2 bytes out
// per pixel.  One launch covers the stack: workgroup b of a frame takes the
// frame's 16-byte vectors [b * kRlVecPerWg, (b + 1) * kRlVecPerWg), four per
// lane, all four loads issued before the first look-up.  Frame f starts at byte
// 2 f h w of the stack, so its first pixels up to a 16-byte boundary ("head")
// and the last < 8 ("tail") go through scalar accesses of workgroup 0; where
// labels and out sit differently relative to 16 bytes the frame is relabelled
// pixel by pixel.  Every pixel is read and written by the same lane, the read
// first, so out == labels is safe.  The frame's table (lut_len uint16, a
// multiple of 8, at a 16-byte boundary of the workspace) is staged in LDS when
// it has at most kRlLdsLabels entries (16 KiB: eight workgroups of four waves,
// as many as a CU's wave slots hold, take 128 of its 160 KiB) and read through
// L2 otherwise; labels >= lut_len give 0.
constexpr int kRlThreads = 256;
constexpr int kRlVecPerLane = 4;
constexpr int kRlVecPerWg = kRlThreads * kRlVecPerLane;
constexpr unsigned kRlLdsLabels = 8192;

typedef unsigned short rl_us8 __attribute__((ext_vector_type(8)));

template <bool kLds>
__global__ __launch_bounds__(kRlThreads) void k_tr_relabel(const uint16_t* in, uint16_t* out, size_t hw, unsigned bpf,
                                                           const uint16_t* __restrict__ luts, unsigned lut_len) {
  extern __shared__ __attribute__((aligned(16))) uint16_t s_lut[];
  const unsigned f = blockIdx.x / bpf, b = blockIdx.x % bpf, tid = threadIdx.x;
  const uint16_t* lut = luts + (size_t)f * lut_len;
  if (kLds) {
    for (unsigned i = tid; i < lut_len / 8; i += kRlThreads)
      reinterpret_cast<rl_us8*>(s_lut)[i] = reinterpret_cast<const rl_us8*>(lut)[i];
    __syncthreads();
  }
  auto look = [&](unsigned v) -> uint16_t { return v < lut_len ? (kLds ? s_lut[v] : lut[v]) : (uint16_t)0; };
  const uint16_t* fi = in + (size_t)f * hw;
  uint16_t* fo = out + (size_t)f * hw;
  const uintptr_t ai = reinterpret_cast<uintptr_t>(fi), ao = reinterpret_cast<uintptr_t>(fo);
  if ((ai ^ ao) & 15) {  // no common 16-byte phase: scalar, strided over the frame's workgroups
    for (size_t p = (size_t)b * kRlThreads + tid; p < hw; p += (size_t)bpf * kRlThreads) fo[p] = look(fi[p]);
    return;
  }
  size_t head = ((16 - (ai & 15)) & 15) >> 1;
  if (head > hw) head = hw;
  const size_t nvec = (hw - head) / 8, tail = head + nvec * 8;
  if (b == 0) {
    if (tid < head) fo[tid] = look(fi[tid]);
    if (tail + tid < hw) fo[tail + tid] = look(fi[tail + tid]);
  }
  const rl_us8* vi = reinterpret_cast<const rl_us8*>(fi + head);
  rl_us8* vo = reinterpret_cast<rl_us8*>(fo + head);
  const size_t v0 = (size_t)b * kRlVecPerWg + tid;
  rl_us8 r[kRlVecPerLane];
#pragma unroll
  for (int k = 0; k < kRlVecPerLane; ++k) {
    const size_t v = v0 + (size_t)k * kRlThreads;
    if (v < nvec) r[k] = vi[v];
  }
#pragma unroll
  for (int k = 0; k < kRlVecPerLane; ++k) {
    const size_t v = v0 + (size_t)k * kRlThreads;
    if (v < nvec) {
      rl_us8 o;
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = look(r[k][q]);
      vo[v] = o;
    }
  }
}

std::atomic<long long> g_relabel_launches{0};

// --------------------------- linear sum assignment ---------------------------
// Shortest augmenting path (Crouse 2016) as scipy implements it: columns are
// scanned from a "remaining" list filled in reverse order, ties go to a column
// that ends the path; a tall matrix is solved transposed and the result sorted
// by row.  Returns 0, or -1 for an infeasible / invalid matrix.
long long augmenting_path(long long nc, const double* cost, std::vector<double>& u, std::vector<double>& v,
                          std::vector<long long>& path, std::vector<long long>& row4col,
                          std::vector<double>& spc, long long i, std::vector<char>& SR, std::vector<char>& SC,
                          std::vector<long long>& remaining, double* p_min) {
  double minVal = 0;
  long long num_remaining = nc;
  for (long long it = 0; it < nc; ++it) remaining[it] = nc - it - 1;
  std::fill(SR.begin(), SR.end(), 0);
  std::fill(SC.begin(), SC.end(), 0);
  std::fill(spc.begin(), spc.end(), INFINITY);
  long long sink = -1;
  while (sink == -1) {
    long long index = -1;
    double lowest = INFINITY;
    SR[i] = 1;
    for (long long it = 0; it < num_remaining; ++it) {
      const long long j = remaining[it];
      const double r = minVal + cost[i * nc + j] - u[i] - v[j];
      if (r < spc[j]) {
        path[j] = i;
        spc[j] = r;
      }
      if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) {
        lowest = spc[j];
        index = it;
      }
    }
    minVal = lowest;
    if (minVal == INFINITY) return -1;
    const long long j = remaining[index];
    if (row4col[j] == -1)
      sink = j;
    else
      i = row4col[j];
    SC[j] = 1;
    remaining[index] = remaining[--num_remaining];
  }
  *p_min = minVal;
  return sink;
}

int lsap(long long nr, long long nc, const double* cost_in, int64_t* a, int64_t* b) {
  if (nr == 0 || nc == 0) return 0;
  const bool transpose = nc < nr;
  std::vector<double> temp;
  const double* cost = cost_in;
  if (transpose) {
    temp.resize((size_t)(nr * nc));
    for (long long i = 0; i < nr; ++i)
      for (long long j = 0; j < nc; ++j) temp[j * nr + i] = cost_in[i * nc + j];
    std::swap(nr, nc);
    cost = temp.data();
  }
  for (long long i = 0; i < nr * nc; ++i)
    if (cost[i] != cost[i] || cost[i] == -INFINITY) return -1;
  std::vector<double> u(nr, 0), v(nc, 0), spc(nc);
  std::vector<long long> path(nc, -1), col4row(nr, -1), row4col(nc, -1), remaining(nc);
  std::vector<char> SR(nr), SC(nc);
  for (long long cur = 0; cur < nr; ++cur) {
    double minVal;
    const long long sink = augmenting_path(nc, cost, u, v, path, row4col, spc, cur, SR, SC, remaining, &minVal);
    if (sink < 0) return -1;
    u[cur] += minVal;
    for (long long i = 0; i < nr; ++i)
      if (SR[i] && i != cur) u[i] += minVal - spc[col4row[i]];
    for (long long j = 0; j < nc; ++j)
      if (SC[j]) v[j] -= minVal - spc[j];
    long long j = sink;
    while (true) {
      const long long i = path[j];
      row4col[j] = i;
      std::swap(col4row[i], j);
      if (i == cur) break;
    }
  }
  if (transpose) {
    std::vector<long long> order(nr);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](long long x, long long y) { return col4row[x] < col4row[y]; });
    for (long long k = 0; k < nr; ++k) {
      a[k] = col4row[order[k]];
      b[k] = order[k];
    }
  } else {
    for (long long i = 0; i < nr; ++i) {
      a[i] = i;
      b[i] = col4row[i];
    }
  }
  return 0;
}

}  // namespace

// ------------------------------- host tracker --------------------------------
struct unet_tracker {
  int h = 0, w = 0;
  double iou_track = 0.3, iou_div = 0.1;
  int max_children = 2;
  struct Track {
    int label, start, end, parent;
  };
  std::vector<Track> tracks;        // track id = index + 1 (next_track_id, :126)
  std::vector<int> active;          // active_tracks_by_obj_label: label -> track id, -1 = absent (:131)
  std::vector<int> prev_labels;     // prev_frame_properties keys (ascending)
  std::vector<long long> prev_area;
  bool first = true;
  bool has_prev_dev = false;        // the device copy of the previous frame is valid
  // UNET_TRACK_SCOPE_FRAME: `active` holds the previous frame's labels only and
  // the current frame's go to `active_next`; the two swap when the step ends
  int scope = UNET_TRACK_SCOPE_SHARED;
  std::vector<int> active_next;
  struct FrameMap {
    int frame;
    std::vector<int> labels, ids;   // ascending labels; track id per label, 0 = none
  };
  std::vector<FrameMap> maps;       // one per step, in the order given
  std::map<int, int> map_of_frame;  // frame number -> index of its last map
  std::vector<uint16_t> lut_stage;  // unet_tracker_relabel's host tables (the upload's source)
  unet_tracker() : active(kLabels, -1) {}

  int new_track(int frame, int parent) {
    tracks.push_back({(int)tracks.size() + 1, frame, frame, parent});
    return (int)tracks.size();
  }

  // one iteration of track_sequence's frame loop (:133-258) from the overlap
  // table inter[i * nc + j] of previous object i and current object j
  int step(int frame, const std::vector<int>& cur, const std::vector<long long>& area,
           const std::vector<long long>& inter) {
    const long long np = (long long)prev_labels.size(), nc = (long long)cur.size();
    const bool scoped = scope == UNET_TRACK_SCOPE_FRAME;
    if (scoped) active_next.assign(kLabels, -1);
    std::vector<int>& now = scoped ? active_next : active;  // where current-frame labels are assigned
    if (first) {
      for (int lab : cur) now[lab] = new_track(frame, -1);
      first = false;
    } else {
      auto iou_of = [&](long long i, long long j) -> double {
        const long long it = inter[i * nc + j];
        const long long un = prev_area[i] + area[j] - it;
        return un == 0 ? 0.0 : (double)it / (double)un;
      };
      std::vector<char> mp(np, 0), mc(nc, 0);
      if (np > 0 && nc > 0) {
        std::vector<double> cost((size_t)(np * nc), 1000.0);
        for (long long i = 0; i < np; ++i)
          for (long long j = 0; j < nc; ++j) {
            const double iou = iou_of(i, j);
            if (iou > 0) cost[i * nc + j] = 1 - iou;
          }
        const long long k = std::min(np, nc);
        std::vector<int64_t> ri(k), ci(k);
        if (lsap(np, nc, cost.data(), ri.data(), ci.data()) != 0) return -EINVAL;
        for (long long q = 0; q < k; ++q) {
          const long long i = ri[q], j = ci[q];
          const int pl = prev_labels[i], cl = cur[j];
          const double iou = 1 - cost[i * nc + j];
          if (iou >= iou_track && active[pl] >= 0) {
            const int tid = active[pl];
            tracks[tid - 1].end = frame;
            active[pl] = -1;
            now[cl] = tid;
            mp[i] = 1;
            mc[j] = 1;
          }
        }
      }
      // division (:204-243): the unmatched lists are taken once, before any
      // division is recorded
      std::vector<long long> up, uc;
      for (long long i = 0; i < np; ++i)
        if (!mp[i]) up.push_back(i);
      for (long long j = 0; j < nc; ++j)
        if (!mc[j]) uc.push_back(j);
      for (long long i : up) {
        const int pl = prev_labels[i];
        if (active[pl] < 0) continue;
        std::vector<long long> kids;
        for (long long j : uc)
          if (iou_of(i, j) >= iou_div) kids.push_back(j);
        if ((int)kids.size() >= 2 && (int)kids.size() <= max_children) {
          const int parent = active[pl];
          tracks[parent - 1].end = frame - 1;
          active[pl] = -1;
          for (long long j : kids) {
            now[cur[j]] = new_track(frame, parent);
            mc[j] = 1;
          }
        }
      }
      for (long long j = 0; j < nc; ++j)  // new objects (:248-254)
        if (!mc[j]) now[cur[j]] = new_track(frame, -1);
    }
    FrameMap m;
    m.frame = frame;
    m.labels = cur;
    m.ids.reserve(cur.size());
    for (int lab : cur) m.ids.push_back(std::max(now[lab], 0));
    map_of_frame[frame] = (int)maps.size();
    maps.push_back(std::move(m));
    if (scoped) active.swap(active_next);
    prev_labels = cur;
    prev_area = area;
    return 0;
  }
};

extern "C" {

int unet_linear_sum_assignment(long long nr, long long nc, const double* cost, int64_t* row_ind, int64_t* col_ind) {
  if (nr < 0 || nc < 0 || ((nr > 0 && nc > 0) && (!cost || !row_ind || !col_ind))) return -EINVAL;
  return lsap(nr, nc, cost, row_ind, col_ind) == 0 ? 0 : -EINVAL;
}

unet_tracker* unet_tracker_create(int h, int w, double iou_track, double iou_division, int max_children) {
  if (h < 1 || w < 1 || max_children < 1) return nullptr;
  auto* t = new unet_tracker();
  t->h = h;
  t->w = w;
  t->iou_track = iou_track;
  t->iou_div = iou_division;
  t->max_children = max_children;
  return t;
}

void unet_tracker_destroy(unet_tracker* t) { delete t; }

size_t unet_tracker_ws_bytes(int h, int w) { return h > 0 && w > 0 ? overlap_ws_bytes(h, w) : 0; }

int unet_tracker_step_host(unet_tracker* t, int frame, int n_curr, const int32_t* labels, const int64_t* areas,
                           const int64_t* inter) {
  if (!t || n_curr < 0 || (n_curr > 0 && (!labels || !areas))) return -EINVAL;
  const long long np = (long long)t->prev_labels.size();
  if (np > 0 && n_curr > 0 && !inter && !t->first) return -EINVAL;
  std::vector<int> cur(labels, labels + n_curr);
  for (int k = 0; k < n_curr; ++k)
    if (cur[k] <= 0 || cur[k] >= kLabels || (k > 0 && cur[k] <= cur[k - 1])) return -EINVAL;
  std::vector<long long> area(areas, areas + n_curr);
  std::vector<long long> it;
  if (!t->first && np > 0 && n_curr > 0) it.assign(inter, inter + np * n_curr);
  return t->step(frame, cur, area, it);
}

int unet_tracker_add_frame(unet_tracker* t, const uint16_t* labels, int frame, void* ws, unet_stream_t stream) {
  if (!t || !labels || !ws) return -EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t n = (size_t)t->h * t->w;
  // the previous frame's copy sits at the end of the workspace
  char* base = reinterpret_cast<char*>(ws);
  uint16_t* prev = reinterpret_cast<uint16_t*>(base + overlap_ws_bytes(t->h, t->w) - ((n * 2 + 255) / 256 * 256));
  std::vector<int> la, lb;
  std::vector<unsigned> tab;
  hipError_t e = overlap(t->has_prev_dev ? prev : nullptr, labels, t->h, t->w, ws, s, la, lb, tab);
  if (e != hipSuccess) {
    g_track_err = std::string("unet_tracker_add_frame: ") + hipGetErrorString(e);
    return e == hipErrorInvalidValue ? -EINVAL : -EIO;
  }
  const long long nb = (long long)lb.size() + 1, na = (long long)la.size() + 1;
  std::vector<long long> area(nb - 1, 0), inter;
  for (long long r = 0; r < na; ++r)
    for (long long j = 1; j < nb; ++j) area[j - 1] += tab[r * nb + j];
  if (t->has_prev_dev) {
    // the previous objects must be the ones the tracker holds (same frame)
    if (la != t->prev_labels) return -EINVAL;
    inter.resize((size_t)((na - 1) * (nb - 1)));
    for (long long i = 1; i < na; ++i)
      for (long long j = 1; j < nb; ++j) inter[(i - 1) * (nb - 1) + (j - 1)] = tab[i * nb + j];
  }
  const int rc = t->step(frame, lb, area, inter);
  if (rc) return rc;
  if ((e = hipMemcpyAsync(prev, labels, n * 2, hipMemcpyDeviceToDevice, s)) != hipSuccess) return -EIO;
  t->has_prev_dev = true;
  return 0;
}

int unet_tracker_num_tracks(const unet_tracker* t) { return t ? (int)t->tracks.size() : -EINVAL; }

int unet_tracker_tracks(const unet_tracker* t, int32_t* out, int cap) {
  if (!t || (cap > 0 && !out)) return -EINVAL;
  // output order and clamping of the res_track.txt writer (:265-272)
  std::vector<int> order(t->tracks.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    const auto &a = t->tracks[x], &b = t->tracks[y];
    return a.start != b.start ? a.start < b.start : a.label < b.label;
  });
  const int k = std::min(cap, (int)order.size());
  for (int q = 0; q < k; ++q) {
    const auto& tr = t->tracks[order[q]];
    out[4 * q + 0] = tr.label;
    out[4 * q + 1] = tr.start;
    out[4 * q + 2] = std::max(tr.start, tr.end);
    out[4 * q + 3] = tr.parent;
  }
  return (int)order.size();
}

int unet_tracker_set_label_scope(unet_tracker* t, int scope) {
  if (!t || (scope != UNET_TRACK_SCOPE_SHARED && scope != UNET_TRACK_SCOPE_FRAME)) return -EINVAL;
  if (!t->maps.empty()) return -EBUSY;
  t->scope = scope;
  return 0;
}

int unet_tracker_num_frames(const unet_tracker* t) { return t ? (int)t->maps.size() : -EINVAL; }

int unet_tracker_frame_map(const unet_tracker* t, int index, int32_t* frame, int32_t* labels, int32_t* track_ids,
                           int cap) {
  if (!t || index < 0 || index >= (int)t->maps.size()) return -EINVAL;
  const auto& m = t->maps[index];
  if (frame) *frame = m.frame;
  const int k = std::min(std::max(cap, 0), (int)m.labels.size());
  for (int q = 0; q < k; ++q) {
    if (labels) labels[q] = m.labels[q];
    if (track_ids) track_ids[q] = m.ids[q];
  }
  return (int)m.labels.size();
}

size_t unet_tracker_relabel_ws_bytes(int t, int h, int w) {
  return t > 0 && h > 0 && w > 0 ? ((size_t)t * kLabels * 2 + 255) / 256 * 256 : 0;
}

int unet_tracker_relabel(unet_tracker* t, const uint16_t* labels, const int32_t* host_frames, int n, uint16_t* out,
                         void* ws, unet_stream_t stream) {
  if (!t || n < 0) return -EINVAL;
  if (n == 0) return 0;
  if (!labels || !out || !host_frames || !ws || (reinterpret_cast<uintptr_t>(labels) & 1) ||
      (reinterpret_cast<uintptr_t>(out) & 1) || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    unet::set_last_error("unet_tracker_relabel: null labels / frames / out / ws, labels or out not 2-byte aligned, or "
                         "ws not 256-byte aligned");
    return -EINVAL;
  }
  const size_t hw = (size_t)t->h * t->w;
  const size_t bpf = std::max<size_t>(1, (hw / 8 + kRlVecPerWg - 1) / kRlVecPerWg);
  if (bpf * (size_t)n > 0x7fffffffull) {
    unet::set_last_error("unet_tracker_relabel: the stack needs more than 2^31 - 1 workgroups");
    return -EINVAL;
  }
  // every error is found from the host maps, before any device call
  std::vector<const unet_tracker::FrameMap*> maps((size_t)n);
  int top = 0;
  for (int i = 0; i < n; ++i) {
    const auto it = t->map_of_frame.find(host_frames[i]);
    if (it == t->map_of_frame.end()) {
      unet::set_last_error("unet_tracker_relabel: frame " + std::to_string(host_frames[i]) +
                           " was never given to this tracker");
      return -ENOENT;
    }
    const auto& m = t->maps[it->second];
    for (int id : m.ids)
      if (id > 65535) {
        unet::set_last_error("unet_tracker_relabel: frame " + std::to_string(m.frame) + " holds track id " +
                             std::to_string(id) + ", above the 65535 a 16-bit mask carries");
        return -ERANGE;
      }
    if (!m.labels.empty()) top = std::max(top, m.labels.back());
    maps[i] = &m;
  }
  const unsigned lut_len = (unsigned)((top + 1 + 7) / 8 * 8);  // <= 65536
  t->lut_stage.assign((size_t)n * lut_len, 0);
  for (int i = 0; i < n; ++i) {
    uint16_t* lut = t->lut_stage.data() + (size_t)i * lut_len;
    for (size_t q = 0; q < maps[i]->labels.size(); ++q) lut[maps[i]->labels[q]] = (uint16_t)maps[i]->ids[q];
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint16_t* luts = reinterpret_cast<uint16_t*>(ws);
  hipError_t e = hipMemcpyAsync(luts, t->lut_stage.data(), t->lut_stage.size() * 2, hipMemcpyHostToDevice, s);
  // lut_stage is rewritten by the next call: the copy has left it before we return
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)(bpf * (size_t)n));
    if (lut_len <= kRlLdsLabels)
      hipLaunchKernelGGL(k_tr_relabel<true>, grid, dim3(kRlThreads), lut_len * 2, s, labels, out, hw, (unsigned)bpf,
                         luts, lut_len);
    else
      hipLaunchKernelGGL(k_tr_relabel<false>, grid, dim3(kRlThreads), 0, s, labels, out, hw, (unsigned)bpf, luts,
                         lut_len);
    g_relabel_launches.fetch_add(1);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    unet::set_last_error(std::string("unet_tracker_relabel: ") + hipGetErrorString(e));
    return -EIO;
  }
  return 0;
}

long long unet_tracker_relabel_launches(int reset) {
  return reset ? g_relabel_launches.exchange(0) : g_relabel_launches.load();
}

int unet_tracker_load_result(unet_tracker* t, const int32_t* rows, int n_rows, const int32_t* frames, int n_frames,
                             const int32_t* map_offsets, const int32_t* labels, const int32_t* ids) {
  if (!t || n_rows < 0 || n_frames < 0 || (n_rows > 0 && !rows) || (n_frames > 0 && (!frames || !map_offsets))) {
    unet::set_last_error("unet_tracker_load_result: null tracker / rows / frames / map_offsets or a negative count");
    return -EINVAL;
  }
  if (!t->maps.empty() || !t->first) return -EBUSY;
  for (int q = 0; q < n_rows; ++q)
    if (rows[4 * q] != q + 1 || rows[4 * q + 3] == 0 || rows[4 * q + 3] > n_rows) {
      unet::set_last_error("unet_tracker_load_result: row " + std::to_string(q) + " must carry track id " +
                           std::to_string(q + 1) + " and a parent of -1 or another row's id");
      return -EINVAL;
    }
  for (int f = 0; f < n_frames; ++f) {
    if ((f > 0 && frames[f] <= frames[f - 1]) || map_offsets[f] < 0 || map_offsets[f + 1] < map_offsets[f] ||
        (map_offsets[f + 1] > map_offsets[f] && (!labels || !ids))) {
      unet::set_last_error("unet_tracker_load_result: frame numbers must ascend strictly and map_offsets ascend");
      return -EINVAL;
    }
    for (int k = map_offsets[f]; k < map_offsets[f + 1]; ++k)
      if (labels[k] <= 0 || labels[k] >= kLabels || (k > map_offsets[f] && labels[k] <= labels[k - 1]) || ids[k] < 0 ||
          ids[k] > n_rows) {
        unet::set_last_error("unet_tracker_load_result: frame " + std::to_string(frames[f]) +
                             " needs ascending labels in [1, 65535] and track ids in [0, n_rows]");
        return -EINVAL;
      }
  }
  t->tracks.reserve((size_t)n_rows);
  for (int q = 0; q < n_rows; ++q)
    t->tracks.push_back({rows[4 * q], rows[4 * q + 1], rows[4 * q + 2], rows[4 * q + 3] < 0 ? -1 : rows[4 * q + 3]});
  for (int f = 0; f < n_frames; ++f) {
    unet_tracker::FrameMap m;
    m.frame = frames[f];
    m.labels.assign(labels + map_offsets[f], labels + map_offsets[f + 1]);
    m.ids.assign(ids + map_offsets[f], ids + map_offsets[f + 1]);
    t->map_of_frame[m.frame] = (int)t->maps.size();
    t->maps.push_back(std::move(m));
  }
  return 0;
}

}  // extern "C"
