// Host-side self test of libunet_hip's pure-host logic, built with
// AddressSanitizer + UndefinedBehaviorSanitizer (csrc/Makefile target
// `sanitize`, host-only objects: no device code, no HIP call is made).
// Covers: plan shape / workspace layout arithmetic over many input sizes, the
// segment table, argument validation of the C ABI, the linear sum assignment
// (random, tied, rectangular, degenerate matrices; checked for a valid
// assignment and against brute force on small ones), the tracker's host step
// on a synthetic sequence, the Cell Tracking Challenge evaluator's host entry
// points (measures, log, error paths), the tuning report, and the GEMM variant selection
// (tile tables, fits, candidate lists, forced knobs) over synthetic launch
// arguments, compared line for line with tests/golden/gemm_selection.txt.
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <algorithm>
#include <string>
#include <vector>

#include "../include/unet_hip.h"
#include "unet_internal.h"

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                     \
    }                                                              \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double urand() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static void test_plans() {
  const int sizes[] = {188, 195, 198, 204, 220, 252, 300, 508, 512, 572, 700};
  for (int prec = 0; prec < 3; ++prec)
    for (int h : sizes)
      for (int n : {1, 2, 8})
        for (int c : {1, 3}) {
          unet_plan* p = unet_plan_create_ex(n, c, h, h + 4 * (n == 2), 2, prec);
          if (!p) continue;  // sizes the valid U-Net cannot take
          int oh = 0, ow = 0;
          CHECK(unet_plan_out_hw(p, &oh, &ow) == 0 && oh > 0 && ow > 0);
          const size_t full = unet_plan_workspace_bytes(p), fwd = unet_plan_forward_workspace_bytes(p);
          CHECK(fwd > 0 && fwd < full && full % 256 == 0);
          CHECK(unet_plan_precision(p) == prec);
          int total = 0;
          for (int s = 0; s < unet_plan_num_segments(p); ++s) {
            int f = -1, k = -1;
            CHECK(unet_plan_segment_grads(p, s, &f, &k) == 0 && f >= 0 && k > 0 && f + k <= 82);
            total += k;
          }
          CHECK(total == 82);
          CHECK(unet_plan_segment_grads(p, 9, nullptr, nullptr) != 0);
          unet_plan_destroy(p);
        }
  CHECK(unet_plan_create(1, 1, 100, 100, 2) == nullptr);  // too small
  CHECK(unet_plan_create(1, 4097, 512, 512, 2) == nullptr);  // c_in > 4096 (kMaxInChannels)
  CHECK(unet_plan_create(1, 1, 512, 512, 4097) == nullptr);  // n_classes > 4096 (kMaxClassCount)
  CHECK(unet_plan_create(1, 0, 512, 512, 2) == nullptr);
  CHECK(unet_plan_create(1, 1, 512, 512, 0) == nullptr);
  if (unet_plan* q = unet_plan_create(1, 5, 188, 188, 5)) {  // 5 channels / 5 classes take a plan
    CHECK(unet_plan_num_params(q) == 136);
    unet_plan_destroy(q);
  } else {
    CHECK(false);
  }
  CHECK(unet_plan_create_ex(1, 1, 512, 512, 2, 7) == nullptr);
  CHECK(unet_plan_forward(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr) != 0);
  CHECK(unet_plan_backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 9, nullptr) != 0);
  unet_plan_destroy(nullptr);
}

static double assignment_cost(const std::vector<double>& c, int nc, const std::vector<int64_t>& r,
                              const std::vector<int64_t>& q) {
  double s = 0;
  for (size_t i = 0; i < r.size(); ++i) s += c[r[i] * nc + q[i]];
  return s;
}

static void test_lsap() {
  for (int trial = 0; trial < 300; ++trial) {
    const int nr = 1 + (int)(urand() * 9), nc = 1 + (int)(urand() * 9);
    const int kind = trial % 3;
    std::vector<double> c((size_t)nr * nc);
    for (auto& v : c) v = kind == 0 ? urand() : kind == 1 ? (double)(int)(urand() * 3) : (urand() < 0.1 ? urand() : 1000.0);
    const int k = std::min(nr, nc);
    std::vector<int64_t> r(k), q(k);
    CHECK(unet_linear_sum_assignment(nr, nc, c.data(), r.data(), q.data()) == 0);
    std::vector<char> ur(nr, 0), uc(nc, 0);
    for (int i = 0; i < k; ++i) {
      CHECK(r[i] >= 0 && r[i] < nr && q[i] >= 0 && q[i] < nc);
      CHECK(!ur[r[i]] && !uc[q[i]]);
      ur[r[i]] = uc[q[i]] = 1;
      if (i) CHECK(r[i] > r[i - 1]);
    }
    // brute force over injections of the smaller side (sizes <= 9)
    const bool rows_small = nr <= nc;
    const int a = rows_small ? nr : nc, b = rows_small ? nc : nr;
    std::vector<int> perm(b);
    std::iota(perm.begin(), perm.end(), 0);
    double best = INFINITY;
    if (b <= 7) {
      do {
        double s = 0;
        for (int i = 0; i < a; ++i) s += rows_small ? c[(size_t)i * nc + perm[i]] : c[(size_t)perm[i] * nc + i];
        best = std::min(best, s);
      } while (std::next_permutation(perm.begin(), perm.end()));
      CHECK(std::fabs(assignment_cost(c, nc, r, q) - best) <= 1e-9 * std::max(1.0, std::fabs(best)));
    }
  }
  std::vector<double> bad = {0.0, NAN, 1.0, 2.0};
  std::vector<int64_t> r(2), q(2);
  CHECK(unet_linear_sum_assignment(2, 2, bad.data(), r.data(), q.data()) != 0);
  CHECK(unet_linear_sum_assignment(0, 3, nullptr, nullptr, nullptr) == 0);
  CHECK(unet_linear_sum_assignment(-1, 3, nullptr, nullptr, nullptr) != 0);
}

static void test_tracker() {
  unet_tracker* t = unet_tracker_create(8, 8, 0.3, 0.1, 2);
  CHECK(t != nullptr);
  // frame 0: objects 3, 9; frame 1: 3 continues, 9 splits into 4 and 5; frame 2: empty
  const int32_t l0[] = {3, 9};
  const int64_t a0[] = {10, 20};
  CHECK(unet_tracker_step_host(t, 0, 2, l0, a0, nullptr) == 0);
  const int32_t l1[] = {3, 4, 5};
  const int64_t a1[] = {10, 6, 6};
  const int64_t i1[] = {10, 0, 0, 0, 5, 5};  // 2 x 3
  CHECK(unet_tracker_step_host(t, 1, 3, l1, a1, i1) == 0);
  CHECK(unet_tracker_step_host(t, 2, 0, nullptr, nullptr, nullptr) == 0);
  const int n = unet_tracker_num_tracks(t);
  CHECK(n == 4);
  std::vector<int32_t> rows(4 * (size_t)n);
  CHECK(unet_tracker_tracks(t, rows.data(), n) == n);
  // track 1 (label 3) 0..1, track 2 (label 9) ends at 0, children 3 and 4 at 1 with parent 2
  CHECK(rows[0] == 1 && rows[1] == 0 && rows[2] == 1 && rows[3] == -1);
  CHECK(rows[4] == 2 && rows[5] == 0 && rows[6] == 0 && rows[7] == -1);
  CHECK(rows[8] == 3 && rows[11] == 2 && rows[12] == 4 && rows[15] == 2);
  const int32_t unsorted[] = {5, 2};
  CHECK(unet_tracker_step_host(t, 3, 2, unsorted, a0, nullptr) != 0);
  CHECK(unet_tracker_tracks(t, nullptr, 0) == n);
  // frame maps: one per accepted step (the rejected one left none)
  CHECK(unet_tracker_num_frames(t) == 3);
  int32_t fr = -1, lab[3] = {0, 0, 0}, ids[3] = {0, 0, 0};
  CHECK(unet_tracker_frame_map(t, 1, &fr, lab, ids, 3) == 3 && fr == 1);
  CHECK(lab[0] == 3 && lab[1] == 4 && lab[2] == 5 && ids[0] == 1 && ids[1] == 3 && ids[2] == 4);
  CHECK(unet_tracker_frame_map(t, 0, nullptr, nullptr, ids, 1) == 2 && ids[0] == 1 && ids[1] == 3);
  CHECK(unet_tracker_frame_map(t, 2, &fr, nullptr, nullptr, 0) == 0 && fr == 2);
  CHECK(unet_tracker_frame_map(t, 3, nullptr, nullptr, nullptr, 0) == -EINVAL);
  CHECK(unet_tracker_frame_map(t, -1, nullptr, nullptr, nullptr, 0) == -EINVAL);
  CHECK(unet_tracker_set_label_scope(t, UNET_TRACK_SCOPE_FRAME) == -EBUSY);
  // relabel's errors come from the host maps: the pointers are never touched
  uint16_t* dummy = reinterpret_cast<uint16_t*>(uintptr_t(0x10000));
  const int32_t absent[] = {9};
  CHECK(unet_tracker_relabel(t, dummy, absent, 1, dummy, dummy, nullptr) == -ENOENT);
  CHECK(std::strstr(unet_last_error(), "frame 9") != nullptr);
  CHECK(unet_tracker_relabel(t, nullptr, absent, 1, dummy, dummy, nullptr) == -EINVAL);
  CHECK(unet_tracker_relabel(t, dummy, absent, 0, dummy, dummy, nullptr) == 0);
  CHECK(unet_tracker_relabel_ws_bytes(2, 8, 8) == 2 * 65536 * 2 && unet_tracker_relabel_ws_bytes(0, 8, 8) == 0);
  unet_tracker_destroy(t);
  CHECK(unet_tracker_create(0, 8, 0.3, 0.1, 2) == nullptr);
  unet_tracker_destroy(nullptr);
  // the two label scopes on the reference's quirk: previous objects 3 and 4, current 4 and 5,
  // "previous 3 -> current 4" then "previous 4 -> current 5"
  for (int scope = 0; scope < 2; ++scope) {
    unet_tracker* s = unet_tracker_create(8, 8, 0.3, 0.1, 2);
    CHECK(s != nullptr);
    CHECK(unet_tracker_set_label_scope(s, 2) == -EINVAL);
    CHECK(unet_tracker_set_label_scope(s, scope) == 0);
    const int32_t p[] = {3, 4}, c[] = {4, 5};
    const int64_t ar[] = {10, 10};
    const int64_t in[] = {10, 0, 0, 10};  // 3 -> 4 and 4 -> 5, IoU 1 each
    CHECK(unet_tracker_step_host(s, 0, 2, p, ar, nullptr) == 0);
    CHECK(unet_tracker_step_host(s, 1, 2, c, ar, in) == 0);
    int32_t l2[2], i2[2];
    CHECK(unet_tracker_frame_map(s, 1, nullptr, l2, i2, 2) == 2 && l2[0] == 4 && l2[1] == 5);
    // shared: current 4's entry replaces previous 4's, so the second link moves track 1 on to
    // current 5 and current 4 is left without a track
    if (scope == UNET_TRACK_SCOPE_SHARED) CHECK(i2[0] == 0 && i2[1] == 1);
    else CHECK(i2[0] == 1 && i2[1] == 2);
    CHECK(unet_tracker_num_tracks(s) == 2);
    unet_tracker_destroy(s);
  }
}

static void test_ctc() {
  // two frames, GT objects 1 and 2 in both
  const int32_t gl[] = {1, 2};
  const int64_t ga[] = {10, 20};
  const int32_t gt_rows[] = {1, 0, 1, 0, 2, 0, 1, 0};
  {  // RES = GT: 1 / 1 / 1, no operation
    unet_ctc* c = unet_ctc_create();
    CHECK(c != nullptr);
    const int64_t pairs[] = {1, 1, 10, 2, 2, 20};
    for (int f = 0; f < 2; ++f) CHECK(unet_ctc_add_frame_host(c, UNET_CTC_TRA, f, 2, gl, ga, 2, gl, ga, 2, pairs) == 0);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 1, 2, gl, ga, 2, gl, ga, 2, pairs) == 0);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 1, 2, gl, ga, 2, gl, ga, 2, pairs) == -EEXIST);
    double out[3];
    int64_t n[8];
    CHECK(unet_ctc_measures(c, out, n) == 0 && out[0] == 1.0 && out[1] == 1.0 && std::isnan(out[2]));  // no tracks yet
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_GT, gt_rows, 2) == 0 && unet_ctc_set_tracks(c, UNET_CTC_RES, gt_rows, 2) == 0);
    CHECK(unet_ctc_measures(c, out, n) == 0 && out[0] == 1.0 && out[1] == 1.0 && out[2] == 1.0);
    CHECK(n[0] + n[1] + n[2] + n[3] + n[4] + n[5] == 0 && n[6] == 4 && n[7] == 2);
    const long long need = unet_ctc_log(c, nullptr, 0);
    CHECK(need > 0);
    std::vector<char> buf((size_t)need), cut(8);
    CHECK(unet_ctc_log(c, buf.data(), buf.size()) == need && std::strlen(buf.data()) + 1 == (size_t)need);
    CHECK(std::strstr(buf.data(), "TRA measure: 1.000000\n") != nullptr);
    CHECK(unet_ctc_log(c, cut.data(), cut.size()) == need && std::strlen(cut.data()) == 7);
    int32_t sz[4];
    CHECK(unet_ctc_num_frames(c, UNET_CTC_TRA) == 2 && unet_ctc_frame_sizes(c, UNET_CTC_TRA, 1, sz) == 0);
    CHECK(sz[0] == 1 && sz[1] == 2 && sz[2] == 2 && sz[3] == 2);
    int64_t pr[6];
    CHECK(unet_ctc_frame_tables(c, UNET_CTC_TRA, 1, nullptr, nullptr, nullptr, nullptr, pr) == 0 && pr[5] == 20);
    CHECK(unet_ctc_frame_sizes(c, UNET_CTC_TRA, 2, sz) != 0);
    unet_ctc_destroy(c);
  }
  {  // a RES vertex over both GT objects, a half-covered object, an extra one
    unet_ctc* c = unet_ctc_create();
    const int32_t r0[] = {1}, r1[] = {1, 3};
    const int64_t a0[] = {30}, a1[] = {10, 20};
    const int64_t p0[] = {1, 1, 10, 2, 1, 20}, p1[] = {1, 1, 10, 2, 3, 10};  // 2 * 10 > 20 is false
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_TRA, 1, 2, gl, ga, 2, r1, a1, 2, p1) == 0);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_TRA, 0, 2, gl, ga, 1, r0, a0, 2, p0) == 0);
    const int32_t res_rows[] = {1, 0, 1, 0, 3, 1, 1, 0};
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_GT, gt_rows, 2) == 0 && unet_ctc_set_tracks(c, UNET_CTC_RES, res_rows, 2) == 0);
    double out[3];
    int64_t n[8];
    CHECK(unet_ctc_measures(c, out, n) == 0);
    CHECK(n[0] == 1 && n[1] == 1 && n[2] == 1 && n[3] == 0 && n[4] == 2 && n[5] == 0 && n[6] == 4 && n[7] == 2);
    CHECK(std::isnan(out[0]) && out[1] == 1.0 - 16.0 / 40.0 && out[2] == 1.0 - 19.0 / 43.0);
    // a label without a row, then a parent without one
    const int32_t short_rows[] = {1, 0, 1, 0}, orphan[] = {1, 0, 1, 0, 3, 1, 1, 7};
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_RES, short_rows, 1) == 0);
    CHECK(unet_ctc_measures(c, out, n) == -ENOENT && std::strstr(unet_last_error(), "RES label 3") != nullptr &&
          std::strstr(unet_last_error(), "frame 1") != nullptr);
    CHECK(unet_ctc_log(c, nullptr, 0) == -ENOENT);
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_RES, orphan, 2) == 0);
    CHECK(unet_ctc_measures(c, out, n) == -ESRCH && std::strstr(unet_last_error(), "parent 7") != nullptr);
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_RES, res_rows, 2) == 0 && unet_ctc_measures(c, out, n) == 0);
    // argument errors
    const int32_t twice[] = {1, 0, 1, 0, 1, 0, 1, 0}, unsorted[] = {2, 1};
    CHECK(unet_ctc_set_tracks(c, UNET_CTC_RES, twice, 2) == -EINVAL);
    CHECK(unet_ctc_set_tracks(c, 2, twice, 1) == -EINVAL);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 5, 2, gl, ga, -1, nullptr, nullptr, 0, nullptr) == -ENODATA);
    CHECK(std::strstr(unet_last_error(), "frame 5") != nullptr);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 5, 2, unsorted, ga, 0, nullptr, nullptr, 0, nullptr) == -EINVAL);
    const int64_t big[] = {1, 1, 11}, missing[] = {1, 2, 1};
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 5, 2, gl, ga, 1, r0, a0, 1, big) == -EINVAL);
    CHECK(unet_ctc_add_frame_host(c, UNET_CTC_SEG, 5, 2, gl, ga, 1, r0, a0, 1, missing) == -EINVAL);
    CHECK(unet_ctc_add_frame_host(c, 7, 5, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == -EINVAL);
    // frame sizes (t = 0 does no device work)
    CHECK(unet_ctc_add_frames(c, UNET_CTC_TRA, nullptr, nullptr, nullptr, 0, 37, 53, nullptr, nullptr) == 0);
    CHECK(unet_ctc_add_frames(c, UNET_CTC_TRA, nullptr, nullptr, nullptr, 0, 37, 54, nullptr, nullptr) == -EINVAL);
    CHECK(std::strstr(unet_last_error(), "sizes differ") != nullptr);
    CHECK(unet_ctc_add_frames(c, UNET_CTC_TRA, nullptr, nullptr, nullptr, 1, 37, 53, nullptr, nullptr) == -EINVAL);
    unet_ctc_destroy(c);
  }
  // workspace formula: grows with the pixels of one frame and the chunk, not with 65536^2
  CHECK(unet_ctc_ws_bytes(0, 8, 8) == 0 && unet_ctc_ws_bytes(1, 65536, 65536) == 0);
  const size_t w1 = unet_ctc_ws_bytes(1, 512, 512), w84 = unet_ctc_ws_bytes(84, 512, 512);
  CHECK(w1 > 0 && w1 % 256 == 0 && w84 > w1 && w84 < (64u << 20));
  CHECK(unet_ctc_ws_bytes(5000, 512, 512) == unet_ctc_ws_bytes(1024, 512, 512));
  // the table and record regions grow with the frames per chunk
  CHECK(unet_set_tuning("ctc_chunk_frames", 8) == 0 && unet_ctc_ws_bytes(84, 64, 64) < w84);
  const size_t s8 = unet_ctc_ws_bytes(84, 64, 64);
  CHECK(unet_set_tuning("ctc_chunk_frames", 64) == 0 && unet_ctc_ws_bytes(84, 64, 64) > s8);
  CHECK(unet_set_tuning("ctc_chunk_frames", 0) != 0 && unet_set_tuning("ctc_chunk_frames", -2) != 0);
  CHECK(unet_set_tuning("ctc_dense_cells", -2) != 0 && unet_set_tuning("ctc_dense_cells", 0) == 0);
  CHECK(unet_set_tuning("ctc_chunk_frames", -1) == 0 && unet_set_tuning("ctc_dense_cells", -1) == 0);  // defaults
  CHECK(unet_ctc_ws_bytes(84, 512, 512) == w84);
  unet_ctc_destroy(nullptr);
}

// the warping error's host side: the simple-point table and the argument checks
// (no launch: every call here is refused first)
static void test_warp() {
  uint8_t t[256];
  unet_simple_point_table(t);
  int ones = 0;
  for (int c = 0; c < 256; ++c) {
    CHECK(t[c] <= 1);
    ones += t[c];
  }
  CHECK(ones == 116);
  CHECK(t[0] == 0 && t[255] == 0);     // an isolated pixel, an interior pixel
  CHECK(t[1] == 1 && t[2] == 1);       // the end of a line, straight or diagonal
  CHECK(t[0x11] == 0);                 // N and S only: the pixel is a bridge
  CHECK(t[0x05] == 1 && t[0x07] == 1);  // N and E stay joined through their diagonal, with or without NE
  CHECK(t[0x55] == 0 && t[0xAA] == 0);  // the four edge neighbours, the four corners
  CHECK(unet_warping_error_ws_bytes(0, 4, 4) == 0 && unet_warping_error_ws_bytes(1, 0, 4) == 0 &&
        unet_warping_error_ws_bytes(1, 4, -1) == 0 && unet_warping_error_ws_bytes(1 << 16, 1 << 15, 1) == 0);
  const size_t one = unet_warping_error_ws_bytes(1, 512, 512);
  CHECK(one >= 4u * 514 * 18 * 4 && one % 256 == 0 && unet_warping_error_ws_bytes(3, 512, 512) >= 3 * (one - 255));
  uint16_t g[4] = {0, 1, 1, 0};
  uint8_t p[4] = {0, 1, 0, 0};
  int64_t c5[5];
  CHECK(unet_warping_error(g, p, 0, 2, 2, 4, 1, 0, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(g, p, 1, 2, 2, -2, 1, 0, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(g, p, 1, 2, 2, 256, 1, 0, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(g, p, 1, 2, 2, 4, 1, -1, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(g, p, 1 << 16, 1 << 15, 1, 4, 1, 0, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(nullptr, p, 1, 2, 2, 4, 1, 0, 0, nullptr, c5, nullptr, nullptr) == -EINVAL);
  CHECK(unet_warping_error(g, p, 1, 2, 2, 4, 1, 0, UNET_WARP_FORCE_WS, nullptr, c5, nullptr, nullptr) == -EINVAL);  // no workspace
  CHECK(std::strstr(unet_last_error(), "unet_warping_error") != nullptr);
  // marker-seeded instance masks: rejected before any launch
  CHECK(unet_split_instances_ws_bytes(0, 4, 4) == 0 && unet_split_instances_ws_bytes(1, 16385, 4) == 0 &&
        unet_split_instances_ws_bytes(1, 4, 16385) == 0 && unet_split_instances_ws_bytes(65536, 1, 1) == 0 &&
        unet_split_instances_ws_bytes(8, 16384, 16384) == 0);
  uint16_t lab[4];
  int32_t info[4];
  CHECK(unet_split_instances(p, nullptr, 0, 2, 2, 4, 1, lab, nullptr, info, nullptr, nullptr) == -EINVAL);
  CHECK(unet_split_instances(p, nullptr, 1, 2, 2, -1, 1, lab, nullptr, info, nullptr, nullptr) == -EINVAL);
  CHECK(unet_split_instances(p, nullptr, 1, 2, 2, (1 << 30) + 1, 1, lab, nullptr, info, nullptr, nullptr) == -EINVAL);
  CHECK(unet_split_instances(p, nullptr, 1, 2, 2, 4, -1, lab, nullptr, info, nullptr, nullptr) == -EINVAL);
  CHECK(unet_split_instances(p, nullptr, 1, 2, 2, 4, 1, lab, nullptr, info, nullptr, nullptr) == -EINVAL);  // no workspace
  CHECK(std::strstr(unet_last_error(), "unet_split_instances") != nullptr);
  CHECK(unet_set_tuning("split_threads", 96) == -EINVAL && unet_set_tuning("split_threads", 128) == 0 &&
        unet_set_tuning("split_threads", -1) == 0);
  // training tiles: rejected before any device call (the buffers are host memory)
  CHECK(unet_tile_warp_ws_bytes(0, 4, 4) == 0 && unet_tile_warp_ws_bytes(2, 0, 4) == 0 &&
        unet_tile_warp_ws_bytes(2, 4, -1) == 0 && unet_tile_warp_ws_bytes(3, 7, 5) == unet_elastic_ws_bytes(3, 7, 5));
  alignas(8) double prm[8] = {1, 0, 0, 0, 1, 0, 1, 0};
  alignas(8) double wsb[64];
  const int32_t fi[1] = {0};
  float xo[4], wo[4];
  uint8_t to[4];
  const double* nz = wsb;
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 2, 2, 2, nullptr, 0, 1, xo, to, nullptr, nullptr, nullptr, nullptr, nullptr) == -EINVAL);   // extend
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 2, 2, 1, nullptr, 0, 1, xo, to, nullptr, nullptr, wo, nullptr, nullptr) == -EINVAL);        // weight_out, no weights
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 0, 2, 1, nullptr, 0, 1, xo, to, nullptr, nullptr, nullptr, nullptr, nullptr) == -EINVAL);   // th
  CHECK(unet_tile_warp(p, lab, nullptr, 0, 2, 2, fi, prm, 1, 2, 2, 1, nullptr, 0, 1, xo, to, nullptr, nullptr, nullptr, nullptr, nullptr) == -EINVAL);   // nframes
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, nullptr, prm, 1, 2, 2, 1, nullptr, 0, 1, xo, to, nullptr, nullptr, nullptr, nullptr, nullptr) == -EINVAL);
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 2, 2, 0, nz, 10, 0.0, xo, to, nullptr, nullptr, nullptr, wsb, nullptr) == -EINVAL);         // sigma
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 2, 2, 0, nz, 10, 40.0, xo, to, nullptr, nullptr, nullptr, wsb, nullptr) == -EINVAL);        // radius 160: LDS rows
  CHECK(unet_tile_warp(p, lab, nullptr, 1, 2, 2, fi, prm, 1, 2, 2, 0, nz, 10, 2.0, xo, to, nullptr, nullptr, nullptr, nullptr, nullptr) == -EINVAL);     // no workspace
  CHECK(std::strstr(unet_last_error(), "unet_tile_warp") != nullptr);
  // sequence inference: rejected before any device call (the buffers are host memory)
  const int32_t wk[2] = {0, 0}, c01[2] = {0, 1}, c08[2] = {0, 8}, cneg[1] = {-1}, c9[9] = {0, 1, 2, 3, 4, 5, 6, 7, 0};
  float tl[16], pr[16];
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 1, 2, 0, 0, 1, wk, 1, c01, 2, tl, nullptr) == -EINVAL);   // tile_in < tile_out
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, wk, 1, c08, 2, tl, nullptr) == -EINVAL);   // code 8
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, wk, 1, cneg, 1, tl, nullptr) == -EINVAL);  // code -1
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, wk, 1, c01, 0, tl, nullptr) == -EINVAL);   // ns 0
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, wk, 1, c9, 9, tl, nullptr) == -EINVAL);    // ns 9
  CHECK(unet_seq_tile_gather(p, 1, 0, 1, 2, 2, 2, 1, 0, 0, 1, wk, 1, c01, 2, tl, nullptr) == -EINVAL);   // nframes
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, wk, 0, c01, 2, tl, nullptr) == -EINVAL);   // ngroups
  CHECK(unet_seq_tile_gather(p, 1, 1, 1, 2, 2, 2, 1, 0, 0, 1, nullptr, 1, c01, 2, tl, nullptr) == -EINVAL);
  CHECK(unet_seq_tile_reduce(tl, 3, 2, 1, wk, 1, c01, 2, 1, 2, 2, 0.5f, pr, to, nullptr, nullptr) == -EINVAL);       // mask, k = 3
  CHECK(unet_seq_tile_reduce(tl, 2, 2, 1, wk, 1, c01, 2, 1, 2, 2, 0.5f, nullptr, nullptr, nullptr, nullptr) == -EINVAL);  // no output
  CHECK(unet_seq_tile_reduce(tl, 2, 2, 1, wk, 1, c01, 2, 1, 2, 2, 0.5f, nullptr, nullptr, pr, nullptr) == -EINVAL);  // logits, ns = 2
  CHECK(unet_seq_tile_reduce(tl, 2, 2, 1, wk, 1, c08, 2, 1, 2, 2, 0.5f, pr, nullptr, nullptr, nullptr) == -EINVAL);  // code 8
  CHECK(unet_seq_tile_reduce(tl, 2, 0, 1, wk, 1, c01, 2, 1, 2, 2, 0.5f, pr, nullptr, nullptr, nullptr) == -EINVAL);  // tile_out
  CHECK(unet_seq_tile_reduce(tl, 2, 2, 1, wk, 1, c01, 2, 1, 2, 0, 0.5f, pr, nullptr, nullptr, nullptr) == -EINVAL);  // w
}

static void test_misc() {
  CHECK(std::strlen(unet_version()) > 0);
  const size_t need = unet_tuning_report(nullptr, 0);
  std::vector<char> buf(need + 1);
  CHECK(unet_tuning_report(buf.data(), buf.size()) == need);
  CHECK(unet_tuning_reset() == 0);
  CHECK(unet_set_tuning("no_such_key", 1) != 0);
}

// ---------------------------------------------------------------------------
// GEMM variant selection.  One record per synthetic launch: the tuning key, the
// heuristic tile, every table tile's fits / workgroup count / slots, the ordered
// candidate list, and what the forced knobs resolve to.  The golden file holds
// each record's key and a 64-bit FNV-1a hash of the whole record; it was
// recorded before the tile tables replaced the per-id switches, so any differing
// line means the selection changed (the full record is then printed).  No GPU
// call is made (num_cus() is 256 without a device).
// ---------------------------------------------------------------------------
namespace unet {
extern int g_tune_igemm, g_tune_wgrad;
}
static float g_dummy[4];

static void appendf(std::string& o, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  o += b;
}

static unet::Src mk_src(int hw, int c, int h16, bool tf) {
  unet::Src s;
  s.ptr = g_dummy;
  s.H = s.W = hw;
  s.C = c;
  s.h16 = h16;
  if (tf) s.scale = s.shift = g_dummy;
  return s;
}

// kind 0: 3x3 stride 1, one source; 1: two sources (c_split = Cg / 2);
// 2: convT forward (1x1 taps, pixel shuffle); 3: convT input gradient (2x2 stride 2)
static unet::IgemmArgs mk_igemm(int kind, int Cg, int N, int hw, int nimg, int h16, bool tf, int fwd, int prec) {
  using namespace unet;
  IgemmArgs a;
  Gather& g = a.a;
  g.Cg = Cg;
  g.c_split = kind == 1 ? Cg / 2 : Cg;
  g.Hg = g.Wg = hw;
  g.nimg = nimg;
  if (kind <= 1) {
    g.taps_h = g.taps_w = 3;
    const int cs = kind == 1 ? Cg / 2 : Cg;
    g.s[0] = mk_src(hw + 2, cs, h16, tf);
    g.s[1] = kind == 1 ? mk_src(hw + 2, cs, h16, false) : g.s[0];
  } else if (kind == 2) {
    g.s[0] = g.s[1] = mk_src(hw, Cg, h16, tf);
    a.e.shuffle_co = N / 4;
  } else {
    g.taps_h = g.taps_w = 2;
    g.stride = 2;
    g.s[0] = g.s[1] = mk_src(2 * hw, Cg, h16, false);
  }
  a.M = nimg * hw * hw;
  a.N = N;
  a.K = g.taps_h * g.taps_w * Cg;
  static uint16_t w16[4];
  if (prec == 0) a.b = g_dummy;
  else a.bh = w16;
  if (prec == 2) a.bl = w16;
  a.e.d[0] = Dst{g_dummy, kind == 2 ? 2 * hw : hw, kind == 2 ? 2 * hw : hw, kind == 2 ? N / 4 : N, 0, 0, 0};
  a.fwd = kind <= 1 ? fwd : 0;
  static double st[4];
  if (a.fwd) a.e.stats = st;
  a.slab = g_dummy;
  if (prec == 0) {
    a.wino_ws = g_dummy;
    a.wino_ws_bytes = (size_t)1 << 31;
  }
  return a;
}

// kind 0 / 1: 3x3 weight gradient (one / two X sources); 2: convT weight gradient
static unet::WgradArgs mk_wgrad(int kind, int Co, int Ci, int hw, int nimg, int h16, bool tf, int prec, bool slab,
                                int accumulate, int batch) {
  using namespace unet;
  WgradArgs a{};
  Gather& ga = a.ga;
  Gather& gb = a.gb;
  ga.Hg = ga.Wg = gb.Hg = gb.Wg = hw;
  ga.nimg = gb.nimg = nimg;
  if (kind <= 1) {  // ga: padded dY (pad 2), gb: X with 3x3 taps
    ga.Cg = ga.c_split = Co;
    ga.s[0] = ga.s[1] = mk_src(hw + 4, Co, h16, false);
    ga.s[0].oy = ga.s[0].ox = ga.s[1].oy = ga.s[1].ox = 2;
    gb.Cg = Ci;
    gb.c_split = kind == 1 ? Ci / 2 : Ci;
    gb.taps_h = gb.taps_w = 3;
    const int cs = kind == 1 ? Ci / 2 : Ci;
    gb.s[0] = mk_src(hw + 2, cs, h16, tf);
    gb.s[1] = kind == 1 ? mk_src(hw + 2, cs, h16, false) : gb.s[0];
    a.Mo = Co;
    a.No = 9 * Ci;
  } else {  // ga: the convT input X (Mo = its channels), gb: dY on the 2x grid, 2x2 stride 2
    ga.Cg = ga.c_split = Co;
    ga.s[0] = ga.s[1] = mk_src(hw, Co, h16, tf);
    gb.Cg = gb.c_split = Ci;
    gb.taps_h = gb.taps_w = 2;
    gb.stride = 2;
    gb.s[0] = gb.s[1] = mk_src(2 * hw, Ci, h16, false);
    a.Mo = Co;
    a.No = 4 * Ci;
  }
  a.P = nimg * hw * hw;
  a.pix_per_split = 0;
  a.out = g_dummy;
  a.bf16 = prec != 0;
  a.split = prec == 2;
  if (slab) {
    a.slab = g_dummy;
    a.slab_bytes = (size_t)256 << 20;
  }
  a.accumulate = accumulate;
  a.batch = batch;
  if (batch > 1) {
    a.batch_a = (long long)a.P * Co;
    a.batch_b = (long long)a.P * Ci;
    a.batch_out = (long long)a.Mo * a.No;
  }
  if (prec == 0) {
    a.wino_ws = g_dummy;
    a.wino_ws_bytes = (size_t)1 << 31;
  }
  return a;
}

static std::string selection_dump() {
  using namespace unet;
  std::string o;
  const int chans[] = {64, 128, 256, 512, 1024}, grids[] = {4, 10, 30, 104};
  const size_t slab_bytes = (size_t)256 << 20;
  int idx = 0;
  for (int kind = 0; kind < 4; ++kind)
    for (int Cg : chans)
      for (int N : chans)
        for (int prec = 0; prec < 3; ++prec, ++idx) {
          // the remaining options cycle so that every value meets every kind and precision
          const int hw = grids[idx % 4], nimg = (idx / 4) % 2 ? 8 : 1, h16 = prec == 1 ? (idx / 8) % 4 != 0 : 0;
          const bool tf = (idx / 3) % 2 != 0;
          const int fwd = (idx / 5) % 2;
          const IgemmArgs a = mk_igemm(kind, Cg, N, hw, nimg, h16, tf, fwd, prec);
          appendf(o, "%s | kind %d h16 %d tf %d fwd %d n %d | heur %d |", igemm_key(a).c_str(), kind, h16, (int)tf, fwd,
                  nimg, igemm_heuristic_tile(a));
          for (const IgemmTile& t : igemm_tiles())
            if (igemm_tile_fits(a, t.id))
              appendf(o, " %d:%lld/%d", t.id, igemm_tile_count(a, t.id), igemm_tile_slots(t.id));
          o += " | cand";
          for (const GemmChoice& c : igemm_candidates(a, slab_bytes)) appendf(o, " %d:%d", c.tile, c.split);
          // forced igemm_variant: the tile the heuristic launch runs and its flops, where they differ
          const double base = igemm_exec_flops(a, GemmChoice{});
          o += " | forced";
          for (const IgemmTile& t : igemm_tiles()) {
            g_tune_igemm = t.id;
            const int h = igemm_heuristic_tile(a);
            const double f = igemm_exec_flops(a, GemmChoice{});
            if (h == t.id) appendf(o, f != base ? " %d:%.6g" : " %d", t.id, f);
          }
          g_tune_igemm = -1;
          o += " | flops";
          for (int t : {4, 21, 70, 71, 72, 73, 74, 75, 76, 77}) appendf(o, " %.6g", igemm_exec_flops(a, GemmChoice{t, 1}));
          o += "\n";
        }
  const int knobs[] = {-1,  1,   2,   8,   10,  11,  12,  13,  14,  20,  21,  22,  23,  24,  25,  26,  27,  28,
                       29,  30,  31,  32,  33,  40,  41,  42,  43,  44,  71,  74,  100, 101, 102, 103, 104, 110,
                       111, 112, 113, 114, 126, 127, 128, 129, 130, 131, 132, 133, 140, 141, 142, 143, 144, 1071, 1074};
  idx = 0;
  for (int kind = 0; kind < 3; ++kind)
    for (int Co : chans)
      for (int Ci : chans)
        for (int prec = 0; prec < 3; ++prec, ++idx) {
          const int hw = grids[idx % 4], nimg = (idx / 4) % 2 ? 8 : 1, h16 = prec == 1 ? (idx / 8) % 4 != 0 : 0;
          const bool tf = (idx / 3) % 2 != 0, slab = (idx / 2) % 3 != 0;
          const int accumulate = (idx / 7) % 4 == 0, batch = (idx / 11) % 5 == 0 ? 16 : 1;
          const WgradArgs a = mk_wgrad(kind, Co, Ci, hw, nimg, h16, tf, prec, slab, accumulate, batch);
          for (int det = 0; det < 2; ++det) {
            g_deterministic = det;
            appendf(o, "%s | kind %d h16 %d tf %d slab %d acc %d batch %d n %d | fits", wgrad_key(a).c_str(), kind, h16,
                    (int)tf, (int)slab, accumulate, batch, nimg);
            for (const WgradTile& t : wgrad_tiles())
              if (wgrad_tile_fits(a, t.id)) appendf(o, " %d", t.id);
            o += " | cand";
            for (const GemmChoice& c : wgrad_candidates(a))
              appendf(o, " %d:%d%s", c.tile, c.split, wgrad_choice_deterministic(c) ? "d" : "");
            if (det) {  // the knobs do not depend on the mode
              o += "\n";
              continue;
            }
            o += " | knob";  // wgrad_variant values that force something, and what
            for (int k : knobs) {
              g_tune_wgrad = k;
              const GemmChoice r = resolve_forced_wgrad(a, k);
              if (r.tile >= 0)
                appendf(o, " %d:%d/%d,%d,%.6g", k, r.tile, r.split, wgrad_winograd_mt(a, GemmChoice{}),
                        wgrad_exec_flops(a, GemmChoice{}));
            }
            g_tune_wgrad = -1;
            appendf(o, " | mt %d %d flops %.6g %.6g", wgrad_winograd_mt(a, GemmChoice{71, 1}),
                    wgrad_winograd_mt(a, GemmChoice{74, 1001}), wgrad_exec_flops(a, GemmChoice{71, 1}),
                    wgrad_exec_flops(a, GemmChoice{0, 8}));
            o += " || ";  // one record for both modes
          }
          g_deterministic = 0;
        }
  return o;
}

// argv[1]: the golden file; argv[2] == "--record": write it instead of comparing
static void test_selection(const char* golden, bool record) {
  const std::string full = selection_dump();
  std::string got;  // per record: its key and the hash of all of it
  for (size_t i = 0; i < full.size();) {
    const size_t e = full.find('\n', i);
    unsigned long long h = 1469598103934665603ull;
    for (size_t k = i; k < e; ++k) h = (h ^ (unsigned char)full[k]) * 1099511628211ull;
    got.append(full, i, full.find(" | ", i) - i);
    appendf(got, " #%016llx\n", h);
    i = e + 1;
  }
  if (record) {
    FILE* f = std::fopen(golden, "w");
    CHECK(f != nullptr);
    if (f) {
      std::fwrite(got.data(), 1, got.size(), f);
      std::fclose(f);
    }
    return;
  }
  FILE* f = std::fopen(golden, "r");
  CHECK(f != nullptr);
  if (!f) return;
  std::string want;
  char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) want.append(buf, n);
  std::fclose(f);
  size_t i = 0, j = 0;
  int line = 1, bad = 0;
  while (i < got.size() || j < want.size()) {
    const size_t ie = std::min(got.find('\n', i), got.size()), je = std::min(want.find('\n', j), want.size());
    if (got.compare(i, ie - i, want, j, je - j) != 0 && ++bad <= 5) {
      size_t f = 0;  // the full record of this line
      for (int l = 1; l < line && f != std::string::npos; ++l) f = full.find('\n', f) + 1;
      std::fprintf(stderr, "gemm selection line %d differs:\n  got  %s\n  want %s\n  record %s\n", line,
                   got.substr(i, ie - i).c_str(), want.substr(j, je - j).c_str(),
                   f < full.size() ? full.substr(f, full.find('\n', f) - f).c_str() : "");
    }
    i = std::min(ie + 1, got.size());
    j = std::min(je + 1, want.size());
    ++line;
  }
  CHECK(bad == 0);
}

// unet_gemm_site_*: the descriptor's validation, the strict knob and the tile
// table's export (host only: nothing is launched, no pointer is read)
static void test_gemm_site() {
  float* const p = reinterpret_cast<float*>(uintptr_t{4096});
  double* const q = reinterpret_cast<double*>(uintptr_t{4096});
  auto base = [&](int site) {
    unet_gemm_site d{};
    d.site = site;
    d.n = 2, d.h = 13, d.w = 19, d.ci = 128, d.co = 128;
    d.tile = 0, d.split = 1;
    d.src0 = d.wt = d.bias = d.scale0 = d.shift0 = p;
    d.dst0 = p;
    d.stats = q;
    return d;
  };
  unet_gemm_site d = base(UNET_SITE_F_PLAIN);
  int tile = 0;
  CHECK(unet_gemm_site_check(&d, &tile) == 0 && tile > 0);
  const size_t ws1 = unet_gemm_site_ws_bytes(&d);
  CHECK(ws1 >= 2 * sizeof(float) * 9 * 128 * 128 && ws1 % 256 == 0);
  d.tile = 1, d.split = 3;  // the slab of an explicit K split lives in ws
  CHECK(unet_gemm_site_check(&d, &tile) == 0 && tile == 1);
  CHECK(unet_gemm_site_ws_bytes(&d) == ws1 + sizeof(float) * 3 * (2 * 13 * 19) * 128);
  d = base(UNET_SITE_F_PLAIN);
  d.ci = 124;
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL && unet_gemm_site_ws_bytes(&d) == 0);
  CHECK(std::strstr(unet_last_error(), "unet_gemm_site") != nullptr);
  d = base(UNET_SITE_F_PLAIN);
  d.co = 100;
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  d = base(UNET_SITE_F_PLAIN);
  d.stats = nullptr;
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  CHECK(unet_gemm_site_run(&d, p, nullptr) == -EINVAL);  // before anything is launched
  d = base(UNET_SITE_F_PLAIN);
  CHECK(unet_gemm_site_run(&d, nullptr, nullptr) == -EINVAL);
  CHECK(unet_gemm_site_run(&d, reinterpret_cast<void*>(uintptr_t{4100}), nullptr) == -EINVAL);  // ws alignment
  d = base(UNET_SITE_D_SPLIT);
  d.ci = 192, d.scale0 = d.shift0 = nullptr, d.dst1 = p, d.colsum1 = q;
  d.n_split = 48;
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  d.n_split = 64;
  CHECK(unet_gemm_site_check(&d, &tile) == 0);
  d.colsum1 = nullptr;
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  d = base(UNET_SITE_F_CAT);
  d.src1 = p, d.c_split = 64, d.skip_h = 20, d.skip_w = 25, d.oy = 2, d.ox = 3;
  CHECK(unet_gemm_site_check(&d, nullptr) == 0);
  d.ox = 5;  // the window leaves the stored grid
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  CHECK(unet_gemm_site_check(nullptr, nullptr) == -EINVAL);
  // strict forcing: a 3x3 halo tile at a convT site
  d = base(UNET_SITE_T_FWD);
  d.co = 64, d.scale0 = d.shift0 = nullptr, d.tile = 52;
  CHECK(unet_gemm_site_check(&d, &tile) == 0 && tile != 52);  // default: the built-in tile in its place
  CHECK(unet_set_tuning("op_strict", 1) == 0);
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  d.tile = 4;
  CHECK(unet_gemm_site_check(&d, &tile) == 0 && tile == 4);
  d.split = 5;  // 8 chunks of K do not make 5 slices
  CHECK(unet_gemm_site_check(&d, nullptr) == -EINVAL);
  CHECK(unet_set_tuning("op_strict", 0) == 0);
  // the tile table's export agrees with the table
  const int n = unet_igemm_tile_table(nullptr, 0);
  CHECK(n == (int)unet::igemm_tiles().size() && n > 60);
  std::vector<int> rows(6 * (size_t)n, -1);
  CHECK(unet_igemm_tile_table(rows.data(), n) == n);
  for (int i = 0; i < n; ++i) {
    const unet::IgemmTile* t = unet::igemm_tile(rows[6 * i]);
    CHECK(t != nullptr && (int)t->family == rows[6 * i + 1] && t->bf16 == (rows[6 * i + 2] != 0) &&
          t->x3 == (rows[6 * i + 3] != 0) && t->ksplit == (rows[6 * i + 4] != 0) && t->wino_m == rows[6 * i + 5]);
  }
}

// unet_region_props_host: exactly sized host buffers (the sanitizer sees any
// access beside them), closed forms of two touching rectangles, -ENOSPC and
// the argument checks
static void test_region() {
  const int n = 2, h = 6, w = 7;
  std::vector<uint16_t> lab((size_t)n * h * w, 0);
  std::vector<uint8_t> img(lab.size());
  for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)(i * 37 + 11);
  auto at = [&](int f, int y, int x) -> uint16_t& { return lab[((size_t)f * h + y) * w + x]; };
  for (int y = 0; y < 3; ++y)
    for (int x = 1; x < 6; ++x) at(0, y, x) = x < 3 ? 65535 : 7;  // 3 x 2 beside 3 x 3, sharing a side of 3
  at(1, 5, 6) = 1;                                                 // one pixel in the last corner
  std::vector<int32_t> off(n + 1, -1);
  long long total = -1;
  std::vector<unet_region_record> rec(3);
  CHECK(unet_region_props_host(lab.data(), img.data(), n, h, w, off.data(), rec.data(), 2, &total) == -ENOSPC);
  CHECK(total == 3 && off[0] == 0 && off[1] == 2 && off[2] == 3);
  CHECK(unet_region_props_host(lab.data(), img.data(), n, h, w, off.data(), rec.data(), 3, &total) == 0);
  CHECK(total == 3 && rec[0].label == 7 && rec[1].label == 65535 && rec[2].label == 1);
  CHECK(rec[0].frame == 0 && rec[0].area == 9 && rec[0].contact == 3 && rec[1].contact == 3 && rec[1].area == 6);
  CHECK(rec[0].min_y == 0 && rec[0].max_y == 2 && rec[0].min_x == 3 && rec[0].max_x == 5);
  CHECK(rec[0].sum_y == 9 && rec[0].sum_x == 36 && rec[0].sum_yy == 15 && rec[0].sum_xx == 150 && rec[0].sum_xy == 36);
  CHECK(rec[0].edge == 3 && rec[0].boundary == 8 && rec[1].boundary == 6);
  long long sv = 0, svv = 0;
  int lo = 255, hi = 0;
  for (int y = 0; y < 3; ++y)
    for (int x = 3; x < 6; ++x) {
      const int v = img[(size_t)y * w + x];
      sv += v, svv += v * v, lo = std::min(lo, v), hi = std::max(hi, v);
    }
  CHECK(rec[0].sum_v == sv && rec[0].sum_vv == svv && rec[0].min_v == lo && rec[0].max_v == hi);
  CHECK(rec[2].frame == 1 && rec[2].area == 1 && rec[2].edge == 1 && rec[2].boundary == 1 && rec[2].contact == 0 &&
        rec[2].min_y == 5 && rec[2].max_x == 6 && rec[2].sum_xy == 30);
  CHECK(unet_region_props_host(lab.data(), nullptr, n, h, w, off.data(), rec.data(), 3, &total) == 0);
  CHECK(rec[0].sum_v == 0 && rec[0].min_v == 0 && rec[0].max_v == 0 && rec[0].area == 9);
  CHECK(unet_region_props_host(lab.data(), nullptr, 0, h, w, off.data(), nullptr, 0, &total) == 0 && total == 0 &&
        off[0] == 0);
  total = -1;
  CHECK(unet_region_props_host(lab.data(), nullptr, 1, 32769, 1, off.data(), rec.data(), 3, &total) == -EINVAL);
  CHECK(total == 0 && std::strstr(unet_last_error(), "32768") != nullptr);
  CHECK(unet_region_props_host(lab.data(), nullptr, 1, 32768, 32769, off.data(), rec.data(), 3, &total) == -EINVAL);
  CHECK(unet_region_props_host(lab.data(), nullptr, -1, h, w, off.data(), rec.data(), 3, &total) == -EINVAL);
  CHECK(unet_region_props_host(nullptr, nullptr, n, h, w, off.data(), rec.data(), 3, &total) == -EINVAL);
  // the device entry point rejects the same sizes before it touches the device
  void* dummy = reinterpret_cast<void*>(uintptr_t{4096});
  CHECK(unet_region_props(lab.data(), nullptr, 1, 1, 32769, off.data(), rec.data(), 3, &total, dummy, nullptr) == -EINVAL);
  CHECK(unet_region_props(lab.data(), nullptr, -1, h, w, off.data(), rec.data(), 3, &total, dummy, nullptr) == -EINVAL);
  CHECK(unet_region_props(lab.data(), nullptr, n, h, w, off.data(), rec.data(), 3, nullptr, dummy, nullptr) == -EINVAL);
  CHECK(unet_region_props_ws_bytes(1, 32769, 1) == 0 && unet_region_props_ws_bytes(3, 5, 7) == 2 * 3 * 8192 + 256);
  CHECK(unet_set_tuning("region_lds_objects", -2) == -EINVAL && unet_set_tuning("region_lds_objects", 2) == 0 &&
        unet_set_tuning("region_lds_objects", -1) == 0);
  CHECK(unet_region_props_launches(1) >= 0 && unet_region_props_launches(0) == 0);
}

// unet_link_frames_host / unet_link_assemble / unet_tracker_load_result on
// exactly sized host buffers: a tie (two predecessors equidistant from one
// successor), the gate's boundary, empty frames, a division, and the argument
// checks.  Records with area 16 and sum = q have the quantised centroid q.
static unet_region_record link_rec(int frame, int label, int qy, int qx, int area = 16) {
  unet_region_record r;
  std::memset(&r, 0, sizeof r);
  r.frame = frame, r.label = label, r.area = area;
  r.sum_y = (int64_t)qy * area / 16, r.sum_x = (int64_t)qx * area / 16;
  return r;
}

static void test_link() {
  {  // the tie: row 1's search reaches row 0's private column first (lowest index), so row 0 gives way
    std::vector<unet_region_record> rec = {link_rec(0, 1, 80, 32), link_rec(0, 2, 80, 128), link_rec(1, 1, 80, 80)};
    const int32_t off[3] = {0, 2, 3};
    std::vector<int32_t> prev(3, 9), mother(3, 9);
    std::vector<int64_t> dist(3, 9), total(1, 9);
    CHECK(unet_link_frames_host(rec.data(), off, 2, 3, 160, 0, prev.data(), dist.data(), mother.data(),
                                total.data()) == 0);
    CHECK(prev[0] == -1 && prev[1] == -1 && prev[2] == 1 && dist[2] == 48 * 48 && mother[2] == -1);
    CHECK(total[0] == 48 * 48 + 160 * 160);
    // on the gate and one past it
    rec = {link_rec(0, 1, 0, 0), link_rec(1, 1, 0, 47)};
    const int32_t off2[3] = {0, 1, 2};
    CHECK(unet_link_frames_host(rec.data(), off2, 2, 2, 47, 0, prev.data(), dist.data(), mother.data(),
                                total.data()) == 0 && prev[1] == 0 && dist[1] == 47 * 47 && total[0] == 47 * 47);
    rec[1] = link_rec(1, 1, 1, 47);
    CHECK(unet_link_frames_host(rec.data(), off2, 2, 2, 47, 0, prev.data(), dist.data(), mother.data(),
                                total.data()) == 0 && prev[1] == -1 && dist[1] == -1 && total[0] == 47 * 47);
    CHECK(unet_link_frames_host(rec.data(), off2, 2, 2, 0, 0, prev.data(), dist.data(), mother.data(),
                                total.data()) == -EINVAL);
    CHECK(unet_link_frames_host(rec.data(), off2, 2, 2, 47, 65536, prev.data(), dist.data(), mother.data(),
                                total.data()) == -EINVAL);
    CHECK(unet_link_frames_host(nullptr, off2, 2, 2, 47, 0, prev.data(), dist.data(), mother.data(),
                                total.data()) == -EINVAL);
    // the device entry point rejects the same before it touches the device
    void* dummy = reinterpret_cast<void*>(uintptr_t{4096});
    CHECK(unet_link_frames(rec.data(), off2, -1, 2, 47, 0, prev.data(), dist.data(), mother.data(), total.data(), dummy,
                           nullptr) == -EINVAL);
    CHECK(unet_link_frames(rec.data(), off2, 2, 2, 47, 0, prev.data(), dist.data(), mother.data(), total.data(),
                           nullptr, nullptr) == -EINVAL);
    CHECK(unet_link_frames(rec.data(), off2, 2, 2, 65536, 0, prev.data(), dist.data(), mother.data(), total.data(),
                           dummy, nullptr) == -EINVAL);
    CHECK(unet_link_frames(nullptr, nullptr, 0, 0, 47, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(unet_link_ws_bytes(1, 5) == 0 && unet_link_ws_bytes(2, 0) == 0 && unet_link_ws_bytes(2, 5) == 9 * 256);
    CHECK(unet_set_tuning("link_lds_objects", -2) == -EINVAL && unet_set_tuning("link_lds_objects", 0) == 0 &&
          unet_set_tuning("link_lds_objects", -1) == 0);
    CHECK(unet_link_launches(1) >= 0 && unet_link_launches(0) == 0);
  }
  {  // empty frames around two objects; no frame at all
    std::vector<unet_region_record> rec = {link_rec(1, 3, 0, 0), link_rec(1, 9, 0, 16), link_rec(3, 5, 0, 0)};
    const int32_t off[5] = {0, 0, 2, 2, 3}, frames[4] = {2, 4, 6, 8};
    std::vector<int32_t> prev(3, 9), mother(3, 9), rows(12, 9), ids(3, 9);
    std::vector<int64_t> dist(3, 9), total(3, 9);
    CHECK(unet_link_frames_host(rec.data(), off, 4, 3, 320, 320, prev.data(), dist.data(), mother.data(),
                                total.data()) == 0);
    CHECK(prev[0] == -1 && prev[1] == -1 && prev[2] == -1 && mother[2] == -1);
    CHECK(total[0] == 0 && total[1] == 2 * 320 * 320 && total[2] == 0);
    CHECK(unet_link_assemble(rec.data(), off, 4, frames, prev.data(), dist.data(), mother.data(), 0.5, 2, rows.data(),
                             3, ids.data()) == 3);
    CHECK(rows[0] == 1 && rows[1] == 4 && rows[2] == 4 && rows[3] == -1 && rows[8] == 3 && rows[9] == 8);
    CHECK(ids[0] == 1 && ids[1] == 2 && ids[2] == 3);
    CHECK(unet_link_frames_host(nullptr, nullptr, 0, 0, 16, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(unet_link_assemble(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0.5, 2, nullptr, 0, nullptr) == 0);
    const int32_t same[4] = {2, 4, 4, 8};
    CHECK(unet_link_assemble(rec.data(), off, 4, same, prev.data(), dist.data(), mother.data(), 0.5, 2, rows.data(), 3,
                             ids.data()) == -EINVAL);
  }
  {  // a division: the mother's successor and the nearest claimant that passes the area ratio become daughters
    std::vector<unet_region_record> rec = {link_rec(0, 1, 160, 160, 32), link_rec(1, 1, 160, 176),
                                           link_rec(1, 2, 192, 160, 4), link_rec(1, 3, 160, 112)};
    const int32_t off[3] = {0, 1, 4}, frames[2] = {3, 5};
    std::vector<int32_t> prev(4, 9), mother(4, 9), rows(16, 9), ids(4, 9);
    std::vector<int64_t> dist(4, 9), total(1, 9);
    CHECK(unet_link_frames_host(rec.data(), off, 2, 4, 24, 96, prev.data(), dist.data(), mother.data(),
                                total.data()) == 0);
    CHECK(prev[1] == 0 && prev[2] == -1 && prev[3] == -1 && mother[1] == -1 && mother[2] == 0 && mother[3] == 0);
    CHECK(unet_link_assemble(rec.data(), off, 2, frames, prev.data(), dist.data(), mother.data(), 0.5, 2, rows.data(),
                             4, ids.data()) == 4);
    CHECK(rows[0] == 1 && rows[1] == 3 && rows[2] == 3 && rows[3] == -1);   // the mother ends in frame 3
    CHECK(ids[1] == 2 && rows[7] == 1 && ids[2] == 3 && rows[11] == -1 && ids[3] == 4 && rows[15] == 1);
    // rows_cap below the count: the count still comes back, nothing is written past the cap
    std::vector<int32_t> two(8, 9);
    CHECK(unet_link_assemble(rec.data(), off, 2, frames, prev.data(), dist.data(), mother.data(), 0.5, 2, two.data(), 2,
                             ids.data()) == 4 && two[4] == 2);
    unet_tracker* t = unet_tracker_create(8, 8, 0.3, 0.1, 2);
    const int32_t labels[4] = {1, 1, 2, 3};
    const int32_t bad_frames[2] = {5, 3};
    CHECK(unet_tracker_load_result(t, rows.data(), 4, bad_frames, 2, off, labels, ids.data()) == -EINVAL);
    CHECK(unet_tracker_num_frames(t) == 0 && unet_tracker_num_tracks(t) == 0);
    CHECK(unet_tracker_load_result(t, rows.data(), 4, frames, 2, off, labels, ids.data()) == 0);
    CHECK(unet_tracker_num_frames(t) == 2 && unet_tracker_num_tracks(t) == 4);
    std::vector<int32_t> back(16, 9), lab(3), got(3);
    int32_t fr = -1;
    CHECK(unet_tracker_tracks(t, back.data(), 4) == 4 && back == rows);
    CHECK(unet_tracker_frame_map(t, 1, &fr, lab.data(), got.data(), 3) == 3 && fr == 5 && lab[2] == 3 && got[2] == 4);
    CHECK(unet_tracker_load_result(t, rows.data(), 4, frames, 2, off, labels, ids.data()) == -EBUSY);
    unet_tracker_destroy(t);
    t = unet_tracker_create(8, 8, 0.3, 0.1, 2);
    CHECK(unet_tracker_load_result(t, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    unet_tracker_destroy(t);
  }
}

int main(int argc, char** argv) {
  test_plans();
  test_gemm_site();
  test_lsap();
  test_tracker();
  test_ctc();
  test_warp();
  test_region();
  test_link();
  test_misc();
  if (argc > 1) test_selection(argv[1], argc > 2 && std::strcmp(argv[2], "--record") == 0);
  else CHECK(!"usage: host_selftest tests/golden/gemm_selection.txt [--record]");
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("host_selftest: all checks passed\n");
  return 0;
}
