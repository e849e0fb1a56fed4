// k_igemm_plane: the batched point GEMMs of the unfused fp32 Winograd forward /
// input-gradient tiles, M[p] = U[p] V[p]^T (winograd.hip, launch_wino), on an
// LDS-DMA ring.
//
// It computes what k_igemm<BM, BN, 2, 2, BK> (igemm.hip) computes for that one
// call shape -- both operands contiguous K-major planes (U = [P T][Cg], V[p] =
// [N][Cg]), one tap, one source, no transform -- on the same grid, XCD order
// and epilogue, bit for bit: the same v_mfma_f32_32x32x2_f32 chain per output
// element (K-steps ascending; inside a step lane half h consumes k = h BK / 2 +
// s, s ascending).  Only the staging differs.  16 k of a tile row are one
// contiguous 64-B run of its plane, so the operands go global -> LDS by
// global_load_lds_dwordx4 from an SGPR base that a K-step bumps and per-lane
// offsets computed once: no K iterator, no 64-bit address arithmetic, no
// staging registers, no ds_write in the loop (on gfx950 the f32 MFMA and the
// VALU do not co-execute: each of those took an issue slot from the MFMAs).
//
// The ring holds NS sub-slots of 16 k each: [BM + BN rows][16] floats, rows
// unpadded, the 16-B chunk c of row r at chunk slot c ^ ((r >> 2) & 3) as in
// k_igemm_g (the source offset carries the permutation, the fragment read
// applies it), which puts the 16 lanes of every ds_read_b128 group on 16
// distinct bank quads.  A BK = 32 step is two consecutive sub-slots: lane half
// h reads all four chunks of sub-slot h, the same rows and swizzle, so the
// banking argument is the BK = 16 one.  NS is the deepest ring that keeps
// k_igemm's resident workgroups per CU for the tile.  Sub-steps past K are not
// issued: the waits count down over the last steps.
#include <atomic>
#include <cstdlib>

#include "gemm_common.h"
#include "ring_common.h"

namespace unet {

namespace {
// resident workgroups per CU of k_igemm for the tile (igemm.hip's tile table)
constexpr int plane_minw(int BM, int BN, int BK) {
  return BK == 32 ? 2 : (BM == 128 && BN == 128 ? 3 : 4);
}
// ring sub-slots: what 160 KB / plane_minw holds
constexpr int plane_ns(int BM, int BN, int BK) { return 163840 / plane_minw(BM, BN, BK) / ((BM + BN) * 64); }
}  // namespace

template <int BM, int BN, int BK>
__global__ __launch_bounds__(256, plane_minw(BM, BN, BK)) void k_igemm_plane(const IgemmArgs args) {
  constexpr int WM = 2, WN = 2, NW = WM * WN, NT = NW * 64;
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int G = BK / 16;                 // sub-slots per K-step
  constexpr int NS = plane_ns(BM, BN, BK);   // ring sub-slots
  constexpr int ASZ = BM * 64, SUB = (BM + BN) * 64;  // bytes: A part, sub-slot
  constexpr int PA = BM / (16 * NW), PB = BN / (16 * NW), D = PA + PB;  // 1-KiB DMAs per wave and sub-step
  constexpr int AHEAD = NS - 2 * G;  // sub-steps still in flight when a K-step starts
  constexpr int KH = BK / 2, KF = KH / 4;
  static_assert(TM >= 1 && TN >= 1 && PA >= 1 && PB >= 1 && (G == 1 || G == 2), "tile");
  static_assert(AHEAD >= 1 && D * AHEAD < 64 && NS * SUB <= 81920 && NS * SUB >= WM * 3 * BN * 4, "ring depth / vmcnt / LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[NS * SUB];
  const unsigned lds0 = (unsigned)(size_t)(lds_u8_t*)lds;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // in an SGPR: the DMAs' LDS addresses stay scalar
  const int wm = wave / WN, wn = wave % WN;
  int bx, by, bz;  // k_igemm's grid order
  xcd_block(bx, by, bz);
  const int m0 = bz * args.batch_rows + bx * BM, n0 = by * BN;
  const int M = (bz + 1) * args.batch_rows, K = args.K;
  const int S = K / 16, nk = K / BK;  // sub-steps, K-steps

  // ---- per-lane DMA pieces: lane = (row lane >> 2, chunk slot lane & 3) of a
  // 16-row piece; its 16 B come from chunk slot ^ ((row >> 2) & 3) of the row.
  // Rows past the batch entry's last row re-read it (k_igemm clamps m alike).
  const unsigned rowb = (unsigned)K * 4u;
  const int mlast = M - 1 - m0;  // >= 0: the grid has no empty row tile
  unsigned long long abase = uniform_u64(args.a.s[0].ptr + (size_t)m0 * K);
  unsigned long long bbase = uniform_u64(args.b + (size_t)bz * args.batch_b + (size_t)n0 * K);
  unsigned aoff[PA], boff[PB];
#pragma unroll
  for (int u = 0; u < PA; ++u) {
    const int r = (wave * PA + u) * 16 + (lane >> 2);
    aoff[u] = (unsigned)min(r, mlast) * rowb + (unsigned)(((lane & 3) ^ ((r >> 2) & 3)) * 16);
  }
#pragma unroll
  for (int u = 0; u < PB; ++u) {
    const int r = (wave * PB + u) * 16 + (lane >> 2);
    boff[u] = (unsigned)r * rowb + (unsigned)(((lane & 3) ^ ((r >> 2) & 3)) * 16);
  }
  // the next 16 k of both operands into sub-slot `slot` (wave-uniform)
  int issued = 0, islot = 0;
  auto issue = [&] {
    const unsigned dst = lds0 + (unsigned)islot * SUB;
#pragma unroll
    for (int u = 0; u < PA; ++u) dma_sv(aoff[u], abase, dst + (wave * PA + u) * 1024);
#pragma unroll
    for (int u = 0; u < PB; ++u) dma_sv(boff[u], bbase, dst + ASZ + (wave * PB + u) * 1024);
    abase += 64;
    bbase += 64;
    ++issued;
    islot = islot + 1 == NS ? 0 : islot + 1;
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5, li = lane & 31;
  const int sw = (li >> 2) & 3;  // chunk swizzle of this lane's fragment rows (row bases are multiples of 32)
  // one K-step from sub-slots cslot (.. cslot + G - 1)
  int cslot = 0;
  auto compute = [&] {
    int sub = cslot, c0 = 2 * h;  // BK = 16: chunks 2 h, 2 h + 1 of the one sub-slot
    if constexpr (G == 2) {       // BK = 32: all four chunks of sub-slot h
      const int nxt = cslot + 1 == NS ? 0 : cslot + 1;
      sub = h ? nxt : cslot;
      c0 = 0;
    }
    const float* As = reinterpret_cast<const float*>(lds + sub * SUB);
    const float* Bs = reinterpret_cast<const float*>(lds + sub * SUB + ASZ);
    float4 fa[TM][KF], fb[TN][KF];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float* pr = As + (wm * TM * 32 + i * 32 + li) * 16;
#pragma unroll
      for (int f = 0; f < KF; ++f) fa[i][f] = ld4(pr + (((c0 + f) ^ sw) << 2));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float* pr = Bs + (wn * TN * 32 + j * 32 + li) * 16;
#pragma unroll
      for (int f = 0; f < KF; ++f) fb[j][f] = ld4(pr + (((c0 + f) ^ sw) << 2));
    }
#pragma unroll
    for (int s = 0; s < KH; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(getc(fa[i][s >> 2], s & 3), getc(fb[j][s >> 2], s & 3),
                                                           acc[i][j], 0, 0, 0);
    cslot += G;
    if (cslot >= NS) cslot -= NS;
  };

  // prologue: sub-steps 0 .. NS - G - 1 (fewer when K is short)
#pragma unroll
  for (int t = 0; t < NS - G; ++t)
    if (t < S) issue();
  for (int kc = 0; kc < nk; ++kc) {
    // sub-steps up to kc G + NS - G - 1 (or S - 1) are issued: all but the
    // newest AHEAD have landed for this wave -- this K-step's among them; the
    // barrier publishes every wave's pieces
    if (S - (kc + 1) * G >= AHEAD) vm_wait<D * AHEAD>();
    else vm_wait<0>();
    raw_barrier();
    // the next G sub-steps into the sub-slots K-step kc - 1 left: every wave
    // passed the barrier after its last read of them
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (issued < S) issue();
    compute();
  }
  // every issued DMA was waited for by the last K-step (vm_wait<0>); the ring
  // now serves as the epilogue's reduction buffer
  __syncthreads();
  igemm_finish<BM, BN, WM, WN, NT>(args, acc, m0, n0, wm, wn, tid, reinterpret_cast<float*>(lds), LinearRows{m0, M},
                                   nullptr, bz);
}

// unet_set_tuning("igemm_plane", v) or UNET_IGEMM_PLANE (default on): 0 runs
// the batched point GEMMs on k_igemm (A/B and bit-identity tests)
int g_igemm_plane = getenv("UNET_IGEMM_PLANE") ? atoi(getenv("UNET_IGEMM_PLANE")) : 1;
std::atomic<long long> g_igemm_plane_launches{0};

static bool plane_tile(int bm, int bn, int bk) {
  return (bk == 16 && ((bm == 128 && bn == 128) || (bm == 64 && bn == 128) || (bm == 128 && bn == 64))) ||
         (bk == 32 && bn == 128 && (bm == 128 || bm == 64));
}

// The call shape k_igemm_plane serves: a batch of dense GEMMs whose A rows are
// one contiguous [batch * batch_rows][K] plane (the operands launch_wino
// builds) and whose output is a linear fp32 tensor
bool igemm_plane_applies(const IgemmArgs& a, int bm, int bn, int bk) {
  if (!g_igemm_plane || !plane_tile(bm, bn, bk) || a.batch <= 1 || a.ksplit != 1 || a.batch_rows < 1) return false;
  const Gather& g = a.a;
  const Src& s = g.s[0];
  if (g.taps_h != 1 || g.taps_w != 1 || g.stride != 1 || g.Hg != 1 || g.nimg != 1) return false;
  if (g.c_split != g.Cg || s.C != g.Cg || a.K != g.Cg || a.K % bk != 0 || a.N % bn != 0) return false;
  if (s.scale || s.h16 || a.bh || !a.b || !s.ptr) return false;
  const long long rows = (long long)a.batch * a.batch_rows;
  if (s.H != 1 || s.oy != 0 || s.ox != 0 || s.W != g.Wg || rows != g.Wg || rows != a.M) return false;
  const Epilogue& e = a.e;
  const Dst& d = e.d[0];
  if (e.shuffle_co || e.n_split < a.N || d.h16 || d.oy != 0 || d.ox != 0 || d.H != 1 || d.W != g.Wg) return false;
  if (((reinterpret_cast<size_t>(s.ptr) | reinterpret_cast<size_t>(a.b)) & 15) != 0 || (a.batch_b * 4) % 16 != 0)
    return false;
  // per-lane byte offsets: a tile's rows from its own base (no over-read: rows
  // are clamped, sub-steps past K not issued)
  return (long long)(bm > bn ? bm : bn) * a.K * 4 < (1ll << 32);
}

hipError_t launch_igemm_plane(const IgemmArgs& a, hipStream_t s, dim3 grid, int bm, int bn, int bk) {
  if (bm == 128 && bn == 128 && bk == 16) hipLaunchKernelGGL((k_igemm_plane<128, 128, 16>), grid, dim3(256), 0, s, a);
  else if (bm == 64 && bn == 128 && bk == 16) hipLaunchKernelGGL((k_igemm_plane<64, 128, 16>), grid, dim3(256), 0, s, a);
  else if (bm == 128 && bn == 64 && bk == 16) hipLaunchKernelGGL((k_igemm_plane<128, 64, 16>), grid, dim3(256), 0, s, a);
  else if (bm == 128 && bn == 128 && bk == 32) hipLaunchKernelGGL((k_igemm_plane<128, 128, 32>), grid, dim3(256), 0, s, a);
  else if (bm == 64 && bn == 128 && bk == 32) hipLaunchKernelGGL((k_igemm_plane<64, 128, 32>), grid, dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  ++g_igemm_plane_launches;
  return hipGetLastError();
}

}  // namespace unet
