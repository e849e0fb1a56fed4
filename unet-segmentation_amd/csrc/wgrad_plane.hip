// k_wgrad_plane: the batched point GEMMs of the fp32 Winograd weight gradients,
// Mw[p] = Vd[p]^T U[p] (winograd.hip, launch_wino_wgrad), on an LDS-DMA ring.
//
// It computes what k_wgrad<BM, BN, 2, 2> (igemm.hip) computes for that one call
// shape -- both operands contiguous [pixel][channel] planes, one tap, no
// transform -- on the same grid, pixel split, XCD order and output addressing,
// bit for bit: the same v_mfma_f32_32x32x2_f32 chain per output element (MFMA
// step s of a 16-pixel group consumes pixels s and 8 + s, groups ascending).
// Only the staging differs.  A pixel's BM (BN) channels are one contiguous
// 256-512-byte run of the plane, so a K-step's operands go global -> LDS by
// global_load_lds_dwordx4 in the layout k_wgrad's fragment reads use: no pixel
// iterator, no staging registers, no ds_write.  Four ring slots of one 16-pixel
// group each, three K-steps in flight, retired by counted vmcnt waits with one
// barrier per K-step (k_wgrad holds one K-step in registers: its waves wait out
// most of an HBM / L2 round trip per 16 pixels).
#include <cstdlib>

#include "gemm_common.h"
#include "ring_common.h"

namespace unet {

namespace {
constexpr int kPlaneBK = 16;  // pixels per K-step (one MFMA group)
constexpr int kPlaneNS = 4;   // ring slots

// workgroups per CU the LDS ring admits (= waves per SIMD: 4 waves per workgroup)
constexpr int plane_minw(int BM, int BN) {
  const int blocks = 163840 / (kPlaneNS * kPlaneBK * (BM + BN) * 4);
  return blocks > 4 ? 4 : blocks;
}
}  // namespace

template <int BM, int BN>
__global__ __launch_bounds__(256, plane_minw(BM, BN)) void k_wgrad_plane(const WgradArgs args) {
  constexpr int BK = kPlaneBK, NS = kPlaneNS, P = NS - 1;  // P K-steps in flight
  constexpr int WM = 2, WN = 2, NW = WM * WN;
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int ASZ = BK * BM * 4, BSZ = BK * BN * 4, SSZ = ASZ + BSZ;  // bytes per slot
  constexpr int DA = ASZ / 1024 / NW, DB = BSZ / 1024 / NW, D = DA + DB;  // DMAs per wave and K-step
  static_assert(TM >= 1 && TN >= 1 && DA >= 1 && DB >= 1 && ASZ % (1024 * NW) == 0 && BSZ % (1024 * NW) == 0, "tile");
  static_assert(NS >= 3 && D * (P - 1) < 64 && NS * SSZ <= 65536, "ring depth / vmcnt / LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[NS * SSZ];
  const unsigned lds0 = (unsigned)(size_t)(lds_u8_t*)lds;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  int bx, by, bz;  // k_wgrad's grid order
  xcd_block(bx, by, bz);
  const int i0 = bx * BM, j0 = by * BN;
  const int nz = gridDim.z / args.batch;  // pixel splits per batch entry
  const int zb = bz / nz;
  const int pbeg = (bz - zb * nz) * args.pix_per_split;
  const int pend = min(args.P, pbeg + args.pix_per_split);
  const int nk = (pend - pbeg + BK - 1) / BK;
  if (nk <= 0) return;

  // ---- per-lane DMA pieces: 16 B of pixel row (pbeg + row) of this K-step ----
  // A piece's byte offset in its plane is pixel * C * 4 + channel bytes; a
  // K-step adds BK * C * 4.  Rows past the plane's last pixel re-read it
  // (their values never reach an accumulator: see the tail below).
  const int Ca = args.ga.s[0].C, Cb = args.gb.s[0].C;
  const unsigned long long abase = uniform_u64(args.ga.s[0].ptr + (long long)zb * args.batch_a);
  const unsigned long long bbase = uniform_u64(args.gb.s[0].ptr + (long long)zb * args.batch_b);
  const unsigned alast = (unsigned)(args.P - 1) * (unsigned)(Ca * 4), blast = (unsigned)(args.P - 1) * (unsigned)(Cb * 4);
  unsigned apo[DA], acb[DA], bpo[DB], bcb[DB];
#pragma unroll
  for (int u = 0; u < DA; ++u) {
    const int b = (wave + NW * u) * 1024 + lane * 16;
    apo[u] = (unsigned)(pbeg + b / (BM * 4)) * (unsigned)(Ca * 4);
    acb[u] = (unsigned)(i0 * 4 + b % (BM * 4));
  }
#pragma unroll
  for (int u = 0; u < DB; ++u) {
    const int b = (wave + NW * u) * 1024 + lane * 16;
    bpo[u] = (unsigned)(pbeg + b / (BN * 4)) * (unsigned)(Cb * 4);
    bcb[u] = (unsigned)(j0 * 4 + b % (BN * 4));
  }
  // DMA u (A pieces, then B pieces) of the next K-step to issue, into `slot`
  auto issue1 = [&](int slot, int u) {
    if (u < DA) {
      dma_sv(min(apo[u], alast) + acb[u], abase, lds0 + slot * SSZ + (wave + NW * u) * 1024);
      apo[u] += (unsigned)(BK * Ca * 4);
    } else {
      const int k = u - DA;
      dma_sv(min(bpo[k], blast) + bcb[k], bbase, lds0 + slot * SSZ + ASZ + (wave + NW * k) * 1024);
      bpo[k] += (unsigned)(BK * Cb * 4);
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5, li = lane & 31;
  // prologue: K-steps 0 .. P-1.  Past the last K-step the ring keeps issuing
  // (clamped rows, into slots no MFMA reads any more), so every step retires D DMAs.
#pragma unroll
  for (int k = 0; k < P; ++k)
#pragma unroll
    for (int u = 0; u < D; ++u) issue1(k, u);

  // one K-step from ring slot kc % NS.  TAIL: the split's last, ragged group --
  // pixels >= pend are 0 in BOTH operands, as k_wgrad stages them.
  auto group = [&](auto tailc, int kc) {
    constexpr bool TAIL = decltype(tailc)::value;
    const int slot = kc % NS;
    const float* As = reinterpret_cast<const float*>(lds + slot * SSZ);
    const float* Bs = reinterpret_cast<const float*>(lds + slot * SSZ + ASZ);
    const int left = pend - (pbeg + kc * BK);  // valid pixels of this group
    // the group's fragments first (8 (TM + TN) registers), so that the MFMA
    // chain waits on counted LDS returns instead of one round trip per step
    float a[8][TM], b[8][TN];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a[s][i] = As[(h * 8 + s) * BM + wm * TM * 32 + i * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[s][j] = Bs[(h * 8 + s) * BN + wn * TN * 32 + j * 32 + li];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if constexpr (TAIL) {
        const bool in = h * 8 + s < left;
#pragma unroll
        for (int i = 0; i < TM; ++i) a[s][i] = in ? a[s][i] : 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) b[s][j] = in ? b[s][j] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
    }
  };
  for (int kc = 0; kc < nk; ++kc) {
    // K-steps kc .. kc + P - 1 are in flight: all but the newest P - 1 have
    // landed for this wave; the barrier publishes every wave's pieces
    vm_wait<D * (P - 1)>();
    raw_barrier();
    // K-step kc + P into the slot K-step kc - 1 left: every wave passed the
    // barrier after its last read of it
#pragma unroll
    for (int u = 0; u < D; ++u) issue1((kc + P) % NS, u);
    if (pbeg + (kc + 1) * BK <= pend) group(std::false_type{}, kc);
    else group(std::true_type{}, kc);
  }
  vm_wait<0>();  // the ring's last DMAs land before the workgroup gives up its LDS

  // k_wgrad's output: atomics into out, or this split's slab plane / out itself
  float* const plane = args.slab ? args.slab + (size_t)bz * args.Mo * args.No : nullptr;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int col = j0 + wn * TN * 32 + j * 32 + li;
        if (plane) plane[(size_t)row * args.No + col] = acc[i][j][r];
        else atomicAdd(args.out + zb * args.batch_out + (size_t)row * args.No + col, acc[i][j][r]);
      }
}

// unet_set_tuning("wgrad_plane", v) or UNET_WGRAD_PLANE (default on): 0 runs
// the batched point GEMMs on k_wgrad (A/B and bit-identity tests)
int g_wgrad_plane = getenv("UNET_WGRAD_PLANE") ? atoi(getenv("UNET_WGRAD_PLANE")) : 1;

// The call shape k_wgrad_plane serves: a batch of GEMMs over single-source
// contiguous planes (the operands launch_wino_wgrad builds), 32-bit byte offsets
static bool plane_gather(const Gather& g, int P) {
  const Src& s = g.s[0];
  return g.Hg == 1 && g.taps_h == 1 && g.taps_w == 1 && g.stride == 1 && g.c_split == g.Cg && g.nimg == 1 &&
         g.Wg == P && !s.scale && !s.h16 && s.H == 1 && s.W == P && s.oy == 0 && s.ox == 0 && s.C == g.Cg &&
         s.C % 4 == 0 && (reinterpret_cast<size_t>(s.ptr) & 15) == 0 &&
         ((long long)P + 2 * kPlaneNS * kPlaneBK) * s.C * 4 < (1ll << 32);  // the ring runs past the last pixel
}
bool wgrad_plane_applies(const WgradArgs& a, int bm, int bn) {
  if (!g_wgrad_plane || a.batch <= 1 || a.bf16 || !plane_gather(a.ga, a.P) || !plane_gather(a.gb, a.P)) return false;
  if (a.ga.Cg != a.Mo || a.gb.Cg != a.No || (a.batch_a | a.batch_b) % 4 != 0) return false;
  return (bm == 128 && bn == 128) || (bm == 64 && (bn == 128 || bn == 64));
}

hipError_t launch_wgrad_plane(const WgradArgs& a, hipStream_t s, dim3 grid, int bm, int bn) {
  if (bm == 128 && bn == 128) hipLaunchKernelGGL((k_wgrad_plane<128, 128>), grid, dim3(256), 0, s, a);
  else if (bm == 64 && bn == 128) hipLaunchKernelGGL((k_wgrad_plane<64, 128>), grid, dim3(256), 0, s, a);
  else if (bm == 64 && bn == 64) hipLaunchKernelGGL((k_wgrad_plane<64, 64>), grid, dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace unet
