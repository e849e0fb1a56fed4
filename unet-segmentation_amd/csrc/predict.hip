// Sequence inference with symmetry averaging (scripts/predict.py's step on
// whole frames; the U-Net paper averages its submissions over rotated inputs).
// A forward's tiles come from several frames: a device work list names one
// (frame, tile) pair per group, and every group is gathered under ns of the
// eight symmetries of the square, S_s(x) = rot90(flip_f(x), r), s = r + 4 f.
// After the network, k_seq_reduce maps each symmetry's output back, averages
// the softmaxes in a fixed order and writes prob / mask / logits of the full
// frames, every pixel once by one thread: no atomics, same bits every run.
//
// Index form of S_s on an n x n array, out[i][j] = x[u][v]:
//   (p, q) = r odd ? (j, i) : (i, j);  u = fu ? n-1-p : p;  v = fv ? n-1-q : q
//   fu = r >= 2,  fv = (r == 1 || r == 2) ^ f
// Both kernels work on 32 x 32 blocks with 256 threads (32 x 8, four rows
// each).  Global reads and writes always run along the fastest axis of their
// array (a reversed run is still one run of whole cache lines); the r-odd
// symmetries exchange the axes through a 32 x 33 fp32 LDS block: rows are
// written with consecutive banks and columns read at stride 33, one bank per
// lane, so neither side conflicts.
#include <cstdint>

#include "unet_internal.h"

namespace unet {

namespace {

constexpr int kB = 32;   // block edge
constexpr int kR = 8;    // thread rows: 256 threads, kB / kR elements each

struct SymCodes {
  int ns;
  int code[8];
};

__device__ __forceinline__ int fold(int i, int n) {  // tiling.hip's mirror
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

__device__ __forceinline__ void sym_bits(int s, bool& tr, bool& fu, bool& fv) {
  const int r = s & 3;
  tr = r & 1;
  fu = r >= 2;
  fv = (r == 1 || r == 2) != ((s >> 2) != 0);
}

// torchvision's ToTensor (v / 255, a true division) and Normalize(0.5, 0.5)
__device__ __forceinline__ float norm_u8(uint8_t v) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), 0.5f), 0.5f);
}

// grid (blocks of the tile, c, groups).  The block at tile rows u0.., columns
// v0.. is read once (mirror folded, normalised) into registers and LDS and
// written under every symmetry: untransposed from the registers, transposed
// from LDS columns.
template <typename T>
__global__ __launch_bounds__(256) void k_seq_gather(const T* __restrict__ frames, int nframes, int c, int h, int w,
                                                    int ti, int to, int top, int left, int nx,
                                                    const int32_t* __restrict__ work, SymCodes sc,
                                                    float* __restrict__ tiles) {
  __shared__ float lds[kB][kB + 1];
  const int g = blockIdx.z, ch = blockIdx.y;
  const int frame = work[2 * g], t = work[2 * g + 1];
  if (frame < 0 || frame >= nframes || t < 0) return;  // block-uniform
  const int nb = (ti + kB - 1) / kB;
  const int u0 = (blockIdx.x / nb) * kB, v0 = (blockIdx.x % nb) * kB;
  const int tx = threadIdx.x & (kB - 1), ty = threadIdx.x >> 5;
  // the tile's origin, reduced modulo the mirror's period first (the work list
  // is device data: any tile number stays inside the frame)
  const int oy = (int)(((long long)(t / nx) * to - top) % (h == 1 ? 1 : 2 * h - 2));
  const int ox = (int)(((long long)(t % nx) * to - left) % (w == 1 ? 1 : 2 * w - 2));
  const T* src = frames + ((size_t)frame * c + ch) * h * (size_t)w;
  float val[kB / kR];
  const int v = v0 + tx;
  const int sx = fold(ox + v, w);
#pragma unroll
  for (int r = 0; r < kB / kR; ++r) {
    const int u = u0 + ty + kR * r;
    float x = 0.f;
    if (u < ti && v < ti) {
      const T raw = src[(size_t)fold(oy + u, h) * w + sx];
      if constexpr (sizeof(T) == 1) x = norm_u8(raw);
      else x = raw;
    }
    val[r] = x;
    lds[ty + kR * r][tx] = x;
  }
  __syncthreads();
  const size_t plane = (size_t)ti * ti;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= sc.ns) break;
    bool tr, fu, fv;
    sym_bits(sc.code[j], tr, fu, fv);
    float* dst = tiles + (((size_t)g * sc.ns + j) * c + ch) * plane;
    if (!tr) {  // out[i][jj]: i from u, jj from v
      const int jj = fv ? ti - 1 - v : v;
#pragma unroll
      for (int r = 0; r < kB / kR; ++r) {
        const int u = u0 + ty + kR * r;
        if (u < ti && v < ti) dst[(size_t)(fu ? ti - 1 - u : u) * ti + jj] = val[r];
      }
    } else {  // out[i][jj]: i from v, jj from u; lanes run along u
      const int u = u0 + tx;
      const int jj = fu ? ti - 1 - u : u;
#pragma unroll
      for (int r = 0; r < kB / kR; ++r) {
        const int vv = v0 + ty + kR * r;
        if (u < ti && vv < ti) dst[(size_t)(fv ? ti - 1 - vv : vv) * ti + jj] = lds[tx][ty + kR * r];
      }
    }
  }
}

// The logits of class q that symmetry (tr, fu, fv) moved this thread's four
// output pixels (rows y0 + ty + 8 r, column x0 + tx of the group's output tile)
// to: S^-1 of the network's output.  Transposed symmetries read the source
// block along its rows into LDS and hand out its columns.  Every thread of the
// block calls this (it synchronises).
__device__ __forceinline__ void fetch4(const float* __restrict__ src, int n, int y0, int x0, int tx, int ty, bool tr,
                                       bool fu, bool fv, float (*lds)[kB + 1], float out[kB / kR]) {
  if (!tr) {
    const int x = x0 + tx;
    const int q = fv ? n - 1 - x : x;
#pragma unroll
    for (int r = 0; r < kB / kR; ++r) {
      const int y = y0 + ty + kR * r;
      out[r] = (y < n && x < n) ? src[(size_t)(fu ? n - 1 - y : y) * n + q] : 0.f;
    }
  } else {  // source (row, column) = (q(x), p(y)); lanes run along y
    const int yy = y0 + tx;
    const int p = fu ? n - 1 - yy : yy;
    __syncthreads();  // the previous call's readers are done
#pragma unroll
    for (int r = 0; r < kB / kR; ++r) {
      const int xx = x0 + ty + kR * r;
      lds[ty + kR * r][tx] = (yy < n && xx < n) ? src[(size_t)(fv ? n - 1 - xx : xx) * n + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kB / kR; ++r) out[r] = lds[tx][ty + kR * r];
  }
}

// grid (blocks of the output tile, groups).  Any class count (two classes run
// k_seq_reduce2 below): two passes over the symmetries so that the state fits
// in registers, first each symmetry's maximum and partition sum, then class
// by class the sum over symmetries.
__global__ __launch_bounds__(256) void k_seq_reduce(const float* __restrict__ lt, int k, int to, int nx,
                                                    const int32_t* __restrict__ work, SymCodes sc, int nframes, int h,
                                                    int w, float threshold, float* __restrict__ prob,
                                                    uint8_t* __restrict__ mask, float* __restrict__ logits) {
  __shared__ float lds[kB][kB + 1];
  constexpr int P = kB / kR;
  const int g = blockIdx.y;
  const int frame = work[2 * g], t = work[2 * g + 1];
  if (frame < 0 || frame >= nframes || t < 0) return;  // block-uniform
  if ((long long)(t / nx) * to >= h || (long long)(t % nx) * to >= w) return;  // a tile past the frame
  const int nb = (to + kB - 1) / kB;
  const int y0 = (blockIdx.x / nb) * kB, x0 = (blockIdx.x % nb) * kB;
  const int tx = threadIdx.x & (kB - 1), ty = threadIdx.x >> 5;
  const int gy0 = (t / nx) * to + y0 + ty, gx = (t % nx) * to + x0 + tx;
  const size_t per = (size_t)to * to, hw = (size_t)h * w;
  const int ns = sc.ns;
  bool live[P];
#pragma unroll
  for (int r = 0; r < P; ++r)
    live[r] = y0 + ty + kR * r < to && x0 + tx < to && gy0 + kR * r < h && gx < w;
  float v[P];

  // ns == 1 at threshold 0.5 decides the mask as unet_tile_scatter does
  const bool sign_mask = mask && ns == 1 && threshold == 0.5f;
  if (ns == 1 && (logits || sign_mask)) {
    // the identity case of the tile farm: copy the logits, decide l1 > l0
    bool tr, fu, fv;
    sym_bits(sc.code[0], tr, fu, fv);
    const float* src = lt + (size_t)g * k * per;
    float l0[P] = {};
    for (int q = 0; q < k; ++q) {
      fetch4(src + q * per, to, y0, x0, tx, ty, tr, fu, fv, lds, v);
#pragma unroll
      for (int r = 0; r < P; ++r) {
        if (logits && live[r]) logits[((size_t)frame * k + q) * hw + (size_t)(gy0 + kR * r) * w + gx] = v[r];
        if (q == 0) l0[r] = v[r];
        if (q == 1 && sign_mask && live[r])
          mask[(size_t)frame * hw + (size_t)(gy0 + kR * r) * w + gx] = v[r] > l0[r] ? 255 : 0;
      }
    }
    if (!prob && !(mask && !sign_mask)) return;  // block-uniform
  }

  float mx[8][P], rz[8][P];  // unrolled over the 8 codes: registers, not scratch
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= ns) break;
    bool tr, fu, fv;
    sym_bits(sc.code[j], tr, fu, fv);
    const float* src = lt + ((size_t)g * ns + j) * k * per;
    float m[P];
    fetch4(src, to, y0, x0, tx, ty, tr, fu, fv, lds, m);
    for (int q = 1; q < k; ++q) {
      fetch4(src + q * per, to, y0, x0, tx, ty, tr, fu, fv, lds, v);
#pragma unroll
      for (int r = 0; r < P; ++r) m[r] = fmaxf(m[r], v[r]);
    }
    float z[P] = {};
    for (int q = 0; q < k; ++q) {
      fetch4(src + q * per, to, y0, x0, tx, ty, tr, fu, fv, lds, v);
#pragma unroll
      for (int r = 0; r < P; ++r) z[r] += expf(v[r] - m[r]);
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
      mx[j][r] = m[r];
      rz[j][r] = z[r];
    }
  }
  const float inv = 1.f / (float)ns;
  const bool want_mask = mask && !sign_mask;
  for (int q = 0; q < k; ++q) {
    float acc[P] = {};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= ns) break;
      bool tr, fu, fv;
      sym_bits(sc.code[j], tr, fu, fv);
      fetch4(lt + (((size_t)g * ns + j) * k + q) * per, to, y0, x0, tx, ty, tr, fu, fv, lds, v);
#pragma unroll
      for (int r = 0; r < P; ++r) acc[r] += expf(v[r] - mx[j][r]) / rz[j][r];
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
      if (!live[r]) continue;
      const float pm = acc[r] * inv;
      const size_t px = (size_t)(gy0 + kR * r) * w + gx;
      if (prob) prob[((size_t)frame * k + q) * hw + px] = pm;
      if (want_mask && q == 1) mask[(size_t)frame * hw + px] = pm > threshold ? 255 : 0;
    }
  }
}

// Two classes (segmentation), same values as k_seq_reduce in one pass: both
// logits of a symmetry sit in registers, so its softmax is done when they
// arrive.  The loads of symmetry j + 1 are issued before symmetry j is worked
// on, and a transposed symmetry stages both classes behind one barrier, in
// one of two LDS images taken in turn (the barrier of the staging in between
// orders a rewrite after every read).
__global__ __launch_bounds__(256) void k_seq_reduce2(const float* __restrict__ lt, int to, int nx,
                                                     const int32_t* __restrict__ work, SymCodes sc, int nframes, int h,
                                                     int w, float threshold, float* __restrict__ prob,
                                                     uint8_t* __restrict__ mask, float* __restrict__ logits) {
  __shared__ float lds[2][2][kB][kB + 1];
  constexpr int P = kB / kR;
  const int g = blockIdx.y;
  const int frame = work[2 * g], t = work[2 * g + 1];
  if (frame < 0 || frame >= nframes || t < 0) return;  // block-uniform
  if ((long long)(t / nx) * to >= h || (long long)(t % nx) * to >= w) return;  // a tile past the frame
  const int nb = (to + kB - 1) / kB;
  const int y0 = (blockIdx.x / nb) * kB, x0 = (blockIdx.x % nb) * kB;
  const int tx = threadIdx.x & (kB - 1), ty = threadIdx.x >> 5;
  const int gy0 = (t / nx) * to + y0 + ty, gx = (t % nx) * to + x0 + tx;
  const size_t per = (size_t)to * to, hw = (size_t)h * w;
  const int ns = sc.ns;
  bool live[P];
#pragma unroll
  for (int r = 0; r < P; ++r)
    live[r] = y0 + ty + kR * r < to && x0 + tx < to && gy0 + kR * r < h && gx < w;
  const bool sign_mask = mask && ns == 1 && threshold == 0.5f;  // unet_tile_scatter's rule
  const bool soft = prob || (mask && !sign_mask);

  // symmetry j's two logits: at this thread's pixels, or (transposed) the
  // elements of the source block's rows that this thread stages
  auto load = [&](int j, float (&o)[2][P]) {
    bool tr, fu, fv;
    sym_bits(sc.code[j], tr, fu, fv);
    const float* src = lt + ((size_t)g * ns + j) * 2 * per;
    const int a = tr ? y0 + tx : x0 + tx;  // lanes: the source's columns
    const int col = (tr ? fu : fv) ? to - 1 - a : a;
#pragma unroll
    for (int r = 0; r < P; ++r) {
      const int b = (tr ? x0 : y0) + ty + kR * r;
      const bool ok = a < to && b < to;
      const size_t idx = (size_t)((tr ? fv : fu) ? to - 1 - b : b) * to + col;
      o[0][r] = ok ? src[idx] : 0.f;
      o[1][r] = ok ? src[per + idx] : 0.f;
    }
  };

  float cur[2][P], nxt[2][P] = {}, acc0[P] = {}, acc1[P] = {};
  load(0, cur);
  int staged = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= ns) break;
    if (j + 1 < ns) load(j + 1, nxt);
    if (sc.code[j] & 1) {  // block-uniform
      float(*buf)[kB][kB + 1] = lds[staged++ & 1];
#pragma unroll
      for (int r = 0; r < P; ++r) {
        buf[0][ty + kR * r][tx] = cur[0][r];
        buf[1][ty + kR * r][tx] = cur[1][r];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < P; ++r) {
        cur[0][r] = buf[0][tx][ty + kR * r];
        cur[1][r] = buf[1][tx][ty + kR * r];
      }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
      const float l0 = cur[0][r], l1 = cur[1][r];
      if (ns == 1 && live[r]) {
        const size_t px = (size_t)(gy0 + kR * r) * w + gx;
        if (logits) {
          logits[(size_t)frame * 2 * hw + px] = l0;
          logits[((size_t)frame * 2 + 1) * hw + px] = l1;
        }
        if (sign_mask) mask[(size_t)frame * hw + px] = l1 > l0 ? 255 : 0;
      }
      if (soft) {
        const float m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m);
        const float z = e0 + e1;
        acc0[r] += e0 / z;
        acc1[r] += e1 / z;
      }
      cur[0][r] = nxt[0][r];
      cur[1][r] = nxt[1][r];
    }
  }
  if (!soft) return;
  const float inv = 1.f / (float)ns;
#pragma unroll
  for (int r = 0; r < P; ++r) {
    if (!live[r]) continue;
    const size_t px = (size_t)(gy0 + kR * r) * w + gx;
    const float p1 = acc1[r] * inv;
    if (prob) {
      prob[(size_t)frame * 2 * hw + px] = acc0[r] * inv;
      prob[((size_t)frame * 2 + 1) * hw + px] = p1;
    }
    if (mask && !sign_mask) mask[(size_t)frame * hw + px] = p1 > threshold ? 255 : 0;
  }
}

bool pack_codes(const int32_t* codes, int ns, SymCodes& sc) {
  if (!codes || ns < 1 || ns > 8) return false;
  sc.ns = ns;
  for (int j = 0; j < 8; ++j) sc.code[j] = 0;
  for (int j = 0; j < ns; ++j) {
    if (codes[j] < 0 || codes[j] > 7) return false;
    sc.code[j] = codes[j];
  }
  return true;
}

}  // namespace

hipError_t launch_seq_tile_gather(const void* frames, int is_u8, int nframes, int c, int h, int w, int ti, int to,
                                  int top, int left, int nx, const int32_t* work, int ngroups, const int32_t* codes,
                                  int ns, float* tiles, hipStream_t s) {
  SymCodes sc;
  if (nframes < 1 || c < 1 || c > 65535 || h < 1 || w < 1 || ti < 1 || to < 1 || to > ti || nx < 1 || ngroups < 1 ||
      ngroups > 65535 || !pack_codes(codes, ns, sc))
    return hipErrorInvalidValue;
  const int nb = (ti + kB - 1) / kB;
  const dim3 grid((unsigned)(nb * nb), (unsigned)c, (unsigned)ngroups);
  if (is_u8)
    hipLaunchKernelGGL(k_seq_gather<uint8_t>, grid, dim3(256), 0, s, static_cast<const uint8_t*>(frames), nframes, c,
                       h, w, ti, to, top, left, nx, work, sc, tiles);
  else
    hipLaunchKernelGGL(k_seq_gather<float>, grid, dim3(256), 0, s, static_cast<const float*>(frames), nframes, c, h,
                       w, ti, to, top, left, nx, work, sc, tiles);
  return hipGetLastError();
}

hipError_t launch_seq_tile_reduce(const float* lt, int k, int to, int nx, const int32_t* work, int ngroups,
                                  const int32_t* codes, int ns, int nframes, int h, int w, float threshold,
                                  float* prob, uint8_t* mask, float* logits, hipStream_t s) {
  SymCodes sc;
  if (k < 1 || to < 1 || nx < 1 || ngroups < 1 || ngroups > 65535 || nframes < 1 || h < 1 || w < 1 ||
      !pack_codes(codes, ns, sc) || (mask && k != 2) || (logits && ns != 1) || (!prob && !mask && !logits))
    return hipErrorInvalidValue;
  const int nb = (to + kB - 1) / kB;
  const dim3 grid((unsigned)(nb * nb), (unsigned)ngroups);
  if (k == 2)
    hipLaunchKernelGGL(k_seq_reduce2, grid, dim3(256), 0, s, lt, to, nx, work, sc, nframes, h, w, threshold, prob, mask,
                       logits);
  else
    hipLaunchKernelGGL(k_seq_reduce, grid, dim3(256), 0, s, lt, k, to, nx, work, sc, nframes, h, w, threshold, prob,
                       mask, logits);
  return hipGetLastError();
}

}  // namespace unet
