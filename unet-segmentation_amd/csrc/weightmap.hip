// Per-pixel loss weight maps: scripts/preprocess_data.py
// :17-77 (calculate_weight_map) for a batch of label maps, on the device.
// weight = fp32(wc[class]) + w0 * exp(-(d1 + d2)^2 / (2 (sigma^2 + 1e-8))), with
// wc = 1 / (count / total) of the pixel's class (fp64, 0 for an empty class)
// and d1 = d2 = 0: the reference's per-object distance, min(edt(obj),
// edt(obj == 0)), is identically zero (each transform is 0 where its mask is
// 0, and one of the two masks is 0 at every pixel), so the separation term is
// exactly w0 (oracle/weightmap_oracle.py states the argument; the fixtures made
// by the reference pin it).  Two launches: a per-sample foreground count
// (wave reduction + one 64-bit atomic per workgroup) and the map.
// Border mode (unet_weight_map_border, second half of this file) is the same
// formula with d1, d2 the exact distances to the two nearest objects.
#include <cmath>
#include <cstdint>

#include "unet_internal.h"

#pragma clang fp contract(off)

namespace unet {

__global__ __launch_bounds__(256) void k_wm_count(const uint16_t* __restrict__ lab, size_t hw,
                                                  unsigned long long* __restrict__ cnt) {
  const int s = blockIdx.y;
  const uint16_t* l = lab + (size_t)s * hw;
  unsigned c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x)
    c += l[i] != 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  __shared__ unsigned part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(cnt + s, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
}

__global__ __launch_bounds__(256) void k_wm_apply(const uint16_t* __restrict__ lab, int n, size_t hw,
                                                  const unsigned long long* __restrict__ cnt, double w0,
                                                  double sigma, float* __restrict__ out, double* __restrict__ out64) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)n * hw) return;
  const int s = (int)(i / hw);
  const double total = (double)hw, fg = (double)cnt[s], bg = total - fg;
  const bool is_fg = lab[i] != 0;
  const double wc = is_fg ? (fg > 0 ? 1.0 / (fg / total) : 0.0) : (bg > 0 ? 1.0 / (bg / total) : 0.0);
  const double d = 0.0;  // d1 + d2
  const double term = w0 * exp(-(d * d) / (2 * (sigma * sigma + 1e-8)));
  const double v = (double)(float)wc + term;
  out[i] = (float)v;
  if (out64) out64[i] = v;
}

size_t weight_map_ws_bytes(int n) { return (size_t)n * sizeof(unsigned long long); }

hipError_t launch_weight_map(const uint16_t* lab, int n, int h, int w, double w0, double sigma, float* out,
                             double* out64, void* ws, hipStream_t s) {
  if (n < 1 || h < 1 || w < 1) return hipErrorInvalidValue;
  auto* cnt = reinterpret_cast<unsigned long long*>(ws);
  hipError_t e = hipMemsetAsync(cnt, 0, weight_map_ws_bytes(n), s);
  if (e != hipSuccess) return e;
  const size_t hw = (size_t)h * w;
  unsigned gx = (unsigned)((hw + 255) / 256);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(k_wm_count, dim3(gx, n), dim3(256), 0, s, lab, hw, cnt);
  const size_t total = (size_t)n * hw;
  hipLaunchKernelGGL(k_wm_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, lab, n, hw, cnt, w0, sigma,
                     out, out64);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------
// Border mode: the U-Net paper's term with d1, d2 the distances to the nearest
// and second-nearest object (dist_l = edt(L != l)), exact, in two passes whose
// cost and workspace do not depend on the number of objects (DESIGN.md "Border
// weight maps").
//
// k_wb_cols (per column, one thread): a downward and an upward scan each carry
// the last object pixel seen (id a, row ra) and the last one with an id != a
// (id b, row rb); every pixel stores the four candidates packed id << 16 | row
// (id 0 = none).  A column's two vertically nearest distinct ids per direction
// suffice for the two smallest per-object distances: were the object attaining
// the second minimum through a column not among them, two other distinct
// objects would be at least as close through that column.
//
// k_wb_rows (per output pixel): sweeps the row's candidates, staged in LDS with
// (y - row)^2 precomputed (a missing candidate carries kWbNone there), keeping
// the best squared distance b1 with its id and the best b2 of any other id;
// every lane reads the same LDS address (broadcast), the loop is int32 VALU
// only.  A wave sweeps outwards from its own columns and stops once the
// columns still to come are farther from every lane than its b2.  Then wc (as
// k_wm_apply), sqrt, exp and the stores.
constexpr int kWbChunk = 512;          // candidate columns per LDS stage (16 KiB)
constexpr int kWbNone = 1 << 30;       // > any h^2 + w^2 (h, w <= 16384), sums stay in int32
constexpr int kWbMaxDim = 16384;

__global__ __launch_bounds__(64) void k_wb_cols(const uint16_t* __restrict__ lab, int h, int w,
                                                uint2* __restrict__ cand) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  const int s = blockIdx.y, up = blockIdx.z;
  const size_t hw = (size_t)h * w, n = gridDim.y;
  const uint16_t* l = lab + (size_t)s * hw + x;
  uint2* c = cand + ((size_t)up * n + s) * hw + x;  // plane 0: downward scan, plane 1: upward
  unsigned a = 0, b = 0;                             // packed id << 16 | row, 0 = none
  const int y0 = up ? h - 1 : 0, dy = up ? -1 : 1;
#pragma unroll 8
  for (int k = 0; k < h; ++k) {
    const int y = y0 + k * dy;
    const unsigned id = l[(size_t)y * w];
    if (id != 0) {
      if (id != (a >> 16)) b = a;  // a == 0 (none) moves "none" into b
      a = id << 16 | (unsigned)y;
    }
    c[(size_t)y * w] = make_uint2(a, b);
  }
}

__global__ __launch_bounds__(256) void k_wb_rows(const uint16_t* __restrict__ lab, const uint2* __restrict__ cand, int n,
                                                 int h, int w, int tiles, const unsigned long long* __restrict__ cnt,
                                                 double w0, double sigma, float* __restrict__ out,
                                                 double* __restrict__ out64, int* __restrict__ d1o,
                                                 int* __restrict__ d2o) {
  __shared__ int4 sh[kWbChunk][2];  // {id, dy^2} x 4 per column
  const int tile = blockIdx.x % tiles;
  const size_t row = blockIdx.x / tiles;  // s * h + y
  const int s = (int)(row / h), y = (int)(row - (size_t)s * h);
  const size_t hw = (size_t)h * w;
  const uint2* cd = cand + row * w;              // downward plane
  const uint2* cu = cd + (size_t)n * hw;         // upward plane
  const int x = tile * 256 + threadIdx.x;
  // this wave's columns [wx0, wx0 + 63]; it sweeps each chunk outwards from the column nearest its centre
  const int wx0 = __builtin_amdgcn_readfirstlane(tile * 256 + (int)(threadIdx.x & ~63u));
  const int nchunk = (w + kWbChunk - 1) / kWbChunk, home = min(tile * 256 + 128, w - 1) / kWbChunk;
  int b1 = 0x7fffffff, b2 = 0x7fffffff, id1 = 0;
  for (int cc = 0; cc < nchunk; ++cc) {  // the workgroup's own chunk first: b2 is tight before the far ones
    const int c0 = (home + cc) % nchunk * kWbChunk;
    const int len = min(kWbChunk, w - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += 256) {
      const uint2 p = cd[c0 + i], q = cu[c0 + i];
      const unsigned v[4] = {p.x, p.y, q.x, q.y};
      int e[8];
      for (int j = 0; j < 4; ++j) {
        const int r = y - (int)(v[j] & 0xffffu);
        e[2 * j] = (int)(v[j] >> 16);
        e[2 * j + 1] = v[j] ? r * r : kWbNone;
      }
      sh[i][0] = make_int4(e[0], e[1], e[2], e[3]);
      sh[i][1] = make_int4(e[4], e[5], e[6], e[7]);
    }
    __syncthreads();
    if (wx0 >= w) continue;  // a wave past the row's end (wave-uniform; it still meets the barriers)
    const int pc = min(max(min(wx0 + 32, w - 1) - c0, 0), len - 1);
    for (int k = 0; pc + k < len || pc - 1 - k >= 0; ++k) {
      // columns still to come are at least g away from every lane's column: once g^2 >= b2 (>= b1) in all
      // lanes, no candidate out there can lower b1 or b2 (its d >= dx^2 >= g^2), so the rest is skipped
      const int ir = pc + k, il = pc - 1 - k;
      const int gr = ir < len ? max(c0 + ir - (wx0 + 63), 0) : 0x7fff, gl = il >= 0 ? max(wx0 - (c0 + il), 0) : 0x7fff;
      const int g = min(gr, gl);
      if (__all(g * g >= b2)) break;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int i = side ? il : ir;
        if (side ? il < 0 : ir >= len) continue;
        const int dx = x - (c0 + i), dx2 = dx * dx;
        const int4 p = sh[i][0], q = sh[i][1];
        const int ids[4] = {p.x, p.z, q.x, q.z}, dy2[4] = {p.y, p.w, q.y, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int d = dx2 + dy2[j];
          // same id as b1: min into b1; else smaller than b1: b1 moves down to b2; else min into b2
          b2 = min(b2, ids[j] == id1 ? 0x7fffffff : max(d, b1));
          id1 = d < b1 ? ids[j] : id1;
          b1 = min(b1, d);
        }
      }
    }
  }
  if (x >= w) return;
  const int d1s = b1 < kWbNone ? b1 : 0, d2s = b2 < kWbNone ? b2 : 0;  // fewer than two objects: d2 = 0
  const size_t i = row * w + x;
  const double total = (double)hw, fg = (double)cnt[s], bg = total - fg;
  const bool is_fg = lab[i] != 0;
  const double wc = is_fg ? (fg > 0 ? 1.0 / (fg / total) : 0.0) : (bg > 0 ? 1.0 / (bg / total) : 0.0);
  const double d = sqrt((double)d1s) + sqrt((double)d2s);
  const double term = w0 * exp(-(d * d) / (2 * (sigma * sigma + 1e-8)));
  const double v = (double)(float)wc + term;
  out[i] = (float)v;
  if (out64) out64[i] = v;
  if (d1o) d1o[i] = d1s;
  if (d2o) d2o[i] = d2s;
}

// counts (n x 8 B, padded to 16) then the two candidate planes (2 x 8 B per pixel)
static size_t wb_cnt_bytes(int n) { return ((size_t)n * sizeof(unsigned long long) + 15) & ~(size_t)15; }

size_t weight_map_border_ws_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || h > kWbMaxDim || w > kWbMaxDim) return 0;
  return wb_cnt_bytes(n) + (size_t)n * h * w * 2 * sizeof(uint2);
}

hipError_t launch_weight_map_border(const uint16_t* lab, int n, int h, int w, double w0, double sigma, float* out,
                                    double* out64, int32_t* d1sq, int32_t* d2sq, void* ws, hipStream_t s) {
  if (n < 1 || h < 1 || w < 1 || h > kWbMaxDim || w > kWbMaxDim) return hipErrorInvalidValue;
  const int tiles = (w + 255) / 256;
  const size_t blocks = (size_t)n * h * tiles;
  if (n > 65535 || blocks > 0x7fffffffu) return hipErrorInvalidValue;  // grid limits
  auto* cnt = reinterpret_cast<unsigned long long*>(ws);
  uint2* cand = reinterpret_cast<uint2*>(reinterpret_cast<char*>(ws) + wb_cnt_bytes(n));
  hipError_t e = hipMemsetAsync(cnt, 0, wb_cnt_bytes(n), s);
  if (e != hipSuccess) return e;
  const size_t hw = (size_t)h * w;
  unsigned gx = (unsigned)((hw + 255) / 256);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(k_wm_count, dim3(gx, n), dim3(256), 0, s, lab, hw, cnt);
  hipLaunchKernelGGL(k_wb_cols, dim3((w + 63) / 64, n, 2), dim3(64), 0, s, lab, h, w, cand);
  hipLaunchKernelGGL(k_wb_rows, dim3((unsigned)blocks), dim3(256), 0, s, lab, cand, n, h, w, tiles, cnt, w0, sigma, out,
                     out64, d1sq, d2sq);
  return hipGetLastError();
}

}  // namespace unet
