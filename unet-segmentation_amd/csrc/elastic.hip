// Elastic-deformation input pipeline on the GPU:
// utils/augmentations.py:4-39 (elastic_deform_image_and_mask) and the
// utils/dataset.py:84-111 steps around it (uint8 casts, ToTensor, mask > 0),
// for a batch of N samples in one stream.
//
//   noise (N, 2, H, W) fp64 uniform [0, 1): field 0 -> dx, field 1 -> dy
//   k_gauss_v:  t = sum_j w[j] (2 u[y + j - r][x] - 1)      (axis 0, zeros outside)
//   k_gauss_h:  d = alpha * sum_j w[j] t[y][x + j - r]       (axis 1, zeros outside)
//   k_warp:     (cy, cx) = (y + dy, x + dx); image bilinear, labels nearest,
//               half-sample-symmetric ("reflect") extension; integer outputs
//               rounded half up and clamped (scipy.ndimage's conversion)
//   x = uint8(image') / 255 (fp32), target = uint8(label') > 0
//   k_tile_warp: the same warp for training tiles cut anywhere in a frame: an
//               affine map (shift, rotation, flips) composed into the
//               coordinate, a second border rule (whole-sample mirror, as the
//               inference tiles), a gain / bias step and a gathered weight plane
//
// Everything that decides a rounding is fp64 in the same operation order as
// oracle/elastic_oracle.py (sequential tap sums, no fma contraction), so the
// outputs are bit-identical to the oracle -- and, through it, to the reference
// (tests/golden/elastic.npz) -- except for interpolated values within ~1e-13 of
// a rounding boundary.  The filters run from LDS tiles (fp64 VALU bound: 2 x
// (2r + 1) multiply-adds per field per pixel); the warp is a gather from the
// L2-resident uint8 / uint16 planes.
#include <cmath>
#include <cstdint>

#include "unet_internal.h"

#pragma clang fp contract(off)

namespace unet {

constexpr int kGaussMaxTaps = 321;  // r <= 160
__constant__ double c_gauss_w[kGaussMaxTaps];

// axis 0: a workgroup = 64 columns x TY output rows of one field; LDS holds
// rows [y0 - r, y0 + TY + r) of the 64 columns (2u - 1, zeros outside)
template <int TY>
__global__ __launch_bounds__(256) void k_gauss_v(const double* __restrict__ u, double* __restrict__ t, int h, int w,
                                                 int r) {
  extern __shared__ double gl[];
  const int fld = blockIdx.z;  // n * 2 + field
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * TY;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const double* src = u + (size_t)fld * h * w;
  const int rows = TY + 2 * r;
  const int x = x0 + tx;
  for (int i = ty; i < rows; i += 4) {
    const int y = y0 - r + i;
    gl[i * 64 + tx] = (y >= 0 && y < h && x < w) ? src[(size_t)y * w + x] * 2 - 1 : 0.0;
  }
  __syncthreads();
  if (x >= w) return;
  const int taps = 2 * r + 1;
  for (int k = ty; k < TY; k += 4) {
    const int y = y0 + k;
    if (y >= h) break;
    double s = 0.0;
    for (int j = 0; j < taps; ++j) s = s + c_gauss_w[j] * gl[(k + j) * 64 + tx];
    t[(size_t)fld * h * w + (size_t)y * w + x] = s;
  }
}

// axis 1: a workgroup = 4 rows x 256 output columns; LDS rows hold columns
// [x0 - r, x0 + 256 + r) (zeros outside); output scaled by alpha
__global__ __launch_bounds__(256) void k_gauss_h(const double* __restrict__ t, double* __restrict__ d, int h, int w,
                                                 int r, double alpha) {
  extern __shared__ double gl[];
  const int fld = blockIdx.z;
  const int x0 = blockIdx.x * 256, y0 = blockIdx.y * 4;
  const int cols = 256 + 2 * r;
  const double* src = t + (size_t)fld * h * w;
  for (int i = threadIdx.x; i < 4 * cols; i += 256) {
    const int ry = i / cols, cx = i - ry * cols;
    const int y = y0 + ry, x = x0 - r + cx;
    gl[i] = (y < h && x >= 0 && x < w) ? src[(size_t)y * w + x] : 0.0;
  }
  __syncthreads();
  const int ry = threadIdx.x >> 6, lx = threadIdx.x & 63;
  const int y = y0 + ry;
  if (y >= h) return;
  const int taps = 2 * r + 1;
  for (int q = 0; q < 4; ++q) {
    const int c = lx + 64 * q, x = x0 + c;
    if (x >= w) break;
    double s = 0.0;
    for (int j = 0; j < taps; ++j) s = s + c_gauss_w[j] * gl[ry * cols + c + j];
    d[(size_t)fld * h * w + (size_t)y * w + x] = s * alpha;
  }
}

// half-sample-symmetric fold of a coordinate into [-0.5, n - 0.5] (numpy's mod)
__device__ __forceinline__ double reflect_coord(double c, int n) {
  if (n == 1) return 0.0;
  const double p = 2.0 * n;
  double m = fmod(c + 0.5, p);
  if (m != 0.0 && m < 0.0) m += p;
  if (m >= n) m = p - m;
  return m - 0.5;
}
__device__ __forceinline__ int reflect_index(int i, int n) {
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - i - 1;
  return i;
}
__device__ __forceinline__ unsigned to_uint(double v, double hi) {
  v = floor(fmax(v, 0.0) + 0.5);
  return (unsigned)(v > hi ? hi : v);
}

__global__ __launch_bounds__(256) void k_warp(const uint8_t* __restrict__ img, const uint16_t* __restrict__ lab,
                                              const double* __restrict__ d, int n, int h, int w,
                                              float* __restrict__ xo, uint8_t* __restrict__ to,
                                              uint8_t* __restrict__ io, uint16_t* __restrict__ ido) {
  const size_t hw = (size_t)h * w;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)n * hw) return;
  const int s = (int)(i / hw);
  const int p = (int)(i - (size_t)s * hw);
  const int y = p / w, x = p - (p / w) * w;
  const double dx = d[(size_t)(2 * s) * hw + p], dy = d[(size_t)(2 * s + 1) * hw + p];
  const double cy = reflect_coord((double)y + dy, h), cx = reflect_coord((double)x + dx, w);
  const uint8_t* im = img + (size_t)s * hw;
  const uint16_t* lb = lab + (size_t)s * hw;
  // order 1 (image)
  const double fy = floor(cy), fx = floor(cx);
  const double ty = cy - fy, tx = cx - fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int ya = reflect_index(y0, h), yb = reflect_index(y0 + 1, h);
  const int xa = reflect_index(x0, w), xb = reflect_index(x0 + 1, w);
  const double v = (1 - ty) * ((1 - tx) * (double)im[ya * w + xa] + tx * (double)im[ya * w + xb]) +
                   ty * ((1 - tx) * (double)im[yb * w + xa] + tx * (double)im[yb * w + xb]);
  const unsigned iv = to_uint(v, 255.0);
  // order 0 (labels): nearest, round half up; the uint16 -> uint8 cast wraps
  const int ny = reflect_index((int)floor(cy + 0.5), h), nx = reflect_index((int)floor(cx + 0.5), w);
  const unsigned id = lb[ny * w + nx];
  const unsigned lv = id & 0xffu;
  xo[i] = (float)iv / 255.0f;
  to[i] = lv != 0 ? 1 : 0;
  if (io) io[i] = (uint8_t)iv;
  if (ido) ido[i] = lv != 0 ? (uint16_t)id : 0;  // the warped instance map; background where the target is
}

static int gauss_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

size_t elastic_ws_bytes(int n, int h, int w) { return (size_t)2 * (2 * (size_t)n * h * w) * sizeof(double); }

// the two Gaussian passes over noise (n, 2, h, w): disp = ws + one plane pair (field 0 dx, field 1 dy)
static hipError_t launch_gauss_field(const double* noise, int n, int h, int w, double alpha, double sigma, void* ws,
                                     const double** disp_out, hipStream_t s) {
  const int r = gauss_radius(sigma);
  if (n < 1 || h < 1 || w < 1 || !(sigma > 0) || r < 0 || 2 * r + 1 > kGaussMaxTaps) return hipErrorInvalidValue;
  // kernel weights exactly as oracle/elastic_oracle.py gaussian_kernel (fp64, normalised by the sum)
  double wts[kGaussMaxTaps];
  double sum = 0.0;
  for (int j = -r; j <= r; ++j) {
    const double x = (double)j;
    wts[j + r] = std::exp(-0.5 / (sigma * sigma) * x * x);
  }
  for (int j = 0; j <= 2 * r; ++j) sum += wts[j];
  for (int j = 0; j <= 2 * r; ++j) wts[j] /= sum;
  hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_gauss_w), wts, sizeof(double) * (2 * r + 1), 0,
                                        hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  double* tmp = reinterpret_cast<double*>(ws);
  double* disp = tmp + (size_t)2 * n * h * w;
  constexpr int TY = 64;
  const size_t lv = (size_t)(TY + 2 * r) * 64 * sizeof(double), lh = (size_t)4 * (256 + 2 * r) * sizeof(double);
  static bool attr = false;
  if (!attr) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gauss_v<TY>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  if (lv > 160 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_gauss_v<TY>), dim3((w + 63) / 64, (h + TY - 1) / TY, 2 * n), dim3(256), lv, s, noise, tmp, h,
                     w, r);
  hipLaunchKernelGGL(k_gauss_h, dim3((w + 255) / 256, (h + 3) / 4, 2 * n), dim3(256), lh, s, tmp, disp, h, w, r,
                     alpha);
  *disp_out = disp;
  return hipSuccess;
}

hipError_t launch_elastic(const uint8_t* img, const uint16_t* lab, int n, int h, int w, const double* noise,
                          double alpha, double sigma, float* x_out, uint8_t* t_out, uint8_t* img_out, uint16_t* ids_out,
                          void* ws, hipStream_t s) {
  const double* disp = nullptr;
  const hipError_t e = launch_gauss_field(noise, n, h, w, alpha, sigma, ws, &disp, s);
  if (e != hipSuccess) return e;
  const size_t total = (size_t)n * h * w;
  hipLaunchKernelGGL(k_warp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, img, lab, disp, n, h, w, x_out,
                     t_out, img_out, ids_out);
  return hipGetLastError();
}

// Training tiles (the U-Net paper's training geometry): sample s is a th x tw
// tile cut from frame fidx[s]; tile pixel (ty, tx) reads the frame at
//   cy = ((a00 ty + a01 tx) + b0) + dy,  cx = ((a10 ty + a11 tx) + b1) + dx
// (prm row: a00 a01 b0 a10 a11 b1 gain bias; d = the elastic field on the tile
// grid or NULL), folded by k_warp's half-sample rule (extend 0) or the
// whole-sample rule unet_tile_gather uses at inference (extend 1).  Sampling,
// rounding and the label outputs are k_warp's; the intensity step acts on the
// rounded uint8 so that image_out stays the reference's warp of the frame.
__device__ __forceinline__ double mirror_coord(double c, int n) {
  if (n == 1) return 0.0;
  const double p = 2.0 * n - 2.0;
  double m = fmod(c, p);
  if (m < 0.0) m += p;
  if (m > (double)(n - 1)) m = p - m;
  return m;
}
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(256) void k_tile_warp(const uint8_t* __restrict__ img, const uint16_t* __restrict__ lab,
                                                   const float* __restrict__ wgt, int nframes, int h, int w,
                                                   const int32_t* __restrict__ fidx, const double* __restrict__ prm,
                                                   const double* __restrict__ d, int n, int th, int tw, int extend,
                                                   float* __restrict__ xo, uint8_t* __restrict__ to,
                                                   uint8_t* __restrict__ io, uint16_t* __restrict__ ido,
                                                   float* __restrict__ wo) {
  const size_t thw = (size_t)th * tw;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)n * thw) return;
  const int s = (int)(i / thw);
  const int p = (int)(i - (size_t)s * thw);
  const int py = p / tw, px = p - (p / tw) * tw;
  const double* a = prm + (size_t)s * 8;
  double dx = 0.0, dy = 0.0;
  if (d) {
    dx = d[(size_t)(2 * s) * thw + p];
    dy = d[(size_t)(2 * s + 1) * thw + p];
  }
  const double qy = ((a[0] * (double)py + a[1] * (double)px) + a[2]) + dy;
  const double qx = ((a[3] * (double)py + a[4] * (double)px) + a[5]) + dx;
  int f = fidx[s];
  f = f < 0 ? 0 : (f >= nframes ? nframes - 1 : f);
  const size_t fo = (size_t)f * h * w;
  const uint8_t* im = img + fo;
  int ya, yb, xa, xb, ny, nx;
  double ty, tx;
  if (extend == 0) {
    const double cy = reflect_coord(qy, h), cx = reflect_coord(qx, w);
    const double fy = floor(cy), fx = floor(cx);
    ty = cy - fy, tx = cx - fx;
    const int y0 = (int)fy, x0 = (int)fx;
    ya = reflect_index(y0, h), yb = reflect_index(y0 + 1, h);
    xa = reflect_index(x0, w), xb = reflect_index(x0 + 1, w);
    ny = reflect_index((int)floor(cy + 0.5), h), nx = reflect_index((int)floor(cx + 0.5), w);
  } else {
    const double cy = mirror_coord(qy, h), cx = mirror_coord(qx, w);
    const double fy = floor(cy), fx = floor(cx);
    ty = cy - fy, tx = cx - fx;
    ya = (int)fy, xa = (int)fx;
    yb = min(ya + 1, h - 1), xb = min(xa + 1, w - 1);
    ny = min((int)floor(cy + 0.5), h - 1), nx = min((int)floor(cx + 0.5), w - 1);
  }
  // no-ops for finite params; a NaN / Inf row must not turn into an address
  ya = clampi(ya, h), yb = clampi(yb, h), ny = clampi(ny, h);
  xa = clampi(xa, w), xb = clampi(xb, w), nx = clampi(nx, w);
  // order 1 (image), k_warp's expression
  const double v = (1 - ty) * ((1 - tx) * (double)im[ya * w + xa] + tx * (double)im[ya * w + xb]) +
                   ty * ((1 - tx) * (double)im[yb * w + xa] + tx * (double)im[yb * w + xb]);
  const unsigned iv = to_uint(v, 255.0);
  const size_t ni = fo + (size_t)(ny * w + nx);
  const unsigned id = lab[ni];
  const unsigned lv = id & 0xffu;
  xo[i] = (float)fmin(fmax(a[6] * (double)iv + a[7], 0.0), 255.0) / 255.0f;
  to[i] = lv != 0 ? 1 : 0;
  if (io) io[i] = (uint8_t)iv;
  if (ido) ido[i] = lv != 0 ? (uint16_t)id : 0;
  if (wo) wo[i] = wgt[ni];
}

bool tile_warp_check(int nframes, int h, int w, int n, int th, int tw, int extend, bool elastic, double sigma) {
  if (nframes < 1 || h < 1 || w < 1 || n < 1 || th < 1 || tw < 1) return false;
  if (extend != 0 && extend != 1) return false;
  // in-plane offsets are int; the grid is one thread per tile pixel
  if ((size_t)h * w > 0x7fffffffu || (size_t)th * tw > 0x7fffffffu) return false;
  if (((size_t)n * th * tw + 255) / 256 > 0x7fffffffu) return false;
  if (elastic) {
    if (!(sigma > 0) || !(sigma < 1e6)) return false;
    const int r = gauss_radius(sigma);
    if (r < 0 || 2 * r + 1 > kGaussMaxTaps) return false;
    if ((size_t)(64 + 2 * r) * 64 * sizeof(double) > 160 * 1024) return false;  // k_gauss_v's LDS rows
  }
  return true;
}

hipError_t launch_tile_warp(const uint8_t* frames, const uint16_t* labels, const float* weights, int nframes, int h,
                            int w, const int32_t* frame_idx, const double* params, int n, int th, int tw, int extend,
                            const double* noise, double alpha, double sigma, float* x_out, uint8_t* t_out,
                            uint8_t* img_out, uint16_t* ids_out, float* w_out, void* ws, hipStream_t s) {
  if (!tile_warp_check(nframes, h, w, n, th, tw, extend, noise != nullptr, sigma)) return hipErrorInvalidValue;
  if ((w_out && !weights) || (noise && !ws)) return hipErrorInvalidValue;
  const double* disp = nullptr;
  if (noise) {
    const hipError_t e = launch_gauss_field(noise, n, th, tw, alpha, sigma, ws, &disp, s);
    if (e != hipSuccess) return e;
  }
  const size_t total = (size_t)n * th * tw;
  hipLaunchKernelGGL(k_tile_warp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, labels, weights,
                     nframes, h, w, frame_idx, params, disp, n, th, tw, extend, x_out, t_out, img_out, ids_out, w_out);
  return hipGetLastError();
}

}  // namespace unet
