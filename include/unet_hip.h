/*
 * unet_hip.h -- C-ABI of libunet_hip.so, the MI355X (gfx950) implementation of
 * the valid-convolution U-Net training / inference hot path of
 * SaurabhIndi/unet-segmentation (reference snapshot 2025-07-25).
 *
 * The reference has no FFI: its boundary is the nn.Module API
 *   models/unet_model.py:66   UNet(n_channels, n_classes, bilinear=False)
 *   models/unet_model.py:105  UNet.forward(x) -> logits (N, n_classes, H-184, W-184)
 *   utils/losses.py:29        WeightedCrossEntropyLoss.forward(inputs, targets, weight_maps)
 *   scripts/train.py:97,131   optim.SGD(lr=1e-4, momentum=0.99).step()
 * These entry points are what a Python (ctypes) binding of that boundary calls;
 * unet-segmentation_amd/unet_amd/_lib.py is that binding.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless the name says host_.  Buffers are
 *    owned by the caller (PyTorch caching allocator); the library never
 *    allocates device memory.
 *  - Activations are NHWC float32 ("_nhwc"); the network input x and the
 *    logits use the reference's NCHW layout.
 *  - Parameter tables are host arrays of device pointers in the reference
 *    state_dict order (136 entries incl. BN buffers; 82 gradient entries in
 *    named_parameters order).  Shapes are PyTorch's (Conv2d OIHW,
 *    ConvTranspose2d IOHW).
 *  - stream is a hipStream_t (torch.cuda.current_stream().cuda_stream).
 *  - Return 0 on success, a negative errno-style code on bad arguments
 *    (-EINVAL) or a HIP launch failure (-EIO); never throws across the ABI.
 *    unet_last_error() returns a static message for the last failure.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* unet_stream_t; /* hipStream_t */

/* "unet_hip <ver> gfx950 ... src <hash>": <hash> = the first 16 hex digits of
 * sha256 over the library's sources (csrc/Makefile SRC_HASH), so a run's record
 * shows which sources the loaded .so was built from. */
const char* unet_version(void);
const char* unet_last_error(void);

/* ------------------------------------------------------------------------
 * Whole-network plan: one plan per (N, C, H, W, n_classes).  Replaces the
 * body of UNet.forward (models/unet_model.py:105-146) and autograd's backward
 * through it.
 * ---------------------------------------------------------------------- */
typedef struct unet_plan unet_plan;

/* Create a plan; returns NULL (and sets unet_last_error) for sizes the valid
 * U-Net cannot take (models/unet_model.py:189: out = in - 184 for clean sizes)
 * and for c_in or n_classes outside 1..4096 (the reference's
 * UNet(n_channels, n_classes), models/unet_model.py:66-85, takes any counts;
 * the bound only keeps the per-plan buffers in reason: the first conv stages
 * its input channels in chunks of 16, the head / loss run register-blocked up
 * to 32 classes and with a run-time class loop above).
 * unet_plan_create() is unet_plan_create_ex(..., UNET_PREC_FP32). */
unet_plan* unet_plan_create(int n, int c_in, int h, int w, int n_classes);

/* Arithmetic of the implicit-GEMM convolutions (the 17 3x3 convs after the
 * first, the 4 ConvTranspose2d, their input and weight gradients):
 *  UNET_PREC_FP32  fp32 operands, exact fp32 MFMA (configs C1/C2, the parity
 *                  configuration);
 *  UNET_PREC_BF16  both operands rounded to bf16 (RNE) when staged, fp32
 *                  accumulation (v_mfma_f32_32x32x16_bf16): the "bf16-in /
 *                  fp32-acc" of configs C3/C5, what torch.autocast(bfloat16)
 *                  asks of the reference's convolutions;
 *  UNET_PREC_BF16X3 fp32-accurate GEMMs on the bf16 matrix cores: each fp32
 *                  operand is split v = hi + lo (hi = bf16(v), lo = bf16(v -
 *                  hi), |v - hi - lo| <= 2^-16 |v|) and a product is taken as
 *                  hi*hi' + hi*lo' + lo*hi' (three v_mfma_f32_32x32x16_bf16,
 *                  fp32 accumulation; the dropped lo*lo' is <= 2^-16 of the
 *                  product).  Storage as in UNET_PREC_FP32; tested against the
 *                  fp64 oracle at the fp32 tolerances.
 * Everything else -- the first conv (any Ci), the 1x1 head, BatchNorm, the
 * loss, gradients and the optimizer -- is fp32 in all three; UNET_PREC_BF16
 * plans also store the GEMM-only tensors and the raw conv outputs in bf16. */
enum { UNET_PREC_FP32 = 0, UNET_PREC_BF16 = 1, UNET_PREC_BF16X3 = 2 };
unet_plan* unet_plan_create_ex(int n, int c_in, int h, int w, int n_classes, int precision);
int unet_plan_precision(const unet_plan* p);
void unet_plan_destroy(unet_plan* p);
/* Output spatial size and the workspace the caller must provide.
 * unet_plan_workspace_bytes: a forward followed by unet_plan_backward.
 * unet_plan_forward_workspace_bytes: a forward that no backward follows (eval
 * mode -- scripts/predict.py -- or a train-mode forward under torch.no_grad);
 * a prefix of the full layout, about 1/3 of it (the gradient buffers are left
 * out).  Running unet_plan_backward on such a workspace is undefined. */
int unet_plan_out_hw(const unet_plan* p, int* out_h, int* out_w);
size_t unet_plan_workspace_bytes(const unet_plan* p);
size_t unet_plan_forward_workspace_bytes(const unet_plan* p);
int unet_plan_num_params(const unet_plan* p);  /* 136 (state_dict entries) */
int unet_plan_num_grads(const unet_plan* p);   /* 82 */

/* Forward.  train=1: BatchNorm uses batch statistics and updates the running
 * buffers in place (momentum 0.1, unbiased var, num_batches_tracked += 1);
 * train=0: running statistics (scripts/predict.py:70 model.eval()).
 * host_params[136]: device pointers of the state_dict tensors.
 * x_nchw: (N, C, H, W) float32 contiguous.  logits_nchw: (N, K, Ho, Wo).
 * workspace: unet_plan_workspace_bytes() bytes, 256-B aligned; it holds the
 * activations the backward needs, so keep it alive until unet_plan_backward. */
int unet_plan_forward(unet_plan* p, void* const* host_params, const float* x_nchw,
                      float* logits_nchw, void* workspace, int train, unet_stream_t stream);

/* Backward of the whole network for dlogits (N, K, Ho, Wo).  Writes (does not
 * accumulate) the 82 parameter gradients to host_grads[].  Segments let a
 * data-parallel caller all-reduce finished gradients while the rest runs:
 * segment s in [seg_begin, seg_end) of unet_plan_num_segments(); the full
 * backward is (0, num_segments).  unet_plan_segment_grads() lists, for a
 * segment, which gradient entries are final after it.  x_nchw is the forward
 * input (inc.c0's weight gradient reads it). */
int unet_plan_num_segments(const unet_plan* p);
int unet_plan_segment_grads(const unet_plan* p, int seg, int* first_grad, int* n_grads);
int unet_plan_backward(unet_plan* p, void* const* host_params, void* const* host_grads,
                       const float* x_nchw, const float* dlogits_nchw, void* workspace,
                       int seg_begin, int seg_end, unet_stream_t stream);
/* Gradient of the network input (the reference's x.grad when the input
 * requires grad; models/unet_model.py:105): after the backward segment that
 * holds inc.c0 (segment 8, i.e. a whole backward), materialises inc.c0's
 * BatchNorm-backward output into `scratch` (fp32,
 * unet_plan_input_grad_scratch_bytes) and writes dx (N, C, H, W) fp32.  Same
 * stream as the backward. */
size_t unet_plan_input_grad_scratch_bytes(const unet_plan* p);
int unet_plan_input_grad(unet_plan* p, void* const* params, float* dx, void* workspace, void* scratch,
                         unet_stream_t stream);
/* The same with flags.  UNET_BWD_DEFER_JOIN: the weight gradients of these
 * segments (which run on the plan's side stream beside the input-gradient
 * chain once the plan is tuned) are NOT joined into `stream` on return, so the
 * next segment's input gradients overlap them; a collective over segment s's
 * gradients must first make its stream wait with unet_plan_wait_segment(s),
 * and unet_plan_join() must be called on `stream` before anything reads the
 * gradients or the workspace again (optimizer step, next forward).  This is
 * the data-parallel schedule (unet_amd/train.py): all-reduce bucket s while
 * segment s+1 computes. */
enum { UNET_BWD_DEFER_JOIN = 1 };
int unet_plan_backward_ex(unet_plan* p, void* const* host_params, void* const* host_grads,
                          const float* x_nchw, const float* dlogits_nchw, void* workspace,
                          int seg_begin, int seg_end, int flags, unet_stream_t stream);
int unet_plan_wait_segment(unet_plan* p, int seg, unet_stream_t stream);
int unet_plan_join(unet_plan* p, unet_stream_t stream);

/* Optional per-kernel timing of the next forward/backward: the plan records a
 * hipEvent pair around each launch (class ids below).  unet_plan_timing()
 * returns accumulated milliseconds and algorithmic FLOP/bytes per class. */
enum {
  UNET_KC_CONV_FWD = 0, UNET_KC_CONV_DGRAD = 1, UNET_KC_CONV_WGRAD = 2,
  UNET_KC_STAGE1 = 3,   /* inc.c0 fwd + its BN/ReLU passes (memory-bound) */
  UNET_KC_ELEMWISE = 4, /* BN / pool / head / repack passes */
  UNET_KC_BOTTLENECK = 5, /* overlaps 0-2: the GEMMs of down4.c0, down4.c1,
                             up1.convT, up1.c0 (SURVEY.md §8d's bottleneck set) */
  UNET_KC_COUNT = 6
};
int unet_plan_set_timing(unet_plan* p, int enable);
int unet_plan_timing(const unet_plan* p, double* ms, double* flops, double* bytes, int* launches);
/* MFMA flops the chosen GEMM variants executed per class over the intervals the
 * last unet_plan_timing() call reported: equal to its `flops` (the direct
 * convolution's 2*M*N*K) except where a Winograd variant ran (igemm tiles
 * 70-72/74, wgrad tiles 71/74: 2 * points * tiles * Cin * Cout). */
int unet_plan_timing_mfma_flops(const unet_plan* p, double* mfma_flops);
/* Per GEMM launch site of the last step unet_plan_timing() collected: one line
 * per site, "<layer> <fwd|dgrad|wgrad>\t<ms>\t<direct flops>\t<MFMA flops>".
 * Copies up to cap bytes (NUL-terminated) into buf; returns the size needed. */
size_t unet_plan_timing_sites(const unet_plan* p, char* buf, size_t cap);

/* ------------------------------------------------------------------------
 * Loss: WeightedCrossEntropyLoss (utils/losses.py:29-57) fused fwd+bwd.
 * logits (N, K, H, W) contiguous; targets int64 and weights float32 are read
 * through element strides (the caller's center-cropped views,
 * scripts/train.py:118-126, need no copy).  Writes loss (1 float) and
 * dlogits = w*(softmax - onehot)/(N*H*W) * grad_scale.  ws: 64*8 bytes; on
 * return-to-host ws[1] (double) is 1 if a target was outside [0, k) and not
 * ignore_index -100 (such pixels contribute nothing), ws[2] one such target:
 * torch's nn.CrossEntropyLoss raises for them (utils/losses.py:27), the caller
 * checks the flag at its next synchronisation point.  1 <= k <= 32. */
int unet_wce_fwd_bwd(const float* logits, const int64_t* targets, const float* weights,
                     int n, int k, int h, int w,
                     const int64_t* t_strides /*host, 3*/, const int64_t* w_strides /*host, 3*/,
                     float* loss_out, float* dlogits, float grad_scale, void* ws,
                     unet_stream_t stream);
/* dlogits *= g[0] (the upstream scalar gradient, device), in place. */
int unet_scale_by_device_scalar(float* x, size_t n, const float* g, unet_stream_t stream);
/* y = x * g[0] (y may alias x): the loss backward scales into a fresh tensor so
 * the saved gradient survives a second backward (retain_graph=True). */
int unet_scale_by_device_scalar_out(const float* x, float* y, size_t n, const float* g, unet_stream_t stream);

/* SGD with momentum (torch.optim.SGD, dampening 0, no weight decay), flat,
 * on the gradient g*grad_scale (grad_scale = 1/world after a SUM all-reduce):
 * first_step: buf = g; else buf = momentum*buf + g;  p -= lr*buf.
 * p, g, buf 16-byte aligned.  scripts/train.py:97,131. */
int unet_sgd_momentum(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                      float grad_scale, int first_step, unet_stream_t stream);

/* Binary IoU of two uint8 masks (utils/metrics.py:6-37), counts on device:
 * out[0] = |pred>0 & gt>0|, out[1] = |pred>0 | gt>0| (uint64). */
int unet_iou_counts(const uint8_t* pred, const uint8_t* gt, size_t n, unsigned long long* out,
                    unet_stream_t stream);
/* mask = (logit1 > logit0) * 255 (scripts/predict.py:85-92), logits NCHW K=2. */
int unet_mask_from_logits(const float* logits, uint8_t* mask, int n, int h, int w,
                          unet_stream_t stream);

/* Elastic-deformation input pipeline: the
 * utils/augmentations.py:4-39 warp and the utils/dataset.py:84-111 steps around
 * it for a batch of n samples (h x w each):
 *   noise  (n, 2, h, w) fp64 uniform [0, 1) -- field 0 drives dx, field 1 dy
 *          (the reference draws them as RandomState(seed).rand(h, w), dx first);
 *   dx|dy = alpha * gaussian_filter(2 noise - 1, sigma, mode="constant")
 *          (truncate 4: radius int(4 sigma + 0.5) <= 160);
 *   image' = map_coordinates(image, (y + dy, x + dx), order=1, mode="reflect"),
 *   label' = same with order=0, both rounded to their integer type;
 *   x_out  (n, h, w) fp32 = uint8(image') / 255   (ToTensor, NCHW with C = 1),
 *   target_out (n, h, w) uint8 = uint8(label') > 0 (the weight map is not
 *          warped, as in the reference);
 *   image_out (optional, may be NULL) = uint8(image').
 * ws >= unet_elastic_ws_bytes(n, h, w), 8-byte aligned. */
size_t unet_elastic_ws_bytes(int n, int h, int w);
int unet_elastic_deform(const uint8_t* image, const uint16_t* labels, int n, int h, int w,
                        const double* noise, double alpha, double sigma, float* x_out,
                        uint8_t* target_out, uint8_t* image_out, void* ws, unet_stream_t stream);
/* The same with the warped instance map: ids_out (n, h, w) uint16 (may be
 * NULL) holds, at each output pixel, the id at the nearest source pixel the
 * target was sampled from, and 0 wherever target_out is 0 (the reference's
 * uint8 cast makes id 256 background; ids_out agrees with the target).
 * unet_elastic_deform is this call with ids_out = NULL. */
int unet_elastic_deform_ex(const uint8_t* image, const uint16_t* labels, int n, int h, int w,
                           const double* noise, double alpha, double sigma, float* x_out,
                           uint8_t* target_out, uint8_t* image_out, uint16_t* ids_out, void* ws,
                           unet_stream_t stream);

/* Training tiles over the whole frame: n augmented (th x tw) tiles cut from
 * nframes resident (h x w) frames in one warp launch (plus the two Gaussian
 * launches when an elastic field is given).  Sample s reads frame
 * frame_idx[s] (clamped to [0, nframes)); its params row is
 * a00 a01 b0 a10 a11 b1 gain bias.  For tile pixel (ty, tx), all in fp64 and
 * in exactly this order, without fma contraction:
 *   cy = ((a00*ty + a01*tx) + b0) + dy,  cx = ((a10*ty + a11*tx) + b1) + dx
 *   dx|dy = the unet_elastic_deform field of noise (n, 2, th, tw) on the TILE
 *          grid (field 0 -> dx, field 1 -> dy), or 0 when noise is NULL (no
 *          Gaussian launch is made then and ws may be NULL);
 *   extend 0: the coordinate is folded half-sample symmetric (scipy "reflect",
 *          d c b a | a b c d | d c b a), as unet_elastic_deform does;
 *   extend 1: whole-sample symmetric (scipy "mirror", np.pad "reflect",
 *          d c b | a b c d | c b a: what unet_tile_gather feeds the network at
 *          inference): m = fmod(c, 2n-2), + (2n-2) if negative, 2n-2-m if
 *          m > n-1; a length-1 axis gives 0; the neighbour index floor(m)+1
 *          and the nearest index floor(m+0.5) are clamped to n-1;
 *   iv = uint8(bilinear image value), rounded as unet_elastic_deform does;
 *   image_out (n, th, tw) uint8 (may be NULL) = iv;
 *   x_out (n, th, tw) fp32 = (float)min(max(gain*iv + bias, 0), 255) / 255
 *          (the intensity step acts on the rounded uint8; gain 1, bias 0 give
 *          unet_elastic_deform's x);
 *   target_out, ids_out (may be NULL): nearest label, as unet_elastic_deform_ex;
 *   weight_out (n, th, tw) fp32 (may be NULL; needs weights (nframes, h, w)
 *          fp32) = the weight plane at the same nearest index.
 * ws >= unet_tile_warp_ws_bytes(n, th, tw), 8-byte aligned (the two Gaussian
 * planes, as unet_elastic_ws_bytes; 0 for non-positive sizes).  Returns
 * -EINVAL before any device call on non-positive sizes, weight_out without
 * weights, extend outside {0, 1}, a NULL required pointer, and (with noise)
 * sigma <= 0, a radius int(4 sigma + 0.5) > 128 (the Gaussian kernels' LDS
 * rows) or a NULL / misaligned ws. */
size_t unet_tile_warp_ws_bytes(int n, int th, int tw);
int unet_tile_warp(const uint8_t* frames, const uint16_t* labels, const float* weights, int nframes, int h, int w,
                   const int32_t* frame_idx, const double* params, int n, int th, int tw, int extend,
                   const double* noise, double alpha, double sigma, float* x_out, uint8_t* target_out,
                   uint8_t* image_out, uint16_t* ids_out, float* weight_out, void* ws, unet_stream_t stream);

/* Overlap-tile inference (scripts/predict1.py:35-49
 * margin rule): tile t of an nx-wide tile grid has its input origin at
 * ((t / nx) * tile_out - top, (t % nx) * tile_out - left) in the image; a call
 * covers tiles first + b * stride, b < ntiles (stride = world for a round-robin deal).
 * unet_tile_gather: tiles (ntiles, c, tile_in, tile_in) fp32, read from image (c, h, w) with the mirror
 *   padding ("reflect", np.pad semantics incl. pads beyond the image) folded
 *   into the index.
 * unet_tile_scatter: tile logits (ntiles, k, tile_out, tile_out) into the full
 *   logits (k, h, w) (may be NULL) and / or the mask (h, w) uint8 =
 *   255 * (l1 > l0) (k == 2; scripts/predict.py:85-92; may be NULL); output
 *   pixels past the image are dropped. */
int unet_tile_gather(const float* image, int c, int h, int w, int tile_in, int tile_out, int top, int left,
                     int nx, int first, int stride, int ntiles, float* tiles, unet_stream_t stream);
int unet_tile_scatter(const float* tile_logits, int k, int tile_out, int nx, int first, int stride, int ntiles,
                      int h, int w, float* logits, uint8_t* mask, unet_stream_t stream);

/* Sequence inference with symmetry averaging (scripts/predict.py's step on
 * whole frames).  A symmetry code s = r + 4 f (0..7) names
 * S_s(x) = rot90(flip_f(x), r): f = 1 reverses the last axis first, then r
 * quarter turns as torch.rot90(x, r, (-2, -1)).  `work` (ngroups, 2) int32 on
 * the DEVICE holds one (frame, tile) pair per group, the tile numbered as for
 * unet_tile_gather; `codes` is a HOST array of ns codes (1 <= ns <= 8), read
 * during the call.  A group whose frame is outside [0, nframes) or whose tile
 * is negative is skipped.
 * unet_seq_tile_gather: frames (nframes, c, h, w), uint8 (frames_u8 != 0) or
 *   fp32.  tiles (ngroups * ns, c, tile_in, tile_in) fp32: entry g * ns + j is
 *   S_{codes[j]} of the mirror-folded tile of group g (as unet_tile_gather
 *   reads it).  uint8 values are normalised ((v / 255) - 0.5) / 0.5 in fp32
 *   with a correctly rounded division (torchvision's ToTensor + Normalize(0.5,
 *   0.5) bit for bit); fp32 values are copied.
 * unet_seq_tile_reduce: tile_logits (ngroups * ns, k, tile_out, tile_out).  Per
 *   output pixel of a group, for j ascending, the k logits at the position
 *   S_{codes[j]} moved the pixel to give a max-subtracted softmax (expf, sum
 *   over classes ascending, division); the softmaxes are summed in that order
 *   and multiplied by 1 / ns.  Outputs (each may be NULL, not all):
 *   prob (nframes, k, h, w) fp32; mask (nframes, h, w) uint8 =
 *   255 * (mean p1 > threshold), k == 2 only, decided as l1 > l0 when ns == 1
 *   and threshold == 0.5 (unet_tile_scatter's rule, same bits); logits
 *   (nframes, k, h, w), the mapped-back logits, ns == 1 only.  Every output
 *   pixel is written once by one thread (no atomics); pixels past the frame are
 *   dropped, pixels of no listed tile are left untouched.
 * Both return an error, with nothing launched, on non-positive sizes,
 * tile_in < tile_out, ns outside 1..8, a code outside 0..7, c or ngroups above
 * 65535, a mask with k != 2, logits with ns != 1, or no output. */
int unet_seq_tile_gather(const void* frames, int frames_u8, int nframes, int c, int h, int w, int tile_in,
                         int tile_out, int top, int left, int nx, const int32_t* work, int ngroups,
                         const int32_t* codes, int ns, float* tiles, unet_stream_t stream);
int unet_seq_tile_reduce(const float* tile_logits, int k, int tile_out, int nx, const int32_t* work, int ngroups,
                         const int32_t* codes, int ns, int nframes, int h, int w, float threshold, float* prob,
                         uint8_t* mask, float* logits, unet_stream_t stream);

/* Loss weight maps (scripts/preprocess_data.py:17-77 with
 * w0, sigma as its :14-15 = 10, 5): per sample of labels (n, h, w) uint16,
 * weights = fp32(wc) + w0 * exp(-(d1 + d2)^2 / (2 (sigma^2 + 1e-8))) where wc =
 * 1 / (class count / h w) of labels > 0 and d1 = d2 = 0 (the reference's
 * min(edt(obj), edt(!obj)) is identically 0).  weights (n, h, w) fp32 (what
 * utils/dataset.py:111 feeds the loss), weights64 (may be NULL) the fp64 map
 * the reference saves.  ws >= unet_weight_map_ws_bytes(n), 8-byte aligned. */
size_t unet_weight_map_ws_bytes(int n);
int unet_weight_map(const uint16_t* labels, int n, int h, int w, double w0, double sigma, float* weights,
                    double* weights64, void* ws, unet_stream_t stream);

/* Border-aware loss weight maps: the formula above with the U-Net paper's
 * distances instead of the reference's zeros.  For each object l (a distinct
 * non-zero id of a sample) dist_l(p) is the Euclidean distance from pixel p to
 * the nearest pixel of l (0 inside l; scipy's distance_transform_edt(L != l)).
 * d1 <= d2 are the two smallest dist_l(p) over the objects; with one object
 * d2 = 0, with none d1 = d2 = 0 (preprocess_data.py:56-64).  Squared distances
 * are exact int32; d = sqrt((double)d^2) is formed only for the exponential.
 *   weights64 = (double)(float)wc + w0 * exp(-(d1 + d2)^2 / (2 (sigma^2 + 1e-8)))
 *   weights   = (float)weights64
 * weights64, d1sq, d2sq (n, h, w) may be NULL.  Cost and workspace do not
 * depend on the number of objects or on the id values; no host
 * synchronisation; bit-reproducible.  n, h, w >= 1 and h, w <= 16384 (h^2 + w^2
 * must fit int32), else -EINVAL before any launch and a workspace size of 0.
 * ws >= unet_weight_map_border_ws_bytes(n, h, w) (16 B per pixel + counts),
 * 16-byte aligned. */
size_t unet_weight_map_border_ws_bytes(int n, int h, int w);
int unet_weight_map_border(const uint16_t* labels, int n, int h, int w, double w0, double sigma, float* weights,
                           double* weights64, int32_t* d1sq, int32_t* d2sq, void* ws, unet_stream_t stream);

/* Post-processing (utils/metrics.py):
 * unet_instance_masks: get_instance_masks (:42-72) for n masks (h, w) uint8
 *   (> 0 = foreground): 8-connected components numbered 1, 2, ... in raster
 *   order of their first pixel (skimage.measure.label(connectivity=2)), those
 *   with fewer than min_size pixels set to 0 without renumbering
 *   (remove_small_objects), uint16 labels out.  n h w < 2^31.
 * unet_rand_index: calculate_rand_index_and_error (:75-139) of two uint16
 *   labelings (h, w): out[0] = Rand index, out[1] = Rand error (fp64, device);
 *   up to 2^24 (gt label, pred label) pairs; synchronises the stream once. */
size_t unet_instance_masks_ws_bytes(int n, int h, int w);
int unet_instance_masks(const uint8_t* mask, int n, int h, int w, int min_size, uint16_t* labels, void* ws,
                        unet_stream_t stream);
size_t unet_rand_index_ws_bytes(int h, int w);
int unet_rand_index(const uint16_t* gt, const uint16_t* pred, int h, int w, double* out, void* ws,
                    unet_stream_t stream);

/* Cell tracking (scripts/track.py:103-275): a tracker
 * consumes the instance labelings of a sequence frame by frame and keeps the
 * lineage (CellTrack :27-36).  Per frame the GPU builds the overlap table of
 * the previous and current objects in one pass (replacing calculate_mask_iou,
 * :73-100, per object pair); the host side runs the reference's control flow:
 * IoU cost matrix (1 - IoU, 1000 where no overlap), linear sum assignment,
 * links with IoU >= iou_track, divisions (an unmatched parent overlapping 2..
 * max_children unmatched objects with IoU >= iou_division), new tracks.
 *   unet_tracker_create(h, w, 0.3, 0.1, 2) = the reference's constants
 *     (:21-24).  NULL for bad sizes.
 *   unet_tracker_add_frame: labels (h, w) uint16 on the device; frame = the
 *     frame number (the reference parses it from mXXX.tif); synchronises the
 *     stream; ws >= unet_tracker_ws_bytes(h, w) bytes, kept for the whole
 *     sequence (it holds the previous frame).
 *   unet_tracker_step_host: the same step from host data -- the current
 *     objects' labels (ascending, > 0), areas, and the overlap counts
 *     inter[i * n_curr + j] with the previous step's objects (NULL on the
 *     first frame).  Host only (no device work).
 *   unet_tracker_tracks: writes up to cap rows (label, start, end, parent) in
 *     the res_track.txt order (start frame, then label; end >= start);
 *     returns the track count.  A root track's parent is -1 as the reference
 *     writes it; the Cell Tracking Challenge's res_track.txt writes 0 there.
 *   Frame maps: for every frame it was given (by either step function) the
 *     tracker keeps the frame number, the frame's ascending object labels and,
 *     per label, the id of the track that holds it when that frame's step ends
 *     (active_tracks_by_obj_label[label] after the step; 0 = the object holds
 *     no track).  A few bytes per object, kept for the tracker's life.
 *     unet_tracker_num_frames: the number of maps.  unet_tracker_frame_map:
 *     map `index` in the order the frames were given; writes the frame number
 *     and up to cap (label, track id) pairs, returns the object count; any
 *     output pointer may be NULL; -EINVAL for a bad index.  Host only.
 *   unet_tracker_set_label_scope: UNET_TRACK_SCOPE_SHARED (default) keeps the
 *     reference's single dictionary for the labels of the previous and the
 *     current frame, with its quirk: a link "previous 3 -> current 4" followed
 *     by "previous 4 -> current 5" takes the track from current object 4
 *     again, which then holds none.  UNET_TRACK_SCOPE_FRAME reads and deletes
 *     previous-frame labels in the table the previous step left and assigns
 *     current-frame labels in a fresh one, which becomes "previous" when the
 *     step ends; the step is otherwise the same.  -EBUSY once a frame was
 *     given, -EINVAL for another value.
 *   unet_tracker_relabel: labels and out (n, h, w) uint16 on the device (h, w
 *     the tracker's), host_frames the n frame numbers.  out[i] = labels[i]
 *     with every pixel replaced by the track id its label holds in the map of
 *     frame host_frames[i] (the last one given under that number); background,
 *     a label the map does not list and an object without a track give 0.
 *     out == labels (in place) is allowed; any other overlap is not.  The
 *     result is a Cell Tracking Challenge mask stack (mask%03d.tif).
 *     One kernel launch for the whole stack: the tables of all n frames go
 *     up in one copy, after which the stream is synchronised once (the host
 *     staging buffer lives in the tracker and is rewritten by the next call),
 *     then the launch; no per-frame launch or synchronisation.  The kernel
 *     streams 16 bytes (8 pixels) per lane with scalar head and tail pixels
 *     where a frame does not start on 16 bytes; each frame has one dense uint16
 *     table of L entries, L = 1 + the highest label in the n maps rounded up
 *     to 8, which a workgroup stages in LDS while L <= 8192 (16 KiB, so 8
 *     workgroups of 256 lanes still share a CU's 160 KiB) and reads through L2
 *     beyond.
 *     ws >= unet_tracker_relabel_ws_bytes(n, h, w) bytes, 256-byte aligned:
 *     n tables x 65,536 entries x 2 B (labels up to 65,535), rounded up to
 *     256 B; 0 for n, h or w < 1.
 *     Errors are returned before any device work, so before any pointer is
 *     touched: -EINVAL (null or misaligned pointers, n < 0, a stack of more
 *     than 2^31 - 1 workgroups of 8,192 pixels), -ENOENT (a frame number that was never given; unet_last_error()
 *     names it), -ERANGE (one of the n maps holds a track id above 65,535,
 *     which a 16-bit mask cannot carry); -EIO for a HIP error.  n = 0: 0.
 *   unet_tracker_relabel_launches: relabel kernel launches of this process
 *     so far (reset != 0 clears the count after reading it).
 *   unet_tracker_load_result (host only): gives a tracker that was given no
 *     frame the tracks and frame maps of another linker (unet_link_assemble):
 *     rows (n_rows x 4: id, start, end, parent; row q carries id q + 1, parent
 *     -1 = root), frames (n_frames numbers, strictly ascending), and for frame
 *     f the ascending labels[map_offsets[f] .. map_offsets[f + 1]) with their
 *     track ids (0 = none).  Afterwards unet_tracker_tracks, _frame_map and
 *     _relabel serve the loaded result.  -EBUSY for a tracker that already has
 *     frames, -EINVAL for anything else that does not hold.
 * unet_linear_sum_assignment: scipy.optimize.linear_sum_assignment's
 *   minimisation on a row-major nr x nc fp64 cost matrix (host pointers,
 *   min(nr, nc) pairs sorted by row); -EINVAL for NaN / -inf / infeasible. */
typedef struct unet_tracker unet_tracker;
unet_tracker* unet_tracker_create(int h, int w, double iou_track, double iou_division, int max_children);
void unet_tracker_destroy(unet_tracker* t);
size_t unet_tracker_ws_bytes(int h, int w);
int unet_tracker_add_frame(unet_tracker* t, const uint16_t* labels, int frame, void* ws, unet_stream_t stream);
int unet_tracker_step_host(unet_tracker* t, int frame, int n_curr, const int32_t* host_labels,
                           const int64_t* host_areas, const int64_t* host_inter);
int unet_tracker_num_tracks(const unet_tracker* t);
int unet_tracker_tracks(const unet_tracker* t, int32_t* host_out, int cap);
enum { UNET_TRACK_SCOPE_SHARED = 0, UNET_TRACK_SCOPE_FRAME = 1 };
int unet_tracker_set_label_scope(unet_tracker* t, int scope);
int unet_tracker_num_frames(const unet_tracker* t);
int unet_tracker_frame_map(const unet_tracker* t, int index, int32_t* host_frame, int32_t* host_labels,
                           int32_t* host_track_ids, int cap);
size_t unet_tracker_relabel_ws_bytes(int t, int h, int w);
int unet_tracker_relabel(unet_tracker* t, const uint16_t* labels, const int32_t* host_frames, int n, uint16_t* out,
                         void* ws, unet_stream_t stream);
long long unet_tracker_relabel_launches(int reset);
int unet_tracker_load_result(unet_tracker* t, const int32_t* host_rows, int n_rows, const int32_t* host_frames,
                             int n_frames, const int32_t* host_map_offsets, const int32_t* host_labels,
                             const int32_t* host_ids);
int unet_linear_sum_assignment(long long nr, long long nc, const double* host_cost, int64_t* host_row_ind,
                               int64_t* host_col_ind);

/* Cell Tracking Challenge measures (the reference's README step 8 and its
 * EvaluationSoftware/{Win,Mac}/{SEG,DET,TRA}Measure binaries, whose Linux
 * builds are absent): SEG, DET and TRA of a 2-D result sequence against its
 * ground truth.  The GPU builds the sparse overlap records of whole stacks of
 * frame pairs, chunk by chunk: 2 + 2 R kernel launches and 1 + R stream
 * synchronisations per chunk of frames, where R, the rounds the chunk's tables
 * take through the workspace, is 1 unless the frames need more than
 * unet_ctc_ws_bytes provides for (below); a round that yields more than
 * 65,536 overlap records takes one more synchronisation.  The host side, plain
 * C++, matches objects, builds the two acyclic oriented graphs and counts the
 * operations.
 *   Matching: in a frame, result object S matches reference object R iff
 *     2 |R and S| > |R| (integers, strict).
 *   SEG: mean over the reference objects of the SEG frames of
 *     |R and S| / |R or S| for the matching S, 0 without one.
 *   Graphs (TRA frames): a vertex is a (frame, label) pair present in the
 *     image.  Per track row "L B E P", in the table's order: if P != 0 the
 *     parent link from P's last present vertex to L's first, then the track
 *     links between L's consecutive present vertices within [B, E].
 *   Operations: NS = m - 1 for a RES vertex matched by m > 1 GT vertices, FN =
 *     unmatched GT vertex, FP = unmatched RES vertex; with "unique" = matched
 *     by exactly one GT vertex: ED = RES edge with both ends unique and no GT
 *     edge between their GT vertices, EC = such an edge whose GT edge has the
 *     other kind, EA = GT edge without (both ends matched, both RES vertices
 *     unique, RES edge between them).
 *   AOGM = 5 NS + 10 FN + FP + ED + 1.5 EA + EC; AOGM0 = 10 |V_GT| + 1.5 |E_GT|;
 *   TRA = 1 - min(AOGM, AOGM0) / AOGM0; DET the same from the vertex terms and
 *     10 |V_GT| alone.
 *   unet_ctc_add_frames: t frame pairs gt[i], res[i] of (h, w) uint16 labels
 *     (any value 0..65535, 0 = background) on the device, frame numbers on the
 *     host; kind UNET_CTC_SEG or UNET_CTC_TRA; ws >= unet_ctc_ws_bytes(t, h, w)
 *     bytes, 256-byte aligned; h w < 2^31.  Synchronises the stream.  t = 0
 *     only records (and checks) the frame size.  All or none: where the call
 *     fails, also in a later chunk, the evaluator holds none of its frames.  -EINVAL where h, w differ
 *     from an earlier call's ("the stacks' sizes differ").
 *   unet_ctc_ws_bytes(t, h, w), with c = min(t, 1024), k = min(t,
 *     "ctc_chunk_frames" as set at the time of the call) and P = h w:
 *     c x (4 B + 2 x 8 KB bitmaps + 2 x 8 KB prefix + 8 B counts + 32 B
 *     descriptor) + a table region of max(8 B x pow2ceil(2 P), k x 256 KB) +
 *     16 B x (1 + max(P, 4096, k x 16384)) records, each part rounded up to
 *     256 B.  A frame is charged n = min((n_gt + 1)(n_res + 1), its runs of
 *     equal non-background (gt, res) keys along 16-pixel pieces, P) records,
 *     and a table of 4 B x (n_gt + 1)(n_res + 1) (dense) or 8 B x pow2ceil(2 n)
 *     (hashed).  A chunk passes in one round while the charges of its frames
 *     fit both regions -- always for frames of up to 16,384 such runs, the
 *     size the regions allow per chunk frame; any single frame fits alone, so
 *     at worst a round holds one frame.
 *   unet_ctc_add_frame_host: the same frame from host tables, no device work:
 *     ascending labels (1..65535) and areas of both sides and n_pairs rows
 *     (gt label, res label, |and|) of int64.  n_res < 0 states that the GT
 *     frame has no RES frame: -ENODATA.
 *   unet_ctc_set_tracks: rows (label, begin, end, parent) of man_track.txt
 *     (UNET_CTC_GT) or res_track.txt (UNET_CTC_RES), host, in file order.
 *   unet_ctc_measures: out[3] = SEG, DET, TRA (NaN where nothing was added for
 *     a measure, TRA also while a side has no track table); counts[8] = NS, FN,
 *     FP, ED, EA, EC, |V_GT|, |E_GT| (may be NULL).  -ENOENT: a label occurs
 *     in an image but has no track row; -ESRCH: a parent id has no row;
 *     unet_last_error() names the side, frame and label.
 *   unet_ctc_log: the text of the evaluator's TRA_log.txt (six sections, the
 *     rule, "TRA measure: %.6f"); copies up to cap - 1 bytes + NUL, returns
 *     the full size including the NUL, or -errno as unet_ctc_measures.
 *   unet_ctc_num_frames / _frame_sizes (out[4] = frame number, n_gt, n_res,
 *     n_pairs) / _frame_tables: read a stored frame back (frames are ordered
 *     by frame number once measures or the log were asked for, by insertion
 *     before); any output pointer may be NULL.
 *   unet_ctc_stats: out[6] = chunks, kernel launches (2 per chunk + 2 per
 *     round), stream synchronisations, frames counted densely, frames counted
 *     by hash, overlap records read.
 * Tuning: "ctc_chunk_frames" and "ctc_dense_cells" of unet_set_tuning. */
enum { UNET_CTC_SEG = 0, UNET_CTC_TRA = 1 };
enum { UNET_CTC_GT = 0, UNET_CTC_RES = 1 };
typedef struct unet_ctc unet_ctc;
unet_ctc* unet_ctc_create(void);
void unet_ctc_destroy(unet_ctc* c);
size_t unet_ctc_ws_bytes(int t, int h, int w);
int unet_ctc_add_frames(unet_ctc* c, int kind, const uint16_t* gt, const uint16_t* res, const int32_t* host_frames,
                        int t, int h, int w, void* ws, unet_stream_t stream);
int unet_ctc_add_frame_host(unet_ctc* c, int kind, int frame, int n_gt, const int32_t* host_gt_labels,
                            const int64_t* host_gt_areas, int n_res, const int32_t* host_res_labels,
                            const int64_t* host_res_areas, int n_pairs, const int64_t* host_pairs);
int unet_ctc_set_tracks(unet_ctc* c, int side, const int32_t* host_rows, int n);
int unet_ctc_measures(unet_ctc* c, double* host_out, int64_t* host_counts);
long long unet_ctc_log(unet_ctc* c, char* buf, size_t cap);
int unet_ctc_num_frames(const unet_ctc* c, int kind);
int unet_ctc_frame_sizes(const unet_ctc* c, int kind, int index, int32_t* host_out);
int unet_ctc_frame_tables(const unet_ctc* c, int kind, int index, int32_t* host_gt_labels, int64_t* host_gt_areas,
                          int32_t* host_res_labels, int64_t* host_res_areas, int64_t* host_pairs);
int unet_ctc_stats(const unet_ctc* c, int64_t* host_out);

/* Per-object measurements of a label stack (scripts/track.py:39-70
 * get_mask_properties is an np.argwhere per label and frame): one record per
 * object per frame, ordered by frame, then by ascending label (np.unique's
 * order).  labels (n, h, w) uint16 on the device, 0 = background; image NULL
 * or (n, h, w) uint8 on the device.
 *   frame: index in the stack; label; area: pixels.
 *   sum_y, sum_x, sum_yy, sum_xx, sum_xy: sums of the row index y, the column
 *     index x and their products over the object's pixels.
 *   min_y, min_x, max_y, max_x: inclusive extent (track.py:61-62).
 *   boundary: pixels with a 4-neighbour that carries another label (background
 *     included) or lies outside the frame.
 *   edge: pixels in the first or last row or column.
 *   contact: ordered 4-neighbour pairs (p, q), p in the object, q in a
 *     different non-background object.
 *   sum_v, sum_vv, min_v, max_v: sums of the intensity and its square, and its
 *     extremes, over the object's pixels; all 0 without an image.
 *   reserved fields are 0.
 * Every field is an integer, so the records are bit-equal from run to run.
 *   unet_region_props: frame_offsets (n + 1 int32, device): the records of
 *     frame f are [frame_offsets[f], frame_offsets[f + 1]).  records: cap
 *     records on the device (NULL with cap 0).  One host synchronisation,
 *     after the index phase: *host_total (host, never NULL) receives the
 *     object total; with total > cap the call returns -ENOSPC before it
 *     touches records, frame_offsets valid.  ws >= unet_region_props_ws_bytes
 *     (n x 16 KB + n x 4 B, each part rounded up to 256), 256-byte aligned.
 *     Then two launches: the records' headers and neutral values, and one
 *     accumulate launch over the whole stack (unet_region_props_launches
 *     counts the latter; reset != 0 also zeroes the count).
 *   unet_region_props_host: the same records from host arrays into host
 *     arrays, in plain loops, no device call.
 * -EINVAL before any device call (and a workspace size of 0) for n < 0, h or
 * w < 1 or > 32768, h w > 2^30, cap < 0, n min(65535, h w) >= 2^31, a null or
 * misaligned pointer: inside these limits no sum passes 63 bits.
 * Tuning: "region_lds_objects" of unet_set_tuning. */
typedef struct unet_region_record {
  int32_t frame, label, area, boundary, edge, min_y, min_x, max_y, max_x, min_v, max_v, reserved0;
  int64_t sum_y, sum_x, sum_yy, sum_xx, sum_xy, sum_v, sum_vv, contact, reserved1[2];
} unet_region_record; /* 128 bytes */
size_t unet_region_props_ws_bytes(int n, int h, int w);
int unet_region_props(const uint16_t* labels, const uint8_t* image, int n, int h, int w, int32_t* frame_offsets,
                      unet_region_record* records, long long cap, long long* host_total, void* ws,
                      unet_stream_t stream);
int unet_region_props_host(const uint16_t* host_labels, const uint8_t* host_image, int n, int h, int w,
                           int32_t* host_frame_offsets, unet_region_record* host_records, long long cap,
                           long long* host_total);
long long unet_region_props_launches(int reset);

/* Distance-based linker ("Distance-based linker", has the
 * definitions): the objects of consecutive frames of a region table are
 * assigned to each other by the squared distance of their quantised centroids.
 *   Quantised centroid, 1/16 pixel: qy = floor((32 sum_y + area) / (2 area)),
 *     qx likewise.  d(i, j) = dqy^2 + dqx^2 in int64.  gate_q = round(16 gate),
 *     g2 = gate_q^2; a pair is permitted iff d <= g2.
 *   Pair f = frames (f, f + 1) of the table, P previous and C current objects
 *     in ascending label order: a P x (C + P) assignment problem, entry
 *     (i, j < C) = d(i, j) where permitted, entry (i, C + i) = g2 (row i's
 *     private "no successor" column), every other entry absent; every row
 *     assigned, least total.  Solved by shortest augmenting paths (Crouse 2016)
 *     with rows in ascending order, int64 duals, the strict update r <
 *     shortest[j], and the next column taken among the unscanned columns of
 *     least distance (a) unassigned before assigned, (b) lowest index -- the
 *     algorithm is part of the definition, since the optimum need not be unique.
 *   unet_link_frames: records / frame_offsets (n + 1) as unet_region_props
 *     leaves them on the device, total = frame_offsets[n] (the host_total of
 *     that call).  Outputs on the device, indexed by record: prev[r] = the
 *     record of the linked predecessor of current object r or -1 (frame 0: all
 *     -1); dist[r] = that link's d or -1; mother[r], for a current object
 *     without predecessor (a birth) and division_gate_q > 0 = the record of the
 *     previous object i with the least d(i, r) <= division_gate_q^2 among those
 *     that have a linked successor (ties to the lowest i), else -1;
 *     pair_total[f] (max(n - 1, 0) int64) = the optimal total of pair f.
 *     One launch for the whole sequence, one workgroup of 256 lanes per frame
 *     pair (unet_link_launches counts the launches of this process; reset != 0
 *     also zeroes the count); no host synchronisation.  A workgroup computes
 *     the centroids of its two frames in its prologue and keeps them with the
 *     duals, shortest, path, col4row, row4col and the scanned flags in LDS
 *     (33 bytes per object + 12 per previous object) where P + C is at most
 *     "link_lds_objects" of unet_set_tuning, in ws otherwise -- the same code
 *     and the same bytes.  The cost matrix is never stored.
 *     ws >= unet_link_ws_bytes(n, total), 256-byte aligned: nine arrays of
 *     16, 16, 8, 8, 8, 4, 8, 8 and 2 bytes x total, each rounded up to 256;
 *     0 for n < 2 or total = 0 (ws may then be NULL).
 *     n = 0 launches nothing; n = 1 only fills frame 0; frames without objects
 *     are valid.
 *   unet_link_frames_host: the same outputs from host records into host
 *     arrays: plain loops over the explicit matrix, no device call.
 *   unet_link_assemble (host only): chains the links into tracks.  frames: the
 *     n frame numbers, strictly ascending.  Frames in order, objects in
 *     ascending label order: a previous object i with successor k and claimants
 *     {j : mother[j] = i} divides when max_children >= 2 and a claimant passes
 *     min(area_k, area_j) / max(area_k, area_j) >= division_min_ratio; of the
 *     passing claimants up to max_children - 1 are taken, nearest first, ties
 *     to the lowest label; then k and the taken claimants start tracks whose
 *     parent is i's track, which ends in the previous frame.  Every other birth
 *     starts a root track, every other linked object extends its predecessor's.
 *     Ids are 1, 2, ... in that order.  rows: up to rows_cap rows (id, start,
 *     end, parent; -1 = root), total rows at most; ids: the track id of every
 *     record (with frame_offsets and the records' labels these are the
 *     per-frame label -> track maps).  Returns the number of tracks.
 *   -EINVAL before any device call: n < 0, total < 0 or >= 2^30, gate_q outside
 *   [1, 65535], division_gate_q outside [0, 65535], a null or misaligned
 *   pointer (frame_offsets, prev, mother 4 bytes; dist, pair_total 8; records
 *   16; ws 256), frame numbers that do not ascend strictly (assemble). */
size_t unet_link_ws_bytes(int n, long long total);
int unet_link_frames(const unet_region_record* records, const int32_t* frame_offsets, int n, long long total,
                     int gate_q, int division_gate_q, int32_t* prev, int64_t* dist, int32_t* mother,
                     int64_t* pair_total, void* ws, unet_stream_t stream);
int unet_link_frames_host(const unet_region_record* host_records, const int32_t* host_frame_offsets, int n,
                          long long total, int gate_q, int division_gate_q, int32_t* host_prev, int64_t* host_dist,
                          int32_t* host_mother, int64_t* host_pair_total);
long long unet_link_launches(int reset);
int unet_link_assemble(const unet_region_record* host_records, const int32_t* host_frame_offsets, int n,
                       const int32_t* host_frames, const int32_t* host_prev, const int64_t* host_dist,
                       const int32_t* host_mother, double division_min_ratio, int max_children, int32_t* host_rows,
                       int rows_cap, int32_t* host_ids);

/* Warping error and pixel error (Jain et al., "Boundary learning by
 * optimization with topological constraints", CVPR 2010; the measures the
 * U-Net paper ranks by; utils/metrics.py ends in a calculate_warping_error
 * placeholder).  gt (n, h, w) uint16 instance ids, pred (n, h, w) uint8 with
 * > 0 = foreground (T); all on the device.
 *   G0: separate == 0: gt > 0; else gt > 0 and no in-frame pixel of the 3x3
 *     neighbourhood carries another non-zero id (a background ridge between
 *     touching cells).
 *   Foreground is 8-connected, background 4-connected; outside the frame is
 *     background and never flips.  A pixel is simple iff the foreground of its
 *     8-neighbourhood N* is one 8-connected component and exactly one
 *     4-connected background component of N* is 4-adjacent to it: a function
 *     of the 8 neighbour bits (bit k = neighbour k of N, NE, E, SE, S, SW, W,
 *     NW), which unet_simple_point_table writes as out[256] of 0 / 1 (116
 *     ones; host only, built from the definition).
 *   Mask M: the pixels whose (2 radius + 1)^2 window, clipped to the frame,
 *     holds both a foreground and a background pixel of G0; radius -1 = the
 *     whole frame, 0 = empty.
 *   Schedule: L = G0; one sweep is four sub-steps s = 0..3, each flipping at
 *     once every pixel with y & 1 == s >> 1, x & 1 == s & 1, in M, L != T and
 *     simple in L as it stands when the sub-step starts.  The loop ends after
 *     a sweep without a flip, or after max_sweeps sweeps (0 = no limit).
 *   counts (device, n x 5 int64): pixel error |G0 != T|, warping error
 *     |L != T| over the frame, flips, sweeps run (the last, empty one
 *     included), converged (1 iff the last sweep flipped nothing).  pixel
 *     error - warping error == flips.
 *   warped (may be NULL): (n, h, w) uint8, the final L as 0 / 1.
 * One workgroup per frame, one launch, no host synchronisation.  The frame's
 * four bit planes live in LDS where they fit (4 (h + 2)(ceil(w / 32) + 2)
 * words within 160 KB: 512 x 512 does), else -- or with UNET_WARP_FORCE_WS in
 * flags -- in ws (>= unet_warping_error_ws_bytes, 256-byte aligned; may be
 * NULL where the planes fit LDS and the flag is clear).
 * -EINVAL before any launch (and a workspace size of 0) for n, h or w < 1,
 * radius < -1 or > 255, max_sweeps < 0, n h w >= 2^31. */
enum { UNET_WARP_FORCE_WS = 1 };
size_t unet_warping_error_ws_bytes(int n, int h, int w);
int unet_warping_error(const uint16_t* gt, const uint8_t* pred, int n, int h, int w, int radius, int separate,
                       int max_sweeps, int flags, uint8_t* warped, int64_t* counts, void* ws, unet_stream_t stream);
void unet_simple_point_table(uint8_t out[256]);

/* Marker-seeded instance masks: unet_instance_masks with touching cells split
 * (the reference's README leaves "instance separation" to a post-processing
 * it does not have).  mask (n, h, w) uint8 on the device; all numbering is
 * per frame.
 *   fg = mask > 0.
 *   d2(p): exact squared Euclidean distance from foreground pixel p to the
 *     nearest background pixel inside the frame (outside the frame is not
 *     background: scipy.ndimage.distance_transform_edt); 0 on background;
 *     2^30 everywhere in a frame without a background pixel.
 *   Marker set: markers == NULL: fg & (d2 >= core_d2), 0 <= core_d2 <= 2^30;
 *     else (markers > 0) & fg (core_d2 is then ignored, d2 computed only if
 *     asked for).  Marker labels: its 8-connected components, numbered 1, 2,
 *     ... in raster order of their first pixel.
 *   Growth: with keys (dist, label) in lexicographic order, (0, label) on
 *     markers, the least fixed point of key(p) = min(key(p), key(q) + (1, 0))
 *     over the foreground 8-neighbours q of foreground p: every foreground
 *     pixel connected to a marker takes the label of the marker at the
 *     smallest 8-connected geodesic distance within fg, the smallest label
 *     among equals.  A foreground component without a marker stays one
 *     segment.
 *   labels (uint16): the segments numbered 1, 2, ... in raster order of their
 *     first pixel; those under min_size pixels set to 0 without renumbering.
 *   d2 (may be NULL): (n, h, w) int32.
 *   info (n x 4 int32): markers, segments before the min_size cut, the largest
 *     geodesic distance assigned, overflow (non-zero when markers or segments
 *     exceed 65535; the frame's labels are then unspecified).  The keys are
 *     64-bit (distance and label 32 bits each), so the distance cannot
 *     saturate.
 * With core_d2 == 0 the labels equal unet_instance_masks's.  One workgroup per
 * frame grows the labels by in-place directional sweeps (down, up, right,
 * left) until one round changes nothing, in one launch; the fixed point is
 * unique, so the result does not depend on the schedule
 * (unet_set_tuning("split_threads", t) sets the workgroup's size).  No host
 * synchronisation.  ws >= unet_split_instances_ws_bytes(n, h, w), 256-byte
 * aligned.  -EINVAL before any launch (and a workspace size of 0) for n, h or
 * w < 1, h or w > 16384, n > 65535, n h w >= 2^31, core_d2 outside [0, 2^30]
 * (markers == NULL), min_size < 0, a null mask / labels / info / ws. */
size_t unet_split_instances_ws_bytes(int n, int h, int w);
int unet_split_instances(const uint8_t* mask, const uint8_t* markers, int n, int h, int w, int core_d2, int min_size,
                         uint16_t* labels, int32_t* d2, int32_t* info, void* ws, unet_stream_t stream);

/* Tuning hooks, process-global:
 *  "autotune"      1 (default, or env UNET_AUTOTUNE) = the plan times the
 *                  applicable GEMM variants (tile shape, split-K, wgrad pixel
 *                  split) the first time it meets a GEMM shape and caches the
 *                  fastest per shape; 0 = built-in heuristic only.
 *  "igemm_variant" heuristic override for A/B measurements (-1 = off, 1..9 =
 *                  forced tile shape; 21-26, 31-36, 41-44 bf16 tiles, 63,
 *                  65-68 bf16 halo tiles with LDS-DMA weights; 70-72, 74 fp32
 *                  Winograd: F(2x2,3x3), F(4x4,3x3), fused F(4x4,3x3),
 *                  F(6x6,3x3), plan GEMMs only -- they need the plan's
 *                  scratch); "wgrad_variant"
 *                  (-1 = off, 1 = 64x64 tile, 2..9 = workgroups per CU for the
 *                  pixel split; bf16 GEMMs: 10-14, 20-21 = forced bf16 tile;
 *                  22-23 fp32 halo tiles; 71 / 74 = Winograd F(4x4,3x3) /
 *                  F(6x6,3x3) weight gradient, plan GEMMs only; 1071 / 1074
 *                  the same in slab mode; 100-104 = fp32 pixel-column tile
 *                  0-4 in slab mode; 110-114 / 126-133 bf16 slab modes);
 *  "wino_max"      largest fp32 Winograd output tile the autotuner may pick
 *                  for forward / input-gradient GEMMs (env UNET_WINO_MAX): 6 =
 *                  F(6x6) and below, 4 (default) = F(4x4) / F(2x2), 2 = F(2x2)
 *                  only, 0 = direct GEMMs only; "wino_wgrad_max" (env
 *                  UNET_WINO_WGRAD_MAX, default 6) the same for weight gradients.
 *  "concurrent"    1 (default, or env UNET_CONCURRENT) = a plan's backward
 *                  runs the weight-gradient GEMMs on a side stream beside the
 *                  dX chain (joined before the call returns); 0 = one stream.
 *  "bf16_norm"     1 (or env UNET_BF16_NORM=1; default 0) = UNET_PREC_BF16 plans
 *                  created afterwards write relu(bn(y)) of every layer once
 *                  as a bf16 tensor, the plain operand of its GEMM consumers
 *                  (LDS-DMA staging; tiles 81-84 need it); 0 = consumers apply
 *                  BatchNorm + ReLU while staging.
 *  "bn_fold"       1 (default, or env UNET_BN_FOLD) = eval forwards fold each
 *                  BatchNorm into its conv (weights x gamma / sqrt(var + eps),
 *                  bias x that + beta - mean x that) and store relu(conv') in
 *                  the GEMM epilogue; 0 = consumers apply BN + ReLU on load.
 *  "force_split"   k > 1: every plan igemm runs split-K k (tests), 0 = off.
 *  "force_tile"    id > 0: every plan igemm whose shape admits tile id runs
 *                  it (tests; 1-4, 6-9 register-staged, 11-14 LDS-DMA, 51-54
 *                  fp32 halo, 70-72 / 74 fp32 Winograd, 21-26 / 31-36 / 63-67
 *                  / 81-84 bf16 operands -- only in UNET_PREC_BF16 / _BF16X3
 *                  plans).
 *  "op_precision"  UNET_PREC_* of the per-op GEMM entry points below
 *                  (unet_conv3x3_*, unet_convT2_*); default fp32.
 *  "op_a16"        1 = with op_precision UNET_PREC_BF16, unet_conv3x3_fwd /
 *                  _dgrad store their A operand bf16 first (x rounded before
 *                  the BN+ReLU transform; padded dY bf16), as a bf16 plan
 *                  does -- the configuration the 61-66 tiles (bf16-stored A
 *                  only) run in; 0 (default) = fp32 A.
 *  "op_strict"     1 = a per-op GEMM entry point (unet_conv3x3_fwd / _dgrad,
 *                  unet_convT2_fwd / _bwd, unet_gemm_site_run) whose forced tile
 *                  ("igemm_variant" > 0, or the descriptor's tile / split)
 *                  does not apply to the call returns -EINVAL before it
 *                  launches anything; 0 (default) = the built-in tile runs in
 *                  its place, silently.  Tests set it to know which tile ran.
 *  "deterministic" 1 (or env UNET_DETERMINISTIC=1; default 0) = every weight
 *                  gradient runs a variant without fp32 atomics (slab
 *                  partials summed in a fixed order) and inc.c0's slab
 *                  reduction runs in one pass: plan steps are
 *                  bit-reproducible run to run (see
 *                  unet_nondeterministic_sites).
 *  "bnb_fuse"      1 (default; env UNET_BNB_FUSE) = fp32 plans form the
 *                  BatchNorm-backward dY of a layer whose weight gradient runs
 *                  Winograd F(6x6) in one pass with that weight gradient's dY
 *                  transform (see unet_fused_bnb_sites; read for the workspace
 *                  layout at plan creation); 0 = the two-pass form
 *                  (bit-identical results).
 *  "wgrad_early_u" 1 (default; env UNET_WGRAD_EARLY_U) = the Winograd weight
 *                  gradients' input transform is issued on the side stream
 *                  before the wait for the layer's dY; 0 = after it
 *                  (bit-identical results).
 *  "wgrad_plane"   1 (default; env UNET_WGRAD_PLANE) = the batched point GEMMs
 *                  of the fp32 Winograd weight gradients run k_wgrad_plane
 *                  (LDS-DMA ring) where their tile has one; 0 = k_wgrad
 *                  (bit-identical results for the same tile and split).
 *  "wgrad_oihw"    1 (default; env UNET_WGRAD_OIHW) = fp32 plans' Winograd
 *                  weight gradients store torch's OIHW gradient from their
 *                  output transform (see unet_wgrad_oihw_sites); 0 = packed
 *                  store + permute (bit-identical results).
 *  "igemm_plane"   1 (default; env UNET_IGEMM_PLANE) = the batched point GEMMs
 *                  of the unfused fp32 Winograd forward / input-gradient tiles
 *                  (70, 71) run k_igemm_plane (LDS-DMA ring) where their tile
 *                  has one (1, 2, 3, 8, 9; see unet_igemm_plane_launches);
 *                  0 = k_igemm (bit-identical results for the same tile).
 *  "wino_persist"  1 (default; env UNET_WINO_PERSIST) = the fused fp32 Winograd
 *                  tiles 76 and 75 run their persistent form: one workgroup
 *                  per CU walks the tile groups, claimed through counters in
 *                  the workspace, and loads the next group's first operands
 *                  under the current group's output stage (see
 *                  unet_wino_persist_launches); 0 = one workgroup per group
 *                  (bit-identical results).
 *  "wino_persist_wgs" n (tests; default -1 = one per CU): workgroups of the
 *                  persistent form's grid.
 *  "wino_point_tile" id (tests; default -1 = off): the unfused Winograd tiles
 *                  run their point GEMMs on register-staged tile id (1-4, 6-9)
 *                  where it fits, instead of the tuned or heuristic one.
 *  "ctc_chunk_frames" frames per chunk of unet_ctc_add_frames (1..1024; -1 =
 *                  the default, 32); unet_ctc_ws_bytes reads it.
 *  "ctc_dense_cells" largest (n_gt + 1)(n_res + 1) that unet_ctc_add_frames
 *                  counts in a dense LDS table (0..8192, 0 = every frame by
 *                  hash; -1 = the default, 4096).
 *  "region_lds_objects" most objects of a frame that unet_region_props
 *                  collects in its LDS table before the global atomics
 *                  (0..512, 0 = every frame straight to global atomics; -1 =
 *                  the default, 512; same records for every value).
 *  "link_lds_objects" most objects P + C of a frame pair that unet_link_frames
 *                  serves from LDS (0..3600, 0 = every pair from the workspace;
 *                  -1 = the default, 3600: what 160 KB hold; same bytes for
 *                  every value).
 *  "split_threads" t (tests; 64..1024, a multiple of 64; -1 = the default,
 *                  1024): threads of unet_split_instances's growth workgroup
 *                  (same bits for every value). */
int unet_set_tuning(const char* key, int value);
/* Text report of the tuned GEMM choices (one line per shape: key, heuristic
 * time, chosen variant and time).  Copies up to len-1 bytes + NUL into buf
 * (buf may be NULL); returns the full report size including the NUL. */
size_t unet_tuning_report(char* buf, size_t len);
/* Forget every tuned choice (the next plan run re-tunes). */
int unet_tuning_reset(void);
/* Slab-mode weight gradients (tuned or forced) that fell back to atomic
 * accumulation because their split partials exceeded the plan's slab; reset
 * != 0 also zeroes the count. */
long long unet_slab_fallbacks(int reset);
/* Deterministic mode (unet_set_tuning("deterministic", 1) or
 * UNET_DETERMINISTIC=1): weight-gradient launch sites that found no
 * atomic-free variant and ran with fp32 atomics; reset != 0 also zeroes the
 * count.  0 after a step means the step is bit-reproducible. */
long long unet_nondeterministic_sites(int reset);
/* Layer backward steps of fp32 plans whose BatchNorm-backward dY was formed by
 * the fused apply + F(6x6) dY-transform pass (unet_set_tuning "bnb_fuse")
 * instead of the standalone apply pass; reset != 0 also zeroes the count.
 * Replaces nothing in the reference: it is a counter of this implementation's
 * schedule (models/unet_model.py:12,16 is the BatchNorm2d it differentiates). */
long long unet_fused_bnb_sites(int reset);
/* 3x3 layers of fp32 plans whose weight gradient ran a Winograd tile with its
 * output transform storing torch's OIHW gradient directly
 * (unet_set_tuning "wgrad_oihw"), so that the packed-gradient permute was
 * skipped; reset != 0 also zeroes the count.  A counter of this
 * implementation's schedule (models/unet_model.py:11,15 is the Conv2d whose
 * weight it differentiates). */
long long unet_wgrad_oihw_sites(int reset);
/* Launches of k_igemm_plane, the LDS-DMA ring form of the batched point GEMMs
 * of the unfused fp32 Winograd forward / input-gradient tiles
 * (unet_set_tuning "igemm_plane"); reset != 0 also zeroes the count.  A counter
 * of this implementation's schedule (models/unet_model.py:11,15 is the Conv2d
 * those GEMMs compute). */
long long unet_igemm_plane_launches(int reset);
/* Launches of the fused fp32 Winograd tiles 76 / 75 in their persistent form
 * (unet_set_tuning "wino_persist"); reset != 0 also zeroes the count.  A counter
 * of this implementation's schedule (models/unet_model.py:11,15 is the Conv2d
 * those kernels compute). */
long long unet_wino_persist_launches(int reset);
/* Tuning database (cf. MIOpen's perf-db): unet_tuning_save writes every tuned
 * choice as "key<TAB>tile<TAB>split" lines (returns the count or -errno);
 * unet_tuning_load merges such a file, overriding equal keys (returns the
 * entries read or -errno).  With env UNET_TUNE_DB=<path> the first tuner lookup
 * loads <path> and each newly tuned shape is appended to it. */
int unet_tuning_save(const char* path);
int unet_tuning_load(const char* path);

/* ------------------------------------------------------------------------
 * Per-op entry points (used by the op-level parity tests and by tools).
 * Shapes: x (N,H,W,Ci) NHWC; W OIHW as in PyTorch; outputs NHWC.
 * ---------------------------------------------------------------------- */
/* y = conv3x3_valid(x) + b; optional BN+ReLU transform of x on load
 * (x_scale/x_shift per Ci channel, NULL = identity).  ws >= unet_conv_ws_bytes(). */
int unet_conv3x3_fwd(const float* x, int n, int h, int w, int ci, const float* wt_oihw,
                     const float* bias, int co, const float* x_scale, const float* x_shift,
                     float* y, void* ws, unet_stream_t stream);
/* dx = full-correlation(dy, W) (input gradient).  dy (N,H-2,W-2,Co). */
int unet_conv3x3_dgrad(const float* dy, int n, int h, int w, int ci, const float* wt_oihw,
                       int co, float* dx, void* ws, unet_stream_t stream);
/* dW (OIHW) = sum over pixels of x (x) dy;  db = sum dy. */
int unet_conv3x3_wgrad(const float* x, const float* dy, int n, int h, int w, int ci, int co,
                       float* dw_oihw, float* db, void* ws, unet_stream_t stream);
size_t unet_conv_ws_bytes(int n, int h, int w, int ci, int co);
/* ConvTranspose2d(k=2, s=2): y (N,2H,2W,Co) = convT(x) + b;  W (Ci,Co,2,2). */
int unet_convT2_fwd(const float* x, int n, int h, int w, int ci, const float* wt, const float* bias,
                    int co, float* y, void* ws, unet_stream_t stream);
/* ConvTranspose2d backward: dx, dW (IOHW), db.  ws >= unet_conv_ws_bytes(n,h,w,ci,co). */
int unet_convT2_bwd(const float* x, const float* dy, int n, int h, int w, int ci, const float* wt,
                    int co, float* dx, float* dw, float* db, void* ws, unet_stream_t stream);
/* MaxPool2d(2) floor mode, first max wins; argmax index 0..3 per output. */
int unet_maxpool2_fwd(const float* x, int n, int h, int w, int c, float* y, uint8_t* arg,
                      unet_stream_t stream);
int unet_maxpool2_bwd(const float* dy, const uint8_t* arg, int n, int h, int w, int c, float* dx,
                      unet_stream_t stream);
/* BatchNorm2d train forward over (N,H,W) per channel (+ running-stat update)
 * and backward; y = (x-mean)*invstd*gamma + beta. */
int unet_bn_train_fwd(const float* x, int n, int h, int w, int c, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, float* y,
                      float* save_mean, float* save_invstd, void* ws, unet_stream_t stream);
int unet_bn_train_bwd(const float* x, const float* dy, int n, int h, int w, int c,
                      const float* gamma, const float* save_mean, const float* save_invstd,
                      float* dx, float* dgamma, float* dbeta, void* ws, unet_stream_t stream);
size_t unet_bn_ws_bytes(int c);

/* Building blocks of the reference submodules' own forwards (DoubleConv / Down
 * / Up / OutConv.forward, models/unet_model.py:20-21, 32-33, 50-54, 62-63) and
 * of the op-by-op network path the drop-in takes for a backward through an
 * eval-mode forward.  NHWC tensors unless marked NCHW. */
/* nn.BatchNorm2d (+ the following nn.ReLU when relu != 0): training = batch
 * statistics over (N,H,W), running_mean / running_var updated with `momentum`
 * (unbiased variance), *nbt += 1 (nbt may be NULL); eval = the running
 * statistics.  save_mean / save_invstd receive the statistics used.  c a
 * multiple of 4 dividing 1024. */
size_t unet_bn_relu_ws_bytes(int n, int h, int w, int c);
int unet_bn_relu_fwd(const float* x, int n, int h, int w, int c, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* nbt, float momentum, float eps,
                     int training, int relu, float* y, float* save_mean, float* save_invstd, void* ws,
                     unet_stream_t stream);
/* Its backward: y = the forward's output (the ReLU mask), dx, dgamma, dbeta;
 * eval mode treats the statistics as constants (dx = gamma * invstd * dz). */
int unet_bn_relu_bwd(const float* x, const float* y, const float* dy, int n, int h, int w, int c,
                     const float* gamma, const float* save_mean, const float* save_invstd, int training,
                     int relu, float* dx, float* dgamma, float* dbeta, void* ws, unet_stream_t stream);
/* The first conv (any Ci -> 64, 3x3 valid, + bias) from an NCHW input; y NHWC.
 * Backward: dW (OIHW), db, and dx (NCHW; NULL = not needed). */
size_t unet_conv_first_ws_bytes(int n, int ci, int h, int w);
int unet_conv_first_fwd(const float* x_nchw, int n, int ci, int h, int w, const float* wt, const float* bias,
                        float* y, unet_stream_t stream);
int unet_conv_first_bwd(const float* x_nchw, const float* dy, int n, int ci, int h, int w, const float* wt,
                        float* dx_nchw, float* dw, float* db, void* ws, unet_stream_t stream);
/* OutConv's 1x1 conv (64 -> k channels, + bias): logits NCHW; backward dx
 * (NHWC, NULL = not needed), dW (k, 64), db. */
size_t unet_conv1x1_ws_bytes(int k);
int unet_conv1x1_fwd(const float* x, int n, int h, int w, int c, const float* wt, const float* bias, int k,
                     float* logits_nchw, unet_stream_t stream);
int unet_conv1x1_bwd(const float* x, const float* dlogits_nchw, int n, int h, int w, int c, const float* wt, int k,
                     float* dx, float* dw, float* db, void* ws, unet_stream_t stream);

/* ------------------------------------------------------------------------
 * One forward / input-gradient GEMM of the network plan, with everything the
 * plan fuses into it at that launch site (for per-element tests and tools).
 * The entry point builds the arguments the plan builds there and runs them on
 * the forced tile, the "igemm_variant" knob's tile, or the built-in choice.
 *
 *  site        GEMM rows (n, h, w)   src0                       fused
 *  F_PLAIN     3x3 conv output grid  (n, h+2, w+2, ci)          scale0/shift0 (BN+ReLU on load), bias, stats
 *  F_CAT       3x3 conv output grid  skip (n, skip_h, skip_w, c_split) read at origin (oy, ox), its own
 *                                    scale0/shift0; src1 (n, h+2, w+2, ci - c_split), scale1/shift1
 *                                    normally NULL; bias, stats
 *  F_EVAL      as F_PLAIN            (n, h+2, w+2, ci)          bias, ReLU on store, no statistics
 *  D_POOL      3x3 conv input grid   padded dY (n, h+2, w+2, co), read at origin 0     plain store
 *  D_MASK      as D_POOL             as D_POOL                  ReLU mask from yref, bstats
 *  D_SPLIT     as D_POOL             as D_POOL                  columns < n_split -> dst0 (C = n_split),
 *                                                               the rest -> dst1 (C = ci - n_split), colsum1
 *  T_FWD       convT input grid      (n, h, w, ci)              pixel shuffle to dst0 (n, 2h, 2w, co), bias
 *  T_MASK      convT input grid      dY (n, 2h, 2w, co)         2x2 stride-2 gather; mask + bstats as D_MASK
 *
 * wt is torch's weight: conv (co, ci, 3, 3), ConvTranspose2d (ci, co, 2, 2).
 * Forward sites produce co columns, D_* / T_MASK ci columns, T_FWD 4 co.
 * dst0 / dst1 / yref live on the row grid (T_FWD: dst0 on the 2h x 2w grid).
 * Every tensor is fp32 NHWC in the caller's buffers, except: with
 * "op_precision" UNET_PREC_BF16 and "op_a16" 1 the entry point rounds the
 * sources and yref to bf16 copies in ws (what a bf16 plan stores) and dst0 /
 * dst1 ARE bf16 (2 bytes per element).  stats / bstats receive the raw
 * [64][columns of dst0][2] fp64 partial sums (sum, sum of squares; sum dz',
 * sum dz' * xhat), colsum1 the [64][columns of dst1] sums; the entry point
 * zeroes them.  Channel counts are multiples of 8 (16 for every tile but the
 * fused F(2x2) Winograd ones), column counts and n_split multiples of 32.
 * tile: > 0 forces that tile of the igemm table, -1 = the "igemm_variant"
 * knob, else the built-in choice.  split: K slices (<= 1: none); the partial
 * planes live in ws.  With "op_strict" 1 a forced tile or split that does not
 * apply is -EINVAL before anything is launched. */
enum {
  UNET_SITE_F_PLAIN = 0, UNET_SITE_F_CAT = 1, UNET_SITE_F_EVAL = 2, UNET_SITE_D_POOL = 3,
  UNET_SITE_D_MASK = 4, UNET_SITE_D_SPLIT = 5, UNET_SITE_T_FWD = 6, UNET_SITE_T_MASK = 7
};
typedef struct unet_gemm_site {
  int site;
  int n, h, w;                 /* row grid of the GEMM */
  int ci, co;                  /* the layer's channels (as in wt) */
  int c_split;                 /* F_CAT: channels of src0 */
  int skip_h, skip_w, oy, ox;  /* F_CAT: stored grid of src0, crop origin */
  int n_split;                 /* D_SPLIT: columns of dst0 */
  int tile, split;
  const float* src0;
  const float* src1;
  const float* scale0;
  const float* shift0;
  const float* scale1;
  const float* shift1;
  const float* wt;
  const float* bias;
  void* dst0;
  void* dst1;
  const float* yref;
  const float* bn_scale;
  const float* bn_shift;
  const float* bn_mean;
  const float* bn_invstd;
  double* stats;
  double* bstats;
  double* colsum1;
} unet_gemm_site;
/* Host only (no device call): 0 when unet_gemm_site_run would launch the
 * descriptor as it stands (same checks, same knobs), -EINVAL otherwise.
 * *tile (may be NULL) receives the tile id it would run. */
int unet_gemm_site_check(const unet_gemm_site* d, int* tile);
size_t unet_gemm_site_ws_bytes(const unet_gemm_site* d);
int unet_gemm_site_run(const unet_gemm_site* d, void* ws, unet_stream_t stream);
/* Host only: the rows of the igemm tile table.  Writes up to cap rows of 6 ints
 * (id, family (IgemmFamily's order), bf16, x3, ksplit, wino_m) into out (may
 * be NULL) and returns the number of rows of the table. */
int unet_igemm_tile_table(int* out, int cap);

/* Ceilings of this device, measured (bench.py's untimed tail; BASELINE.md asks
 * for roofline fractions against peaks measured on the box): kind 0 = dense
 * bf16 MFMA (v_mfma_f32_32x32x16_bf16) TFLOP/s, 1 = f32 MFMA
 * (v_mfma_f32_16x16x4_f32) TFLOP/s, 2 = HBM float4 copy GB/s (read + write),
 * 3 = HBM read-only stream GB/s.
 * Best of `reps` timed launches after a warm-up; allocates its own buffers. */
int unet_peak_probe(int kind, int reps, double* result, unet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
