"""GPU input pipeline: the reference's elastic augmentation for a whole batch.

``utils/augmentations.py:4-39`` (``elastic_deform_image_and_mask``) plus the
``utils/dataset.py:84-111`` steps around it (uint8 casts, ``ToTensor``,
``mask > 0``) as three HIP kernels behind ``unet_elastic_deform``
(include/unet_hip.h): two separable fp64 Gaussian passes over the uniform noise
fields and one warp.  The reference spends ~83 ms per 512x512 sample on one CPU
core; here a batch is a few launches on the training
stream.

Randomness: the reference draws ``RandomState(seed).rand(H, W)`` twice per
sample (dx, then dy) with a fresh random seed.  ``noise="numpy"`` reproduces
that draw on the host for given seeds (bit-identical outputs to the reference);
``noise="device"`` draws the same distribution with ``torch.rand`` on the GPU
(no host work; a different stream of numbers, as the reference's own seeds are
random anyway).

    aug = ElasticDeform(alpha=2000, sigma=20)        # scripts/train.py:35-36
    x, target = aug(images_u8, labels_u16)             # (N,1,H,W) fp32, (N,1,H,W) uint8

``TileAugment`` is the U-Net paper's training geometry on top of it: input tiles
whose output window lies anywhere in the frame, the missing context mirrored as
at inference, plus shift / rotation / flips / gray-value changes
(``unet_tile_warp``, one more kernel in csrc/elastic.hip).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


class ElasticDeform:
    def __init__(self, alpha: float = 2000.0, sigma: float = 20.0, noise: str = "device",
                 generator: torch.Generator | None = None):
        if noise not in ("device", "numpy"):
            raise ValueError("noise must be 'device' or 'numpy'")
        self.alpha, self.sigma, self.noise = float(alpha), float(sigma), noise
        self.generator = generator
        self.lib = _lib.load()
        self._ws = None

    def draw_noise(self, n, h, w, device, seeds=None):
        """(n, 2, h, w) fp64 uniform noise: per sample the reference's two
        RandomState(seed).rand(h, w) draws (noise="numpy"), or torch.rand."""
        if self.noise == "numpy":
            if seeds is None:
                seeds = np.random.randint(0, 2 ** 32 - 1, size=n, dtype=np.int64)
            buf = np.empty((n, 2, h, w), np.float64)
            for i, s in enumerate(seeds):
                rs = np.random.RandomState(int(s))
                buf[i, 0] = rs.rand(h, w)
                buf[i, 1] = rs.rand(h, w)
            return torch.from_numpy(buf).to(device, non_blocking=True)
        return torch.rand((n, 2, h, w), dtype=torch.float64, device=device, generator=self.generator)

    def __call__(self, images: torch.Tensor, labels: torch.Tensor, seeds=None, noise: torch.Tensor | None = None,
                 return_image: bool = False, return_ids: bool = False):
        """images (N, H, W) uint8, labels (N, H, W) uint16 (instance ids; the
        reference casts them to uint8 before `> 0`), both on the HIP device.
        return_ids appends the warped instance map (N, H, W) uint16: the id at
        the source pixel the target was sampled from, 0 where the target is 0."""
        if images.device.type != "cuda" or labels.device.type != "cuda":
            raise ValueError("ElasticDeform runs on the HIP device only (no CPU fallback)")
        if images.dtype != torch.uint8 or images.dim() != 3:
            raise ValueError("images must be (N, H, W) uint8")
        if labels.shape != images.shape:
            raise ValueError("labels must match images")
        if labels.dtype != torch.uint16:  # same low 16 bits, reinterpreted
            labels = labels.to(torch.int32).to(torch.int16).view(torch.uint16)
        n, h, w = images.shape
        images, labels = images.contiguous(), labels.contiguous()
        if noise is None:
            noise = self.draw_noise(n, h, w, images.device, seeds)
        noise = noise.to(torch.float64).contiguous()
        if tuple(noise.shape) != (n, 2, h, w):
            raise ValueError(f"noise must be (N, 2, H, W) = {(n, 2, h, w)}")
        need = self.lib.unet_elastic_ws_bytes(n, h, w)
        if self._ws is None or self._ws.numel() < need or self._ws.device != images.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=images.device)
        x = torch.empty((n, 1, h, w), dtype=torch.float32, device=images.device)
        t = torch.empty((n, 1, h, w), dtype=torch.uint8, device=images.device)
        img = torch.empty((n, h, w), dtype=torch.uint8, device=images.device) if return_image else None
        ids = torch.empty((n, h, w), dtype=torch.uint16, device=images.device) if return_ids else None
        _lib.check(self.lib.unet_elastic_deform_ex(images.data_ptr(), labels.data_ptr(), n, h, w, noise.data_ptr(),
                                                   ctypes.c_double(self.alpha), ctypes.c_double(self.sigma),
                                                   x.data_ptr(), t.data_ptr(), _lib.ptr(img), _lib.ptr(ids),
                                                   self._ws.data_ptr(), _lib.stream_of()), "unet_elastic_deform_ex")
        out = (x, t, img) if return_image else (x, t)
        return out + (ids,) if return_ids else out


TILE_EXTEND = {"reflect": 0, "mirror": 1}


class TileAugment:
    """Training tiles over the whole frame (the U-Net paper's training geometry).

    Each sample is a (th, tw) input tile cut from one resident frame by
    ``unet_tile_warp``: an affine map (integer shift of the tile centre,
    rotation, flips) composed with the elastic field of ``ElasticDeform`` (drawn
    on the tile grid), the context that falls outside the frame filled by
    mirroring (``extend="mirror"``: whole-sample symmetric, exactly what
    ``TileFarm`` / ``unet_tile_gather`` feed the network at inference;
    ``"reflect"``: scipy's half-sample rule of the reference's warp), and a
    gain / bias step on the rounded uint8 image.  One warp launch per batch,
    plus the two Gaussian launches when ``elastic``.

    Geometry.  ``params`` rows are ``a00 a01 b0 a10 a11 b1 gain bias``; tile
    pixel (ty, tx) reads the frame at ``(a00 ty + a01 tx + b0, a10 ty + a11 tx
    + b1)``.  ``affine`` maps the tile centre ((th-1)/2, (tw-1)/2) to the frame
    centre + shift with A = [[c, -s], [s, c]] (a positive angle turns the image
    content clockwise on the screen: 90 degrees on a square frame is
    ``np.rot90(frame, -1)``); ``flip_h`` negates A's second column (the tile is
    ``[:, ::-1]`` of the unflipped one), ``flip_v`` its first.

    ``sample_params`` draws on the host.  Its shifts are whole pixels measured
    from the floor-aligned position (tile origin ``(H - th) // 2``, the
    convention of ``center_crop_views``), so an unrotated tile copies frame
    pixels without interpolation whatever the parities.  ``max_shift="cover"``
    is the range in which the output window (``out_hw``, centre-cropped from
    the tile; default the tile itself) reaches every frame pixel and never
    leaves the frame: +-(H - oh) // 2 and +-(W - ow) // 2 when the parities of
    frame, tile and window agree.
    """

    def __init__(self, tile_hw, extend: str = "mirror", alpha: float = 2000.0, sigma: float = 20.0,
                 elastic: bool = True, max_rotate: float = 0.0, flip: bool = False, max_shift="cover", out_hw=None,
                 gain: float = 0.0, bias: float = 0.0, noise: str = "device",
                 generator: torch.Generator | None = None, seed: int = 0):
        if extend not in TILE_EXTEND:
            raise ValueError("extend must be 'mirror' (whole-sample, as the inference tiles) or 'reflect'")
        if noise not in ("device", "numpy"):
            raise ValueError("noise must be 'device' or 'numpy'")
        self.tile_hw = (int(tile_hw[0]), int(tile_hw[1]))
        if min(self.tile_hw) < 1:
            raise ValueError(f"tile_hw must be positive, got {self.tile_hw}")
        self.out_hw = None if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if max_shift != "cover":
            ms = (max_shift, max_shift) if np.isscalar(max_shift) else tuple(max_shift)
            max_shift = (int(ms[0]), int(ms[1]))
            if min(max_shift) < 0:
                raise ValueError("max_shift must be 'cover', a non-negative integer or a pair of them")
        if max_rotate < 0 or gain < 0 or bias < 0:
            raise ValueError("max_rotate, gain and bias are half-widths: they must be >= 0")
        self.extend, self.alpha, self.sigma, self.elastic = extend, float(alpha), float(sigma), bool(elastic)
        self.max_rotate, self.flip, self.max_shift = float(max_rotate), bool(flip), max_shift
        self.gain, self.bias, self.noise, self.generator = float(gain), float(bias), noise, generator
        self.rng = np.random.default_rng(seed)
        self._ws = None  # the geometry needs no library; __call__ loads it

    # ---- geometry (host, fp64) ----
    def affine(self, angle=0.0, flip_h=False, flip_v=False, shift=(0.0, 0.0), frame_hw=None):
        """(a00, a01, b0, a10, a11, b1) as fp64: the tile centre maps to the
        frame centre + shift; multiples of 90 degrees give exact 0 / +-1."""
        th, tw = self.tile_hw
        H, W = frame_hw
        q = float(angle) / 90.0
        if q == np.floor(q):
            c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
        else:
            c, s = float(np.cos(np.deg2rad(angle))), float(np.sin(np.deg2rad(angle)))
        fv, fh = (-1.0 if flip_v else 1.0), (-1.0 if flip_h else 1.0)
        a00, a01, a10, a11 = c * fv, -s * fh, s * fv, c * fh
        a00, a01, a10, a11 = a00 + 0.0, a01 + 0.0, a10 + 0.0, a11 + 0.0  # no -0.0 entries
        cty, ctx = (th - 1) / 2.0, (tw - 1) / 2.0
        cfy, cfx = (H - 1) / 2.0 + float(shift[0]), (W - 1) / 2.0 + float(shift[1])
        b0 = cfy - (a00 * cty + a01 * ctx)
        b1 = cfx - (a10 * cty + a11 * ctx)
        return np.array([a00, a01, b0, a10, a11, b1], np.float64)

    def align(self, frame_hw):
        """The sub-pixel offset that puts an unrotated, unshifted tile on the
        floor-aligned origin ((H - th) // 2, (W - tw) // 2): -0.5 on an axis
        where frame and tile differ in parity, else 0."""
        return tuple(-0.5 * ((f - t) % 2) for f, t in zip(frame_hw, self.tile_hw))

    def shift_range(self, frame_hw):
        """((lo_y, hi_y), (lo_x, hi_x)): the integer shifts sample_params draws from."""
        if self.max_shift != "cover":
            return tuple((-m, m) for m in self.max_shift)
        out = self.out_hw or self.tile_hw
        rng = []
        for f, t, o in zip(frame_hw, self.tile_hw, out):
            if o > t:
                raise ValueError(f"out_hw {out} exceeds the tile {self.tile_hw}")
            base = (f - t) // 2 + (t - o) // 2   # window start in the frame at shift 0
            lo, hi = -base, (f - o) - base
            rng.append((min(lo, hi), max(lo, hi)))
        return tuple(rng)

    def sample_params(self, n, frame_hw, return_draws=False):
        """(n, 8) fp64 params rows drawn from the seeded numpy Generator; with
        return_draws also the dict of the raw draws (angle in degrees, flip_h,
        flip_v, shift (n, 2) whole pixels, gain, bias)."""
        g = self.rng
        (ly, hy), (lx, hx) = self.shift_range(frame_hw)
        d = {
            "angle": g.uniform(-self.max_rotate, self.max_rotate, n) if self.max_rotate > 0 else np.zeros(n),
            "flip_h": g.integers(0, 2, n).astype(bool) if self.flip else np.zeros(n, bool),
            "flip_v": g.integers(0, 2, n).astype(bool) if self.flip else np.zeros(n, bool),
            "shift": np.stack([g.integers(ly, hy + 1, n), g.integers(lx, hx + 1, n)], 1).astype(np.int64),
            "gain": g.uniform(1.0 - self.gain, 1.0 + self.gain, n) if self.gain > 0 else np.ones(n),
            "bias": g.uniform(-self.bias, self.bias, n) if self.bias > 0 else np.zeros(n),
        }
        ay, ax = self.align(frame_hw)
        rows = np.empty((n, 8), np.float64)
        for i in range(n):
            sh = (d["shift"][i, 0] + ay, d["shift"][i, 1] + ax)
            rows[i, :6] = self.affine(d["angle"][i], d["flip_h"][i], d["flip_v"][i], sh, frame_hw)
            rows[i, 6], rows[i, 7] = d["gain"][i], d["bias"][i]
        return (rows, d) if return_draws else rows

    def draw_noise(self, n, device):
        """(n, 2, th, tw) fp64 uniform noise on the tile grid."""
        th, tw = self.tile_hw
        if self.noise == "numpy":
            return torch.from_numpy(self.rng.random((n, 2, th, tw))).to(device, non_blocking=True)
        return torch.rand((n, 2, th, tw), dtype=torch.float64, device=device, generator=self.generator)

    def __call__(self, frames: torch.Tensor, labels: torch.Tensor, frame_idx, params=None, noise=None,
                 weights: torch.Tensor | None = None, return_image: bool = False, return_ids: bool = False):
        """frames (F, H, W) uint8 and labels (F, H, W) uint16 resident on the
        HIP device; frame_idx: the n frames the tiles are cut from (no copy of
        the frames is made).  params (n, 8) / noise (n, 2, th, tw) fix the
        draw.  weights (F, H, W) fp32 planes are carried into the tile at the
        label's nearest index.  Returns (x (n,1,th,tw) fp32, target (n,1,th,tw)
        uint8[, image (n,th,tw) uint8][, ids (n,th,tw) uint16][, w (n,th,tw)])."""
        if frames.device.type != "cuda" or labels.device.type != "cuda":
            raise ValueError("TileAugment runs on the HIP device only (no CPU fallback)")
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise ValueError("frames must be (F, H, W) uint8")
        if labels.shape != frames.shape:
            raise ValueError("labels must match frames")
        dev, lib = frames.device, _lib.load()
        if labels.dtype != torch.uint16:  # same low 16 bits, reinterpreted
            labels = labels.to(torch.int32).to(torch.int16).view(torch.uint16)
        frames, labels = frames.contiguous(), labels.contiguous()
        nf, h, w = frames.shape
        th, tw = self.tile_hw
        if torch.is_tensor(frame_idx):  # device indices: the kernel clamps them to [0, F)
            fidx = frame_idx.to(dev, torch.int32).contiguous()
        else:
            host = np.asarray(frame_idx, dtype=np.int64)
            if host.size and (host.min() < 0 or host.max() >= nf):
                raise ValueError(f"frame_idx must lie in [0, {nf})")
            fidx = torch.as_tensor(host.astype(np.int32), device=dev)
        if fidx.dim() != 1 or fidx.numel() < 1:
            raise ValueError("frame_idx must be a non-empty 1-d list of frame numbers")
        n = fidx.numel()
        if params is None:
            params = self.sample_params(n, (h, w))
        if not torch.is_tensor(params):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64))
        params = params.to(dev, torch.float64).contiguous()
        if tuple(params.shape) != (n, 8):
            raise ValueError(f"params must be (n, 8) = {(n, 8)}")
        if weights is not None:
            if weights.device != dev or weights.dtype != torch.float32 or tuple(weights.shape) != (nf, h, w):
                raise ValueError("weights must be (F, H, W) fp32 on the frames' device")
            weights = weights.contiguous()
        ws = None
        if self.elastic:
            if noise is None:
                noise = self.draw_noise(n, dev)
            noise = noise.to(dev, torch.float64).contiguous()
            if tuple(noise.shape) != (n, 2, th, tw):
                raise ValueError(f"noise must be (n, 2, th, tw) = {(n, 2, th, tw)}")
            need = lib.unet_tile_warp_ws_bytes(n, th, tw)
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            ws = self._ws
        elif noise is not None:
            raise ValueError("noise given to a TileAugment built with elastic=False")
        x = torch.empty((n, 1, th, tw), dtype=torch.float32, device=dev)
        t = torch.empty((n, 1, th, tw), dtype=torch.uint8, device=dev)
        img = torch.empty((n, th, tw), dtype=torch.uint8, device=dev) if return_image else None
        ids = torch.empty((n, th, tw), dtype=torch.uint16, device=dev) if return_ids else None
        wout = torch.empty((n, th, tw), dtype=torch.float32, device=dev) if weights is not None else None
        _lib.check(lib.unet_tile_warp(frames.data_ptr(), labels.data_ptr(), _lib.ptr(weights), nf, h, w,
                                      fidx.data_ptr(), params.data_ptr(), n, th, tw, TILE_EXTEND[self.extend],
                                      _lib.ptr(noise), ctypes.c_double(self.alpha), ctypes.c_double(self.sigma),
                                      x.data_ptr(), t.data_ptr(), _lib.ptr(img), _lib.ptr(ids), _lib.ptr(wout),
                                      _lib.ptr(ws), _lib.stream_of()), "unet_tile_warp")
        out = (x, t)
        if return_image:
            out += (img,)
        if return_ids:
            out += (ids,)
        if weights is not None:
            out += (wout,)
        return out


WEIGHT_MAP_MODES = ("reference", "border")


def weight_maps(labels: torch.Tensor, w0: float = 10.0, sigma: float = 5.0, fp64: bool = False,
                mode: str = "reference", return_distances: bool = False):
    """scripts/preprocess_data.py:17-77 on the device for a batch of label maps
    (N, H, W) (uint16 instance ids, or any integer type): the per-pixel loss
    weights (N, H, W) fp32 utils/dataset.py:111 feeds the loss, and with
    fp64=True also the fp64 map the reference saves as weight_map_*.npy.

    mode="reference" is what the reference computes (its distances are
    identically zero: a per-class constant).  mode="border" is the U-Net
    paper's term, with d1 and d2 the exact Euclidean distances to the nearest
    and second-nearest object (unet_weight_map_border); return_distances=True
    appends their squares (d1sq, d2sq), (N, H, W) int32 (zeros in reference
    mode, as in the reference)."""
    if mode not in WEIGHT_MAP_MODES:
        raise ValueError(f"mode must be one of {WEIGHT_MAP_MODES}, got {mode!r}")
    lib = _lib.load()
    if labels.device.type != "cuda" or labels.dim() != 3:
        raise ValueError("labels must be an (N, H, W) tensor on the HIP device")
    if labels.dtype != torch.uint16:
        labels = labels.to(torch.int32).to(torch.int16).view(torch.uint16)
    labels = labels.contiguous()
    n, h, w = labels.shape
    out = torch.empty((n, h, w), dtype=torch.float32, device=labels.device)
    out64 = torch.empty((n, h, w), dtype=torch.float64, device=labels.device) if fp64 else None
    d1 = d2 = None
    if mode == "border":
        need = lib.unet_weight_map_border_ws_bytes(n, h, w)
        if need == 0:
            raise ValueError(f"border weight maps need 1 <= h, w <= 16384, got {(n, h, w)}")
        if return_distances:
            d1 = torch.empty((n, h, w), dtype=torch.int32, device=labels.device)
            d2 = torch.empty((n, h, w), dtype=torch.int32, device=labels.device)
        ws = torch.empty(need, dtype=torch.uint8, device=labels.device)
        _lib.check(lib.unet_weight_map_border(labels.data_ptr(), n, h, w, ctypes.c_double(w0), ctypes.c_double(sigma),
                                              out.data_ptr(), _lib.ptr(out64), _lib.ptr(d1), _lib.ptr(d2),
                                              ws.data_ptr(), _lib.stream_of()), "unet_weight_map_border")
    else:
        ws = torch.empty(lib.unet_weight_map_ws_bytes(n), dtype=torch.uint8, device=labels.device)
        _lib.check(lib.unet_weight_map(labels.data_ptr(), n, h, w, ctypes.c_double(w0), ctypes.c_double(sigma),
                                       out.data_ptr(), _lib.ptr(out64), ws.data_ptr(), _lib.stream_of()),
                   "unet_weight_map")
        if return_distances:
            d1 = torch.zeros((n, h, w), dtype=torch.int32, device=labels.device)
            d2 = torch.zeros((n, h, w), dtype=torch.int32, device=labels.device)
    res = (out, out64) if fp64 else (out,)
    if return_distances:
        res = res + (d1, d2)
    return res if len(res) > 1 else res[0]
