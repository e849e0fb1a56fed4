"""Post-processing on the GPU (utils/metrics.py): instance labelling of
predicted masks (plain, or with touching cells split), the Rand index, and the
warping and pixel error, behind unet_instance_masks / unet_split_instances /
unet_rand_index / unet_warping_error (include/unet_hip.h).

    labels = instance_masks(mask_u8, min_size=15)   # get_instance_masks (:42-72), uint16
    s = split_instances(mask_u8, core_radius=30)     # the same with touching cells separated
    s.labels, s.markers, s.segments, s.levels        # uint16 labels; per-frame counts on the device
    ri, re = rand_index(gt_labels, labels)           # calculate_rand_index_and_error (:75-139)
    r = warping_error(gt_labels, mask_u8, radius=4)  # the calculate_warping_error placeholder
    r.warping_error, r.pixel_error                   # fractions of H W per frame, on the device
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib


def _u16(t):
    if t.dtype == torch.uint16:
        return t.contiguous()
    return t.to(torch.int32).to(torch.int16).view(torch.uint16).contiguous()


def instance_masks(mask: torch.Tensor, min_size: int = 15) -> torch.Tensor:
    """(N, H, W) or (H, W) mask on the HIP device, > 0 = foreground -> uint16
    labels: 8-connected components numbered in raster order of their first
    pixel, components under min_size pixels zeroed (not renumbered)."""
    if mask.device.type != "cuda":
        raise ValueError("instance_masks runs on the HIP device only (no CPU fallback)")
    squeeze = mask.dim() == 2
    m = mask[None] if squeeze else mask
    if m.dim() != 3:
        raise ValueError("mask must be (H, W) or (N, H, W)")
    m = (m > 0).to(torch.uint8).contiguous()
    n, h, w = m.shape
    lib = _lib.load()
    ws = torch.empty(lib.unet_instance_masks_ws_bytes(n, h, w), dtype=torch.uint8, device=m.device)
    out = torch.empty((n, h, w), dtype=torch.uint16, device=m.device)
    _lib.check(lib.unet_instance_masks(m.data_ptr(), n, h, w, int(min_size), out.data_ptr(), ws.data_ptr(),
                                       _lib.stream_of()), "unet_instance_masks")
    return out[0] if squeeze else out


@dataclass
class SplitResult:
    """Results of split_instances, all on the device: `labels` uint16, `info`
    (N, 4) int32 = markers, segments before the min_size cut, largest geodesic
    distance assigned, overflow (a (4,) row for an (H, W) input), `d2` the int32
    squared distance to the background when it was asked for."""
    labels: torch.Tensor
    info: torch.Tensor
    d2: Optional[torch.Tensor] = None

    @property
    def markers(self):
        return self.info[..., 0]

    @property
    def segments(self):
        return self.info[..., 1]

    @property
    def levels(self):
        return self.info[..., 2]

    @property
    def overflow(self):
        return self.info[..., 3] != 0


def split_instances(mask: torch.Tensor, core_radius: Optional[float] = None, *, core_d2: Optional[int] = None,
                    markers: Optional[torch.Tensor] = None, min_size: int = 15,
                    return_distance: bool = False) -> SplitResult:
    """instance_masks with touching cells separated: (N, H, W) or (H, W) mask
    on the HIP device, > 0 = foreground.  The markers are the 8-connected
    components of the foreground pixels whose squared distance to the nearest
    background pixel of the frame is >= core_d2 (core_radius r: core_d2 =
    ceil(r^2)), or of `markers` > 0 within the foreground; every foreground
    pixel connected to a marker joins the marker nearest along the foreground
    (8-connected steps, the smaller marker number among equals); a component
    without a marker stays one segment.  Segments are numbered in raster order
    of their first pixel, those under min_size pixels zeroed (not renumbered).
    Exactly one of core_radius, core_d2, markers is given; core_d2 = 0 gives
    instance_masks's labels.  include/unet_hip.h has the exact definition."""
    if sum(a is not None for a in (core_radius, core_d2, markers)) != 1:
        raise ValueError("give exactly one of core_radius, core_d2, markers")
    if mask.device.type != "cuda" or (markers is not None and markers.device.type != "cuda"):
        raise ValueError("split_instances runs on the HIP device only (no CPU fallback)")
    squeeze = mask.dim() == 2
    m = mask[None] if squeeze else mask
    if m.dim() != 3:
        raise ValueError("mask must be (H, W) or (N, H, W)")
    m = (m > 0).to(torch.uint8).contiguous()
    n, h, w = m.shape
    mk = None
    if markers is not None:
        if markers.shape != mask.shape:
            raise ValueError("markers must have the mask's shape")
        mk = (markers > 0).to(torch.uint8).contiguous()
        core_d2 = 0
    elif core_radius is not None:
        if not 0 <= core_radius <= 32768:
            raise ValueError("core_radius must be within [0, 32768]")
        core_d2 = math.ceil(core_radius * core_radius)
    if int(core_d2) != core_d2 or not 0 <= core_d2 <= 1 << 30:
        raise ValueError("core_d2 must be an integer within [0, 2^30]")
    if min_size < 0:
        raise ValueError("min_size must be >= 0")
    lib = _lib.load()
    need = lib.unet_split_instances_ws_bytes(n, h, w)
    if need == 0:
        raise ValueError("split_instances needs 1 <= H, W <= 16384, N <= 65535 and N H W < 2^31")
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    labels = torch.empty((n, h, w), dtype=torch.uint16, device=m.device)
    info = torch.empty((n, 4), dtype=torch.int32, device=m.device)
    d2 = torch.empty((n, h, w), dtype=torch.int32, device=m.device) if return_distance else None
    _lib.check(lib.unet_split_instances(m.data_ptr(), _lib.ptr(mk), n, h, w, int(core_d2), int(min_size),
                                        labels.data_ptr(), _lib.ptr(d2), info.data_ptr(), ws.data_ptr(),
                                        _lib.stream_of()), "unet_split_instances")
    if squeeze:
        labels, info, d2 = labels[0], info[0], None if d2 is None else d2[0]
    return SplitResult(labels, info, d2)


def rand_index(gt: torch.Tensor, pred: torch.Tensor):
    """(Rand index, Rand error) of two (H, W) instance labelings on the device
    (labels < 65536)."""
    if gt.shape != pred.shape or gt.dim() != 2:
        raise ValueError("gt and pred must be (H, W) of the same shape")
    if gt.device.type != "cuda" or pred.device.type != "cuda":
        raise ValueError("rand_index runs on the HIP device only (no CPU fallback)")
    g, p = _u16(gt), _u16(pred)
    h, w = g.shape
    lib = _lib.load()
    ws = torch.empty(lib.unet_rand_index_ws_bytes(h, w), dtype=torch.uint8, device=g.device)
    out = torch.empty(2, dtype=torch.float64, device=g.device)
    _lib.check(lib.unet_rand_index(g.data_ptr(), p.data_ptr(), h, w, out.data_ptr(), ws.data_ptr(),
                                   _lib.stream_of()), "unet_rand_index")
    ri, re = out.tolist()
    return ri, re


FORCE_WS = 1  # UNET_WARP_FORCE_WS: keep the bit planes in the workspace (tests)


@dataclass
class WarpingResult:
    """Per-frame results of warping_error, all on the device: `counts` is
    (N, 5) int64 = pixel error, warping error, flips, sweeps, converged (a (5,)
    row for an (H, W) input); the properties read its columns, the errors as
    the fractions of H W the ISBI tables quote."""
    counts: torch.Tensor
    pixels: int
    warped: Optional[torch.Tensor] = None

    @property
    def pixel_error_count(self):
        return self.counts[..., 0]

    @property
    def warping_error_count(self):
        return self.counts[..., 1]

    @property
    def flips(self):
        return self.counts[..., 2]

    @property
    def sweeps(self):
        return self.counts[..., 3]

    @property
    def converged(self):
        return self.counts[..., 4] != 0

    @property
    def pixel_error(self):
        return self.counts[..., 0].double() / self.pixels

    @property
    def warping_error(self):
        return self.counts[..., 1].double() / self.pixels


def warping_error(gt: torch.Tensor, pred: torch.Tensor, radius: int = 4, separate: bool = True, max_sweeps: int = 0,
                  return_warped: bool = False, flags: int = 0) -> WarpingResult:
    """Warping error of a binary prediction against instance ground truth:
    gt (N, H, W) or (H, W) instance ids (< 65536), pred of the same shape with
    > 0 = foreground, both on the HIP device.  The ground truth -- with a
    background ridge between touching cells when `separate` -- is warped onto
    the prediction by flipping simple points within `radius` of its boundary
    (-1 = anywhere, 0 = nowhere) until none is left or `max_sweeps` sweeps ran
    (0 = no limit); what still differs is the warping error, the topological
    part of the pixel error (include/unet_hip.h has the exact schedule).  The
    counts stay on the device until they are read."""
    if gt.shape != pred.shape or gt.dim() not in (2, 3):
        raise ValueError("gt and pred must be (H, W) or (N, H, W) of the same shape")
    if gt.device.type != "cuda" or pred.device.type != "cuda":
        raise ValueError("warping_error runs on the HIP device only (no CPU fallback)")
    squeeze = gt.dim() == 2
    g = _u16(gt[None] if squeeze else gt)
    p = ((pred[None] if squeeze else pred) > 0).to(torch.uint8).contiguous()
    n, h, w = g.shape
    lib = _lib.load()
    ws = torch.empty(lib.unet_warping_error_ws_bytes(n, h, w), dtype=torch.uint8, device=g.device)
    counts = torch.empty((n, 5), dtype=torch.int64, device=g.device)
    warped = torch.empty((n, h, w), dtype=torch.uint8, device=g.device) if return_warped else None
    _lib.check(lib.unet_warping_error(g.data_ptr(), p.data_ptr(), n, h, w, int(radius), 1 if separate else 0,
                                      int(max_sweeps), int(flags), _lib.ptr(warped), counts.data_ptr(),
                                      ws.data_ptr(), _lib.stream_of()), "unet_warping_error")
    if squeeze:
        counts = counts[0]
        warped = None if warped is None else warped[0]
    return WarpingResult(counts, h * w, warped)


def pixel_error(gt: torch.Tensor, pred: torch.Tensor, separate: bool = True) -> torch.Tensor:
    """Pixels at which the binary ground truth of warping_error (gt > 0, with
    the background ridge between touching cells when `separate`) differs from
    pred > 0: an int64 count per frame, on the device (divide by H W for the
    fraction)."""
    return warping_error(gt, pred, radius=0, separate=separate).pixel_error_count
