"""Distance-based linker on the MI355X: every frame pair of a sequence is one
assignment problem over the squared distances of the objects' quantised
centroids, inside a gate, and all of them are solved in one kernel launch
(unet_link_frames, csrc/link.hip), one workgroup per pair.  A host pass
(unet_link_assemble) chains the links into tracks, with divisions where a
birth next to a linked object passes the area test.  DESIGN.md, "Distance-based
linker", has the definitions.

    res = link_stack(stack)                     # (n, h, w) labels on the device
    res.rows                                    # (tracks, 4) int32: id start end parent (-1 = root)
    res.prev, res.dist, res.mother              # per record of res.table (a RegionTable)
    res.pair_total                              # (n - 1) int64: the optimum of every frame pair
    masks = res.masks()                         # (n, h, w) uint16: pixel = track id
    write_result(res.rows, masks, res.frames, "01_RES")
    link_stack_host(stack_numpy)                # the same bytes through the host twins
"""
from __future__ import annotations

import ctypes
import glob
import os

import numpy as np

from . import _lib
from .measure import _host_u16, _vp, region_props, region_props_host


def gate_q(gate, what="gate", lowest=1):
    """round(16 gate): the gate in the 1/16 pixel of the quantised centroids."""
    q = int(np.floor(16.0 * float(gate) + 0.5))
    if q < lowest or q > 65535:
        raise ValueError(f"{what} must give {lowest} <= round(16 {what}) <= 65535, got {gate!r}")
    return q


class LinkResult:
    """What link_stack / link_stack_host return.

    rows (tracks, 4) int32: id, start, end, parent (-1 = root), as
    Tracker.tracks() gives them; table: the RegionTable of the stack; prev,
    dist, mother: per record (the record index of the linked predecessor / that
    link's squared distance in 1/256 pixel^2 / the record index of a birth's
    division candidate; -1 = none); pair_total (n - 1) int64; ids: the track id
    of every record; frames: the frame numbers."""

    def __init__(self, rows, prev, dist, mother, pair_total, ids, table, frames, stack):
        self.rows, self.prev, self.dist, self.mother = rows, prev, dist, mother
        self.pair_total, self.ids, self.table, self.frames = pair_total, ids, table, frames
        self._stack = stack
        self._tracker = None

    def frame_map(self, index):
        """(frame number, ascending labels, track ids) of the index-th frame."""
        a, b = int(self.table.frame_offsets[index]), int(self.table.frame_offsets[index + 1])
        return int(self.frames[index]), self.table.label[a:b].astype(np.int32), self.ids[a:b].copy()

    def tracker(self):
        """A Tracker that holds this result (unet_tracker_load_result): its
        tracks(), frame_map() and relabel() serve the linker's output."""
        if self._tracker is None:
            from .track import Tracker
            _, h, w = self.table.shape
            dev = self._stack.device if hasattr(self._stack, "device") else "cpu"   # (a host stack: no relabel)
            tr = Tracker(max(h, 1), max(w, 1), device=dev)
            n = len(self.frames)
            rows = np.ascontiguousarray(self.rows, np.int32)
            labels = np.ascontiguousarray(self.table.label, np.int32)
            offsets = np.ascontiguousarray(self.table.frame_offsets, np.int32)
            ids = np.ascontiguousarray(self.ids, np.int32)
            frames = np.ascontiguousarray(self.frames, np.int32)
            rc = tr.lib.unet_tracker_load_result(tr.handle, _vp(rows), len(rows), _vp(frames), n,
                                                 offsets.ctypes.data_as(ctypes.c_void_p), _vp(labels), _vp(ids))
            _lib.check(rc, "unet_tracker_load_result")
            self._tracker = tr
        return self._tracker

    def masks(self):
        """tracker().relabel(stack, frames): (n, h, w) uint16 on the device,
        pixel = track id.  The stack must be a device tensor."""
        import torch
        if not isinstance(self._stack, torch.Tensor):
            raise ValueError("masks() relabels on the HIP device: link a device stack (no CPU fallback)")
        return self.tracker().relabel(self._stack, self.frames)


def _frames(frames, n):
    fr = np.arange(n, dtype=np.int32) if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1),
                                                                                   np.int32)
    if len(fr) != n:
        raise ValueError(f"{len(fr)} frame numbers for {n} frames")
    if np.any(np.diff(fr) <= 0):
        raise ValueError("frame numbers must ascend strictly")
    return fr


def _assemble(lib, table, fr, prev, dist, mother, pair_total, division_min_ratio, max_children, stack):
    n = len(fr)
    total = len(table)
    rec = np.ascontiguousarray(table.records)
    offsets = np.ascontiguousarray(table.frame_offsets, np.int32)
    rows = np.zeros((total, 4), np.int32)
    ids = np.zeros(total, np.int32)
    k = lib.unet_link_assemble(_vp(rec), offsets.ctypes.data_as(ctypes.c_void_p), n, _vp(fr), _vp(prev), _vp(dist),
                               _vp(mother), float(division_min_ratio), int(max_children), _vp(rows), total, _vp(ids))
    if k < 0:
        _lib.check(k, "unet_link_assemble")
    return LinkResult(rows[:k].copy(), prev, dist, mother, pair_total, ids, table, fr, stack)


def link_stack(stack, frames=None, image=None, gate=20.0, division_gate=0.0, division_min_ratio=0.5,
               max_children=2) -> LinkResult:
    """Links a (n, h, w) device stack of instance labelings by centroid
    distance.  gate: the largest centroid distance of a link, in pixels;
    division_gate: the largest distance between a birth and the mother it
    names (0, the default, turns divisions off: a bare call links only);
    division_min_ratio: the least area ratio between the mother's successor and
    the birth; max_children: the most daughters of one division.

    The gate and the ratio are starting values: their effect on TRA has not
    been measured.

    unet_region_props writes the records into device buffers, unet_link_frames
    runs on them (one launch for all n - 1 frame pairs), the three small arrays
    and the records return to the host, and unet_link_assemble builds the
    tracks."""
    import torch
    gq = gate_q(gate)
    dq = gate_q(division_gate, "division_gate", 0)
    lib = _lib.load()
    table, rec_dev, off_dev = region_props(stack, image, keep_device=True)
    n = table.shape[0]
    fr = _frames(frames, n)
    total = len(table)
    dev = rec_dev.device
    prev = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    mother = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    dist = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    pair_total = torch.empty(max(n - 1, 1), dtype=torch.int64, device=dev)
    ws = torch.empty(max(lib.unet_link_ws_bytes(n, total), 256), dtype=torch.uint8, device=dev)
    _lib.check(lib.unet_link_frames(rec_dev.data_ptr(), off_dev.data_ptr(), n, total, gq, dq, prev.data_ptr(),
                                    dist.data_ptr(), mother.data_ptr(), pair_total.data_ptr(), ws.data_ptr(),
                                    _lib.stream_of(dev)), "unet_link_frames")
    return _assemble(lib, table, fr, prev[:total].cpu().numpy(), dist[:total].cpu().numpy(),
                     mother[:total].cpu().numpy(), pair_total[:max(n - 1, 0)].cpu().numpy(), division_min_ratio,
                     max_children, stack)


def link_table_host(table, gate=20.0, division_gate=0.0):
    """(prev, dist, mother, pair_total) of a RegionTable through the host twin
    (unet_link_frames_host): plain loops, no device."""
    gq = gate_q(gate)
    dq = gate_q(division_gate, "division_gate", 0)
    lib = _lib.load()
    n, total = table.shape[0], len(table)
    rec = np.ascontiguousarray(table.records)
    offsets = np.ascontiguousarray(table.frame_offsets, np.int32)
    prev = np.zeros(total, np.int32)
    mother = np.zeros(total, np.int32)
    dist = np.zeros(total, np.int64)
    pair_total = np.zeros(max(n - 1, 0), np.int64)
    rc = lib.unet_link_frames_host(_vp(rec), offsets.ctypes.data_as(ctypes.c_void_p), n, total, gq, dq, _vp(prev),
                                   _vp(dist), _vp(mother), _vp(pair_total))
    _lib.check(rc, "unet_link_frames_host")
    return prev, dist, mother, pair_total


def link_stack_host(stack, frames=None, image=None, gate=20.0, division_gate=0.0, division_min_ratio=0.5,
                    max_children=2) -> LinkResult:
    """link_stack over NumPy arrays through region_props_host and the host twin
    of the kernel: the same bytes, no device (masks() needs a device stack)."""
    gate_q(gate), gate_q(division_gate, "division_gate", 0)
    lab = _host_u16(stack, "link_stack_host")
    table = region_props_host(lab, image)
    fr = _frames(frames, table.shape[0])
    prev, dist, mother, pair_total = link_table_host(table, gate, division_gate)
    return _assemble(_lib.load(), table, fr, prev, dist, mother, pair_total, division_min_ratio, max_children, lab)


def link_directory(instance_masks_dir, device=None, **link_kwargs):
    """Links instance_masks_dir/mXXX.tif (sorted; XXX = the frame number), as
    track_directory does for the IoU tracker: (LinkResult, frame numbers, the
    (n, h, w) device stack), or None with the reference's message when no mask
    is found."""
    import torch
    from PIL import Image
    files = sorted(glob.glob(os.path.join(instance_masks_dir, "m*.tif")))
    if not files:
        print(f"Error: No instance masks (mXXX.tif) found in {instance_masks_dir}.")
        return None
    dev = torch.device("cuda") if device is None else torch.device(device)
    frames = [int(os.path.basename(p)[1:4]) for p in files]
    stack = torch.from_numpy(np.stack([np.array(Image.open(p)).astype(np.int32) for p in files])).to(dev)
    res = link_stack(stack, frames, **link_kwargs)
    return res, frames, stack
