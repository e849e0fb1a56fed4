"""Cell tracking over instance labelings (scripts/track.py:103-275) on the
MI355X: the per-frame object overlaps come from one GPU pass
(unet_tracker_add_frame), the lineage logic runs in the library's native
host tracker.

    tr = Tracker(h, w)                 # IOU 0.3 / 0.1, <= 2 children (track.py:21-24)
    for frame, labels in enumerate(instance_label_maps):   # (h, w) uint16 on the device
        tr.add_frame(labels, frame)
    rows = tr.tracks()                 # (n, 4) int32: label start end parent
    track_sequence(instance_masks_dir, output_track_file)  # the reference's entry point

Track-labelled result masks (what the Cell Tracking Challenge calls a result
sequence, and tools/ctc_measures.py --res reads): the tracker keeps, per frame,
which track each object holds when the frame's step ends; relabel() rewrites a
stack of instance labelings with those ids in one kernel launch.

    masks = tr.relabel(stack, frames)  # (n, h, w) uint16: pixel = track id
    rows, masks = track_stack(stack)   # both in one call
    write_result(rows, masks, frames, "01_RES")   # mask%03d.tif + res_track.txt (parent 0 = root)
"""
from __future__ import annotations

import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib
from .postproc import _u16

LABEL_SCOPES = {"shared": 0, "frame": 1}   # UNET_TRACK_SCOPE_*


class Tracker:
    def __init__(self, height, width, iou_track=0.3, iou_division=0.1, max_children=2, device=None,
                 label_scope="shared"):
        """label_scope "shared": the reference's single label -> track dictionary
        for the previous and the current frame (an object whose label equals a
        previous-frame label that is linked later in the same step loses its
        track again).  "frame": one table per frame, no such loss."""
        if label_scope not in LABEL_SCOPES:
            raise ValueError(f"label_scope must be one of {sorted(LABEL_SCOPES)}, got {label_scope!r}")
        self.lib = _lib.load()
        self.h, self.w = int(height), int(width)
        self.handle = self.lib.unet_tracker_create(self.h, self.w, float(iou_track), float(iou_division),
                                                   int(max_children))
        if not self.handle:
            raise ValueError(f"unet_tracker_create({height}, {width}, ...) rejected the arguments")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ws = None
        self.relabel_ws = None
        _lib.check(self.lib.unet_tracker_set_label_scope(self.handle, LABEL_SCOPES[label_scope]),
                   "unet_tracker_set_label_scope")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.unet_tracker_destroy(h)
            self.handle = None

    def _device_u16(self, labels, shape, what):
        if labels.device.type != "cuda":
            raise ValueError(f"Tracker.{what} runs on the HIP device only (no CPU fallback)")
        if tuple(labels.shape[-2:]) != (self.h, self.w) or labels.dim() != len(shape):
            raise ValueError(f"labels must be {shape}, got {tuple(labels.shape)}")
        if labels.dtype != torch.uint16 and labels.numel():
            # the device tables index labels as uint16: a wider label would wrap
            # (e.g. 65536 -> 0 = background, or merge with another object)
            lo, hi = torch.aminmax(labels)
            if int(lo) < 0 or int(hi) >= 65536:
                raise ValueError(f"labels must lie in [0, 65535], got [{int(lo)}, {int(hi)}]")
        return _u16(labels)

    def add_frame(self, labels: torch.Tensor, frame: int):
        """One frame's instance labeling (h, w), integer labels < 65536, on the
        HIP device (0 = background)."""
        lab = self._device_u16(labels, (self.h, self.w), "add_frame")
        if self.ws is None:
            self.ws = torch.empty(self.lib.unet_tracker_ws_bytes(self.h, self.w), dtype=torch.uint8,
                                  device=lab.device)
        _lib.check(self.lib.unet_tracker_add_frame(self.handle, lab.data_ptr(), int(frame), self.ws.data_ptr(),
                                                   _lib.stream_of(lab.device)), "unet_tracker_add_frame")

    def tracks(self) -> np.ndarray:
        n = self.lib.unet_tracker_num_tracks(self.handle)
        out = np.zeros((max(n, 0), 4), np.int32)
        _lib.check(0 if self.lib.unet_tracker_tracks(self.handle, out.ctypes.data_as(ctypes.c_void_p), n) == n
                   else -1, "unet_tracker_tracks")
        return out

    def num_frames(self) -> int:
        return int(self.lib.unet_tracker_num_frames(self.handle))

    def frame_map(self, index: int):
        """(frame number, ascending labels, track ids) of the index-th frame given:
        the track each object holds when that frame's step ends (0 = none)."""
        n = self.lib.unet_tracker_frame_map(self.handle, int(index), None, None, None, 0)
        if n < 0:
            raise IndexError(f"frame_map({index}): the tracker holds {self.num_frames()} frames")
        frame = ctypes.c_int32(0)
        labels = np.zeros(n, np.int32)
        ids = np.zeros(n, np.int32)
        self.lib.unet_tracker_frame_map(self.handle, int(index), ctypes.byref(frame),
                                        labels.ctypes.data_as(ctypes.c_void_p), ids.ctypes.data_as(ctypes.c_void_p), n)
        return int(frame.value), labels, ids

    def relabel(self, stack: torch.Tensor, frames, out=None) -> torch.Tensor:
        """(n, h, w) instance labelings on the HIP device -> uint16 masks whose
        pixels are track ids: frame i through the map of frame number frames[i]
        (background, unknown labels and trackless objects -> 0).  out may be
        the uint16 stack itself (in place).  One kernel launch."""
        fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), np.int32)
        n = len(fr)
        if stack.dim() != 3 or stack.shape[0] != n:
            raise ValueError(f"stack must be ({n}, {self.h}, {self.w}) for {n} frame numbers, "
                             f"got {tuple(stack.shape)}")
        lab = self._device_u16(stack, (n, self.h, self.w), "relabel")
        if out is None:
            out = torch.empty_like(lab)
        elif (out.dtype != torch.uint16 or out.shape != lab.shape or out.device != lab.device
              or not out.is_contiguous()):
            raise ValueError("out must be a contiguous uint16 tensor of the stack's shape on its device")
        if n == 0:
            return out
        need = self.lib.unet_tracker_relabel_ws_bytes(n, self.h, self.w)
        if self.relabel_ws is None or self.relabel_ws.numel() < need or self.relabel_ws.device != lab.device:
            self.relabel_ws = torch.empty(need, dtype=torch.uint8, device=lab.device)
        _lib.check(self.lib.unet_tracker_relabel(self.handle, lab.data_ptr(), fr.ctypes.data_as(ctypes.c_void_p), n,
                                                 out.data_ptr(), self.relabel_ws.data_ptr(),
                                                 _lib.stream_of(lab.device)), "unet_tracker_relabel")
        return out


def track_stack(stack: torch.Tensor, frames=None, **tracker_kwargs):
    """Tracks a (n, h, w) device stack of instance labelings (frame numbers
    0..n-1 unless given) and relabels it: (rows, masks) with rows as
    Tracker.tracks() and masks (n, h, w) uint16 whose pixels are track ids."""
    if stack.dim() != 3:
        raise ValueError(f"stack must be (n, h, w), got {tuple(stack.shape)}")
    n = stack.shape[0]
    frames = np.arange(n) if frames is None else np.asarray(frames).reshape(-1)
    if len(frames) != n:
        raise ValueError(f"{len(frames)} frame numbers for {n} frames")
    tr = Tracker(stack.shape[1], stack.shape[2], device=stack.device, **tracker_kwargs)
    for i in range(n):
        tr.add_frame(stack[i], int(frames[i]))
    return tr.tracks(), tr.relabel(stack, frames)


def ctc_rows(rows):
    """The rows with a root track's parent as 0 (the Cell Tracking Challenge's
    res_track.txt) instead of the reference's -1."""
    out = np.array(rows, np.int32).reshape(-1, 4)
    out[out[:, 3] < 0, 3] = 0
    return out


def write_result(rows, masks, frames, out_dir):
    """A Cell Tracking Challenge result sequence: out_dir/mask%03d.tif (uint16,
    pixel = track id, one per frame number) and out_dir/res_track.txt with
    parent 0 for root tracks.  masks: (n, h, w), a tensor or an array."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    m = masks.cpu() if isinstance(masks, torch.Tensor) else masks
    m = np.ascontiguousarray(m.view(torch.int16).numpy().view(np.uint16) if isinstance(m, torch.Tensor)
                             else np.asarray(m))
    if m.ndim != 3 or len(frames) != m.shape[0]:
        raise ValueError(f"masks must be (n, h, w) with one frame number each, got {m.shape} and {len(frames)}")
    if m.dtype != np.uint16:
        if m.size and (m.min() < 0 or m.max() > 65535):
            raise ValueError("track ids must lie in [0, 65535] for 16-bit masks")
        m = m.astype(np.uint16)
    for f, img in zip(frames, m):
        Image.fromarray(img).save(os.path.join(out_dir, f"mask{int(f):03d}.tif"))
    write_track_file(ctc_rows(rows), os.path.join(out_dir, "res_track.txt"))


def write_track_file(rows, path):
    """res_track.txt, one "label start end parent" line per track (track.py:265-272)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(f"{int(r[0])} {int(r[1])} {int(r[2])} {int(r[3])}\n")


def track_sequence(instance_masks_dir, output_track_file, device=None, result_dir=None, label_scope="shared"):
    """scripts/track.py:103 track_sequence: reads mXXX.tif (sorted), tracks,
    writes output_track_file (root parents -1, as the reference).  Returns the
    rows (None when no mask is found).  With result_dir it also writes the
    track-labelled masks and res_track.txt there (write_result)."""
    got = track_directory(instance_masks_dir, device=device, keep_stack=result_dir is not None,
                          label_scope=label_scope)
    if got is None:
        return None
    tr, frames, stack = got
    rows = tr.tracks()
    write_track_file(rows, output_track_file)
    if result_dir is not None:
        write_result(rows, tr.relabel(stack, frames), frames, result_dir)
    return rows


def track_directory(instance_masks_dir, device=None, keep_stack=True, **tracker_kwargs):
    """Tracks instance_masks_dir/mXXX.tif (sorted; XXX = the frame number):
    (tracker, frame numbers, the (n, h, w) device stack or None), or None with
    the reference's message when no mask is found."""
    from PIL import Image
    files = sorted(glob.glob(os.path.join(instance_masks_dir, "m*.tif")))
    if not files:
        print(f"Error: No instance masks (mXXX.tif) found in {instance_masks_dir}.")
        return None
    dev = torch.device("cuda") if device is None else torch.device(device)
    tr = None
    frames, kept = [], []
    for path in files:
        frame = int(os.path.basename(path)[1:4])
        m = np.array(Image.open(path))
        if tr is None:
            tr = Tracker(m.shape[0], m.shape[1], device=dev, **tracker_kwargs)
        d = torch.from_numpy(m.astype(np.int32)).to(dev)
        tr.add_frame(d, frame)
        frames.append(frame)
        if keep_stack:
            kept.append(d)
    return tr, frames, (torch.stack(kept) if keep_stack else None)


def result_stats(tracker, rows=None):
    """What a result sequence holds: the number of tracks, the objects left
    without a track (their pixels are 0 in the masks) and the rows that hold no
    pixel in some frame of their [start, end] -- the reference lets two parents
    claim one unmatched object as a child, and the second claim overwrites the
    first; the evaluator links present vertices only, so such rows are kept."""
    rows = tracker.tracks() if rows is None else rows
    present, frames, trackless = {}, [], 0   # track id -> the frames that show it
    for i in range(tracker.num_frames()):
        f, _, ids = tracker.frame_map(i)
        frames.append(f)
        trackless += int((ids == 0).sum())
        for t in ids[ids > 0].tolist():
            present.setdefault(t, set()).add(f)
    frames = np.sort(np.array(frames, np.int64))
    gaps = 0
    for tid, start, end, _ in np.asarray(rows).reshape(-1, 4).tolist():
        span = frames[np.searchsorted(frames, start, "left"):np.searchsorted(frames, end, "right")].tolist()
        gaps += any(f not in present.get(tid, ()) for f in span)
    return {"tracks": len(rows), "objects_without_track": trackless, "rows_with_absent_frames": gaps}
