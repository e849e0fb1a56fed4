"""Per-object measurements and track dynamics of a whole sequence on the
MI355X: what the reference's README calls "insights into cellular dynamics"
and its step 8 an "Average Displacement Error", neither of which it computes.

One kernel pass (unet_region_props, csrc/region.hip) turns a (n, h, w) label
stack into one all-integer record per object per frame; everything else here is
derived from those integers in float64 on the host, so the device path and the
host twin (region_props_host) give bit-equal tables.

    t = region_props(labels, image)          # (n, h, w) device tensors -> RegionTable
    t.area, t.centroid_y, t.major_axis, t.eccentricity, t.touches_edge, ...
    traj = trajectories(masks, frames, rows) # masks: pixel = track id (Tracker.relabel / track_stack)
    tables = dynamics(traj, rows, frame_interval=5.0, pixel_size=0.645)
    tables["tracks"], tables["divisions"], tables["frames"]   # dicts of columns
    displacement_error(gt_masks, gt_rows, res_masks, res_rows, frames)

The formulas are written out in DESIGN.md, "Object measurements and track
dynamics".
"""
from __future__ import annotations

import ctypes
import errno

import numpy as np

from . import _lib

# unet_region_record of include/unet_hip.h
INT32_FIELDS = ("frame", "label", "area", "boundary", "edge", "min_y", "min_x", "max_y", "max_x", "min_v", "max_v")
INT64_FIELDS = ("sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy", "sum_v", "sum_vv", "contact")
RECORD = np.dtype([(k, np.int32) for k in INT32_FIELDS + ("reserved0",)]
                  + [(k, np.int64) for k in INT64_FIELDS] + [("reserved1", np.int64, (2,))])
assert RECORD.itemsize == 128
DERIVED = ("centroid_y", "centroid_x", "mu_yy", "mu_xx", "mu_xy", "major_axis", "minor_axis", "eccentricity",
           "orientation", "mean_v", "std_v", "touches_edge")


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def _central(n, s1a, s1b, s2):
    """(n s2 - s1a s1b) / n^2 with the numerator exact: in int64 where it
    fits, in Python integers where a term may pass 2^62."""
    n, s1a, s1b, s2 = (np.asarray(v, np.int64) for v in (n, s1a, s1b, s2))
    big = (n.astype(np.float64) * np.abs(s2) >= 2.0 ** 62) | (np.abs(s1a).astype(np.float64) * np.abs(s1b) >= 2.0 ** 62)
    num = np.where(big, 0, n * s2 - s1a * s1b).astype(np.float64)
    for i in np.flatnonzero(big):
        num[i] = float(int(n[i]) * int(s2[i]) - int(s1a[i]) * int(s1b[i]))
    nf = n.astype(np.float64)
    return num / (nf * nf)


class RegionTable:
    """The records of region_props / region_props_host.

    records: structured array (RECORD), ordered by frame, then ascending label;
    frame_offsets: (n + 1) int32, the records of frame f are
    [frame_offsets[f], frame_offsets[f + 1]); shape: (n, h, w); has_image.
    Every integer field is an attribute (area, sum_y, ...), and so is every
    derived float64 column (DERIVED), computed from the integers on first use."""

    def __init__(self, records, frame_offsets, shape, has_image):
        self.records = records
        self.frame_offsets = frame_offsets
        self.shape = tuple(int(v) for v in shape)
        self.has_image = bool(has_image)
        self._derived = None

    def __len__(self):
        return len(self.records)

    def __getattr__(self, name):
        if name in INT32_FIELDS or name in INT64_FIELDS:
            return self.records[name]
        if name in DERIVED:
            if self._derived is None:
                self._derived = derive(self.records)
            return self._derived[name]
        raise AttributeError(name)

    def columns(self):
        """Every integer and derived column, in a fixed order, as a dict."""
        return {k: getattr(self, k) for k in INT32_FIELDS + INT64_FIELDS + DERIVED}

    def take(self, index):
        """The table of records[index] (no frame_offsets: the order is the caller's)."""
        return RegionTable(self.records[index], None, self.shape, self.has_image)


def derive(rec):
    """The float64 columns of DESIGN.md from the integer records."""
    a = rec["area"].astype(np.int64)
    af = a.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cy = rec["sum_y"] / af
        cx = rec["sum_x"] / af
        myy = _central(a, rec["sum_y"], rec["sum_y"], rec["sum_yy"])
        mxx = _central(a, rec["sum_x"], rec["sum_x"], rec["sum_xx"])
        mxy = _central(a, rec["sum_y"], rec["sum_x"], rec["sum_xy"])
        half = 0.5 * (myy + mxx)
        dev = np.sqrt((0.5 * (myy - mxx)) ** 2 + mxy * mxy)
        l1 = half + dev
        l2 = np.maximum(half - dev, 0.0)
        major = 4.0 * np.sqrt(l1)
        minor = 4.0 * np.sqrt(l2)
        ecc = np.where(l1 > 0, np.sqrt(np.maximum(1.0 - l2 / np.where(l1 > 0, l1, 1.0), 0.0)), 0.0)
        # angle of the major axis from the +x (column) axis towards +y (row), in (-pi/2, pi/2]
        orient = 0.5 * np.arctan2(2.0 * mxy, mxx - myy)
        mean_v = rec["sum_v"] / af
        std_v = np.sqrt(np.maximum(_central(a, rec["sum_v"], rec["sum_v"], rec["sum_vv"]), 0.0))
    return {"centroid_y": cy, "centroid_x": cx, "mu_yy": myy, "mu_xx": mxx, "mu_xy": mxy, "major_axis": major,
            "minor_axis": minor, "eccentricity": ecc, "orientation": orient, "mean_v": mean_v, "std_v": std_v,
            "touches_edge": rec["edge"] > 0}


def _device_stack(x, what):
    import torch
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise ValueError(f"{what} runs on the HIP device only (no CPU fallback)")
    if x.dim() != 3:
        raise ValueError(f"{what}: the stack must be (n, h, w), got {tuple(x.shape)}")
    return x


def region_props(labels, image=None, cap=None, keep_device=False) -> RegionTable:
    """labels (n, h, w) integer labels on the HIP device (0 = background, uint16
    or any integer dtype within [0, 65535]); image None or (n, h, w) uint8 on
    the same device.  cap: records to provide for on the first try (default: a
    guess of 256 per frame); if the stack holds more the call is repeated once
    with the exact total.  keep_device: return (table, the device buffer of the
    records, the device frame offsets) for a kernel that reads them in place."""
    import torch
    from .postproc import _u16
    lab = _device_stack(labels, "region_props")
    if lab.dtype != torch.uint16 and lab.numel():
        if lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise ValueError(f"labels must be integers, got {lab.dtype}")
        lo, hi = torch.aminmax(lab)
        if int(lo) < 0 or int(hi) >= 65536:
            raise ValueError(f"labels must lie in [0, 65535], got [{int(lo)}, {int(hi)}]")
    lab = _u16(lab).contiguous()
    n, h, w = (int(v) for v in lab.shape)
    img = None
    if image is not None:
        img = _device_stack(image, "region_props")
        if img.dtype != torch.uint8 or tuple(img.shape) != tuple(lab.shape) or img.device != lab.device:
            raise ValueError(f"image must be a uint8 stack of the labels' shape {tuple(lab.shape)} on their device, "
                             f"got {img.dtype} {tuple(img.shape)}")
        img = img.contiguous()
    lib = _lib.load()
    need = lib.unet_region_props_ws_bytes(n, h, w)
    if need == 0:
        raise ValueError(f"region_props: unsupported stack size {(n, h, w)}: {_lib.last_error()}")
    ws = torch.empty(need, dtype=torch.uint8, device=lab.device)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=lab.device)
    cap = max(256 * n, 1024) if cap is None else int(cap)
    total = ctypes.c_longlong(0)
    for _ in range(2):
        rec = torch.empty((cap, RECORD.itemsize), dtype=torch.uint8, device=lab.device)
        rc = lib.unet_region_props(lab.data_ptr() if n else None, None if img is None else img.data_ptr(), n, h, w,
                                   offsets.data_ptr(), rec.data_ptr() if cap else None, cap, ctypes.byref(total),
                                   ws.data_ptr(), _lib.stream_of(lab.device))
        if rc != -errno.ENOSPC:
            break
        cap = int(total.value)
    _lib.check(rc, "unet_region_props")
    records = rec[:int(total.value)].cpu().numpy().reshape(-1).view(RECORD).copy()
    table = RegionTable(records, offsets.cpu().numpy(), (n, h, w), img is not None)
    return (table, rec, offsets) if keep_device else table


def _host_u16(labels, what):
    a = np.asarray(labels)
    if a.ndim != 3:
        raise ValueError(f"{what}: the stack must be (n, h, w), got {a.shape}")
    if a.dtype != np.uint16:
        if a.dtype.kind not in "iu":
            raise ValueError(f"labels must be integers, got {a.dtype}")
        if a.size and (a.min() < 0 or a.max() >= 65536):
            raise ValueError(f"labels must lie in [0, 65535], got [{a.min()}, {a.max()}]")
    return np.ascontiguousarray(a, np.uint16)


def region_props_host(labels, image=None, cap=None) -> RegionTable:
    """region_props over NumPy arrays, through the library's host twin
    (unet_region_props_host): plain loops, no device."""
    lab = _host_u16(labels, "region_props_host")
    n, h, w = lab.shape
    img = None
    if image is not None:
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.shape != lab.shape:
            raise ValueError(f"image must be a uint8 stack of the labels' shape {lab.shape}, got {img.dtype} {img.shape}")
        img = np.ascontiguousarray(img)
    lib = _lib.load()
    offsets = np.zeros(n + 1, np.int32)
    cap = max(256 * n, 1024) if cap is None else int(cap)
    total = ctypes.c_longlong(0)
    for _ in range(2):
        rec = np.zeros(cap, RECORD)
        rc = lib.unet_region_props_host(_vp(lab), _vp(img), n, h, w, _vp(offsets), _vp(rec), cap, ctypes.byref(total))
        if rc != -errno.ENOSPC:
            break
        cap = int(total.value)
    if rc == -errno.EINVAL:
        raise ValueError(f"region_props_host: {_lib.last_error()}")
    _lib.check(rc, "unet_region_props_host")
    return RegionTable(rec[:int(total.value)].copy(), offsets, (n, h, w), img is not None)


def _props(stack, images):
    """Device tensors go to the kernel, NumPy arrays to the host twin."""
    if isinstance(stack, np.ndarray):
        return region_props_host(stack, images)
    return region_props(stack, images)


def _rows(rows):
    r = np.array(rows, np.int64).reshape(-1, 4)
    if len(np.unique(r[:, 0])) != len(r):
        raise ValueError("a track id is listed twice")
    return r


class Trajectories:
    """The records of a track-labelled sequence sorted by (track, frame).

    table: RegionTable in that order (table.label is the track id); frame: the
    frame number of each record (frames[table.frame]); tracks: the ascending
    ids that occur; track_offsets: (len(tracks) + 1), the records of tracks[k]
    are [track_offsets[k], track_offsets[k + 1]); frames: the sequence's frame
    numbers; per_frame: the unsorted table (frame order), for per-frame sums."""

    def __init__(self, table, frame, tracks, track_offsets, frames, per_frame):
        self.table, self.frame, self.tracks, self.track_offsets = table, frame, tracks, track_offsets
        self.frames, self.per_frame = frames, per_frame

    def of(self, track):
        """slice of the records of one track id (empty if it never occurs)"""
        k = int(np.searchsorted(self.tracks, track))
        if k == len(self.tracks) or self.tracks[k] != track:
            return slice(0, 0)
        return slice(int(self.track_offsets[k]), int(self.track_offsets[k + 1]))


def trajectories(masks, frames, rows, images=None) -> Trajectories:
    """masks (n, h, w): track-labelled masks (pixel = track id), device tensor
    or NumPy array (host twin); frames: their n frame numbers, ascending; rows:
    (label, start, end, parent) track rows -- every id in the masks must have
    one."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    if frames.size != masks.shape[0]:
        raise ValueError(f"{masks.shape[0]} frames but {frames.size} frame numbers")
    if np.any(np.diff(frames) <= 0):
        raise ValueError("frame numbers must ascend")
    r = _rows(rows)
    t = _props(masks, images)
    unknown = np.setdiff1d(t.label, r[:, 0])
    if unknown.size:
        raise ValueError(f"track ids {unknown[:8].tolist()} occur in the masks but have no track row")
    order = np.lexsort((t.frame, t.label))     # (track, frame): frame index ascends with frame number
    s = t.take(order)
    tracks, first = np.unique(s.label, return_index=True)
    offsets = np.append(first, len(s)).astype(np.int64)
    return Trajectories(s, frames[s.frame], tracks.astype(np.int64), offsets, frames, t)


def dynamics(traj: Trajectories, rows, frame_interval=1.0, pixel_size=1.0):
    """{"tracks", "divisions", "frames"}: dicts of equally long columns.
    Lengths are in pixel_size units, areas in pixel_size^2, times in
    frame_interval units (DESIGN.md has the definitions)."""
    r = _rows(rows)
    px, dt = float(pixel_size), float(frame_interval)
    T = traj.table
    cy, cx, area = T.centroid_y * px, T.centroid_x * px, T.area.astype(np.float64) * px * px
    n = len(r)
    ids, start, end = r[:, 0], r[:, 1], r[:, 2]
    parent = np.where(r[:, 3] > 0, r[:, 3], 0)
    children = {}
    for k in range(n):
        if parent[k]:
            children.setdefault(int(parent[k]), []).append(int(ids[k]))
    tr = {k: np.zeros(n, np.float64) for k in ("path_length", "net_displacement", "mean_speed", "straightness",
                                               "mean_area", "first_area", "last_area")}
    present = np.zeros(n, np.int64)
    # a step: two successive present records of one track; it belongs to the frame it ends in
    step_frame, step_len = [], []
    for k in range(n):
        sl = traj.of(ids[k])
        m = sl.stop - sl.start
        present[k] = m
        if m == 0:
            continue
        y, x, f = cy[sl], cx[sl], traj.frame[sl]
        d = np.hypot(np.diff(y), np.diff(x))
        step_frame.extend(f[1:].tolist())
        step_len.extend(d.tolist())
        path = float(d.sum())
        net = float(np.hypot(y[-1] - y[0], x[-1] - x[0]))
        span = float(f[-1] - f[0]) * dt
        tr["path_length"][k] = path
        tr["net_displacement"][k] = net
        tr["mean_speed"][k] = path / span if span > 0 else 0.0
        tr["straightness"][k] = net / path if path > 0 else 0.0
        tr["mean_area"][k] = float(area[sl].mean())
        tr["first_area"][k] = float(area[sl][0])
        tr["last_area"][k] = float(area[sl][-1])
    nchild = np.array([len(children.get(int(i), ())) for i in ids], np.int64)
    cycle = np.where((parent > 0) & (nchild > 0), end - start + 1, -1)
    tracks = {"track": ids, "start": start, "end": end, "parent": parent, "frames_present": present, **tr,
              "children": nchild, "cycle_length": cycle}
    # divisions: a parent with two or more children; the first two by id are the daughters
    begin = {int(i): int(s) for i, s in zip(ids, start)}
    div = {k: [] for k in ("parent", "frame", "children", "child_a", "child_b", "area_ratio", "centroid_distance")}
    for p in sorted(children):
        ch = sorted(children[p])
        if len(ch) < 2:
            continue
        a, b = (traj.of(c) for c in ch[:2])
        ratio = dist = float("nan")
        if a.stop > a.start and b.stop > b.start:   # both daughters occur: their first records
            aa, ab = area[a.start], area[b.start]
            ratio = float(min(aa, ab) / max(aa, ab))
            dist = float(np.hypot(cy[a.start] - cy[b.start], cx[a.start] - cx[b.start]))
        for k, v in zip(div, (p, min(begin[c] for c in ch), len(ch), ch[0], ch[1], ratio, dist)):
            div[k].append(v)
    divisions = {k: np.array(v, np.float64 if k in ("area_ratio", "centroid_distance") else np.int64)
                 for k, v in div.items()}
    # frames
    P = traj.per_frame
    nf = len(traj.frames)
    fo = P.frame_offsets.astype(np.int64)
    hw = float(P.shape[1] * P.shape[2])

    def sums(v):   # per frame, in integers
        out = np.zeros(nf, np.int64)
        np.add.at(out, P.frame, v)
        return out

    step_frame, step_len = np.array(step_frame, np.int64), np.array(step_len, np.float64)
    mean_step = np.zeros(nf, np.float64)
    for i, f in enumerate(traj.frames):
        sel = step_len[step_frame == f]
        mean_step[i] = float(sel.mean()) if sel.size else 0.0
    frames = {"frame": traj.frames, "cells": fo[1:] - fo[:-1],
              "area_fraction": sums(P.area.astype(np.int64)) / hw if hw else np.zeros(nf),
              "contact": sums(P.contact), "mean_step": mean_step,
              "divisions": np.array([int(np.sum(divisions["frame"] == f)) for f in traj.frames], np.int64)}
    return {"tracks": tracks, "divisions": divisions, "frames": frames}


def _host_tables(gt, res, frames):
    """add_frame_host's dicts of two host stacks (the overlap tables in NumPy)."""
    out = []
    for f, g, r in zip(frames, gt, res):
        g, r = g.astype(np.int64).ravel(), r.astype(np.int64).ravel()
        gl, ga = np.unique(g[g > 0], return_counts=True)
        rl, ra = np.unique(r[r > 0], return_counts=True)
        both = (g > 0) & (r > 0)
        key, cnt = np.unique(g[both] << 16 | r[both], return_counts=True)
        out.append({"frame": int(f), "gt_labels": gl, "gt_areas": ga, "res_labels": rl, "res_areas": ra,
                    "pairs": np.stack([key >> 16, key & 0xffff, cnt], 1).reshape(-1, 3)})
    return out


def displacement_error(gt_masks, gt_rows, res_masks, res_rows, frames):
    """The README's "Average Displacement Error": the mean centroid distance
    (pixels) between every ground-truth object and the result object matched to
    it by the evaluator's rule -- a result object matches a ground-truth object
    when their overlap exceeds half the ground-truth object's area.

    gt_masks, res_masks (n, h, w) track-labelled, both device tensors or both
    NumPy arrays; frames their frame numbers; gt_rows / res_rows the track rows
    (res_rows may be None: the matching does not read it).  Returns {"ade",
    "matched", "total", "per_track": {"track", "matched", "total", "ade"}} with
    one per_track entry per gt_rows row; a mean over no match is NaN."""
    from .ctc import CTCEvaluator
    frames = np.asarray(frames, np.int64).reshape(-1)
    host = isinstance(gt_masks, np.ndarray)
    if host != isinstance(res_masks, np.ndarray):
        raise ValueError("gt_masks and res_masks must both be device tensors or both NumPy arrays")
    if tuple(gt_masks.shape) != tuple(res_masks.shape) or gt_masks.shape[0] != frames.size:
        raise ValueError(f"the stacks' sizes differ: gt {tuple(gt_masks.shape)}, res {tuple(res_masks.shape)}, "
                         f"{frames.size} frame numbers")
    if host:
        ev = CTCEvaluator.from_host_tables(tra_frames=_host_tables(_host_u16(gt_masks, "displacement_error"),
                                                                   _host_u16(res_masks, "displacement_error"), frames))
    else:
        ev = CTCEvaluator()
        ev.add_frames("TRA", gt_masks, res_masks, frames)
    G, R = _props(gt_masks, None), _props(res_masks, None)
    index_of = {int(f): i for i, f in enumerate(frames)}
    gt_ids = _rows(gt_rows)[:, 0]
    dist_sum = {int(t): 0.0 for t in gt_ids}
    hits = {int(t): 0 for t in gt_ids}
    seen = {int(t): 0 for t in gt_ids}
    dists = []
    for fr in sorted(ev.frames("TRA"), key=lambda d: d["frame"]):
        i = index_of[fr["frame"]]
        g0, r0 = int(G.frame_offsets[i]), int(R.frame_offsets[i])
        gl, rl = fr["gt_labels"], fr["res_labels"]
        garea = dict(zip(gl.tolist(), fr["gt_areas"].tolist()))
        for l in gl.tolist():
            if l not in seen:
                raise ValueError(f"ground-truth label {l} (frame {fr['frame']}) has no track row")
            seen[l] += 1
        for g, r, nn in fr["pairs"].tolist():
            if 2 * nn > garea[g]:
                a = g0 + int(np.searchsorted(gl, g))
                b = r0 + int(np.searchsorted(rl, r))
                d = float(np.hypot(G.centroid_y[a] - R.centroid_y[b], G.centroid_x[a] - R.centroid_x[b]))
                dists.append(d)
                dist_sum[g] += d
                hits[g] += 1
    nan = float("nan")
    per = {"track": gt_ids, "matched": np.array([hits[int(t)] for t in gt_ids], np.int64),
           "total": np.array([seen[int(t)] for t in gt_ids], np.int64),
           "ade": np.array([dist_sum[int(t)] / hits[int(t)] if hits[int(t)] else nan for t in gt_ids], np.float64)}
    return {"ade": float(np.sum(dists) / len(dists)) if dists else nan, "matched": len(dists), "total": len(G),
            "per_track": per}
