"""Cell Tracking Challenge measures SEG / DET / TRA on the MI355X: the step the
reference's README calls "Evaluate Segmentation and Tracking", for which it
ships only Windows and macOS binaries.  The overlap records of whole label
stacks come from the GPU (unet_ctc_add_frames), the matching and the graph
comparison run in the library's native host code (csrc/ctc.hip).

    ev = CTCEvaluator()
    ev.add_frames("SEG", gt_seg, res_at_seg_frames, seg_frame_numbers)   # (T, h, w) uint16, device
    ev.add_frames("TRA", gt_tra, res, frame_numbers)
    ev.set_tracks("GT", man_track_rows); ev.set_tracks("RES", res_track_rows)
    ev.measures()   # {"SEG":, "DET":, "TRA":, "counts": {"NS":, "FN":, ...}}
    ev.log()        # the text of the evaluator's TRA_log.txt
    seg_measure(gt_stack, res_stack)
    evaluate_sequence("data/01_GT", "data/01_RES")
"""
from __future__ import annotations

import ctypes
import glob
import os
import re

import numpy as np

from . import _lib

KINDS = {"SEG": 0, "TRA": 1}
SIDES = {"GT": 0, "RES": 1}
COUNT_NAMES = ("NS", "FN", "FP", "ED", "EA", "EC", "V_GT", "E_GT")
STAT_NAMES = ("chunks", "launches", "syncs", "dense_frames", "hashed_frames", "records")


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


class CTCEvaluator:
    def __init__(self):
        self.lib = _lib.load()
        self.handle = self.lib.unet_ctc_create()
        self.ws = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.unet_ctc_destroy(h)
            self.handle = None

    # ------------------------------ device path ------------------------------
    def add_frames(self, kind, gt, res, frames):
        """T frame pairs: gt, res (T, h, w) integer label stacks on the HIP
        device (labels 0..65535, 0 = background), frames their T frame numbers."""
        import torch
        from .postproc import _u16
        if gt.device.type != "cuda" or res.device.type != "cuda":
            raise ValueError("CTCEvaluator.add_frames runs on the HIP device only (from_host_tables is the CPU path)")
        if gt.dim() != 3 or tuple(gt.shape) != tuple(res.shape):
            raise ValueError(f"the stacks' sizes differ: gt {tuple(gt.shape)}, res {tuple(res.shape)}")
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        t, h, w = (int(v) for v in gt.shape)
        if frames.size != t:
            raise ValueError(f"{t} frames but {frames.size} frame numbers")
        for x in (gt, res):
            if x.dtype != torch.uint16 and x.numel():
                lo, hi = torch.aminmax(x)
                if int(lo) < 0 or int(hi) >= 65536:
                    raise ValueError(f"labels must lie in [0, 65535], got [{int(lo)}, {int(hi)}]")
        g, r = _u16(gt).contiguous(), _u16(res).contiguous()
        need = self.lib.unet_ctc_ws_bytes(max(t, 1), h, w)
        if t and (self.ws is None or self.ws.numel() < need or self.ws.device != g.device):
            self.ws = torch.empty(need, dtype=torch.uint8, device=g.device)
        _lib.check(self.lib.unet_ctc_add_frames(self.handle, KINDS[kind], g.data_ptr() if t else None,
                                                r.data_ptr() if t else None, _vp(frames), t, h, w,
                                                self.ws.data_ptr() if t else None, _lib.stream_of(g.device)),
                   "unet_ctc_add_frames")

    # ------------------------------- host path -------------------------------
    def add_frame_host(self, kind, frame, gt_labels, gt_areas, res_labels, res_areas, pairs):
        """One frame from host tables: ascending labels and areas of both
        sides, pairs (n, 3) = (gt label, res label, overlap).  res_labels None
        = the GT frame has no RES frame (an error the library words)."""
        gl = np.ascontiguousarray(gt_labels, np.int32)
        ga = np.ascontiguousarray(gt_areas, np.int64)
        if res_labels is None:
            rl = ra = None
            nr = -1
        else:
            rl = np.ascontiguousarray(res_labels, np.int32)
            ra = np.ascontiguousarray(res_areas, np.int64)
            nr = rl.size
        pr = np.ascontiguousarray(pairs, np.int64).reshape(-1, 3)
        if ga.size != gl.size or (rl is not None and ra.size != rl.size):
            raise ValueError("one area per label")
        _lib.check(self.lib.unet_ctc_add_frame_host(self.handle, KINDS[kind], int(frame), gl.size, _vp(gl), _vp(ga), nr,
                                                    _vp(rl), _vp(ra), pr.shape[0], _vp(pr)),
                   "unet_ctc_add_frame_host")

    @classmethod
    def from_host_tables(cls, seg_frames=(), tra_frames=(), gt_tracks=None, res_tracks=None):
        """The CPU path: frames as dicts with the keys of add_frame_host
        (frame, gt_labels, gt_areas, res_labels, res_areas, pairs)."""
        ev = cls()
        for kind, frames in (("SEG", seg_frames), ("TRA", tra_frames)):
            for f in frames:
                ev.add_frame_host(kind, f["frame"], f["gt_labels"], f["gt_areas"], f["res_labels"], f["res_areas"],
                                  f["pairs"])
        if gt_tracks is not None:
            ev.set_tracks("GT", gt_tracks)
        if res_tracks is not None:
            ev.set_tracks("RES", res_tracks)
        return ev

    # --------------------------------- both ----------------------------------
    def set_tracks(self, side, rows):
        """man_track.txt (side "GT") or res_track.txt ("RES") rows
        (label, begin, end, parent), in file order."""
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1, 4)
        _lib.check(self.lib.unet_ctc_set_tracks(self.handle, SIDES[side], _vp(rows), rows.shape[0]),
                   "unet_ctc_set_tracks")

    def measures(self):
        out = np.zeros(3, np.float64)
        cnt = np.zeros(8, np.int64)
        _lib.check(self.lib.unet_ctc_measures(self.handle, _vp(out), _vp(cnt)), "unet_ctc_measures")
        return {"SEG": float(out[0]), "DET": float(out[1]), "TRA": float(out[2]),
                "counts": {k: int(v) for k, v in zip(COUNT_NAMES, cnt)}}

    def log(self) -> str:
        n = self.lib.unet_ctc_log(self.handle, None, 0)
        if n < 0:
            _lib.check(int(n), "unet_ctc_log")
        buf = ctypes.create_string_buffer(int(n))
        self.lib.unet_ctc_log(self.handle, buf, int(n))
        return buf.value.decode()

    def frames(self, kind):
        """The stored frames of a kind as add_frame_host's dicts."""
        out = []
        k = KINDS[kind]
        for i in range(self.lib.unet_ctc_num_frames(self.handle, k)):
            sz = np.zeros(4, np.int32)
            _lib.check(self.lib.unet_ctc_frame_sizes(self.handle, k, i, _vp(sz)), "unet_ctc_frame_sizes")
            gl, ga = np.zeros(sz[1], np.int32), np.zeros(sz[1], np.int64)
            rl, ra = np.zeros(sz[2], np.int32), np.zeros(sz[2], np.int64)
            pr = np.zeros((sz[3], 3), np.int64)
            _lib.check(self.lib.unet_ctc_frame_tables(self.handle, k, i, _vp(gl), _vp(ga), _vp(rl), _vp(ra), _vp(pr)),
                       "unet_ctc_frame_tables")
            out.append({"frame": int(sz[0]), "gt_labels": gl, "gt_areas": ga, "res_labels": rl, "res_areas": ra,
                        "pairs": pr})
        return out

    def stats(self):
        out = np.zeros(6, np.int64)
        _lib.check(self.lib.unet_ctc_stats(self.handle, _vp(out)), "unet_ctc_stats")
        return {k: int(v) for k, v in zip(STAT_NAMES, out)}


def seg_measure(gt_stack, res_stack, frames=None):
    """SEG of two (T, h, w) device label stacks (frame i against frame i)."""
    ev = CTCEvaluator()
    ev.add_frames("SEG", gt_stack, res_stack, np.arange(gt_stack.shape[0]) if frames is None else frames)
    return ev.measures()["SEG"]


def read_track_file(path):
    with open(path) as f:
        rows = [list(map(int, ln.split())) for ln in f if ln.strip()]
    return np.array(rows, np.int32).reshape(-1, 4)


def _numbered(pattern):
    """frame number -> path for files whose name ends in digits"""
    out = {}
    for p in glob.glob(pattern):
        m = re.search(r"(\d+)\.tiff?$", os.path.basename(p))
        if m:
            out[int(m.group(1))] = p
    return out


def _stack(paths):
    from PIL import Image
    arrs = [np.array(Image.open(p)) for p in paths]
    for p, a in zip(paths, arrs):
        if a.ndim != 2:
            raise ValueError(f"{p}: the measures are for 2-D sequences, got an image of shape {a.shape}")
        if a.shape != arrs[0].shape:
            raise ValueError(f"the stacks' sizes differ: {p} is {a.shape}, {paths[0]} is {arrs[0].shape}")
    return np.stack(arrs).astype(np.int32)


def evaluate_sequence(gt_dir, res_dir, device=None):
    """Scores <seq>_RES against <seq>_GT: reads <gt_dir>/SEG/man_seg*.tif,
    <gt_dir>/TRA/man_track*.tif + man_track.txt and <res_dir>/mask*.tif +
    res_track.txt; a missing SEG or TRA part leaves its measures NaN.
    Returns {"SEG", "DET", "TRA", "counts", "log"}."""
    import torch
    dev = torch.device("cuda") if device is None else torch.device(device)
    res = _numbered(os.path.join(res_dir, "mask*.tif"))
    ev = CTCEvaluator()
    for kind, pattern in (("SEG", os.path.join(gt_dir, "SEG", "man_seg*.tif")),
                          ("TRA", os.path.join(gt_dir, "TRA", "man_track*.tif"))):
        gt = _numbered(pattern)
        if not gt:
            continue
        frames = sorted(gt)
        for n in frames:
            if n not in res:  # the library words the error
                ev.add_frame_host(kind, n, [], [], None, None, np.zeros((0, 3)))
        g = _stack([gt[n] for n in frames])
        r = _stack([res[n] for n in frames])
        if g.shape != r.shape:
            raise ValueError(f"the stacks' sizes differ: {gt_dir} {g.shape[1:]}, {res_dir} {r.shape[1:]}")
        ev.add_frames(kind, torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev), frames)
    gt_track = os.path.join(gt_dir, "TRA", "man_track.txt")
    res_track = os.path.join(res_dir, "res_track.txt")
    if os.path.exists(gt_track):
        ev.set_tracks("GT", read_track_file(gt_track))
    if os.path.exists(res_track):
        ev.set_tracks("RES", read_track_file(res_track))
    out = ev.measures()
    out["log"] = ev.log()
    return out
