"""Small region tables for the linker tests (test_link_cpu.py and
test_gpu_link.py share them), and the calls of the library's host twin.

A table is (frame_offsets int32 (n + 1), cols): region_oracle's columns.
from_labels: through region_oracle of a label stack.  from_points: crafted
records with area 16 and sum_y = qy, sum_x = qx, which the quantisation maps to
exactly (qy, qx): floor((32 q + 16) / 32) = q -- any centroid in 1/16 pixel.
"""
import ctypes

import numpy as np

import region_oracle as RO


def from_labels(labels, oracle=RO.vectorised):
    return oracle(np.asarray(labels))


def from_points(frames):
    """frames: per frame a list of (qy, qx) or (qy, qx, area) in 1/16 pixel;
    labels are 1.. in list order."""
    cols = {k: [] for k in RO.FIELDS}
    offsets = [0]
    for f, pts in enumerate(frames):
        for k, p in enumerate(pts):
            area = p[2] if len(p) > 2 else 16
            assert p[0] * area % 16 == 0 and p[1] * area % 16 == 0
            row = dict.fromkeys(RO.FIELDS, 0)
            row.update(frame=f, label=k + 1, area=area, sum_y=p[0] * area // 16, sum_x=p[1] * area // 16)
            for key in RO.FIELDS:
                cols[key].append(row[key])
        offsets.append(len(cols["frame"]))
    return np.array(offsets, np.int32), {k: np.array(v, np.int64) for k, v in cols.items()}


def records(cols):
    """The columns as unet_region_record bytes (unet_amd.measure.RECORD)."""
    from unet_amd.measure import RECORD
    rec = np.zeros(len(cols["frame"]), RECORD)
    for k in RO.FIELDS:
        rec[k] = cols[k]
    return rec


def single_pixels(counts, h=24, w=24, seed=0):
    """A stack whose frame f holds counts[f] single-pixel objects at random
    places, labels 1.. in random order."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(counts), h, w), np.uint16)
    for f, c in enumerate(counts):
        at = rng.choice(h * w, c, replace=False)
        out[f].reshape(-1)[at] = rng.permutation(c) + 1
    return out


def lattice():
    """A 6 x 6 lattice of single-pixel objects, spacing 4, then the same shifted
    by half a spacing along x: every inner object is equidistant from two."""
    a = np.zeros((2, 24, 24), np.uint16)
    k = 1
    for y in range(1, 24, 4):
        for x in range(1, 24, 4):
            a[0, y, x] = k
            a[1, y, x + 2] = k
            k += 1
    return a


def chain(reverse):
    """64 objects on a line, 10 pixels apart, that all move 6 pixels to the
    right: each is nearest (4 pixels) to its left neighbour's successor.  With
    the labels descending along the line (reverse) every row first takes that
    nearest column and the last row's augmentation displaces all 63 others."""
    xs = [160 * i for i in range(64)]
    prev = [(80, x) for x in (reversed(xs) if reverse else xs)]
    cur = [(80, x + 96) for x in xs]
    return from_points([prev, cur])


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def host_link(lib, offsets, cols, gq, dq=0):
    """unet_link_frames_host: (rc, prev, dist, mother, pair_total)."""
    rec = records(cols)
    off = np.ascontiguousarray(offsets, np.int32)
    n, total = len(off) - 1, len(rec)
    prev = np.full(total, -7, np.int32)
    mother = np.full(total, -7, np.int32)
    dist = np.full(total, -7, np.int64)
    pair_total = np.full(max(n - 1, 0), -7, np.int64)
    rc = lib.unet_link_frames_host(vp(rec), off.ctypes.data_as(ctypes.c_void_p), n, total, gq, dq, vp(prev), vp(dist),
                                   vp(mother), vp(pair_total))
    return rc, prev, dist, mother, pair_total


def host_assemble(lib, offsets, cols, frames, prev, dist, mother, ratio=0.5, max_children=2):
    """unet_link_assemble: (count or error, rows, ids)."""
    rec = records(cols)
    off = np.ascontiguousarray(offsets, np.int32)
    fr = np.ascontiguousarray(frames, np.int32)
    total = len(rec)
    rows = np.zeros((total, 4), np.int32)
    ids = np.zeros(total, np.int32)
    k = lib.unet_link_assemble(vp(rec), off.ctypes.data_as(ctypes.c_void_p), len(off) - 1, vp(fr),
                               vp(np.ascontiguousarray(prev, np.int32)), vp(np.ascontiguousarray(dist, np.int64)),
                               vp(np.ascontiguousarray(mother, np.int32)), float(ratio), int(max_children), vp(rows),
                               total, vp(ids))
    return k, rows[:max(k, 0)], ids
