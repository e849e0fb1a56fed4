"""NumPy oracles of the per-object records (unet_region_props) and of the
displacement error, int64 throughout.

direct(labels, image): one np.argwhere per label and frame, as the reference's
get_mask_properties (scripts/track.py:39-70) walks a frame; for small cases.
vectorised(labels, image): sort + np.add.reduceat / np.minimum.reduceat over the
foreground pixels of the whole stack; for the full stacks.
Both return (frame_offsets int32 (n + 1), dict of int64 columns), objects
ordered by frame, then ascending label (np.unique's order).
ade(...): the matching rule and the mean centroid distance in plain NumPy.
"""
import numpy as np

FIELDS = ("frame", "label", "area", "boundary", "edge", "min_y", "min_x", "max_y", "max_x", "min_v", "max_v",
          "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy", "sum_v", "sum_vv", "contact")
OUT = 1 << 16   # a neighbour outside the frame: equals no label


def neighbours(frame):
    """(up, down, left, right) label planes of an (h, w) frame, OUT outside."""
    p = np.full((frame.shape[0] + 2, frame.shape[1] + 2), OUT, np.int64)
    p[1:-1, 1:-1] = frame
    return p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]


def direct(labels, image=None):
    labels = np.asarray(labels).astype(np.int64)
    n, h, w = labels.shape
    cols = {k: [] for k in FIELDS}
    offsets = [0]
    for f in range(n):
        frame = labels[f]
        nb = neighbours(frame)
        for lab in np.unique(frame):
            if lab == 0:
                continue
            coords = np.argwhere(frame == lab)           # track.py:53
            y, x = coords[:, 0], coords[:, 1]
            around = [q[y, x] for q in nb]
            row = dict(frame=f, label=int(lab), area=len(coords), sum_y=y.sum(), sum_x=x.sum(), sum_yy=(y * y).sum(),
                       sum_xx=(x * x).sum(), sum_xy=(y * x).sum(),
                       min_y=y.min(), min_x=x.min(), max_y=y.max(), max_x=x.max(),    # track.py:61-62
                       boundary=int(np.any([q != lab for q in around], axis=0).sum()),
                       edge=int(((y == 0) | (y == h - 1) | (x == 0) | (x == w - 1)).sum()),
                       contact=int(sum(((q != lab) & (q != 0) & (q != OUT)).sum() for q in around)),
                       sum_v=0, sum_vv=0, min_v=0, max_v=0)
            if image is not None:
                v = np.asarray(image)[f][y, x].astype(np.int64)
                row.update(sum_v=v.sum(), sum_vv=(v * v).sum(), min_v=v.min(), max_v=v.max())
            for k in FIELDS:
                cols[k].append(int(row[k]))
        offsets.append(len(cols["frame"]))
    return np.array(offsets, np.int32), {k: np.array(v, np.int64) for k, v in cols.items()}


def vectorised(labels, image=None):
    labels = np.asarray(labels)
    n, h, w = labels.shape
    lab = labels.astype(np.int64)
    p = np.full((n, h + 2, w + 2), OUT, np.int64)
    p[:, 1:-1, 1:-1] = lab
    f, y, x = np.nonzero(lab)
    l = lab[f, y, x]
    key = f * 65536 + l
    order = np.argsort(key, kind="stable")
    f, y, x, l, key = f[order], y[order], x[order], l[order], key[order]
    first = np.flatnonzero(np.append(True, key[1:] != key[:-1])) if key.size else np.zeros(0, np.int64)
    add = (lambda v: np.add.reduceat(v.astype(np.int64), first)) if key.size else (lambda v: np.zeros(0, np.int64))
    lo = (lambda v: np.minimum.reduceat(v, first)) if key.size else (lambda v: np.zeros(0, np.int64))
    hi = (lambda v: np.maximum.reduceat(v, first)) if key.size else (lambda v: np.zeros(0, np.int64))
    around = [p[f, y, x + 1], p[f, y + 2, x + 1], p[f, y + 1, x], p[f, y + 1, x + 2]]   # up, down, left, right
    boundary = np.zeros(len(l), bool)
    contact = np.zeros(len(l), np.int64)
    for q in around:
        boundary |= q != l
        contact += (q != l) & (q != 0) & (q != OUT)
    cols = dict(frame=f[first], label=l[first], area=add(np.ones(len(l), np.int64)), sum_y=add(y), sum_x=add(x),
                sum_yy=add(y * y), sum_xx=add(x * x), sum_xy=add(y * x), min_y=lo(y), min_x=lo(x), max_y=hi(y),
                max_x=hi(x), boundary=add(boundary), contact=add(contact),
                edge=add((y == 0) | (y == h - 1) | (x == 0) | (x == w - 1)))
    zero = np.zeros(len(first), np.int64)
    if image is None:
        cols.update(sum_v=zero, sum_vv=zero, min_v=zero, max_v=zero)
    else:
        v = np.asarray(image)[f, y, x].astype(np.int64)
        cols.update(sum_v=add(v), sum_vv=add(v * v), min_v=lo(v), max_v=hi(v))
    cols = {k: np.asarray(cols[k], np.int64) for k in FIELDS}
    offsets = np.searchsorted(cols["frame"], np.arange(n + 1), "left").astype(np.int32)
    return offsets, cols


def table_columns(table):
    """The integer columns of a unet_amd.measure.RegionTable as the oracles give them."""
    return {k: np.asarray(getattr(table, k), np.int64) for k in FIELDS}


def assert_equal(table, want):
    offsets, cols = want
    np.testing.assert_array_equal(table.frame_offsets, offsets)
    got = table_columns(table)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], cols[k], err_msg=k)
    assert not table.records["reserved0"].any() and not table.records["reserved1"].any()


def ade(gt, res, frames=None):
    """Mean centroid distance over the ground-truth objects that a result object
    overlaps by more than half their area: (ade, matched, total, {gt label:
    [distances]})."""
    gt, res = np.asarray(gt).astype(np.int64), np.asarray(res).astype(np.int64)
    dists, per, total = [], {}, 0
    for g, r in zip(gt, res):
        for lab in np.unique(g):
            if lab == 0:
                continue
            total += 1
            per.setdefault(int(lab), [])
            at = np.argwhere(g == lab)
            under, cnt = np.unique(r[g == lab], return_counts=True)
            for u, c in zip(under, cnt):
                if u != 0 and 2 * c > len(at):
                    d = float(np.hypot(*(at.mean(0) - np.argwhere(r == u).mean(0))))
                    dists.append(d)
                    per[int(lab)].append(d)
    return (float(np.mean(dists)) if dists else float("nan")), len(dists), total, per
