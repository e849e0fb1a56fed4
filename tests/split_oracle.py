"""NumPy / scipy.ndimage oracle of the marker-seeded instance masks
(include/unet_hip.h, unet_split_instances), following the definition step by
step: exact EDT, ndimage.label with the 3 x 3 structure, growth one geodesic
level at a time with a minimum filter, renumbering by first pixel.  Plus the
Cell Tracking Challenge's SEG by its definition, for the tests that compare
the split labelling with the plain one."""
import numpy as np
from scipy import ndimage

S8 = np.ones((3, 3), int)
NONE = 1 << 30  # d2 of a frame without a background pixel


def distance(fg):
    """Exact int32 squared distance to the nearest background pixel of the
    frame; 0 on background; NONE everywhere where there is no background."""
    if fg.all():
        return np.full(fg.shape, NONE, np.int32)
    idx = ndimage.distance_transform_edt(fg, return_distances=False, return_indices=True)
    yy, xx = np.indices(fg.shape)
    return ((yy - idx[0]).astype(np.int64) ** 2 + (xx - idx[1]).astype(np.int64) ** 2).astype(np.int32)


def grow(fg, lab):
    """lab: int64 marker labels (0 = none) within fg.  Every foreground pixel
    connected to a marker gets the label of the geodesically nearest one, the
    smallest label among equals; returns (labels, largest distance)."""
    lab = lab.copy()
    big = 1 << 40  # above any label
    level = 0
    while True:
        m = ndimage.minimum_filter(np.where(lab > 0, lab, big), footprint=S8, mode="constant", cval=big)
        new = fg & (lab == 0) & (m < big)
        if not new.any():
            return lab, level
        level += 1
        lab[new] = m[new]


def renumber(seg):
    """ids > 0 renumbered 1, 2, ... in raster order of their first pixel"""
    flat = seg.ravel()
    ids, first = np.unique(flat, return_index=True)
    first = first[ids > 0]
    ids = ids[ids > 0]
    lut = np.zeros(int(flat.max()) + 1, np.int64)
    lut[ids[np.argsort(first)]] = np.arange(1, ids.size + 1)
    return lut[seg]


def split(mask, core_d2=None, markers=None, min_size=15):
    """One (h, w) frame -> {"labels" uint16, "info" int32 (4,), "d2" int32}."""
    fg = np.asarray(mask) > 0
    d2 = distance(fg)
    mset = (fg & (d2 >= core_d2)) if markers is None else ((np.asarray(markers) > 0) & fg)
    lab, nm = ndimage.label(mset, S8)  # raster order of the first pixel
    lab, levels = grow(fg, lab.astype(np.int64))
    rest, _ = ndimage.label(fg & (lab == 0), S8)  # components without a marker
    seg = renumber(np.where(rest > 0, rest + nm, lab))
    ns = int(seg.max())
    sizes = np.bincount(seg.ravel(), minlength=ns + 1)
    out = np.where(sizes[seg] < min_size, 0, seg)
    info = np.array([nm, ns, levels, int(nm > 65535 or ns > 65535)], np.int32)
    return {"labels": out.astype(np.uint16), "info": info, "d2": d2}


def split_stack(masks, core_d2=None, markers=None, min_size=15):
    r = [split(m, core_d2, None if markers is None else markers[i], min_size) for i, m in enumerate(masks)]
    return {k: np.stack([f[k] for f in r]) for k in ("labels", "info", "d2")}


def plain(mask, min_size=15):
    """instance_masks: 8-connected components, small ones zeroed"""
    lab, n = ndimage.label(np.asarray(mask) > 0, S8)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    return np.where(sizes[lab] < min_size, 0, lab).astype(np.uint16)


def seg_measure(gt, res):
    """SEG of one frame pair: the mean over the ground-truth objects R of the
    Jaccard index with the result object S that covers more than half of R
    (0 where there is none)."""
    scores = []
    for l in np.unique(gt[gt > 0]):
        r = gt == l
        ids, cnt = np.unique(res[r], return_counts=True)
        cnt, ids = cnt[ids > 0], ids[ids > 0]
        j = 0.0
        if ids.size and 2 * cnt.max() > r.sum():
            s = res == ids[cnt.argmax()]
            j = (r & s).sum() / (r | s).sum()
        scores.append(j)
    return float(np.mean(scores))


def dumbbell(shift=0):
    """Two discs of radius 10 at (15, 15) and (15, 40 + shift), joined by the
    bar |y - 15| <= 1, in a 31 x 56 frame."""
    yy, xx = np.indices((31, 56))
    m = ((yy - 15) ** 2 + (xx - 15) ** 2 <= 100) | ((yy - 15) ** 2 + (xx - 40 - shift) ** 2 <= 100)
    m |= (abs(yy - 15) <= 1) & (xx >= 15) & (xx <= 40 + shift)
    return m.astype(np.uint8)


def random_stack(seed, n, h, w, density):
    g = np.random.default_rng(seed)
    return (ndimage.uniform_filter(g.random((n, h, w)), (0, 5, 5)) < 0.5 * density + 0.3).astype(np.uint8)


SHAPES = [(9, 31), (9, 32), (9, 33), (33, 65), (37, 45), (64, 64), (1, 1), (1, 70), (70, 1), (97, 130)]
