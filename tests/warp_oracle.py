"""NumPy oracle of the warping error (include/unet_hip.h, unet_warping_error):
the simple-point table by component counting with scipy.ndimage.label, the
separation rule, the mask and the vectorised four-sub-field schedule, which can
stop after k sweeps.  Independent of the library: nothing here calls it."""
import numpy as np
from scipy import ndimage

# neighbour k of N, NE, E, SE, S, SW, W, NW as (dy, dx)
NB = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))
S8 = np.ones((3, 3), bool)
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)

_TABLE = None


def simple_table():
    """(256,) uint8: 1 where the configuration of the 8 neighbours (bit k =
    neighbour k of NB) makes the centre a simple point: the foreground of N* is
    one 8-connected component and exactly one 4-connected background component
    of N* is 4-adjacent to the centre."""
    global _TABLE
    if _TABLE is None:
        t = np.zeros(256, np.uint8)
        for c in range(256):
            fg = np.zeros((3, 3), bool)
            for k, (dy, dx) in enumerate(NB):
                fg[1 + dy, 1 + dx] = (c >> k) & 1
            bg = ~fg
            bg[1, 1] = False
            nf = ndimage.label(fg, S8)[1]
            lab = ndimage.label(bg, S4)[0]
            adjacent = {int(lab[0, 1]), int(lab[1, 0]), int(lab[1, 2]), int(lab[2, 1])} - {0}
            t[c] = nf == 1 and len(adjacent) == 1
        _TABLE = t
    return _TABLE


def ground_truth(gt, separate=True):
    """G0: gt > 0; with `separate`, minus the pixels whose 3 x 3 neighbourhood
    holds another non-zero id (out-of-frame pixels hold none)."""
    gt = np.asarray(gt).astype(np.int64)
    fg = gt > 0
    if separate:
        h, w = gt.shape
        p = np.pad(gt, 1)
        for dy, dx in NB:
            nb = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            fg &= ~((nb != 0) & (nb != gt))
    return fg


def mask(g0, radius):
    """M: the (2 radius + 1)^2 window, clipped to the frame, holds both a
    foreground and a background pixel; -1 = everywhere, 0 = nowhere."""
    if radius < 0:
        return np.ones(g0.shape, bool)
    if radius == 0:
        return np.zeros(g0.shape, bool)
    k = 2 * radius + 1
    has_fg = ndimage.maximum_filter(g0.astype(np.uint8), size=k, mode="constant", cval=0) > 0
    has_bg = ndimage.maximum_filter((~g0).astype(np.uint8), size=k, mode="constant", cval=0) > 0
    return has_fg & has_bg


def neighbour_index(lab, ys, xs):
    """the table index of the pixels (ys, xs) of the boolean labelling"""
    p = np.pad(lab, 1).astype(np.int64)
    idx = np.zeros(len(ys), np.int64)
    for k, (dy, dx) in enumerate(NB):
        idx |= p[ys + 1 + dy, xs + 1 + dx] << k
    return idx


def simple_at(lab, ys, xs):
    return simple_table()[neighbour_index(lab, ys, xs)].astype(bool)


def warp(g0, t, m, max_sweeps=0):
    """The schedule: returns (L, flips, sweeps, converged)."""
    lab = g0.copy()
    yy, xx = np.indices(lab.shape)
    fields = [((yy & 1) == (s >> 1)) & ((xx & 1) == (s & 1)) & m for s in range(4)]
    flips = sweeps = 0
    while True:
        n = 0
        for s in range(4):
            ys, xs = np.nonzero(fields[s] & (lab != t))
            keep = simple_at(lab, ys, xs)  # all evaluated on lab as it stands, then flipped at once
            ys, xs = ys[keep], xs[keep]
            lab[ys, xs] ^= True
            n += len(ys)
        sweeps += 1
        flips += n
        if n == 0:
            return lab, flips, sweeps, 1
        if max_sweeps > 0 and sweeps >= max_sweeps:
            return lab, flips, sweeps, 0


def evaluate(gt, pred, radius=4, separate=True, max_sweeps=0):
    """One frame: {"counts": int64 (pixel error, warping error, flips, sweeps,
    converged), "warped": uint8 0 / 1, "g0", "t", "m": bool}."""
    g0 = ground_truth(gt, separate)
    t = np.asarray(pred) > 0
    m = mask(g0, radius)
    lab, flips, sweeps, conv = warp(g0, t, m, max_sweeps)
    counts = np.array([int((g0 != t).sum()), int((lab != t).sum()), flips, sweeps, conv], np.int64)
    return {"counts": counts, "warped": lab.astype(np.uint8), "g0": g0, "t": t, "m": m}


def evaluate_stack(gt, pred, **kw):
    """(N, H, W) stacks: (counts (N, 5), warped (N, H, W))."""
    r = [evaluate(g, p, **kw) for g, p in zip(gt, pred)]
    return np.stack([x["counts"] for x in r]), np.stack([x["warped"] for x in r])
