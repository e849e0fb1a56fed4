"""CPU oracle of the training-tile warp (unet_tile_warp, csrc/elastic.hip
k_tile_warp): NumPy fp64, the same operations in the same order as the kernel.

TEST INFRASTRUCTURE ONLY.  The elastic field, the half-sample fold
(``reflect_*``), the bilinear expression and the integer conversion are
oracle/elastic_oracle.py's (pinned there to scipy and to the reference's own
outputs); this file adds the affine coordinate, the whole-sample ("mirror")
fold, the gain / bias step and the gathered weight plane.
"""
import numpy as np

from oracle import elastic_oracle as E


def mirror_coord(c, n):
    """Whole-sample-symmetric fold of a coordinate into [0, n - 1] (scipy
    mode="mirror", np.pad "reflect", tiling.mirror_index): C fmod, then the
    two folds.  A length-1 axis gives 0."""
    c = np.asarray(c, np.float64)
    if n == 1:
        return np.zeros_like(c)
    p = 2.0 * n - 2.0
    m = np.fmod(c, p)
    m = np.where(m < 0.0, m + p, m)
    return np.where(m > float(n - 1), p - m, m)


def fold(cy, cx, h, w, extend):
    """Folded coordinates and the six indices (ya, yb, xa, xb, ny, nx) the
    kernel reads, for extend 0 (reflect) / 1 (mirror)."""
    if extend == 0:
        cy, cx = E.reflect_coord(np.asarray(cy, np.float64), h), E.reflect_coord(np.asarray(cx, np.float64), w)
        y0, x0 = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
        ya, yb = E.reflect_index(y0, h), E.reflect_index(y0 + 1, h)
        xa, xb = E.reflect_index(x0, w), E.reflect_index(x0 + 1, w)
        ny = E.reflect_index(np.floor(cy + 0.5).astype(np.int64), h)
        nx = E.reflect_index(np.floor(cx + 0.5).astype(np.int64), w)
    elif extend == 1:
        cy, cx = mirror_coord(cy, h), mirror_coord(cx, w)
        ya, xa = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
        yb, xb = np.minimum(ya + 1, h - 1), np.minimum(xa + 1, w - 1)
        ny = np.minimum(np.floor(cy + 0.5).astype(np.int64), h - 1)
        nx = np.minimum(np.floor(cx + 0.5).astype(np.int64), w - 1)
    else:
        raise ValueError("extend must be 0 or 1")
    return cy, cx, (ya, yb, xa, xb, ny, nx)


def sample(img, cy, cx, order, extend):
    """fp64 value of the order-0 / order-1 sampling of `img` at (cy, cx) before
    the integer conversion (map_coordinates with mode="reflect" / "mirror")."""
    h, w = img.shape
    img = np.asarray(img, np.float64)
    cy, cx, (ya, yb, xa, xb, ny, nx) = fold(cy, cx, h, w, extend)
    if order == 0:
        return img[ny, nx]
    ty, tx = cy - np.floor(cy), cx - np.floor(cx)
    return ((1 - ty) * ((1 - tx) * img[ya, xa] + tx * img[ya, xb]) +
            ty * ((1 - tx) * img[yb, xa] + tx * img[yb, xb]))


def coords(row, th, tw, dy=0.0, dx=0.0):
    """cy = ((a00 ty + a01 tx) + b0) + dy, cx = ((a10 ty + a11 tx) + b1) + dx."""
    ty, tx = np.meshgrid(np.arange(th, dtype=np.float64), np.arange(tw, dtype=np.float64), indexing="ij")
    cy = ((row[0] * ty + row[1] * tx) + row[2]) + dy
    cx = ((row[3] * ty + row[4] * tx) + row[5]) + dx
    return cy, cx


def tile_warp(frames, labels, frame_idx, params, tile_hw, extend, noise=None, alpha=0.0, sigma=1.0, weights=None):
    """unet_tile_warp on the host.  Returns dict(x fp32, target uint8, image
    uint8, ids uint16[, w fp32]), each (n, th, tw)."""
    th, tw = tile_hw
    n = len(frame_idx)
    nf, h, w = frames.shape
    out = {"x": np.empty((n, th, tw), np.float32), "target": np.empty((n, th, tw), np.uint8),
           "image": np.empty((n, th, tw), np.uint8), "ids": np.empty((n, th, tw), np.uint16)}
    if weights is not None:
        out["w"] = np.empty((n, th, tw), np.float32)
    for s in range(n):
        f = min(max(int(frame_idx[s]), 0), nf - 1)
        row = np.asarray(params[s], np.float64)
        dx = dy = 0.0
        if noise is not None:
            dx = E.displacement(noise[s, 0], alpha, sigma)
            dy = E.displacement(noise[s, 1], alpha, sigma)
        cy, cx = coords(row, th, tw, dy, dx)
        _, _, (_, _, _, _, ny, nx) = fold(cy, cx, h, w, extend)
        iv = E.to_uint(sample(frames[f], cy, cx, 1, extend), np.uint8)
        g = np.minimum(np.maximum(row[6] * iv.astype(np.float64) + row[7], 0.0), 255.0)
        out["image"][s] = iv
        out["x"][s] = g.astype(np.float32) / np.float32(255.0)
        ids = labels[f][ny, nx].astype(np.uint16)
        tgt = (ids & 0xff) != 0
        out["target"][s] = tgt.astype(np.uint8)
        out["ids"][s] = np.where(tgt, ids, 0).astype(np.uint16)
        if weights is not None:
            out["w"][s] = weights[f][ny, nx]
    return out
