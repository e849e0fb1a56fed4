"""CPU checks of the warping error (no GPU): the library's simple-point table
against the oracle's (tests/warp_oracle.py), the oracle's vectorised schedule
against a plain one-pixel-at-a-time loop, and properties and known answers of
the oracle that do not depend on either implementation."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

import warp_oracle as W

G = os.path.join(os.path.dirname(__file__), "golden")


def test_library_table_equals_the_oracle_table():
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    buf = (ctypes.c_uint8 * 256)()
    _lib.load().unet_simple_point_table(buf)
    got = np.frombuffer(buf, np.uint8)
    assert int(got.sum()) == 116
    np.testing.assert_array_equal(got, W.simple_table())


def test_library_rejects_bad_arguments_before_any_launch():
    """-EINVAL and a workspace size of 0 (host code only: nothing is launched)."""
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1 << 16, 1 << 15, 1), (2, 1 << 15, 1 << 15)):
        assert lib.unet_warping_error_ws_bytes(n, h, w) == 0
        assert lib.unet_warping_error(None, None, n, h, w, 4, 1, 0, 0, None, None, None, None) == -22
    for radius, max_sweeps in ((-2, 0), (256, 0), (4, -1)):
        assert lib.unet_warping_error(None, None, 1, 4, 4, radius, 1, max_sweeps, 0, None, None, None, None) == -22
        with pytest.raises(RuntimeError, match="unet_warping_error"):
            _lib.check(lib.unet_warping_error(None, None, 1, 4, 4, radius, 1, max_sweeps, 0, None, None, None, None),
                       "unet_warping_error")
    assert lib.unet_warping_error_ws_bytes(1, 512, 512) >= 4 * 514 * 18 * 4


def test_oracle_table_basics():
    t = W.simple_table()
    assert int(t.sum()) == 116
    assert t[0] == 0 and t[255] == 0            # isolated pixel, interior pixel
    assert t[0b00010001] == 0                   # N and S only: a bridge
    assert t[0b00000001] == 1 and t[0b00000010] == 1


def random_case(g, h, w, density):
    """gt: random blobs with ids 1..3 (touching ids exercise the separation
    rule); pred: the ground truth with some pixels toggled, or unrelated."""
    gt = (ndimage.uniform_filter(g.random((h, w)), 3) < 0.5 * density + 0.25).astype(np.uint16)
    gt *= g.integers(1, 4, (h, w)).astype(np.uint16)
    if g.random() < 0.5:
        pred = (gt > 0) ^ (g.random((h, w)) < 0.15)
    else:
        pred = g.random((h, w)) < density
    return gt, pred.astype(np.uint8)


def sequential(g0, t, m, max_sweeps=0):
    """The plain restatement: one pixel at a time in raster order within each
    sub-field, simplicity recomputed from the labelling after every flip."""
    tab = W.simple_table()
    lab = np.pad(g0, 1)
    h, w = g0.shape
    flips = sweeps = 0
    while True:
        n = 0
        for s in range(4):
            for y in range(s >> 1, h, 2):
                for x in range(s & 1, w, 2):
                    if not m[y, x] or lab[y + 1, x + 1] == t[y, x]:
                        continue
                    idx = sum(int(lab[y + 1 + dy, x + 1 + dx]) << k for k, (dy, dx) in enumerate(W.NB))
                    if tab[idx]:
                        lab[y + 1, x + 1] ^= True
                        n += 1
        sweeps += 1
        flips += n
        if n == 0:
            return lab[1:-1, 1:-1], flips, sweeps, 1
        if max_sweeps > 0 and sweeps >= max_sweeps:
            return lab[1:-1, 1:-1], flips, sweeps, 0


SHAPES = ((24, 40), (17, 33), (9, 31), (1, 13))


@pytest.mark.parametrize("radius", [-1, 1, 3])
@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
def test_oracle_equals_one_pixel_at_a_time(radius, density):
    g = np.random.default_rng(int(density * 10) * 7 + radius + 1)
    for h, w in SHAPES:  # 9 x 4 = 36 frames
        gt, pred = random_case(g, h, w, density)
        g0 = W.ground_truth(gt, True)
        t = pred > 0
        m = W.mask(g0, radius)
        a = W.warp(g0, t, m)
        b = sequential(g0, t, m)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1:] == b[1:]
        a3, b3 = W.warp(g0, t, m, 2), sequential(g0, t, m, 2)
        np.testing.assert_array_equal(a3[0], b3[0])
        assert a3[1:] == b3[1:]


def topology(lab):
    """(8-connected foreground components, 4-connected background components
    of the frame padded with background)"""
    return ndimage.label(lab, W.S8)[1], ndimage.label(~np.pad(lab, 1), W.S4)[1]


def check_properties(gt, pred, radius, separate):
    r = W.evaluate(gt, pred, radius, separate)
    g0, t, m, lab = r["g0"], r["t"], r["m"], r["warped"].astype(bool)
    pix, warp, flips, sweeps, conv = (int(v) for v in r["counts"])
    assert conv == 1 and sweeps >= 1
    assert not ((lab != g0) & ~m).any()                      # flips only inside M
    assert topology(lab) == topology(g0)                     # the warping is homotopic
    ys, xs = np.nonzero(m & (lab != t))
    assert not W.simple_at(lab, ys, xs).any()                # nothing left to flip
    assert pix - warp == flips and pix == int((g0 != t).sum()) and warp == int((lab != t).sum())
    assert int((lab != g0).sum()) == flips                   # every flip removes a disagreement for good
    return r


@pytest.mark.parametrize("radius", [-1, 2, 4])
def test_oracle_properties_random(radius):
    g = np.random.default_rng(100 + radius)
    for density in (0.2, 0.5, 0.8):
        for separate in (True, False):
            gt, pred = random_case(g, 37, 45, density)
            check_properties(gt, pred, radius, separate)


def test_oracle_properties_hela():
    z = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)
    gts = z["segs"][:, 94:418, 94:418]
    for i in range(gts.shape[0]):
        # the separation rule gives every cell its own component
        assert ndimage.label(W.ground_truth(gts[i], True), W.S8)[1] == len(np.unique(gts[i])) - 1
        r = check_properties(gts[i], z["masks"][i], 4, True)
        assert 0 < r["counts"][1] < r["counts"][0]
    check_properties(gts[0], z["masks"][0], 4, False)


def disc(n=48, r=14):
    yy, xx = np.indices((n, n))
    return ((yy - n // 2) ** 2 + (xx - n // 2) ** 2 <= r * r)


def test_known_answers():
    d = disc()
    gt = d.astype(np.uint16)
    same = W.evaluate(gt, d.astype(np.uint8), 4)["counts"]
    assert same.tolist() == [0, 0, 0, 1, 1]
    for pred in (ndimage.binary_erosion(d, W.S8, iterations=2), ndimage.binary_dilation(d, W.S8, iterations=3)):
        c = W.evaluate(gt, pred.astype(np.uint8), 4)["counts"]
        assert c[0] > 0 and c[1] == 0 and c[2] == c[0]
    hole = d.copy()
    hole[22:26, 22:26] = False
    for radius in (4, -1):
        c = W.evaluate(gt, hole.astype(np.uint8), radius)["counts"]
        assert c[0] == 16 and c[1] == 16 and c[2] == 0
    c = W.evaluate(gt, np.zeros_like(gt, dtype=np.uint8), -1)["counts"]
    assert c[0] == int(d.sum()) and c[1] == 1            # the last pixel cannot go
    shifted = np.roll(d, 3, axis=1)
    c = W.evaluate(gt, shifted.astype(np.uint8), 0)["counts"]
    assert c[0] > 0 and c[1] == c[0] and c[2] == 0 and c[3] == 1
