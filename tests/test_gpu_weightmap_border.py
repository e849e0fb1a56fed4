"""Border-aware weight maps on the GPU (unet_weight_map_border /
weight_maps(mode="border")): the squared distances to the two nearest objects
exact (integers, against scipy's per-object EDT in tests/golden/
border_weightmap.npz or a numpy brute force), the fp64 map against numpy at
rtol 1e-11, the fp32 map its cast bit for bit.

The rtol is derived, not measured: both sides take a correctly-rounded-or-1-ulp
sqrt and exp of the same integers; the exponent is at most ~745 in magnitude
before the term underflows, so the term's relative error stays below about
745 x 4 ulp ~ 7e-13, and the weight is never below 1 (wc = total / count >= 1).
"""
import os
import sys

import numpy as np
import pytest

from oracle import fixtures as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, G)
import make_golden_border as MB  # noqa: E402  (numpy-only helpers; scipy is imported by its generator alone)

RTOL = 1e-11
CHUNK = 512  # candidate columns per LDS stage in k_wb_rows


@pytest.fixture(scope="module")
def wm():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd.augment import weight_maps
    return weight_maps


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "border_weightmap.npz"), allow_pickle=False)


def brute(lab):
    """(d1sq, d2sq) by definition: per object the minimum over its pixels of
    the squared distance (h w <= ~2500)."""
    h, w = lab.shape
    assert h * w <= 2600
    yy, xx = np.mgrid[0:h, 0:w]
    per = []
    for l in np.unique(lab[lab > 0]):
        oy, ox = np.nonzero(lab == l)
        d = (yy[..., None] - oy) ** 2 + (xx[..., None] - ox) ** 2
        per.append(d.min(-1))
    zero = np.zeros((h, w), np.int32)
    if not per:
        return zero, zero
    if len(per) == 1:
        return per[0].astype(np.int32), zero
    s = np.sort(np.stack(per, -1), -1)
    return s[..., 0].astype(np.int32), s[..., 1].astype(np.int32)


def run(wm, labs, w0=10.0, sigma=5.0):
    w32, w64, d1, d2 = wm(torch.from_numpy(np.ascontiguousarray(labs)).cuda(), w0, sigma, fp64=True, mode="border",
                          return_distances=True)
    torch.cuda.synchronize()
    return w32.cpu().numpy(), w64.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()


def check(lab, got, i, d1sq, d2sq, w64_ref=None, w0=10.0, sigma=5.0):
    w32, w64, d1, d2 = (a[i] for a in got)
    np.testing.assert_array_equal(d1, d1sq)
    np.testing.assert_array_equal(d2, d2sq)
    if w64_ref is None:
        w64_ref = MB.weight64_from(lab, d1sq, d2sq, w0, sigma)
    err = np.abs(w64 - w64_ref) / np.abs(w64_ref)
    print(f"weight64 max rel err {err.max():.3e} (bound {RTOL:g}), min weight {w64_ref.min():.4f}")
    np.testing.assert_allclose(w64, w64_ref, rtol=RTOL, atol=0)
    np.testing.assert_array_equal(w32.view(np.uint32), w64.astype(np.float32).view(np.uint32))


def check_brute(wm, lab, **kw):
    lab = np.asarray(lab, np.uint16)
    got = run(wm, lab[None], **kw)
    check(lab, got, 0, *brute(lab), **kw)
    return got


def test_hela_batch(wm, gold):
    segs = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)["segs"]
    got = run(wm, segs)
    for i in range(3):
        d1sq, d2sq = MB.squares(gold, f"hela{i}")
        check(segs[i], got, i, d1sq, d2sq)
        # the rows of the fp64 map the fixture stores (made next to scipy)
        np.testing.assert_allclose(got[1][i][::MB.HELA_ROW_STEP], gold[f"hela{i}/weight64_rows"], rtol=RTOL, atol=0)


@pytest.mark.parametrize("case", ["multi", "one", "empty", "full"])
def test_synthetic(wm, gold, case):
    lab = F.weightmap_synthetic_cases()[case]
    d1sq, d2sq = MB.squares(gold, case)
    check(lab, run(wm, lab[None]), 0, d1sq, d2sq, gold[f"{case}/weight64"])


def test_ragged_batch_high_byte_ids(wm):
    """Ids that differ only in the high byte or wrap in uint8; an empty sample,
    a single-id one and one without background between ordinary ones: each
    sample equals its own single-sample result (nothing leaks between them)."""
    g = np.random.default_rng(5)
    ids = np.array([0, 1, 256, 257, 513, 65535], np.uint16)
    lab = ids[g.integers(0, 6, (5, 37, 301))]
    lab[g.random(lab.shape) < 0.9] = 0       # sparse: distances of several pixels
    lab[1] = 0
    lab[2] = np.where(lab[2] != 0, 256, 0)
    lab[3] = ids[g.integers(1, 6, (37, 301))]
    got = run(wm, lab)
    for i in range(5):
        one = run(wm, lab[i][None])
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a[i], b[0])
    assert not got[2][1].any() and not got[3][1].any()          # no object: d1 = d2 = 0
    assert not got[3][2].any() and got[2][2].any()              # one object: d2 = 0, d1 its distance
    assert not got[2][3].any() and got[3][3].all()              # no background: d1 = 0, d2 > 0
    # exactness on a window small enough for the brute force (all six ids present)
    sub = lab[0][:, :64]
    check_brute(wm, sub)
    check_brute(wm, lab[3][:, 100:164])


@pytest.mark.parametrize("shape", [(1, 40), (30, 1)])
def test_degenerate_shapes(wm, shape):
    g = np.random.default_rng(shape[0])
    lab = np.array([0, 0, 0, 2, 300, 65535], np.uint16)[g.integers(0, 6, shape)]
    check_brute(wm, lab)


def test_row_longer_than_one_lds_chunk(wm):
    w = 2 * CHUNK + 76
    lab = np.zeros((3, w), np.uint16)   # 3 x 1100 > 2500 pixels: per-pixel brute force over the few object pixels
    pix = {(0, 3): 7, (2, CHUNK - 1): 263, (1, CHUNK): 7, (0, w - 1): 9, (2, 2 * CHUNK + 5): 263}
    for (y, x), l in pix.items():
        lab[y, x] = l
    yy, xx = np.mgrid[0:3, 0:w]
    per = []
    for l in (7, 9, 263):
        per.append(np.min([(yy - y) ** 2 + (xx - x) ** 2 for (y, x), v in pix.items() if v == l], 0))
    s = np.sort(np.stack(per, -1), -1)
    check(lab, run(wm, lab[None]), 0, s[..., 0].astype(np.int32), s[..., 1].astype(np.int32))


def test_two_objects_in_one_column_or_row(wm):
    col = np.zeros((40, 31), np.uint16)
    col[3:6, 17], col[30, 17] = 4, 260
    check_brute(wm, col)
    row = np.zeros((31, 60), np.uint16)
    row[12, 2:5], row[12, 50] = 4, 260
    check_brute(wm, row)


def test_touching_objects(wm):
    lab = np.zeros((20, 24), np.uint16)
    lab[5:15, 4:12], lab[5:15, 12:20] = 1, 257
    got = check_brute(wm, lab)
    assert got[3][0][10, 11] == 1 and got[3][0][10, 12] == 1     # d2 = 1 inside each, at the shared edge
    assert got[2][0][lab > 0].max() == 0


def test_three_equidistant_single_pixel_objects(wm):
    lab = np.zeros((21, 21), np.uint16)
    lab[10, 5], lab[10, 15], lab[5, 10] = 1, 2, 3   # all at distance 5 from (10, 10)
    got = check_brute(wm, lab)
    assert got[2][0][10, 10] == 25 and got[3][0][10, 10] == 25


def test_many_single_pixel_objects(wm):
    g = np.random.default_rng(11)
    lab = np.zeros(40 * 60, np.uint16)
    lab[g.choice(40 * 60, 300, replace=False)] = g.choice(np.arange(1, 65536), 300, replace=False)
    check_brute(wm, lab.reshape(40, 60))


def test_sigma_zero(wm):
    lab = np.zeros((16, 19), np.uint16)
    lab[2:5, 3:6], lab[9:12, 10:15] = 8, 9
    got = check_brute(wm, lab, sigma=0.0)
    assert np.isfinite(got[1]).all()


def test_two_calls_bit_identical(wm):
    segs = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)["segs"]
    a, b = run(wm, segs[:2]), run(wm, segs[:2])
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint8), v.view(np.uint8))


def test_default_mode_unchanged_and_bad_mode(wm):
    lab = torch.from_numpy(F.weightmap_synthetic_cases()["multi"][None]).cuda()
    np.testing.assert_array_equal(wm(lab).cpu().numpy(), wm(lab, mode="reference").cpu().numpy())
    with pytest.raises(ValueError):
        wm(lab, mode="paper")
