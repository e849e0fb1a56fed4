"""Per-object records, derived columns, track dynamics and the displacement
error without a GPU: unet_amd.measure over the library's host twin
(unet_region_props_host), against tests/region_oracle.py, scipy.ndimage,
closed forms and numbers written out by hand.
"""
import ctypes
import errno
import os

import numpy as np
import pytest

import region_oracle as O
import track_map_oracle as M

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def measure():
    from unet_amd import measure as m
    return m


@pytest.fixture(scope="module")
def hela_real():
    d = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)
    return d["segs"], d["images"]


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


def edge_sequence():
    """The six 40 x 50 frames of tests/test_track.py::test_gpu_tracker_edge_cases."""
    h, w = 40, 50
    seq = np.zeros((6, h, w), np.int32)
    seq[0, 5:25, 5:25] = 7                  # one cell
    seq[1, 5:25, 5:25] = 9                  # moved label, same place -> linked
    seq[2, 5:25, 5:10] = 3                  # divides: two children, IoU 0.25 each
    seq[2, 5:25, 20:25] = 65535
    seq[3] = 0                              # empty frame
    seq[4, 30:35, 40:48] = 2                # new object
    seq[5, 30:35, 40:48] = 2
    seq[5, 0:3, 0:3] = 1
    return seq


def edge_tracked():
    """(rows, track-labelled masks, frame numbers) of the edge sequence, tracked by the NumPy oracle."""
    seq = edge_sequence()
    rows, maps, _ = M.track_maps(seq)
    return np.asarray(rows), M.relabel(seq, maps).astype(np.uint16), np.arange(6)


def small_cases():
    rng = np.random.default_rng(5)
    yield rng.integers(0, 7, (3, 5, 7)).astype(np.uint16), rng.integers(0, 256, (3, 5, 7)).astype(np.uint8)
    yield np.ones((1, 1, 1), np.uint16), None
    yield rng.integers(0, 3, (1, 1, 9)).astype(np.uint16), None
    yield rng.integers(0, 3, (2, 9, 1)).astype(np.uint16), rng.integers(0, 256, (2, 9, 1)).astype(np.uint8)
    yield rng.choice(np.array([0, 1, 300, 65535], np.uint16), size=(2, 13, 17)), None
    yield np.zeros((2, 4, 4), np.uint16), None


def test_the_two_oracles_agree_and_the_host_twin_equals_them(measure):
    for labels, image in small_cases():
        a, b = O.direct(labels, image), O.vectorised(labels, image)
        np.testing.assert_array_equal(a[0], b[0])
        for k in O.FIELDS:
            np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=k)
        O.assert_equal(measure.region_props_host(labels, image), a)


def test_oracles_and_host_twin_on_real_frames(measure, hela_real):
    segs, images = hela_real
    crop = (slice(0, 2), slice(100, 260), slice(40, 231))      # the direct oracle is an argwhere per label
    a, b = O.direct(segs[crop], images[crop]), O.vectorised(segs[crop], images[crop])
    for k in O.FIELDS:
        np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=k)
    O.assert_equal(measure.region_props_host(segs[crop], images[crop]), a)
    O.assert_equal(measure.region_props_host(segs, images), O.vectorised(segs, images))
    t = measure.region_props_host(segs)                          # no image: the intensity fields are 0
    for k in ("sum_v", "sum_vv", "min_v", "max_v"):
        assert not getattr(t, k).any()


def test_against_scipy_ndimage(measure, hela_real):
    from scipy import ndimage
    segs, images = hela_real
    t = measure.region_props_host(segs, images)
    assert len(t) > 0
    for f in range(segs.shape[0]):
        sl = slice(int(t.frame_offsets[f]), int(t.frame_offsets[f + 1]))
        idx = t.label[sl]
        np.testing.assert_array_equal(idx, np.unique(segs[f])[1:])
        lab, img = segs[f].astype(np.int32), images[f].astype(np.float64)
        np.testing.assert_array_equal(t.area[sl], ndimage.sum(np.ones_like(img), lab, idx))
        np.testing.assert_array_equal(t.sum_v[sl], ndimage.sum(img, lab, idx))
        np.testing.assert_array_equal(t.sum_vv[sl], ndimage.sum(img * img, lab, idx))
        np.testing.assert_array_equal(t.min_v[sl], ndimage.minimum(img, lab, idx))
        np.testing.assert_array_equal(t.max_v[sl], ndimage.maximum(img, lab, idx))
        com = np.array(ndimage.center_of_mass(np.ones_like(img), lab, idx))
        # two float64 means of at most 2^18 integers below 2^9: a few ulp of 512
        np.testing.assert_allclose(t.centroid_y[sl], com[:, 0], rtol=0, atol=1e-10)
        np.testing.assert_allclose(t.centroid_x[sl], com[:, 1], rtol=0, atol=1e-10)
        boxes = ndimage.find_objects(lab)
        for k, l in enumerate(idx):
            ys, xs = boxes[l - 1]
            assert (t.min_y[sl][k], t.max_y[sl][k], t.min_x[sl][k], t.max_x[sl][k]) == \
                (ys.start, ys.stop - 1, xs.start, xs.stop - 1)
        np.testing.assert_allclose(t.mean_v[sl], ndimage.mean(img, lab, idx), rtol=1e-13)
        np.testing.assert_allclose(t.std_v[sl], ndimage.standard_deviation(img, lab, idx), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("a,b", [(1, 1), (1, 6), (4, 4), (7, 3), (20, 5)])
def test_rectangle_closed_forms(measure, a, b):
    labels = np.zeros((1, 30, 31), np.uint16)
    labels[0, 3:3 + a, 4:4 + b] = 5
    t = measure.region_props_host(labels)
    assert len(t) == 1 and t.area[0] == a * b and t.contact[0] == 0 and t.edge[0] == 0
    # sums of small integers: the variances are exact rationals rounded once
    assert t.mu_yy[0] == pytest.approx((a * a - 1) / 12, rel=1e-15, abs=0)
    assert t.mu_xx[0] == pytest.approx((b * b - 1) / 12, rel=1e-15, abs=0)
    assert t.mu_xy[0] == 0
    assert t.boundary[0] == (a * b if min(a, b) <= 2 else 2 * a + 2 * b - 4)
    assert (t.centroid_y[0], t.centroid_x[0]) == (3 + (a - 1) / 2, 4 + (b - 1) / 2)
    assert t.major_axis[0] == pytest.approx(4 * np.sqrt((max(a, b) ** 2 - 1) / 12), rel=1e-14)
    assert t.minor_axis[0] == pytest.approx(4 * np.sqrt((min(a, b) ** 2 - 1) / 12), rel=1e-14)
    if a == b == 1:
        assert t.eccentricity[0] == 0 and t.major_axis[0] == 0
    if a > b:
        assert abs(abs(t.orientation[0]) - np.pi / 2) < 1e-15     # the major axis runs along y
    if b > a:
        assert t.orientation[0] == 0


@pytest.mark.parametrize("s", [1, 4, 9])
def test_two_rectangles_sharing_a_side(measure, s):
    labels = np.zeros((1, 20, 20), np.uint16)
    labels[0, 0:s, 2:6] = 1            # touches the first row: edge pixels
    labels[0, 0:s, 6:11] = 2
    t = measure.region_props_host(labels)
    assert t.contact.tolist() == [s, s]
    assert t.edge.tolist() == [4, 5]   # their pixels in row 0
    assert t.touches_edge.all()
    assert t.area.tolist() == [4 * s, 5 * s]
    # interior: rows 1..s-2 (row 0 has the frame's edge above, row s-1 background below), without the end columns
    inner = max(s - 2, 0)
    assert t.boundary.tolist() == [4 * s - 2 * inner, 5 * s - 3 * inner]


def test_dynamics_of_the_edge_sequence(measure):
    rows, masks, frames = edge_tracked()
    # one cell (1), its two children (2, 3), after an empty frame a new object (4), then another (5)
    assert sorted(map(tuple, np.where(rows[:, 3:] < 0, 0, rows[:, 3:]).tolist())) == [(0,), (0,), (0,), (1,), (1,)]
    traj = measure.trajectories(masks, frames, rows)
    T = traj.table
    assert traj.tracks.tolist() == [1, 2, 3, 4, 5]
    assert traj.track_offsets.tolist() == [0, 2, 3, 4, 6, 7]
    assert T.label.tolist() == [1, 1, 2, 3, 4, 4, 5] and traj.frame.tolist() == [0, 1, 2, 2, 4, 5, 5]
    assert T.area.tolist() == [400, 400, 100, 100, 40, 40, 9]
    assert T.centroid_y.tolist() == [14.5, 14.5, 14.5, 14.5, 32.0, 32.0, 1.0]
    assert T.centroid_x[:2].tolist() == [14.5, 14.5] and sorted(T.centroid_x[2:4].tolist()) == [7.0, 22.0]
    assert T.centroid_x[4:].tolist() == [43.5, 43.5, 1.0]
    assert T.touches_edge.tolist() == [False] * 6 + [True]
    d = measure.dynamics(traj, rows)
    tr, dv, fr = d["tracks"], d["divisions"], d["frames"]
    by = {int(t): k for k, t in enumerate(tr["track"])}
    order = [by[t] for t in (1, 2, 3, 4, 5)]
    col = lambda name: [tr[name][k] for k in order]
    assert col("start") == [0, 2, 2, 4, 5] and col("end") == [1, 2, 2, 5, 5]
    assert col("parent") == [0, 1, 1, 0, 0]
    assert col("frames_present") == [2, 1, 1, 2, 1]
    assert col("path_length") == [0.0] * 5 and col("net_displacement") == [0.0] * 5
    assert col("mean_speed") == [0.0] * 5 and col("straightness") == [0.0] * 5
    assert col("mean_area") == [400.0, 100.0, 100.0, 40.0, 9.0]
    assert col("first_area") == col("last_area") == col("mean_area")
    assert col("children") == [2, 0, 0, 0, 0]
    assert col("cycle_length") == [-1] * 5                   # roots and leaves have no cycle
    assert {k: v.tolist() for k, v in dv.items()} == dict(parent=[1], frame=[2], children=[2], child_a=[2], child_b=[3],
                                                         area_ratio=[1.0], centroid_distance=[15.0])
    assert fr["frame"].tolist() == [0, 1, 2, 3, 4, 5]
    assert fr["cells"].tolist() == [1, 1, 2, 0, 1, 2]
    assert fr["area_fraction"].tolist() == [0.2, 0.2, 0.1, 0.0, 0.02, 49 / 2000]
    assert fr["contact"].tolist() == [0] * 6 and fr["mean_step"].tolist() == [0.0] * 6
    assert fr["divisions"].tolist() == [0, 0, 1, 0, 0, 0]


def test_dynamics_of_a_moving_dividing_lineage(measure):
    """A hand-made lineage with motion: a 2 x 2 cell steps (0, 3) then (4, 0),
    divides; one daughter divides again, so it has a parent and children."""
    masks = np.zeros((5, 32, 32), np.uint16)
    masks[0, 10:12, 10:12] = 1
    masks[1, 10:12, 13:15] = 1
    masks[2, 14:16, 13:15] = 1
    masks[3, 14:16, 10:12] = 2
    masks[3, 14:16, 16:20] = 3      # twice the area of 2, touching nothing
    masks[4, 14:16, 10:11] = 4
    masks[4, 14:16, 11:12] = 5      # 4 and 5 touch along a side of 2
    masks[4, 14:16, 16:20] = 3
    rows = np.array([[1, 10, 12, 0], [2, 13, 13, 1], [3, 13, 14, 1], [4, 14, 14, 2], [5, 14, 14, 2]])
    frames = [10, 11, 12, 13, 14]
    traj = measure.trajectories(masks, frames, rows)
    d = measure.dynamics(traj, rows, frame_interval=2.0, pixel_size=0.5)
    tr, dv, fr = d["tracks"], d["divisions"], d["frames"]
    assert tr["path_length"].tolist() == [3.5, 0.0, 0.0, 0.0, 0.0]         # (3 + 4) pixels of 0.5
    assert tr["net_displacement"].tolist() == [2.5, 0.0, 0.0, 0.0, 0.0]    # hypot(4, 3) pixels of 0.5
    assert tr["mean_speed"].tolist() == [3.5 / 4.0, 0.0, 0.0, 0.0, 0.0]    # over 2 frames of 2.0
    assert tr["straightness"].tolist() == [2.5 / 3.5, 0.0, 0.0, 0.0, 0.0]
    assert tr["mean_area"].tolist() == [1.0, 1.0, 2.0, 0.5, 0.5]
    assert tr["children"].tolist() == [2, 2, 0, 0, 0]
    assert tr["cycle_length"].tolist() == [-1, 1, -1, -1, -1]              # track 2: parent and children, 1 frame
    assert dv["parent"].tolist() == [1, 2] and dv["frame"].tolist() == [13, 14]
    assert dv["area_ratio"].tolist() == [0.5, 1.0]
    assert dv["centroid_distance"].tolist() == [0.5 * 7.0, 0.5 * 1.0]
    assert fr["cells"].tolist() == [1, 1, 1, 2, 3] and fr["contact"].tolist() == [0, 0, 0, 0, 4]
    assert fr["mean_step"].tolist() == [0.0, 1.5, 2.0, 0.0, 0.0]
    assert fr["divisions"].tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(ValueError, match="no track row"):
        measure.trajectories(masks, frames, rows[:4])


def test_displacement_error_on_tra03(measure, tra03):
    want, matched, total, per = O.ade(tra03["gt"], tra03["res"])
    got = measure.displacement_error(tra03["gt"], tra03["gt_track"], tra03["res"], tra03["res_track"], tra03["frames"])
    print(f"ADE {got['ade']!r} (oracle {want!r}), matched {got['matched']} of {got['total']}")
    assert (matched, total) == (20, 25)
    assert (got["matched"], got["total"]) == (20, 25)
    assert abs(got["ade"] - want) <= 1e-12 * want
    p = got["per_track"]
    assert p["track"].tolist() == tra03["gt_track"][:, 0].tolist()
    for t, m, n, e in zip(p["track"].tolist(), p["matched"].tolist(), p["total"].tolist(), p["ade"].tolist()):
        assert m == len(per[t]) and n == int((np.any(tra03["gt"] == t, axis=(1, 2))).sum())
        if m:
            assert abs(e - np.mean(per[t])) <= 1e-12 * np.mean(per[t])
        else:
            assert np.isnan(e)


def test_argument_errors():
    from unet_amd import _lib as L
    from unet_amd.measure import RECORD
    lib = L.load()
    fake = ctypes.c_void_p(0x10000)      # aligned, never dereferenced
    total = ctypes.c_longlong(-7)

    def device(n, h, w, cap=1):
        return lib.unet_region_props(fake, None, n, h, w, fake, fake, cap, ctypes.byref(total), fake, None)

    def host(n, h, w, cap=1):
        return lib.unet_region_props_host(fake, None, n, h, w, fake, fake, cap, ctypes.byref(total))

    for call in (device, host):          # rejected before any access (and any device call)
        for n, h, w in ((1, 32769, 1), (1, 1, 32769), (1, 32768, 32767 + 2), (-1, 4, 4), (1, 0, 4), (1, 4, 0)):
            total.value = -7
            assert call(n, h, w) == -errno.EINVAL, (call.__name__, n, h, w)
            assert total.value == 0
            assert "32768" in L.last_error()
        assert call(1, 4, 4, cap=-1) == -errno.EINVAL
    assert lib.unet_region_props(fake, None, 1, 4, 4, fake, fake, 1, ctypes.byref(total), ctypes.c_void_p(0x10010),
                                 None) == -errno.EINVAL     # ws not 256-byte aligned
    assert lib.unet_region_props(fake, None, 1, 4, 4, fake, fake, 1, None, fake, None) == -errno.EINVAL
    assert lib.unet_region_props_ws_bytes(1, 32769, 1) == 0
    assert lib.unet_region_props_ws_bytes(-1, 4, 4) == 0
    assert lib.unet_region_props_ws_bytes(1, 32768, 32768) == 2 * 8192 + 256      # h w = 2^30 is inside
    assert lib.unet_region_props_ws_bytes(3, 5, 7) == 2 * 3 * 8192 + 256
    # -ENOSPC: host_total and frame_offsets are set, the records untouched
    labels = np.zeros((2, 4, 5), np.uint16)
    labels[0, 0, 0], labels[0, 3, 4], labels[1, 2, 2] = 9, 4, 9
    off = np.full(3, -1, np.int32)
    rec = np.full(2, 0x5A, np.uint8).repeat(64 * 2).view(RECORD)
    keep = rec.copy()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.unet_region_props_host(vp(labels), None, 2, 4, 5, vp(off), vp(rec), 2, ctypes.byref(total)) \
        == -errno.ENOSPC
    assert total.value == 3 and off.tolist() == [0, 2, 3]
    assert rec.tobytes() == keep.tobytes()
    rec = np.zeros(3, RECORD)
    assert lib.unet_region_props_host(vp(labels), None, 2, 4, 5, vp(off), vp(rec), 3, ctypes.byref(total)) == 0
    assert rec["label"].tolist() == [4, 9, 9] and rec["frame"].tolist() == [0, 0, 1]
    assert lib.unet_region_props_launches(0) >= 0


def test_python_argument_errors(measure):
    import torch
    with pytest.raises(ValueError, match=r"runs on the HIP device only \(no CPU fallback\)"):
        measure.region_props(torch.zeros((1, 4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"runs on the HIP device only \(no CPU fallback\)"):
        measure.region_props(np.zeros((1, 4, 4), np.uint16))
    with pytest.raises(ValueError, match="65535"):
        measure.region_props_host(np.full((1, 2, 2), 65536, np.int32))
    with pytest.raises(ValueError, match="65535"):
        measure.region_props_host(np.full((1, 2, 2), -1, np.int32))
    t = measure.region_props_host(np.arange(600, dtype=np.int32).reshape(1, 20, 30), cap=1)   # one retry
    assert len(t) == 599 and t.label.tolist() == list(range(1, 600))
