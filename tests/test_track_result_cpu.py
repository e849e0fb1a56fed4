"""Frame maps, label scopes and the host side of track-labelled result masks
(unet_tracker_frame_map / _set_label_scope / _relabel's error paths,
unet_amd.track.ctc_rows / write_result), no GPU: the library's host tracker is
fed the oracle's overlap tables through unet_tracker_step_host, as
tests/test_track.py does, and compared with tests/track_map_oracle.py.
"""
import ctypes
import errno
import os

import numpy as np
import pytest

import track_map_oracle as M
from test_ctc_cpu import rules, stack_tables

G = os.path.join(os.path.dirname(__file__), "golden")
SCOPES = {"shared": 0, "frame": 1}


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _lib():
    from unet_amd import _lib as L
    return L.load()


class HostTracker:
    """unet_tracker_* through ctypes, host entry points only."""

    def __init__(self, h, w, scope="shared"):
        self.lib = _lib()
        self.t = self.lib.unet_tracker_create(h, w, 0.3, 0.1, 2)
        assert self.t
        assert self.lib.unet_tracker_set_label_scope(self.t, SCOPES[scope]) == 0

    def close(self):
        self.lib.unet_tracker_destroy(self.t)
        self.t = None

    def step(self, frame, labels, areas, inter):
        lab = np.ascontiguousarray(labels, np.int32)
        area = np.ascontiguousarray(areas, np.int64)
        it = None if inter is None else np.ascontiguousarray(inter, np.int64)
        return self.lib.unet_tracker_step_host(self.t, int(frame), len(lab), _vp(lab), _vp(area), _vp(it))

    def rows(self):
        n = self.lib.unet_tracker_num_tracks(self.t)
        out = np.zeros((n, 4), np.int32)
        assert self.lib.unet_tracker_tracks(self.t, _vp(out), n) == n
        return out

    def maps(self):
        """[(frame, {label: track id})] in the order the frames were given."""
        out = []
        for i in range(self.lib.unet_tracker_num_frames(self.t)):
            n = self.lib.unet_tracker_frame_map(self.t, i, None, None, None, 0)
            assert n >= 0
            frame = ctypes.c_int32(-1)
            lab, ids = np.zeros(n, np.int32), np.zeros(n, np.int32)
            assert self.lib.unet_tracker_frame_map(self.t, i, ctypes.byref(frame), _vp(lab), _vp(ids), n) == n
            assert np.all(np.diff(lab) > 0)
            out.append((int(frame.value), dict(zip(lab.tolist(), ids.tolist()))))
        return out


def host_track(masks, frames, scope):
    """(oracle rows, oracle maps, library rows, library maps) of a stack."""
    rows, maps, steps = M.track_maps(masks, frames, scope)
    tr = HostTracker(masks.shape[1], masks.shape[2], scope)
    try:
        for s in steps:
            assert tr.step(*s) == 0
        return rows, maps, tr.rows(), tr.maps()
    finally:
        tr.close()


@pytest.fixture(scope="module")
def hela():
    return np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def hela_tracked(hela):
    return {s: host_track(hela["labels"], hela["frames"], s) for s in SCOPES}


def consistent(frames, maps, rows):
    """Every non-zero id of a map has a row whose [start, end] holds the frame."""
    span = {int(r[0]): (int(r[1]), int(r[2])) for r in rows}
    assert len(span) == len(rows)
    for f, mp in zip(frames, maps):
        for lab, tid in mp.items():
            if tid:
                assert tid in span, (f, lab, tid)
                assert span[tid][0] <= f <= span[tid][1], (f, lab, tid, span[tid])


def test_hela_shared_scope_maps_equal_the_oracles(hela, hela_tracked):
    rows, maps, lrows, lmaps = hela_tracked["shared"]
    np.testing.assert_array_equal(rows, hela["res_track"])
    np.testing.assert_array_equal(lrows, hela["res_track"])
    assert len(lmaps) == 84
    assert [f for f, _ in lmaps] == [int(f) for f in hela["frames"]]
    assert [m for _, m in lmaps] == maps
    # the reference's single dictionary drops the track of 5 objects of 11,412
    assert sum(len(m) for m in maps) == 11412
    assert len(M.trackless(maps)) == 5


def test_hela_frame_scope_maps_equal_the_scoped_oracles(hela, hela_tracked):
    rows, maps, lrows, lmaps = hela_tracked["frame"]
    assert len(rows) == 10806
    np.testing.assert_array_equal(lrows, rows)
    assert [m for _, m in lmaps] == maps
    assert M.trackless(maps) == []
    for mp in maps:  # a track id is held by at most one label of a frame
        assert len(set(mp.values())) == len(mp)


@pytest.mark.parametrize("scope", list(SCOPES))
def test_map_ids_have_rows_that_span_the_frame(hela, hela_tracked, scope):
    _, _, lrows, lmaps = hela_tracked[scope]
    consistent([f for f, _ in lmaps], [m for _, m in lmaps], lrows)


def test_set_label_scope_after_a_frame_is_busy():
    lib = _lib()
    tr = HostTracker(4, 4)
    try:
        assert lib.unet_tracker_set_label_scope(tr.t, 2) == -errno.EINVAL
        assert lib.unet_tracker_set_label_scope(tr.t, 1) == 0
        assert tr.step(0, [3], [2], None) == 0
        assert lib.unet_tracker_set_label_scope(tr.t, 0) == -errno.EBUSY
        assert lib.unet_tracker_set_label_scope(tr.t, 1) == -errno.EBUSY
    finally:
        tr.close()


def test_frame_map_bad_index():
    lib = _lib()
    tr = HostTracker(4, 4)
    try:
        assert lib.unet_tracker_num_frames(tr.t) == 0
        assert lib.unet_tracker_frame_map(tr.t, 0, None, None, None, 0) == -errno.EINVAL
        assert tr.step(7, [3, 9], [2, 2], None) == 0
        assert lib.unet_tracker_num_frames(tr.t) == 1
        assert lib.unet_tracker_frame_map(tr.t, 1, None, None, None, 0) == -errno.EINVAL
        assert lib.unet_tracker_frame_map(tr.t, -1, None, None, None, 0) == -errno.EINVAL
        # cap below the object count: the count is returned, cap pairs are written
        lab, ids = np.full(2, -5, np.int32), np.full(2, -5, np.int32)
        assert lib.unet_tracker_frame_map(tr.t, 0, None, _vp(lab), _vp(ids), 1) == 2
        assert lab.tolist() == [3, -5] and ids.tolist() == [1, -5]
        assert tr.maps() == [(7, {3: 1, 9: 2})]
    finally:
        tr.close()


def test_relabel_errors_come_before_any_device_work():
    """-ERANGE for a track id beyond 16 bits, -ENOENT for an unknown frame,
    -EINVAL for bad arguments; the device pointers are made up and never
    touched, so this passes without a GPU."""
    from unet_amd import _lib as L
    lib = L.load()
    tr = HostTracker(256, 256)
    fake = ctypes.c_void_p(0x10000)   # aligned, never dereferenced
    try:
        n = 65535
        assert tr.step(0, np.arange(1, n + 1), np.ones(n), None) == 0
        assert tr.step(1, [1], [1], np.zeros((n, 1))) == 0
        assert lib.unet_tracker_num_tracks(tr.t) == 65536
        assert tr.maps()[1] == (1, {1: 65536})

        def relabel(frames, labels=fake, out=fake, ws=fake, count=None):
            fr = np.asarray(frames, np.int32)
            return lib.unet_tracker_relabel(tr.t, labels, _vp(fr), len(fr) if count is None else count, out, ws, None)

        assert relabel([1]) == -errno.ERANGE
        assert "65536" in L.last_error()
        assert relabel([0, 1]) == -errno.ERANGE
        assert relabel([2]) == -errno.ENOENT
        assert "frame 2" in L.last_error()
        assert relabel([0, 5]) == -errno.ENOENT
        assert relabel([0], labels=None) == -errno.EINVAL
        assert relabel([0], out=None) == -errno.EINVAL
        assert relabel([0], ws=None) == -errno.EINVAL
        assert relabel([0], ws=ctypes.c_void_p(0x10010)) == -errno.EINVAL
        assert relabel([0], labels=ctypes.c_void_p(0x10001)) == -errno.EINVAL
        assert relabel([0], count=-1) == -errno.EINVAL
        assert relabel([], count=0) == 0
        assert lib.unet_tracker_relabel(None, fake, None, 1, fake, fake, None) == -errno.EINVAL
    finally:
        tr.close()
    assert lib.unet_tracker_relabel_ws_bytes(3, 5, 7) == 3 * 65536 * 2
    assert lib.unet_tracker_relabel_ws_bytes(0, 5, 7) == 0
    assert lib.unet_tracker_relabel_ws_bytes(1, 0, 7) == 0


def test_ctc_rows_and_write_result(tmp_path):
    from PIL import Image
    from unet_amd.track import ctc_rows, write_result
    rows = np.array([[1, 0, 1, -1], [2, 0, 0, -1], [3, 1, 5, 2], [40000, 5, 5, -1]], np.int32)
    c = ctc_rows(rows)
    np.testing.assert_array_equal(c, [[1, 0, 1, 0], [2, 0, 0, 0], [3, 1, 5, 2], [40000, 5, 5, 0]])
    assert rows[0, 3] == -1           # a copy
    rng = np.random.default_rng(3)
    masks = rng.choice(np.array([0, 1, 2, 3, 255, 256, 40000, 65535], np.uint16), size=(3, 9, 13))
    frames = [0, 5, 123]
    out = tmp_path / "01_RES"
    write_result(rows, masks, frames, str(out))
    assert sorted(os.listdir(out)) == ["mask000.tif", "mask005.tif", "mask123.tif", "res_track.txt"]
    for f, m in zip(frames, masks):
        a = np.array(Image.open(out / f"mask{f:03d}.tif"))
        assert a.dtype == np.uint16
        np.testing.assert_array_equal(a, m)
    assert (out / "res_track.txt").read_text().splitlines() == ["1 0 1 0", "2 0 0 0", "3 1 5 2", "40000 5 5 0"]
    with pytest.raises(ValueError):
        write_result(rows, masks, frames[:2], str(out))


TRA03 = {  # tracking the fixture's own frames as instance masks, scored against gt / gt_track
    "gt": dict(tracks=None, DET=1.0, TRA=1 - 5.5 / 278.5, NS=0, FN=0, FP=0, ED=0, EA=3, EC=1),
    "res": dict(tracks=13, DET=0.688, TRA=0.628366, NS=5, FN=5, FP=3, ED=0, EA=17, EC=0),
}


def check_tra03(got, want):
    """Counts exactly; the measures, from those counts and the ground truth's
    25 vertices and 19 edges (AOGM0 = 278.5), to 1e-12."""
    ops = ("NS", "FN", "FP", "ED", "EA", "EC")
    assert {k: got["counts"][k] for k in ops} == {k: want[k] for k in ops}
    assert (got["counts"]["V_GT"], got["counts"]["E_GT"]) == (25, 19)
    vertex = 5 * want["NS"] + 10 * want["FN"] + want["FP"]
    det = 1 - vertex / 250
    tra = 1 - (vertex + want["ED"] + 1.5 * want["EA"] + want["EC"]) / 278.5
    assert abs(got["DET"] - det) < 1e-12 and abs(got["TRA"] - tra) < 1e-12
    # the same figures as quoted in DESIGN.md (three and six decimals for "res")
    assert abs(det - want["DET"]) < 5e-4 and abs(tra - want["TRA"]) < 5e-7


@pytest.mark.parametrize("scope", list(SCOPES))
@pytest.mark.parametrize("which", ["gt", "res"])
def test_tra03_end_to_end_from_host_maps(tra03, which, scope):
    """The fixture's frames tracked as instance masks, relabelled through the
    library's maps, rows through ctc_rows: rules() gives the expected measures."""
    from unet_amd.track import ctc_rows
    stack, frames = tra03[which], tra03["frames"]
    rows, maps, lrows, lmaps = host_track(stack, frames, scope)
    np.testing.assert_array_equal(lrows, rows)
    assert [m for _, m in lmaps] == maps
    if TRA03[which]["tracks"] is not None:
        assert len(lrows) == TRA03[which]["tracks"]
    masks = M.relabel(stack, [m for _, m in lmaps])
    got = rules(stack_tables(tra03["gt"], masks, frames), tra03["gt_track"], ctc_rows(lrows))
    check_tra03(got, TRA03[which])
