"""The distance-based linker without a GPU: the library's host twin
(unet_link_frames_host), the track assembly (unet_link_assemble) and
unet_tracker_load_result against tests/link_oracle.py -- scipy's assignment for
the optimal total (and the links where the optimum is unique), the definition's
algorithm in plain Python on tie-laden cases.
"""
import ctypes
import errno
import os

import numpy as np
import pytest

import link_cases as K
import link_oracle as LO
import region_oracle as RO

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def lib():
    from unet_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def hela_table():
    return K.from_labels(np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)["labels"])


def against_scipy(lib, table, gate, division_gate=0.0, unique_pairs=None):
    """pair_total everywhere; prev / dist / mother on the pairs whose optimum is
    unique.  Returns (host outputs, oracle outputs)."""
    offsets, cols = table
    want = LO.link(offsets, cols, gate, division_gate, unique_pairs=unique_pairs)
    rc, prev, dist, mother, pair_total = K.host_link(lib, offsets, cols, LO.gate_q(gate), LO.gate_q(division_gate))
    assert rc == 0
    np.testing.assert_array_equal(pair_total, want["pair_total"])
    assert (prev[:offsets[1]] == -1).all() and (dist[:offsets[1]] == -1).all() and (mother[:offsets[1]] == -1).all()
    for f, uniq in enumerate(want["unique"]):
        if uniq:
            s = slice(int(offsets[f + 1]), int(offsets[f + 2]))
            for k, got in (("prev", prev), ("dist", dist), ("mother", mother)):
                np.testing.assert_array_equal(got[s], want[k][s], err_msg=f"{k} of pair {f}")
    return (prev, dist, mother, pair_total), want


def against_algorithm(lib, table, gate, division_gate=0.0):
    offsets, cols = table
    want = LO.link(offsets, cols, gate, division_gate, solver="algorithm")
    rc, prev, dist, mother, pair_total = K.host_link(lib, offsets, cols, LO.gate_q(gate), LO.gate_q(division_gate))
    assert rc == 0
    scipy_total = LO.link(offsets, cols, gate, division_gate, unique_pairs=())["pair_total"]
    np.testing.assert_array_equal(want["pair_total"], scipy_total)     # the plain-Python algorithm is optimal too
    np.testing.assert_array_equal(pair_total, scipy_total)
    for k, got in (("prev", prev), ("dist", dist), ("mother", mother)):
        np.testing.assert_array_equal(got, want[k], err_msg=k)
    return prev, dist, mother, pair_total


@pytest.mark.parametrize("key", ["gt", "res"])
def test_tra03_at_gate_40(lib, tra03, key):
    table = K.from_labels(tra03[key])
    _, want = against_scipy(lib, table, 40.0, 60.0)
    assert all(want["unique"])        # the prototype found every pair's optimum unique


def test_hela_every_tenth_pair_and_the_link_count(lib, hela_table):
    offsets, _ = hela_table
    assert offsets[-1] == 11412
    tenth = set(range(0, len(offsets) - 2, 10))
    (prev, _, _, _), want = against_scipy(lib, hela_table, 20.0, unique_pairs=tenth)
    assert all(want["unique"][f] for f in tenth)
    links = int((want["prev"] >= 0).sum())
    print(f"hela_postproc at gate 20: {links} links (oracle), {int((prev >= 0).sum())} (host twin); "
          f"the CPU prototype reported 8,242")
    assert int((prev >= 0).sum()) == links
    tracks = 11412 - links            # every object without a predecessor starts a track
    k, rows, _ = K.host_assemble(lib, offsets, hela_table[1], np.arange(len(offsets) - 1), prev,
                                 np.zeros_like(prev, np.int64), np.full_like(prev, -1))
    assert k == tracks == len(rows)


def test_tie_lattice_follows_the_definition(lib):
    table = K.from_labels(K.lattice(), RO.direct)
    prev, _, _, total = against_algorithm(lib, table, 5.0)
    assert (prev[36:] >= 0).all() and total[0] == 36 * 32 * 32


def test_two_predecessors_equidistant_from_one_successor(lib):
    table = K.from_points([[(80, 32), (80, 128)], [(80, 80)]])
    prev, dist, _, total = against_algorithm(lib, table, 10.0)
    # both assignments cost 48^2 + g2.  Row 1's search reaches row 0's private column (index 1) and its own
    # (index 2) at the same distance: rule (b) takes the lower one, so row 0 gives the successor up
    assert prev.tolist() == [-1, -1, 1] and dist[2] == 48 * 48 and total[0] == 48 * 48 + 160 * 160


@pytest.mark.parametrize("reverse", [False, True])
def test_chain_follows_the_definition(lib, reverse):
    prev, _, _, total = against_algorithm(lib, K.chain(reverse), 40.0)
    assert (prev[64:] >= 0).all() and total[0] == 64 * 96 * 96


def test_gate_boundary(lib):
    # d = 47^2 + 1; g2 = 47^2 excludes it, the same d with the y offset 0 is on the gate
    for pts, links in (([[(0, 0)], [(0, 47)]], True), ([[(0, 0)], [(1, 47)]], False)):
        offsets, cols = K.from_points(pts)
        rc, prev, dist, _, total = K.host_link(lib, offsets, cols, 47)
        assert rc == 0
        d = 47 * 47 + (0 if links else 1)
        assert prev.tolist() == [-1, 0 if links else -1] and dist[1] == (d if links else -1)
        assert total[0] == 47 * 47          # the link on the gate costs what the private column costs
        against_scipy(lib, (offsets, cols), 47 / 16)
    offsets, cols = K.from_points([[(0, 0)], [(1, 47)]])
    assert K.host_link(lib, offsets, cols, 48)[1].tolist() == [-1, 0]


def division_table():
    """Frame 0: a mother (area 32) and a bystander; frame 1: the mother's
    successor (area 16) and claimants of area 16, 4 and 16 at 3, 2 and 4 pixels
    from her, and the bystander's successor."""
    return K.from_points([[(160, 160, 32), (800, 800)],
                          [(160, 176), (160, 112), (192, 160, 4), (160, 224), (800, 816)]])


@pytest.mark.parametrize("ratio,max_children,division_gate,want_children", [
    (0.5, 2, 6.0, [2, 3]),          # taken: the nearest claimant that passes (the 2-pixel one has a quarter of the area)
    (0.2, 2, 6.0, [2, 4]),          # the ratio admits the nearest one
    (0.5, 3, 6.0, [2, 3, 5]),       # three claimants, two pass: both taken with max_children 3
    (0.5, 2, 2.5, []),              # only the small claimant is inside the division gate: refused by the area ratio
    (1.01, 2, 6.0, []),             # refused by the area ratio
    (0.5, 1, 6.0, []),              # max_children 1: no division
    (0.5, 2, 0.0, []),              # division_gate 0
])
def test_assembly_divisions(lib, ratio, max_children, division_gate, want_children):
    offsets, cols = division_table()
    frames = [3, 5]
    (prev, dist, mother, _), want = against_scipy(lib, (offsets, cols), 1.5, division_gate)
    assert all(want["unique"]) and prev.tolist() == [-1, -1, 0, -1, -1, -1, 1]
    assert mother.tolist() == ([-1] * 7 if division_gate == 0 else
                               [-1, -1, -1, -1, 0, -1, -1] if division_gate < 3 else [-1, -1, -1, 0, 0, 0, -1])
    k, rows, ids = K.host_assemble(lib, offsets, cols, frames, prev, dist, mother, ratio, max_children)
    orows, oids = LO.assemble(offsets, cols, frames, want["prev"], want["mother"], ratio, max_children)
    assert k == len(orows)
    np.testing.assert_array_equal(rows, orows)
    np.testing.assert_array_equal(ids, oids)
    children = [r for r in range(2, 7) if rows[ids[r] - 1][3] == 1]
    assert children == want_children
    if want_children:
        assert rows[0].tolist() == [1, 3, 3, -1]                   # the mother's track ends in the previous frame
        assert ids[children].tolist() == sorted(ids[children].tolist())     # ids ascend with the label
        assert all(rows[ids[r] - 1].tolist() == [ids[r], 5, 5, 1] for r in children)
    else:
        assert rows[0].tolist() == [1, 3, 5, -1] and ids[2] == 1
    for r in (3, 4, 5):                                            # a claimant that was not taken is a root birth
        if r not in children:
            assert rows[ids[r] - 1].tolist() == [ids[r], 5, 5, -1]


def load_result(lib, rows, frames, offsets, labels, ids, t=None):
    own = t is None
    if own:
        t = lib.unet_tracker_create(8, 8, 0.3, 0.1, 2)
    a = [np.ascontiguousarray(v, np.int32) for v in (rows, frames, offsets, labels, ids)]
    rc = lib.unet_tracker_load_result(t, K.vp(a[0]), len(a[0]), K.vp(a[1]), len(a[1]),
                                      a[2].ctypes.data_as(ctypes.c_void_p), K.vp(a[3]), K.vp(a[4]))
    return rc, t


def test_tracker_load_result_round_trip_and_errors(lib):
    offsets, cols = division_table()
    (prev, dist, mother, _), _ = against_scipy(lib, (offsets, cols), 1.5, 6.0)
    k, rows, ids = K.host_assemble(lib, offsets, cols, [3, 5], prev, dist, mother)
    rc, t = load_result(lib, rows, [3, 5], offsets, cols["label"], ids)
    assert rc == 0 and lib.unet_tracker_num_tracks(t) == k and lib.unet_tracker_num_frames(t) == 2
    out = np.zeros((k, 4), np.int32)
    assert lib.unet_tracker_tracks(t, K.vp(out), k) == k
    np.testing.assert_array_equal(out, rows)
    for i in range(2):
        a, b = int(offsets[i]), int(offsets[i + 1])
        frame = ctypes.c_int32(-1)
        labels, got = np.zeros(b - a, np.int32), np.zeros(b - a, np.int32)
        assert lib.unet_tracker_frame_map(t, i, ctypes.byref(frame), K.vp(labels), K.vp(got), b - a) == b - a
        assert frame.value == [3, 5][i]
        np.testing.assert_array_equal(labels, cols["label"][a:b])
        np.testing.assert_array_equal(got, ids[a:b])
    # a tracker that already has frames
    assert load_result(lib, rows, [3, 5], offsets, cols["label"], ids, t)[0] == -errno.EBUSY
    lib.unet_tracker_destroy(t)
    t = lib.unet_tracker_create(8, 8, 0.3, 0.1, 2)
    one = np.array([4], np.int32)
    assert lib.unet_tracker_step_host(t, 0, 1, K.vp(one), K.vp(one.astype(np.int64)), None) == 0
    assert load_result(lib, rows, [3, 5], offsets, cols["label"], ids, t)[0] == -errno.EBUSY
    lib.unet_tracker_destroy(t)
    # frame numbers that do not ascend strictly
    for frames in ([5, 3], [3, 3]):
        rc, t = load_result(lib, rows, frames, offsets, cols["label"], ids)
        assert rc == -errno.EINVAL and lib.unet_tracker_num_frames(t) == 0
        lib.unet_tracker_destroy(t)
        assert K.host_assemble(lib, offsets, cols, frames, prev, dist, mother)[0] == -errno.EINVAL


def test_empty_frames_and_argument_errors(lib):
    offsets, cols = K.from_points([[], [(0, 0), (0, 16)], [], [(0, 0)]])
    rc, prev, dist, mother, total = K.host_link(lib, offsets, cols, 320, 320)
    assert rc == 0 and prev.tolist() == [-1] * 3 and mother.tolist() == [-1] * 3 and total.tolist() == [0, 2 * 320 * 320, 0]
    k, rows, ids = K.host_assemble(lib, offsets, cols, [0, 1, 2, 3], prev, dist, mother)
    assert k == 3 and rows.tolist() == [[1, 1, 1, -1], [2, 1, 1, -1], [3, 3, 3, -1]] and ids.tolist() == [1, 2, 3]
    assert K.host_link(lib, np.zeros(1, np.int32), {k: np.zeros(0, np.int64) for k in RO.FIELDS}, 1)[0] == 0   # n = 0
    offsets, cols = K.from_points([[(0, 0)], [(0, 16)]])
    for gq, dq in ((0, 0), (65536, 0), (1, -1), (1, 65536)):
        assert K.host_link(lib, offsets, cols, gq, dq)[0] == -errno.EINVAL
    assert K.host_link(lib, offsets, cols, 65535, 65535)[0] == 0
    assert lib.unet_link_frames(None, None, -1, 0, 16, 0, None, None, None, None, None, None) == -errno.EINVAL
    assert lib.unet_link_frames(None, None, 2, 2, 16, 0, None, None, None, None, None, None) == -errno.EINVAL
    assert lib.unet_link_ws_bytes(1, 5) == 0 and lib.unet_link_ws_bytes(2, 0) == 0
    assert lib.unet_link_ws_bytes(2, 5) == 9 * 256 and lib.unet_link_ws_bytes(3, 100) == 2 * 1792 + 5 * 1024 + 512 + 256
    assert lib.unet_set_tuning(b"link_lds_objects", -2) == -errno.EINVAL
    assert lib.unet_set_tuning(b"link_lds_objects", 0) == 0 and lib.unet_set_tuning(b"link_lds_objects", -1) == 0


def test_link_stack_host_matches_the_oracle(tra03):
    from unet_amd import link as L
    res = L.link_stack_host(tra03["gt"], gate=40.0, division_gate=60.0)
    offsets, cols = K.from_labels(tra03["gt"])
    want = LO.link(offsets, cols, 40.0, 60.0)
    np.testing.assert_array_equal(res.prev, want["prev"])
    np.testing.assert_array_equal(res.mother, want["mother"])
    rows, ids = LO.assemble(offsets, cols, range(len(offsets) - 1), want["prev"], want["mother"])
    np.testing.assert_array_equal(res.rows, rows)
    np.testing.assert_array_equal(res.ids, ids)
    tr = res.tracker()
    np.testing.assert_array_equal(tr.tracks(), rows)
    f, labels, got = tr.frame_map(3)
    assert f == 3
    np.testing.assert_array_equal(labels, res.frame_map(3)[1])
    np.testing.assert_array_equal(got, res.frame_map(3)[2])
    with pytest.raises(ValueError, match="no CPU fallback"):
        res.masks()
    with pytest.raises(ValueError, match="gate"):
        L.link_stack_host(tra03["gt"], gate=0.0)
