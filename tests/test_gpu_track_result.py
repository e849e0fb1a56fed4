"""Track-labelled result masks on the device (unet_tracker_relabel,
unet_amd.track.Tracker.relabel / track_stack / track_sequence(result_dir=...),
tools/track_sequence.py) against tests/track_map_oracle.py, and the written
result sequence through unet_amd.ctc.evaluate_sequence.

Shapes: (3, 5, 7) -- 35 pixels per frame, so frames 1 and 2 start off a
16-byte boundary and the vector body is followed by a tail of under 8 pixels,
table in LDS; (2, 37, 41) with labels up to 65535 -- the table is read through
L2; 40 x 50 and the 324 x 324 HeLa stack -- more than one workgroup per frame.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import track_map_oracle as M
from test_track_result_cpu import TRA03, check_tra03

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def track():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import track
    return track


@pytest.fixture(scope="module")
def hela():
    return np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def host(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def launches(reset=False):
    from unet_amd import _lib
    return int(_lib.load().unet_tracker_relabel_launches(1 if reset else 0))


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


def test_misaligned_frames_and_in_place(track):
    rng = np.random.default_rng(11)
    seq = rng.integers(0, 7, (3, 5, 7)).astype(np.int32)
    rows, maps, _ = M.track_maps(seq)
    want = M.relabel(seq, maps)
    launches(reset=True)
    grows, masks = track.track_stack(dev(seq))
    assert launches() == 1                  # one launch for the three frames
    np.testing.assert_array_equal(grows, rows)
    assert masks.dtype == torch.uint16 and tuple(masks.shape) == seq.shape
    np.testing.assert_array_equal(host(masks), want)
    # in place, through a tracker of its own
    tr = track.Tracker(5, 7)
    stack = torch.from_numpy(seq.astype(np.uint16).view(np.int16)).cuda().view(torch.uint16)
    for i in range(3):
        tr.add_frame(stack[i], i)
    assert tr.relabel(stack, [0, 1, 2], out=stack) is stack
    np.testing.assert_array_equal(host(stack), want)
    assert launches() == 2


def test_labels_up_to_65535_read_the_table_through_l2(track):
    rng = np.random.default_rng(12)
    seq = rng.choice(np.array([0, 1, 2, 300, 40000, 65535]), size=(2, 37, 41)).astype(np.int32)
    rows, maps, _ = M.track_maps(seq)
    grows, masks = track.track_stack(dev(seq))
    np.testing.assert_array_equal(grows, rows)
    np.testing.assert_array_equal(host(masks), M.relabel(seq, maps))


def test_edge_sequence_masks_and_rows(track):
    seq = edge_sequence()
    rows, maps, _ = M.track_maps(seq)
    grows, masks = track.track_stack(dev(seq))
    np.testing.assert_array_equal(grows, rows)
    m = host(masks)
    np.testing.assert_array_equal(m, M.relabel(seq, maps))
    kids = rows[rows[:, 3] > 0]
    assert len(kids) == 2 and set(kids[:, 1]) == {2}
    left, right = np.unique(m[2, 5:25, 5:10]), np.unique(m[2, 5:25, 20:25])
    assert len(left) == 1 and len(right) == 1
    assert {int(left[0]), int(right[0])} == set(int(k) for k in kids[:, 0])
    assert not m[3].any()                   # the empty frame
    np.testing.assert_array_equal(m > 0, seq > 0)


def test_maps_are_chosen_by_frame_number(track):
    seq = edge_sequence()
    _, maps, _ = M.track_maps(seq)
    d = dev(seq)
    tr = track.Tracker(40, 50)
    for i in range(6):
        tr.add_frame(d[i], i)
    launches(reset=True)
    got = host(tr.relabel(d[[4, 1]], [4, 1]))
    assert launches() == 1
    np.testing.assert_array_equal(got, M.relabel(seq[[4, 1]], [maps[4], maps[1]]))
    # frame 1's labels through frame 4's map: label 9 is not listed there -> 0
    assert not host(tr.relabel(d[1:2], [4])).any()
    with pytest.raises(RuntimeError, match="frame 6"):
        tr.relabel(d[:1], [6])
    with pytest.raises(ValueError):
        tr.relabel(d[:2], [0])
    with pytest.raises(ValueError):
        tr.relabel(d.cpu(), list(range(6)))
    with pytest.raises(ValueError):
        tr.relabel(d + 65536, list(range(6)))


@pytest.mark.parametrize("scope", ["shared", "frame"])
def test_hela_fixture(track, hela, scope):
    labels, frames = hela["labels"], hela["frames"]
    rows, maps, _ = M.track_maps(labels, frames, scope)
    want = M.relabel(labels, maps)
    d = dev(labels)
    tr = track.Tracker(labels.shape[1], labels.shape[2], label_scope=scope)
    for i in range(len(labels)):
        tr.add_frame(d[i], int(frames[i]))
    launches(reset=True)
    grows, masks = tr.tracks(), tr.relabel(d, frames)
    assert launches() == 1                  # 84 frames, one launch
    np.testing.assert_array_equal(grows, rows)
    # what tools/track_sequence.py prints, from the oracle's maps and rows
    shown = {}
    for f, mp in zip(frames, maps):
        for tid in mp.values():
            shown.setdefault(tid, set()).add(int(f))
    given = set(int(f) for f in frames)
    gaps = sum(1 for t, s, e, _ in rows.tolist()
               if any(f in given and f not in shown.get(t, ()) for f in range(s, e + 1)))
    assert track.result_stats(tr) == {"tracks": len(rows), "objects_without_track": len(M.trackless(maps)),
                                      "rows_with_absent_frames": gaps}
    print(scope, track.result_stats(tr))
    m = host(masks)
    np.testing.assert_array_equal(m, want)
    lost = np.zeros(labels.shape, bool)
    for i, lab in M.trackless(maps):
        lost[i] |= labels[i] == lab
    assert lost.any() == (scope == "shared")
    if scope == "shared":
        assert len(M.trackless(maps)) == 5
    np.testing.assert_array_equal((m > 0) != (labels > 0), lost)


def write_tifs(directory, pattern, frames, stack):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for f, img in zip(frames, stack):
        Image.fromarray(np.ascontiguousarray(img).astype(np.uint16)).save(os.path.join(directory, pattern % int(f)))


def read_dir(directory):
    from PIL import Image
    return {n: (open(os.path.join(directory, n)).read() if n.endswith(".txt")
                else np.array(Image.open(os.path.join(directory, n)))) for n in sorted(os.listdir(directory))}


@pytest.mark.parametrize("which", ["gt", "res"])
def test_files_end_to_end_on_tra03(track, tra03, tmp_path, which):
    """instance masks on disk -> track_sequence / tools/track_sequence.py ->
    <seq>_RES -> evaluate_sequence against <seq>_GT."""
    from unet_amd import ctc
    frames = [int(f) for f in tra03["frames"]]
    inst, res, res_tool, gt = (str(tmp_path / n) for n in ("03_RES_INST", "03_RES", "03_RES_TOOL", "03_GT"))
    write_tifs(inst, "m%03d.tif", frames, tra03[which])
    write_tifs(os.path.join(gt, "TRA"), "man_track%03d.tif", frames, tra03["gt"])
    track.write_track_file(tra03["gt_track"], os.path.join(gt, "TRA", "man_track.txt"))
    rows = track.track_sequence(inst, str(tmp_path / "reference_style.txt"), result_dir=res)
    if TRA03[which]["tracks"] is not None:
        assert len(rows) == TRA03[which]["tracks"]
    # the reference's file keeps -1, the result directory's has 0
    assert (tmp_path / "reference_style.txt").read_text().splitlines()[0].endswith(" -1")
    want_names = [f"mask{f:03d}.tif" for f in frames] + ["res_track.txt"]
    assert sorted(os.listdir(res)) == want_names
    np.testing.assert_array_equal(ctc.read_track_file(os.path.join(res, "res_track.txt")), track.ctc_rows(rows))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "track_sequence.py"), "--masks", inst,
                        "--out", res_tool], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"tracks: {len(rows)}" in r.stdout
    a, b = read_dir(res), read_dir(res_tool)
    assert list(a) == list(b) == want_names
    for n in want_names:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
    got = ctc.evaluate_sequence(gt, res_tool)
    print(which, got["DET"], got["TRA"], got["counts"])
    check_tra03(got, TRA03[which])
