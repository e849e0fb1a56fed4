"""Cell Tracking Challenge measures SEG / DET / TRA: the library's host logic
(unet_ctc_add_frame_host, no device work) against

* the log the evaluator itself wrote for its demo set 03
  (EvaluationSoftware/testing_dataset/03_RES/TRA_log.txt, in
  tests/golden/ctc_tra03.npz): every penalised operation, line for line, and
  "TRA measure: 0.622980" = 1 - 105 / 278.5;
* for SEG, of which no tool output exists, the definition itself (mean Jaccard
  index of the reference objects with their matches, a match being
  2 |R and S| > |R|), evaluated by brute force in NumPy here;
* a small pure-Python statement of the graph rules (rules()) on synthetic
  graphs.

The overlap tables are made with NumPy in this file (host_tables)."""
import errno
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")
COUNTS = ("NS", "FN", "FP", "ED", "EA", "EC", "V_GT", "E_GT")


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def seg01():
    return np.load(os.path.join(G, "ctc_seg01.npz"), allow_pickle=False)


def host_tables(gt, res, frame):
    """add_frame_host's tables of one frame pair."""
    gl, ga = np.unique(gt[gt > 0], return_counts=True)
    rl, ra = np.unique(res[res > 0], return_counts=True)
    both = (gt > 0) & (res > 0)
    key, n = np.unique(gt[both].astype(np.int64) << 16 | res[both], return_counts=True)
    return {"frame": int(frame), "gt_labels": gl, "gt_areas": ga, "res_labels": rl, "res_areas": ra,
            "pairs": np.stack([key >> 16, key & 0xFFFF, n], 1).reshape(-1, 3)}


def stack_tables(gt, res, frames):
    return [host_tables(g, r, f) for g, r, f in zip(gt, res, frames)]


def seg_brute_force(gt, res):
    """SEG by its definition, one boolean mask pair per object."""
    js = []
    for g, r in zip(gt, res):
        for lab in np.unique(g[g > 0]):
            R = g == lab
            j = 0.0
            for s in np.unique(r[R & (r > 0)]):
                S = r == s
                inter = int((R & S).sum())
                if 2 * inter > int(R.sum()):
                    j = inter / int((R | S).sum())
            js.append(j)
    return float(np.mean(js)), sum(1 for j in js if j == 0.0), len(js)


def rules(tables, gt_rows, res_rows):
    """The contract, stated plainly: counts and measures of TRA frames given as
    host tables and the two track tables."""
    tables = sorted(tables, key=lambda f: f["frame"])

    def graph(side, rows):
        present = {(f["frame"], int(l)) for f in tables for l in f[side + "_labels"]}
        edges = {}
        by_label = {int(r[0]): r for r in rows}
        def verts(l):
            _, b, e, _ = by_label[l]
            return [(t, l) for t in sorted(f["frame"] for f in tables) if b <= t <= e and (t, l) in present]
        for l, b, e, p in (map(int, r) for r in rows):
            v = verts(l)
            if p and v and verts(p):
                edges.setdefault((verts(p)[-1], v[0]), "parent")
            for a, c in zip(v, v[1:]):
                edges.setdefault((a, c), "track")
        return present, edges

    VG, EG = graph("gt", gt_rows)
    VR, ER = graph("res", res_rows)
    match = {}
    for f in tables:
        area = dict(zip(map(int, f["gt_labels"]), map(int, f["gt_areas"])))
        for g, r, n in np.asarray(f["pairs"]).reshape(-1, 3):
            if 2 * int(n) > area[int(g)]:
                match[(f["frame"], int(g))] = (f["frame"], int(r))
    hits = {}
    for g, r in match.items():
        hits.setdefault(r, []).append(g)
    c = dict.fromkeys(COUNTS, 0)
    c["NS"] = sum(len(h) - 1 for h in hits.values())
    c["FN"] = sum(1 for v in VG if v not in match)
    c["FP"] = sum(1 for v in VR if v not in hits)
    unique = {r: h[0] for r, h in hits.items() if len(h) == 1}
    for (a, b), kind in ER.items():
        if a in unique and b in unique:
            k = EG.get((unique[a], unique[b]))
            c["ED"] += k is None
            c["EC"] += k is not None and k != kind
    for (a, b) in EG:
        ok = a in match and b in match and match[a] in unique and match[b] in unique and (match[a], match[b]) in ER
        c["EA"] += not ok
    c["V_GT"], c["E_GT"] = len(VG), len(EG)
    det = 5 * c["NS"] + 10 * c["FN"] + c["FP"]
    aogm = det + c["ED"] + 1.5 * c["EA"] + c["EC"]
    a0 = 10 * c["V_GT"] + 1.5 * c["E_GT"]
    return {"DET": 1 - min(det, 10 * c["V_GT"]) / (10 * c["V_GT"]), "TRA": 1 - min(aogm, a0) / a0,
            "counts": {k: int(v) for k, v in c.items()}}


def evaluator(tra=(), seg=(), gt_rows=None, res_rows=None):
    from unet_amd.ctc import CTCEvaluator
    return CTCEvaluator.from_host_tables(seg_frames=seg, tra_frames=tra, gt_tracks=gt_rows, res_tracks=res_rows)


def log_lines(text):
    return [ln.rstrip() for ln in text.rstrip().splitlines()]


# ------------------------------ the demo sets --------------------------------
def test_tra03_matches_the_evaluators_log(tra03):
    tabs = stack_tables(tra03["gt"], tra03["res"], tra03["frames"])
    ev = evaluator(tra=tabs, gt_rows=tra03["gt_track"], res_rows=tra03["res_track"])
    m = ev.measures()
    print(m)
    assert m["counts"] == dict(NS=5, FN=5, FP=3, ED=1, EA=16, EC=2, V_GT=25, E_GT=19)
    assert abs(m["TRA"] - (1 - 105 / 278.5)) < 1e-12
    assert "%.6f" % m["TRA"] == "0.622980"
    # the tool left no DET log: the value follows from the counts its TRA log pins
    assert m["DET"] == 1 - 78 / 250
    assert np.isnan(m["SEG"])
    assert log_lines(ev.log()) == log_lines(tra03["tra_log"].tobytes().decode())
    assert rules(tabs, tra03["gt_track"], tra03["res_track"]) == {k: m[k] for k in ("DET", "TRA", "counts")}


def test_seg01_matches_the_definition(seg01):
    """No tool output exists for SEG: the definition is the reference."""
    want, unmatched, n = seg_brute_force(seg01["gt"], seg01["res"])
    print(want, unmatched, n)
    assert n == 121 and unmatched == 71
    ev = evaluator(seg=stack_tables(seg01["gt"], seg01["res"], seg01["frames"]))
    m = ev.measures()
    assert abs(m["SEG"] - want) < 1e-12
    assert np.isnan(m["DET"]) and np.isnan(m["TRA"])


# ------------------------------ synthetic graphs -----------------------------
def blobs(h, w, boxes):
    """boxes: {label: (y0, y1, x0, x1)} -> uint16 image"""
    img = np.zeros((h, w), np.uint16)
    for l, (y0, y1, x0, x1) in boxes.items():
        img[y0:y1, x0:x1] = l
    return img


def check(tabs, gt_rows, res_rows, want_counts=None):
    gt_rows, res_rows = np.asarray(gt_rows, np.int32).reshape(-1, 4), np.asarray(res_rows, np.int32).reshape(-1, 4)
    ev = evaluator(tra=tabs, gt_rows=gt_rows, res_rows=res_rows)
    m = ev.measures()
    want = rules(tabs, gt_rows, res_rows)
    assert m["counts"] == want["counts"]
    assert m["DET"] == want["DET"] and m["TRA"] == want["TRA"]
    if want_counts is not None:
        assert {k: m["counts"][k] for k in want_counts} == want_counts
    return m, ev.log()


def moving(frames, labels=(1, 2), gap=None):
    """Each label a 4x4 box that drifts one pixel per frame; gap = (label, frame) left out."""
    out = []
    for t in frames:
        boxes = {l: (2, 6, 6 * k + t, 6 * k + t + 4) for k, l in enumerate(labels) if (l, t) != gap}
        out.append(blobs(12, 40, boxes))
    return np.stack(out)


def test_identical_sequences_score_one():
    gt = moving(range(4))
    rows = [[1, 0, 3, 0], [2, 0, 3, 0]]
    m, log = check(stack_tables(gt, gt, range(4)), rows, rows, dict(NS=0, FN=0, FP=0, ED=0, EA=0, EC=0, V_GT=8, E_GT=6))
    assert m["DET"] == 1.0 and m["TRA"] == 1.0
    sections = [ln for ln in log.splitlines() if not ln.startswith(("-", "="))]
    assert sections == ["TRA measure: 1.000000"]
    seg = evaluator(seg=stack_tables(gt, gt, range(4))).measures()
    assert seg["SEG"] == 1.0


def test_empty_result_scores_zero():
    gt = moving(range(3))
    m, _ = check(stack_tables(gt, np.zeros_like(gt), range(3)), [[1, 0, 2, 0], [2, 0, 2, 0]], [],
                 dict(FN=6, EA=4, FP=0))
    assert m["DET"] == 0.0 and m["TRA"] == 0.0


def test_aogm_above_aogm0_clamps_to_zero():
    gt = moving(range(2), labels=(1,))
    res = np.stack([blobs(12, 40, {l: (8, 10, 3 * l, 3 * l + 2) for l in range(1, 13)})] * 2)  # 12 false positives each
    rows = [[l, 0, 1, 0] for l in range(1, 13)]
    m, _ = check(stack_tables(gt, res, range(2)), [[1, 0, 1, 0]], rows, dict(FN=2, FP=24, EA=1))
    assert 20 + 24 + 1.5 > 20 + 1.5 and m["TRA"] == 0.0 and m["DET"] == 0.0


def test_track_with_a_gap_frame_links_the_present_neighbours():
    gt = moving(range(4), gap=(2, 1))
    rows = [[1, 0, 3, 0], [2, 0, 3, 0]]
    m, _ = check(stack_tables(gt, gt, range(4)), rows, rows, dict(V_GT=7, E_GT=5, EA=0, ED=0))
    assert m["TRA"] == 1.0
    # the result breaks the track at the gap instead: the GT edge 0 -> 2 is to be added
    res = gt.copy()
    res[2:][res[2:] == 2] = 3
    m, log = check(stack_tables(gt, res, range(4)), rows, [[1, 0, 3, 0], [2, 0, 0, 0], [3, 2, 3, 0]], dict(EA=1, ED=0))
    assert "[T=0 GT_label=2] -> [T=2 GT_label=2]" in log


def test_parent_link_from_a_parent_that_ended_two_frames_earlier():
    gt = np.stack([blobs(12, 40, {1: (2, 8, 2, 8)}), blobs(12, 40, {1: (2, 8, 2, 8)}), blobs(12, 40, {}),
                   blobs(12, 40, {2: (2, 5, 2, 8), 3: (5, 8, 2, 8)})])
    rows = [[1, 0, 1, 0], [2, 3, 3, 1], [3, 3, 3, 1]]
    m, _ = check(stack_tables(gt, gt, range(4)), rows, rows, dict(V_GT=4, E_GT=3, EA=0))
    assert m["TRA"] == 1.0
    # the result calls the daughters a continuation and a new track: one edge has the wrong kind, one is missing
    res_rows = [[1, 0, 1, 0], [2, 3, 3, 0], [3, 3, 3, 0]]
    m, log = check(stack_tables(gt, gt, range(4)), rows, res_rows, dict(EA=2, EC=0, ED=0))
    res = gt.copy()
    res[3][res[3] == 2] = 1
    m, log = check(stack_tables(gt, res, range(4)), rows, [[1, 0, 3, 0], [3, 3, 3, 0]], dict(EC=1, EA=1, ED=0))
    assert "[T=1 Label=1] -> [T=3 Label=1]" in log.split("Wrong Semantics")[1]


def test_one_result_vertex_over_three_markers():
    gt = np.stack([blobs(12, 40, {1: (2, 4, 2, 4), 2: (2, 4, 6, 8), 3: (2, 4, 10, 12)})] * 2)
    res = np.stack([blobs(12, 40, {7: (1, 5, 1, 13)}),
                    blobs(12, 40, {8: (2, 4, 2, 4), 9: (2, 4, 6, 8), 10: (2, 4, 10, 12)})])
    gt_rows = [[1, 0, 1, 0], [2, 0, 1, 0], [3, 0, 1, 0]]
    # three parent links leave the vertex that is not unique: none is redundant
    # or of the wrong kind, and no GT edge finds its counterpart
    m, log = check(stack_tables(gt, res, range(2)), gt_rows,
                   [[7, 0, 0, 0], [8, 1, 1, 7], [9, 1, 1, 7], [10, 1, 1, 7]],
                   dict(NS=2, FN=0, FP=0, ED=0, EC=0, EA=3))
    assert log.count("T=0 Label=7") == 2


def test_half_covered_is_no_match_half_plus_one_is():
    gt = blobs(12, 40, {1: (2, 6, 2, 6)})[None]  # 16 pixels
    half = blobs(12, 40, {1: (2, 6, 2, 4)})[None]  # 8 of them
    m, _ = check(stack_tables(gt, half, [0]), [[1, 0, 0, 0]], [[1, 0, 0, 0]], dict(FN=1, FP=1))
    assert evaluator(seg=stack_tables(gt, half, [0])).measures()["SEG"] == 0.0
    half[0, 2, 4] = 1  # 9 of them
    m, _ = check(stack_tables(gt, half, [0]), [[1, 0, 0, 0]], [[1, 0, 0, 0]], dict(FN=0, FP=0))
    assert evaluator(seg=stack_tables(gt, half, [0])).measures()["SEG"] == 9 / 16


# ---------------------------------- errors -----------------------------------
def _raises(rc, *words):
    class Ctx:
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert et is RuntimeError, f"expected a RuntimeError, got {et}"
            msg = str(ev)
            assert f"rc={-rc}" in msg and all(w in msg for w in words), msg
            return True
    return Ctx()


def test_error_cases():
    from unet_amd import _lib
    from unet_amd.ctc import CTCEvaluator
    gt = moving(range(2))
    tabs = stack_tables(gt, gt, [4, 5])
    rows = [[1, 4, 5, 0], [2, 4, 5, 0]]
    with _raises(errno.ENOENT, "RES", "label 2", "frame 4", "no track row"):
        evaluator(tra=tabs, gt_rows=rows, res_rows=rows[:1]).measures()
    with _raises(errno.ENOENT, "GT", "label 1", "frame 4"):
        evaluator(tra=tabs, gt_rows=rows[1:], res_rows=rows).log()
    with _raises(errno.ESRCH, "GT", "label 2", "parent 9", "frame 4"):
        evaluator(tra=tabs, gt_rows=[[1, 4, 5, 0], [2, 4, 5, 9]], res_rows=rows).measures()
    ev = CTCEvaluator()
    with _raises(errno.ENODATA, "SEG", "frame 7", "no RES frame"):
        ev.add_frame_host("SEG", 7, tabs[0]["gt_labels"], tabs[0]["gt_areas"], None, None, np.zeros((0, 3)))
    lib = _lib.load()
    assert lib.unet_ctc_add_frames(ev.handle, 1, None, None, None, 0, 37, 53, None, None) == 0
    rc = lib.unet_ctc_add_frames(ev.handle, 1, None, None, None, 0, 53, 37, None, None)
    assert rc == -errno.EINVAL and "sizes differ" in _lib.last_error() and "53 x 37" in _lib.last_error()
    with _raises(errno.EEXIST, "frame 4"):
        evaluator(tra=tabs + tabs[:1])
