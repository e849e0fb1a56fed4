"""Cell Tracking Challenge measures on the device (unet_ctc_add_frames,
unet_amd.ctc): the overlap records of whole label stacks against NumPy
(labels, areas and pair records exactly; counts are integers), both demo-set
fixtures through the device path against the CPU path (bit for bit), and a
sequence scored against itself and against a shifted copy."""
import os

import numpy as np
import pytest

from test_ctc_cpu import evaluator, seg_brute_force, stack_tables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctc():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import ctc
    return ctc


@pytest.fixture
def tuning():
    """set(key, value) for the evaluator's knobs; the defaults come back afterwards."""
    from unet_amd import _lib
    lib = _lib.load()

    def set_(key, value):
        assert lib.unet_set_tuning(key.encode(), value) == 0
    yield set_
    set_("ctc_chunk_frames", -1)  # -1 = the library's default
    set_("ctc_dense_cells", -1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def same_tables(got, want):
    assert len(got) == len(want)
    for a, b in zip(sorted(got, key=lambda f: f["frame"]), sorted(want, key=lambda f: f["frame"])):
        assert a["frame"] == b["frame"]
        for k in ("gt_labels", "gt_areas", "res_labels", "res_areas", "pairs"):
            np.testing.assert_array_equal(a[k], np.asarray(b[k]).reshape(a[k].shape), err_msg=f"frame {a['frame']} {k}")


def small_stacks():
    """3 frames of 37 x 53, labels {1, 2, 255, 256, 65535}: frame 0 = random
    blocks against an object that fills the frame, frame 1 = GT all background
    against a 1-pixel checkerboard of two labels, frame 2 = the checkerboard
    against an all-background RES."""
    h, w = 37, 53
    rng = np.random.default_rng(5)
    labs = np.array([0, 1, 2, 255, 256, 65535], np.uint16)
    yy, xx = np.mgrid[:h, :w]
    board = np.where((yy + xx) % 2 == 0, 256, 65535).astype(np.uint16)
    blocks = labs[rng.integers(0, 6, (h // 5 + 1, w // 7 + 1))].repeat(5, 0).repeat(7, 1)[:h, :w]
    gt = np.stack([blocks, np.zeros((h, w), np.uint16), board])
    res = np.stack([np.full((h, w), 65535, np.uint16), board, np.zeros((h, w), np.uint16)])
    return gt, res


@pytest.mark.parametrize("mode", ["dense", "hash"])
@pytest.mark.parametrize("chunk,t", [(32, 3), (2, 3), (32, 1)])
def test_overlap_records_small(ctc, tuning, mode, chunk, t):
    gt, res = small_stacks()
    gt, res = gt[:t], res[:t]
    tuning("ctc_chunk_frames", chunk)
    tuning("ctc_dense_cells", 4096 if mode == "dense" else 0)
    ev = ctc.CTCEvaluator()
    ev.add_frames("TRA", dev(gt), dev(res), [10, 11, 12][:t])
    same_tables(ev.frames("TRA"), stack_tables(gt, res, [10, 11, 12][:t]))
    st = ev.stats()
    print(st)
    assert st["chunks"] == -(-t // chunk)
    assert st["dense_frames" if mode == "dense" else "hashed_frames"] == t
    assert st["hashed_frames" if mode == "dense" else "dense_frames"] == 0
    # per chunk: mark + rank, one synchronisation, then one round of count +
    # compact with one synchronisation -- per chunk, not per frame
    assert st["launches"] == 4 * st["chunks"] and st["syncs"] == 2 * st["chunks"]


def test_overlap_records_many_objects(ctc):
    """One 600 x 600 frame of 2 x 2 cells, 300 x 300 distinct label pairs: far
    beyond the dense table, so the frame is counted by hash."""
    yy, xx = np.mgrid[:600, :600]
    gt = (1 + yy // 2).astype(np.uint16)[None]
    res = (65535 - xx // 2).astype(np.uint16)[None]
    ev = ctc.CTCEvaluator()
    ev.add_frames("SEG", dev(gt), dev(res), [0])
    (f,) = ev.frames("SEG")
    assert f["pairs"].shape == (90000, 3) and (f["pairs"][:, 2] == 4).all()
    same_tables([f], stack_tables(gt, res, [0]))
    assert ev.stats()["hashed_frames"] == 1 and ev.stats()["dense_frames"] == 0


def test_mixed_dense_and_hashed_frames_in_one_chunk(ctc):
    yy, xx = np.mgrid[:64, :96]
    many = (1 + (yy // 2) * 48 + xx // 2).astype(np.uint16)  # 1536 objects
    few = (1 + (yy // 32) * 2 + xx // 48).astype(np.uint16)  # 4 objects
    gt, res = np.stack([few, many, few]), np.stack([few, np.roll(many, 1, 1), np.roll(few, 5, 0)])
    ev = ctc.CTCEvaluator()
    ev.add_frames("TRA", dev(gt), dev(res), [0, 1, 2])
    same_tables(ev.frames("TRA"), stack_tables(gt, res, [0, 1, 2]))
    st = ev.stats()
    assert st["hashed_frames"] == 1 and st["dense_frames"] == 2
    assert st["chunks"] == 1 and st["launches"] == 4 and st["syncs"] == 2


def discs(t, h, w, n, seed, shift=0.0):
    """t frames of n drifting discs (radius 3..6), labels 1..n"""
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(6, h - 6, n), rng.uniform(6, w - 6, n)
    vy, vx, rad = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 6, n)
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((t, h, w), np.uint16)
    for f in range(t):
        for k in range(n):
            out[f][(yy - cy[k] - vy[k] * f - shift) ** 2 + (xx - cx[k] - vx[k] * f + shift) ** 2 <= rad[k] ** 2] = k + 1
    return out


def test_a_chunk_of_many_object_frames_is_one_round(ctc, tuning):
    """40 frames of 150 objects each (151 x 151 cells: counted by hash) at 8
    frames per chunk: every chunk passes in one round -- 4 launches and 2
    synchronisations per chunk, whatever the number of frames or objects."""
    gt, res = discs(40, 128, 160, 150, 1), discs(40, 128, 160, 150, 1, shift=1.5)
    tuning("ctc_chunk_frames", 8)
    ev = ctc.CTCEvaluator()
    ev.add_frames("TRA", dev(gt), dev(res), range(40))
    st = ev.stats()
    print(st)
    assert st["hashed_frames"] == 40 and st["chunks"] == 5
    assert st["launches"] == 4 * st["chunks"] and st["syncs"] == 2 * st["chunks"]
    same_tables(ev.frames("TRA")[::13], stack_tables(gt, res, range(40))[::13])


def test_frames_beyond_the_regions_take_more_rounds(ctc, tuning):
    """The stated bound where one round is not enough: frames with another
    label pair at every pixel are charged a whole frame's worst case, 24,576
    records and a 512 KB table each, where the regions hold 256 KB per chunk
    frame (768 KB here): one frame per round, so a chunk of 3 takes 3 rounds,
    2 + 2 R launches and 1 + R synchronisations."""
    h, w = 128, 192
    yy, xx = np.mgrid[:h, :w]
    gt = np.stack([(1 + (yy * w + xx + k) % 12000).astype(np.uint16) for k in range(3)])
    res = np.stack([(1 + (xx * h + yy + 7 * k) % 11000).astype(np.uint16) for k in range(3)])
    tuning("ctc_chunk_frames", 3)
    ev = ctc.CTCEvaluator()
    ev.add_frames("SEG", dev(gt), dev(res), [0, 1, 2])
    st = ev.stats()
    print(st)
    rounds = 3
    assert st["chunks"] == 1 and st["launches"] == 2 + 2 * rounds and st["syncs"] == 1 + rounds
    same_tables(ev.frames("SEG"), stack_tables(gt, res, [0, 1, 2]))


def test_a_failed_call_adds_no_frame(ctc, tuning):
    """Frame 11 exists already: the call fails after its chunks ran, and the
    evaluator keeps none of the call's frames."""
    gt, res = small_stacks()
    tuning("ctc_chunk_frames", 2)
    ev = ctc.CTCEvaluator()
    ev.add_frames("TRA", dev(gt[1:2]), dev(res[1:2]), [11])
    with pytest.raises(RuntimeError, match="frame 11 was added twice"):
        ev.add_frames("TRA", dev(gt), dev(res), [10, 11, 12])
    assert [f["frame"] for f in ev.frames("TRA")] == [11]


def test_fixtures_through_the_device_path(ctc):
    tra = np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)
    seg = np.load(os.path.join(G, "ctc_seg01.npz"), allow_pickle=False)
    ev = ctc.CTCEvaluator()
    ev.add_frames("TRA", dev(tra["gt"]), dev(tra["res"]), tra["frames"])
    ev.set_tracks("GT", tra["gt_track"])
    ev.set_tracks("RES", tra["res_track"])
    cpu = evaluator(tra=stack_tables(tra["gt"], tra["res"], tra["frames"]), gt_rows=tra["gt_track"],
                    res_rows=tra["res_track"])
    m, c = ev.measures(), cpu.measures()
    assert m["counts"] == c["counts"] == dict(NS=5, FN=5, FP=3, ED=1, EA=16, EC=2, V_GT=25, E_GT=19)
    assert m["TRA"] == c["TRA"] and m["DET"] == c["DET"] and "%.6f" % m["TRA"] == "0.622980"
    assert ev.log() == cpu.log()
    # the SEG set has another frame size: an evaluator of its own
    es = ctc.CTCEvaluator()
    es.add_frames("SEG", dev(seg["gt"]), dev(seg["res"]), seg["frames"])
    cs = evaluator(seg=stack_tables(seg["gt"], seg["res"], seg["frames"]))
    assert es.measures()["SEG"] == cs.measures()["SEG"]
    assert es.measures()["SEG"] == ctc.seg_measure(dev(seg["gt"]), dev(seg["res"]), seg["frames"])
    with pytest.raises(RuntimeError, match="sizes differ"):
        ev.add_frames("SEG", dev(seg["gt"]), dev(seg["res"]), seg["frames"])


def test_self_evaluation_and_shift(ctc):
    """The reference's own instance masks (tests/golden/hela_postproc.npz)
    scored against themselves give 1 / 1 / 1; against a copy shifted by 3
    pixels, the SEG of the NumPy evaluation."""
    lab = np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)["labels"][:6]
    frames = np.arange(6)
    # labels are per-frame component numbers: one row per label over the frames it occurs in
    rows = []
    for l in np.unique(lab[lab > 0]):
        t = np.nonzero((lab == l).any(axis=(1, 2)))[0]
        rows.append([int(l), int(t[0]), int(t[-1]), 0])
    ev = ctc.CTCEvaluator()
    d = dev(lab)
    ev.add_frames("TRA", d, d, frames)
    ev.add_frames("SEG", d, d, frames)
    ev.set_tracks("GT", rows)
    ev.set_tracks("RES", rows)
    m = ev.measures()
    assert (m["SEG"], m["DET"], m["TRA"]) == (1.0, 1.0, 1.0)
    assert sum(m["counts"][k] for k in ("NS", "FN", "FP", "ED", "EA", "EC")) == 0 and m["counts"]["V_GT"] > 100
    shifted = np.roll(lab, 3, axis=2)
    shifted[:, :, :3] = 0
    want, _, n = seg_brute_force(lab, shifted)
    got = ctc.seg_measure(d, dev(shifted))
    print(got, want, n)
    assert abs(got - want) < 1e-12 and 0.0 < got < 1.0


def test_evaluate_sequence_reads_a_ctc_directory(ctc, tmp_path, capsys):
    from PIL import Image
    tra = np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)
    gt_dir, res_dir = tmp_path / "03_GT", tmp_path / "03_RES"
    (gt_dir / "TRA").mkdir(parents=True)
    (gt_dir / "SEG").mkdir()
    res_dir.mkdir()
    for g, r, n in zip(tra["gt"], tra["res"], tra["frames"]):
        Image.fromarray(g).save(gt_dir / "TRA" / f"man_track{n:03d}.tif")
        Image.fromarray(r).save(res_dir / f"mask{n:03d}.tif")
    Image.fromarray(tra["gt"][2]).save(gt_dir / "SEG" / "man_seg002.tif")
    for name, rows in ((gt_dir / "TRA" / "man_track.txt", tra["gt_track"]), (res_dir / "res_track.txt", tra["res_track"])):
        name.write_text("".join("%d %d %d %d\n" % tuple(r) for r in rows))
    out = ctc.evaluate_sequence(str(gt_dir), str(res_dir))
    assert "%.6f" % out["TRA"] == "0.622980" and out["DET"] == 1 - 78 / 250
    assert out["log"].rstrip().endswith("TRA measure: 0.622980")
    assert out["SEG"] == seg_brute_force(tra["gt"][2:3], tra["res"][2:3])[0]
    # the command-line tool, in this process
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ctc_measures", os.path.join(os.path.dirname(__file__), "..", "tools", "ctc_measures.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(["--gt", str(gt_dir), "--res", str(res_dir), "--log", str(tmp_path / "log.txt")]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["SEG measure: %.6f" % out["SEG"], "DET measure: 0.688000", "TRA measure: 0.622980"]
    assert (tmp_path / "log.txt").read_text() == out["log"]
    os.remove(res_dir / "mask002.tif")
    with pytest.raises(RuntimeError, match="frame 2 has no RES frame"):
        ctc.evaluate_sequence(str(gt_dir), str(res_dir))
