"""trajectories / dynamics / displacement_error on the MI355X equal the host
twin's results exactly (both derive every float from equal integers with the
same code), and tools/track_dynamics.py writes tables that parse back to them.
"""
import csv
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_region_cpu import edge_sequence, edge_tracked

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def measure():
    from unet_amd import measure as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def same(a, b):
    """Integers equal, floats bit-equal (NaN included), key by key."""
    assert list(a) == list(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), k


def test_trajectories_and_dynamics_equal_the_host_twins(measure):
    rows, masks, frames = edge_tracked()
    rng = np.random.default_rng(3)
    images = rng.integers(0, 256, masks.shape).astype(np.uint8)
    host = measure.trajectories(masks, frames, rows, images)
    got = measure.trajectories(dev(masks), frames, rows, torch.from_numpy(images).cuda())
    assert got.table.records.tobytes() == host.table.records.tobytes()
    same(got.table.columns(), host.table.columns())
    assert got.table.mean_v.tolist() == [images[f][masks[f] == t].mean() for t, f in zip(host.table.label, host.frame)]
    for k in ("frame", "tracks", "track_offsets", "frames"):
        np.testing.assert_array_equal(getattr(got, k), getattr(host, k))
    a = measure.dynamics(got, rows, frame_interval=5.0, pixel_size=0.645)
    b = measure.dynamics(host, rows, frame_interval=5.0, pixel_size=0.645)
    for name in ("tracks", "divisions", "frames"):
        same(a[name], b[name])
    assert a["divisions"]["centroid_distance"].tolist() == [15 * 0.645]


def test_displacement_error_equals_the_host_twins(measure):
    z = np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)
    host = measure.displacement_error(z["gt"], z["gt_track"], z["res"], z["res_track"], z["frames"])
    got = measure.displacement_error(dev(z["gt"]), z["gt_track"], dev(z["res"]), z["res_track"], z["frames"])
    assert (got["matched"], got["total"]) == (host["matched"], host["total"]) == (20, 25)
    assert np.float64(got["ade"]).tobytes() == np.float64(host["ade"]).tobytes()
    same(got["per_track"], host["per_track"])
    with pytest.raises(ValueError):
        measure.displacement_error(dev(z["gt"]), z["gt_track"], z["res"], z["res_track"], z["frames"])


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def parsed(columns, header, rows):
    """The CSV's columns in the dtypes of the table it was written from."""
    assert header == list(columns)
    out = {}
    for i, k in enumerate(header):
        want = np.asarray(columns[k])
        vals = [r[i] for r in rows]
        if want.dtype.kind == "f":
            out[k] = np.array([float(v) for v in vals], np.float64)
        else:
            out[k] = np.array([int(v) for v in vals], np.int64).astype(want.dtype)
    return out


def test_tool_on_a_tracked_sequence(measure, tmp_path, capsys):
    from PIL import Image
    from unet_amd import track
    from unet_amd.ctc import read_track_file
    seq = edge_sequence()
    inst = tmp_path / "inst"
    inst.mkdir()
    for f, m in enumerate(seq):
        Image.fromarray(m.astype(np.uint16)).save(inst / f"m{f:03d}.tif")
    res = tmp_path / "01_RES"
    rows = track.track_sequence(str(inst), str(tmp_path / "tracks.txt"), result_dir=str(res))
    assert rows is not None and len(rows) == 5
    # the result as its own ground truth: every object matches itself at distance 0
    tra = tmp_path / "01_GT" / "TRA"
    tra.mkdir(parents=True)
    for f in range(len(seq)):
        shutil.copy(res / f"mask{f:03d}.tif", tra / f"man_track{f:03d}.tif")
    shutil.copy(res / "res_track.txt", tra / "man_track.txt")
    out = tmp_path / "dyn"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "track_dynamics.py"), "--res", str(res), "--gt",
                        str(tmp_path / "01_GT"), "--frame-interval", "5", "--pixel-size", "0.645", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    summary = json.loads(p.stdout.strip().splitlines()[-1])
    assert summary == {"frames": 6, "objects": 7, "tracks": 5, "divisions": 1, "ade": 0.0, "ade_matched": 7,
                       "ade_total": 7}
    assert sorted(os.listdir(out)) == ["divisions.csv", "frames.csv", "objects.csv", "tracks.csv"]
    # the same tables in this process, from the files the tool read
    masks = np.stack([np.array(Image.open(res / f"mask{f:03d}.tif")) for f in range(len(seq))])
    file_rows = read_track_file(str(res / "res_track.txt"))
    traj = measure.trajectories(dev(masks), np.arange(len(seq)), file_rows)
    tables = measure.dynamics(traj, file_rows, 5.0, 0.645)
    for name in ("tracks", "divisions", "frames"):
        same(parsed(tables[name], *read_csv(out / f"{name}.csv")), {k: np.asarray(v) for k, v in tables[name].items()})
    objects = {"track": traj.table.label, "frame_number": traj.frame}
    objects.update({k: v for k, v in traj.table.columns().items() if k != "label"})
    same(parsed(objects, *read_csv(out / "objects.csv")), {k: np.asarray(v) for k, v in objects.items()})
    # a directory without masks: an error message, no traceback
    spec = importlib.util.spec_from_file_location("track_dynamics", os.path.join(ROOT, "tools", "track_dynamics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(["--res", str(inst), "--out", str(out)]) == 1
    assert "no mask*.tif" in capsys.readouterr().err
