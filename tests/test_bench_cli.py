"""bench.py's command line: a plain run prints the contract line and nothing
that belongs to ``--full``; ``--dump-outputs`` writes the last timed step's
arrays as float32 .npy within 64 MB; two runs that execute the same number of
steps write identical arrays.

Both runs use the smallest valid U-Net input at batch 2 (the process start
dominates their time).  profiles/tune_db.txt holds no choices for that shape,
so the first run tunes it live and saves its choices, and the second replays
them: the deterministic mode fixes the summation order of a kernel, not which
kernel a timing picks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FILES = ["bn_running_stats.npy", "logits.npy", "loss.npy", "params.npy"]


def run_bench(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "188", "--batch", "2", *extra]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = tmp_path_factory.mktemp("bench_a")
    line = run_bench(d, "--steps", "3", "--warmup", "1", "--dump-outputs", "out", "--tune-db-out", "tune.db")
    return d, line


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(first_run):
    d, line = first_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "fp32" and line["unit"] == "images/s"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert line["lib"]["deterministic"] is True  # the headline leg: no fp32 atomics
    assert line["value"] == pytest.approx(2 / (line["ms_per_step"] * 1e-3), rel=1e-3)  # batch 2 on one GPU
    # what --full adds stays out of a plain run, and it leaves no file behind but what was asked for
    for k in ("roofline", "bottleneck", "stage1", "bf16", "c5", "farm", "iou", "cpu_baseline", "peaks", "detail"):
        assert k not in line
    assert sorted(os.listdir(d)) == ["out", "tune.db"]
    assert sorted(os.listdir(d / "out")) == FILES
    arrays = {f[:-4]: np.load(d / "out" / f, allow_pickle=False) for f in FILES}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        assert list(a.shape) == line["outputs"]["arrays"][name]
    assert arrays["logits"].shape == (2, 2, 4, 4) and arrays["loss"].shape == ()
    # 31 M parameters: written as the fixed sample
    assert arrays["params"].shape == (1 << 22,) and np.abs(arrays["params"]).max() > 0


@pytest.mark.gpu
def test_same_number_of_steps_writes_identical_outputs(first_run, tmp_path):
    """2 warm-up + 2 timed steps leave what 1 + 3 left, bit for bit: the inputs
    are the same every run, --warmup and --steps set how many steps run, and the
    arrays are those of the last one."""
    d, _ = first_run
    line = run_bench(tmp_path, "--steps", "2", "--warmup", "2", "--dump-outputs", "out",
                     "--tune-db", str(d / "tune.db"))
    assert line["steps"] == 2 and line["warmup"] == 2
    for f in FILES:
        np.testing.assert_array_equal(np.load(tmp_path / "out" / f), np.load(d / "out" / f), err_msg=f)


@pytest.mark.gpu
def test_steps_sets_the_number_of_timed_steps(first_run, tmp_path):
    """One timed step fewer after the same warm-up leaves other parameters
    (every step moves them), where the same total left identical ones above."""
    d, _ = first_run
    line = run_bench(tmp_path, "--steps", "2", "--warmup", "1", "--dump-outputs", "out",
                     "--tune-db", str(d / "tune.db"))
    assert line["steps"] == 2 and line["warmup"] == 1
    assert not np.array_equal(np.load(tmp_path / "out" / "params.npy"), np.load(d / "out" / "params.npy"))
    assert not np.array_equal(np.load(tmp_path / "out" / "loss.npy"), np.load(d / "out" / "loss.npy"))
