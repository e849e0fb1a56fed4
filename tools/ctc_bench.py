"""Times the Cell Tracking Challenge evaluator on a synthetic 84-frame 512x512
sequence of moving discs (RES = GT shifted by (1.5, -1) pixels, shrunk by one):

* the device part (CTCEvaluator.add_frames of both stacks, as SEG and as TRA
  frames) with the stacks resident as uint16, at three chunk sizes, for 120
  discs per frame (121 x 121 cells: the hash path) and for 20 (the dense path).
  A timed window is a loop of LOOP evaluations, long enough to stand above the
  clock and the scheduler; WINDOWS windows after a warm-up one, host clock around
  calls that end in a stream synchronisation;
* unet_amd.ctc.evaluate_sequence as a whole on the 120-disc sequence written
  out as TIFF files (8 calls, the first dropped), with the share spent in
  add_frames;
* the NumPy brute force of tests/test_ctc_cpu.py (SEG only) on the same frames.

Prints one JSON object (profiles/ctc_bench.json is a run of it); --out FILE
also writes it there."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from unet_amd import _lib, ctc  # noqa: E402
from test_ctc_cpu import seg_brute_force  # noqa: E402

T, H, W = 84, 512, 512
LOOP, WINDOWS = 50, 5


def sequence(n, seed=3):
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(20, H - 20, n), rng.uniform(20, W - 20, n)
    vy, vx = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    rad = rng.uniform(6, 14, n)
    yy, xx = np.mgrid[:H, :W]

    def render(t, dy, dx, shrink):
        img = np.zeros((H, W), np.uint16)
        for k in range(n):
            y, x = cy[k] + vy[k] * t + dy, cx[k] + vx[k] * t + dx
            y0, y1, x0, x1 = max(int(y) - 16, 0), min(int(y) + 17, H), max(int(x) - 16, 0), min(int(x) + 17, W)
            if y0 >= y1 or x0 >= x1:
                continue
            win = img[y0:y1, x0:x1]
            win[(yy[y0:y1, x0:x1] - y) ** 2 + (xx[y0:y1, x0:x1] - x) ** 2 <= (rad[k] - shrink) ** 2] = k + 1
        return img
    return (np.stack([render(t, 0.0, 0.0, 0.0) for t in range(T)]),
            np.stack([render(t, 1.5, -1.0, 1.0) for t in range(T)]))


def track_rows(stack):
    out = []
    for l in np.unique(stack[stack > 0]):
        tt = np.nonzero((stack == l).any(axis=(1, 2)))[0]
        out.append(f"{l} {tt[0]} {tt[-1]} 0\n")
    return "".join(out)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def resident(gt, res, chunk):
    """seconds per evaluation (both stacks as SEG and TRA frames), per window"""
    lib = _lib.load()
    lib.unet_set_tuning(b"ctc_chunk_frames", chunk)
    g = torch.from_numpy(gt.astype(np.int32)).cuda().to(torch.int16).view(torch.uint16)
    s = torch.from_numpy(res.astype(np.int32)).cuda().to(torch.int16).view(torch.uint16)
    per = []
    for w in range(WINDOWS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(LOOP):
            ev = ctc.CTCEvaluator()
            ev.add_frames("SEG", g, s, range(T))
            ev.add_frames("TRA", g, s, range(T))  # ends in a stream synchronisation
        per.append((time.perf_counter() - t0) / LOOP)
    lib.unet_set_tuning(b"ctc_chunk_frames", -1)
    return {"s_per_evaluation": spread(per[1:]), "window_s": per[1] * LOOP, "stats_one_evaluation": ev.stats(),
            "ws_bytes": int(ev.ws.numel())}


def main():
    out = {"frames": T, "size": [H, W], "loop": LOOP, "windows": WINDOWS, "resident": {}}
    gt, res = sequence(120)
    for name, (a, b) in (("120_discs", (gt, res)), ("20_discs", sequence(20, seed=4))):
        out["resident"][name] = {str(c): resident(a, b, c) for c in (8, 32, 84)}

    with tempfile.TemporaryDirectory() as d:
        gd, rd = os.path.join(d, "01_GT"), os.path.join(d, "01_RES")
        os.makedirs(os.path.join(gd, "SEG"))
        os.makedirs(os.path.join(gd, "TRA"))
        os.makedirs(rd)
        for t in range(T):
            Image.fromarray(gt[t]).save(os.path.join(gd, "SEG", f"man_seg{t:03d}.tif"))
            Image.fromarray(gt[t]).save(os.path.join(gd, "TRA", f"man_track{t:03d}.tif"))
            Image.fromarray(res[t]).save(os.path.join(rd, f"mask{t:03d}.tif"))
        with open(os.path.join(gd, "TRA", "man_track.txt"), "w") as f:
            f.write(track_rows(gt))
        with open(os.path.join(rd, "res_track.txt"), "w") as f:
            f.write(track_rows(res))
        # the share of add_frames (device part; it ends in a stream synchronisation)
        spent = [0.0]
        inner = ctc.CTCEvaluator.add_frames

        def timed(self, *a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inner(self, *a, **k)
            spent[0] += time.perf_counter() - t0
        ctc.CTCEvaluator.add_frames = timed
        tot, dev = [], []
        for i in range(8):
            spent[0] = 0.0
            t0 = time.perf_counter()
            r = ctc.evaluate_sequence(gd, rd)
            tot.append(time.perf_counter() - t0)
            dev.append(spent[0])
        ctc.CTCEvaluator.add_frames = inner
    out["evaluate_sequence"] = {"measures": {k: r[k] for k in ("SEG", "DET", "TRA")}, "total_s": spread(tot[1:]),
                                "add_frames_s": spread(dev[1:]), "first_call_s": tot[0]}
    t0 = time.perf_counter()
    want = seg_brute_force(gt, res)
    out["numpy_brute_force_seg_s"] = time.perf_counter() - t0
    out["seg_equal_to_1e-12"] = abs(want[0] - r["SEG"]) < 1e-12
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
