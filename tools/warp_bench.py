"""Times the warping error (unet_amd.postproc.warping_error) on the 84 frames of
tests/golden/hela_postproc.npz: frame t's committed instance labelling warped
onto frame t + 1's predicted mask (the last onto the first), radius 4, with the
background ridge between touching cells:

* one batched call (84 workgroups, the planes in LDS), REPS repetitions after a
  warm-up, device events around each call; the same through the workspace
  planes; and a call of one frame;
* the NumPy oracle of tests/warp_oracle.py for the same work, once, and whether
  the counts agree;
* the worst case for the sweep loop: a one-pixel serpentine at 512 x 512
  against a single-pixel prediction with no mask (tens of thousands of sweeps
  of a flip or two), SERP_REPS repetitions.

Prints one JSON object (profiles/warp_bench.json is a run of it); --out FILE
also writes it there."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from unet_amd import postproc  # noqa: E402
import warp_oracle  # noqa: E402

REPS, SERP_REPS = 50, 5


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def timed(fn, reps):
    """milliseconds per call by device events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return spread(out), r


def serpentine(h, w):
    m = np.zeros((h, w), np.uint16)
    for y in range(0, h, 4):
        m[y, :] = 1
        if y + 3 < h:
            m[y + 1:y + 4, (w - 1) if (y // 4) % 2 == 0 else 0] = 1
    return m


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hela_postproc.npz"), allow_pickle=False)
    t, h, w = (int(v) for v in z["mask_shape"])
    masks = (np.unpackbits(z["mask_bits"], axis=-1)[..., :w] * 255).astype(np.uint8)
    gt = z["labels"].astype(np.uint16)
    pred = np.roll(masks, -1, axis=0)
    g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    out = {"frames": t, "size": [h, w], "radius": 4, "separate": True, "reps": REPS}

    ms, r = timed(lambda: postproc.warping_error(g, p, radius=4), REPS)
    counts = r.counts.cpu().numpy()
    out["batched_lds_ms"] = ms
    out["batched_workspace_ms"] = timed(lambda: postproc.warping_error(g, p, radius=4, flags=postproc.FORCE_WS),
                                        REPS)[0]
    out["one_frame_lds_ms"] = timed(lambda: postproc.warping_error(g[0], p[0], radius=4), REPS)[0]
    out["sweeps"] = {"min": int(counts[:, 3].min()), "max": int(counts[:, 3].max())}
    out["flips_mean"] = float(counts[:, 2].mean())
    out["pixel_error_mean"] = float(counts[:, 0].mean() / (h * w))
    out["warping_error_mean"] = float(counts[:, 1].mean() / (h * w))

    t0 = time.perf_counter()
    want = warp_oracle.evaluate_stack(gt, pred, radius=4, separate=True)[0]
    out["numpy_oracle_ms"] = (time.perf_counter() - t0) * 1e3
    out["counts_equal_to_oracle"] = bool(np.array_equal(counts, want))

    sg = torch.from_numpy(serpentine(512, 512)).cuda()
    sp = torch.zeros((512, 512), dtype=torch.uint8, device="cuda")
    sp[0, 0] = 1
    ms, r = timed(lambda: postproc.warping_error(sg, sp, radius=-1, separate=False), SERP_REPS)
    c = r.counts.tolist()
    out["serpentine_512"] = {"reps": SERP_REPS, "lds_ms": ms, "pixel_error": c[0], "warping_error": c[1], "flips": c[2],
                             "sweeps": c[3], "converged": c[4]}
    out["serpentine_512"]["workspace_ms"] = timed(
        lambda: postproc.warping_error(sg, sp, radius=-1, separate=False, flags=postproc.FORCE_WS), 2)[0]
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
