"""Times the marker-seeded instance masks (unet_amd.postproc.split_instances) at
core_d2 = 900 on the 84 predicted 324 x 324 masks of
tests/golden/hela_postproc.npz and on the three 512 x 512 frames of
tests/golden/hela_real.npz (their ground truth binarised):

* one batched call per stack and a call of one frame, REPS repetitions after a
  warm-up, device events around each call (the wrapper's mask conversion and
  allocations included);
* unet_amd.postproc.instance_masks, the plain labelling, on the same stacks in
  the same way: the yardstick;
* the NumPy oracle of tests/split_oracle.py for the same work, once, and
  whether labels and info agree.

Prints one JSON object (profiles/split_bench.json is a run of it); --out FILE
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
import split_oracle  # noqa: E402

REPS, CORE_D2, MIN_SIZE = 50, 900, 15


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
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}, r


def workload(name, masks):
    d = torch.from_numpy(masks).cuda()
    n, h, w = masks.shape
    out = {"frames": n, "size": [h, w]}
    ms, r = timed(lambda: postproc.split_instances(d, core_d2=CORE_D2, min_size=MIN_SIZE), REPS)
    out["split_ms"] = ms
    out["split_with_d2_ms"] = timed(
        lambda: postproc.split_instances(d, core_d2=CORE_D2, min_size=MIN_SIZE, return_distance=True), REPS)[0]
    out["instance_masks_ms"] = timed(lambda: postproc.instance_masks(d, MIN_SIZE), REPS)[0]
    out["split_over_instance_masks"] = ms["median"] / out["instance_masks_ms"]["median"]
    out["split_ms_per_frame"] = ms["median"] / n
    one, _ = timed(lambda: postproc.split_instances(d[0], core_d2=CORE_D2, min_size=MIN_SIZE), REPS)
    out["one_frame_split_ms"] = one
    out["one_frame_instance_masks_ms"] = timed(lambda: postproc.instance_masks(d[0], MIN_SIZE), REPS)[0]
    info = r.info.cpu().numpy()
    out["markers"] = int(info[:, 0].sum())
    out["segments"] = int(info[:, 1].sum())
    out["components"] = int(sum(int(x.max()) for x in postproc.instance_masks(d, 0).cpu().numpy()))
    out["levels"] = {"min": int(info[:, 2].min()), "max": int(info[:, 2].max())}
    t0 = time.perf_counter()
    want = split_oracle.split_stack(masks, CORE_D2, min_size=MIN_SIZE)
    out["numpy_oracle_ms"] = (time.perf_counter() - t0) * 1e3
    out["equal_to_oracle"] = bool(np.array_equal(r.labels.cpu().numpy(), want["labels"]) and
                                  np.array_equal(info, want["info"]))
    return out


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hela_postproc.npz"), allow_pickle=False)
    w = int(z["mask_shape"][2])
    golden = (np.unpackbits(z["mask_bits"], axis=-1)[..., :w] * 255).astype(np.uint8)
    real = (np.load(os.path.join(ROOT, "tests", "golden", "hela_real.npz"), allow_pickle=False)["segs"] > 0)
    out = {"core_d2": CORE_D2, "min_size": MIN_SIZE, "reps": REPS,
           "golden_84x324": workload("golden", golden), "hela_3x512": workload("hela", real.astype(np.uint8) * 255)}
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
