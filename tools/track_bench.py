"""Times the track-labelled result masks (unet_amd.track) on the 84 instance
labelings of tests/golden/hela_postproc.npz (324 x 324) and on the same stack
zero-padded to 512 x 512:

* Tracker.relabel alone (table upload, one stream synchronisation, one kernel);
* track_stack (84 add_frame steps + relabel);
* the same relabelling as a torch gather on the device,
  lut[frame_index, labels.long()] with the (84, L) table already resident;
* NumPy on the host (tests/track_map_oracle.relabel), once.

relabel and the torch expression are timed in alternating windows of LOOP calls
between two device events, WINDOWS windows each, after a warm-up window; the
rate is the 4 bytes per pixel the relabelling must move (2 read, 2 written)
over the time per call, beside the 6.29 TB/s a float4 copy reaches on this GPU.

Prints one JSON object; --out FILE also writes it
(profiles/track_relabel_bench.json is a run of it)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from unet_amd import track  # noqa: E402
import track_map_oracle as M  # noqa: E402

LOOP, WINDOWS, COPY_TBS = 50, 5, 6.29


def window(fn, loop):
    """milliseconds per call: loop calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(loop):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / loop


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def workload(labels, frames):
    n, h, w = labels.shape
    d32 = torch.from_numpy(labels.astype(np.int32)).cuda()
    d16 = torch.from_numpy(labels.astype(np.uint16).view(np.int16)).cuda().view(torch.uint16)
    tr = track.Tracker(h, w)
    for i in range(n):
        tr.add_frame(d16[i], int(frames[i]))
    maps = [dict(zip(*(a.tolist() for a in tr.frame_map(i)[1:]))) for i in range(n)]
    top = max(max(m) for m in maps if m)
    lut = np.zeros((n, top + 1), np.uint16)
    for i, m in enumerate(maps):
        for lab, tid in m.items():
            lut[i, lab] = tid
    lut_d = torch.from_numpy(lut.view(np.int16)).cuda()
    fidx = torch.arange(n, device="cuda").view(n, 1, 1)
    out = torch.empty_like(d16)

    def ours():
        return tr.relabel(d16, frames, out=out)

    def gather():
        return lut_d[fidx, d32.long()]

    want = M.relabel(labels, maps)
    equal = bool(np.array_equal(ours().cpu().view(torch.int16).numpy().view(np.uint16), want) and
                 np.array_equal(gather().cpu().numpy().view(np.uint16), want))
    window(ours, LOOP), window(gather, LOOP)  # warm-up
    t_ours, t_gather = [], []
    for _ in range(WINDOWS):
        t_ours.append(window(ours, LOOP))
        t_gather.append(window(gather, LOOP))
    stack_ms = [window(lambda: track.track_stack(d16, frames), 2) for _ in range(3)]
    t0 = time.perf_counter()
    M.relabel(labels, maps)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    moved = 4 * n * h * w
    r = {"frames": n, "size": [h, w], "highest_label": int(top), "bytes_moved": moved,
         "relabel_ms": spread(t_ours), "torch_gather_ms": spread(t_gather),
         "relabel_over_torch_gather": statistics.median(t_ours) / statistics.median(t_gather),
         "relabel_TB_per_s": moved / (statistics.median(t_ours) * 1e-3) / 1e12,
         "torch_gather_TB_per_s": moved / (statistics.median(t_gather) * 1e-3) / 1e12,
         "ms_at_copy_rate": moved / (COPY_TBS * 1e12) * 1e3,
         "track_stack_ms": spread(stack_ms), "numpy_relabel_ms": numpy_ms, "equal_to_numpy": equal}
    return r


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hela_postproc.npz"), allow_pickle=False)
    labels, frames = z["labels"], [int(f) for f in z["frames"]]
    n, h, w = labels.shape
    padded = np.zeros((n, 512, 512), labels.dtype)
    padded[:, :h, :w] = labels
    out = {"loop": LOOP, "windows": WINDOWS, "copy_rate_TB_per_s": COPY_TBS,
           "torch_gather": "lut[frame_index, labels.long()]: int16 (n, L) table and int32 labels resident on the device",
           "hela_84x324": workload(labels, frames), "hela_84x512_padded": workload(padded, frames)}
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
