"""Times the per-object measurements (unet_region_props) on the 84 instance
labelings of tests/golden/hela_postproc.npz (324 x 324) and on the same stack
zero-padded to 512 x 512:

* one unet_region_props call on resident buffers, without and with an image
  stack (index phase, one host synchronisation, record set-up, one accumulate
  launch), and the same call with cap 0, which returns after the
  synchronisation: the share of the call spent before the accumulate phase;
* unet_amd.measure.region_props (the call plus its allocations and the copy of
  the records to the host);
* a torch baseline on the same GPU that computes a fifth of the fields -- area,
  sum y, sum x and the extent -- with index_add_ / scatter_reduce_ over
  frame * 65536 + label keys, its int64 keys and coordinates already resident,
  over every pixel and over the foreground pixels only (selected beforehand);
* the NumPy oracle (tests/region_oracle.vectorised), once.

The device variants are timed in alternating windows of LOOP calls (SLOW_LOOP
for the torch baseline, whose calls take tens of milliseconds) between two
device events, WINDOWS windows each, after a warm-up window.  bytes_read is the
2 (labels) or 3 (with image) bytes per pixel the measurement must read, beside
the time those bytes take at the 6.29 TB/s a float4 copy reaches on this GPU.

Prints one JSON object; --out FILE also writes it
(profiles/region_bench.json is a run of it)."""
import ctypes
import errno
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from unet_amd import _lib, measure  # noqa: E402
import region_oracle as O  # noqa: E402

LOOP, SLOW_LOOP, WINDOWS, COPY_TBS = 200, 3, 5, 6.29


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


def workload(labels):
    lib = _lib.load()
    n, h, w = labels.shape
    d16 = torch.from_numpy(labels.astype(np.uint16).view(np.int16)).cuda().view(torch.uint16)
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, labels.shape).astype(np.uint8)).cuda()
    t0 = time.perf_counter()
    want = O.vectorised(labels)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    total = len(want[1]["frame"])
    ws = torch.empty(lib.unet_region_props_ws_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    rec = torch.empty((total, 128), dtype=torch.uint8, device="cuda")
    got = ctypes.c_longlong(0)
    stream = _lib.stream_of(d16.device)

    def call(image=None, cap=total):
        return lib.unet_region_props(d16.data_ptr(), image, n, h, w, off.data_ptr(), rec.data_ptr(), cap,
                                     ctypes.byref(got), ws.data_ptr(), stream)

    variants = {"call": lambda: call(), "call_with_image": lambda: call(img.data_ptr()),
                "index_phase_and_sync": lambda: call(cap=0), "python_region_props": lambda: measure.region_props(d16)}
    # torch baseline: area, sum y, sum x, extent
    key = (torch.arange(n, device="cuda").view(n, 1, 1) * 65536 + torch.from_numpy(labels.astype(np.int64)).cuda()).view(-1)
    yy = torch.arange(h, device="cuda").view(1, h, 1).expand(n, h, w).reshape(-1).contiguous()
    xx = torch.arange(w, device="cuda").view(1, 1, w).expand(n, h, w).reshape(-1).contiguous()
    ones = torch.ones_like(key)

    def baseline(key=key, yy=yy, xx=xx, ones=ones):
        m = n * 65536
        area = torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, key, ones)
        sy = torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, key, yy)
        sx = torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, key, xx)
        lo_y = torch.full((m,), h, dtype=torch.int64, device="cuda").scatter_reduce_(0, key, yy, "amin")
        lo_x = torch.full((m,), w, dtype=torch.int64, device="cuda").scatter_reduce_(0, key, xx, "amin")
        hi_y = torch.full((m,), -1, dtype=torch.int64, device="cuda").scatter_reduce_(0, key, yy, "amax")
        hi_x = torch.full((m,), -1, dtype=torch.int64, device="cuda").scatter_reduce_(0, key, xx, "amax")
        return area, sy, sx, lo_y, lo_x, hi_y, hi_x

    variants["torch_baseline"] = baseline
    # the same over the foreground pixels only, selected beforehand: without the
    # background keys, one address per frame that most pixels add to
    fg = key % 65536 != 0
    kf, yf, xf, of = key[fg], yy[fg], xx[fg], ones[fg]
    variants["torch_baseline_foreground"] = lambda: baseline(kf, yf, xf, of)
    # the results first
    assert call() == 0 and got.value == total
    table = measure.RegionTable(rec.cpu().numpy().reshape(-1).view(measure.RECORD), off.cpu().numpy(), labels.shape, False)
    equal = bool(np.array_equal(table.frame_offsets, want[0]) and
                 all(np.array_equal(getattr(table, k), want[1][k]) for k in O.FIELDS))
    assert call(cap=0) == -errno.ENOSPC
    sel = (want[1]["frame"] * 65536 + want[1]["label"])
    b = [v.cpu().numpy()[sel] for v in baseline()]
    base_equal = bool(all(np.array_equal(x, want[1][k]) for x, k in
                          zip(b, ("area", "sum_y", "sum_x", "min_y", "min_x", "max_y", "max_x"))))
    loops = {k: SLOW_LOOP if k.startswith("torch_baseline") else LOOP for k in variants}
    for k, fn in variants.items():     # warm-up
        window(fn, loops[k])
    times = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, fn in variants.items():
            times[k].append(window(fn, loops[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    px = n * h * w
    return {"frames": n, "size": [h, w], "objects": total, "equal_to_numpy": equal, "torch_baseline_equal": base_equal,
            "ms": {k: spread(v) for k, v in times.items()}, "numpy_oracle_ms": numpy_ms,
            "bytes_read": {"labels": 2 * px, "labels_and_image": 3 * px},
            "ms_at_copy_rate": {"labels": 2 * px / (COPY_TBS * 1e12) * 1e3, "labels_and_image": 3 * px / (COPY_TBS * 1e12) * 1e3},
            "share_before_accumulate": med["index_phase_and_sync"] / med["call"],
            "call_over_torch_baseline": med["call"] / med["torch_baseline"],
            "call_over_torch_baseline_foreground": med["call"] / med["torch_baseline_foreground"]}


def main():
    if not torch.cuda.is_available():
        sys.exit("region_bench: no HIP device")
    labels = np.load(os.path.join(ROOT, "tests", "golden", "hela_postproc.npz"), allow_pickle=False)["labels"]
    n, h, w = labels.shape
    padded = np.zeros((n, 512, 512), labels.dtype)
    padded[:, :h, :w] = labels
    out = {"loop": LOOP, "torch_baseline_loop": SLOW_LOOP, "windows": WINDOWS, "copy_rate_TB_per_s": COPY_TBS,
           "torch_baseline": "area, sum y, sum x by index_add_, extent by scatter_reduce_ amin / amax over "
                             "frame * 65536 + label; int64 keys and coordinates resident",
           "hela_84x324": workload(labels), "hela_84x512_padded": workload(padded)}
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
