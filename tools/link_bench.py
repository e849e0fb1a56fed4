"""Times the distance-based linker (unet_link_frames, unet_amd.link) on

* the 84 instance labelings of tests/golden/hela_postproc.npz (324 x 324, about
  136 objects per frame: every frame pair is served from LDS), gate 20, and
* a synthetic dense scene: DENSE_FRAMES frames of 324 x 324 with about 2,000
  single-pixel objects each that jitter by up to 2 pixels from frame to frame,
  gate 5 -- P + C is about 4,000, above what the LDS holds, so every pair runs
  from the workspace.

Per workload:
  link_kernel          unet_link_frames alone on resident records (one launch)
  link_kernel_forced_global   the same with link_lds_objects = 0
  region_props_call    unet_region_props alone on the resident stack (its own
                       host synchronisation included)
  python_link_stack    unet_amd.link.link_stack: region records, the link
                       launch, the copies to the host, the host assembly
  host_twin_ms         unet_link_frames_host on the same table, once
  host_assemble_ms     unet_link_assemble, once
  scipy_oracle_ms      tests/link_oracle.link (scipy's assignment per pair,
                       without the uniqueness check) on the same table, once
The device variants are timed in alternating windows of LOOP calls between two
device events, WINDOWS windows each, after a warm-up window; the figure is the
median window.  The kernel is bound by barrier latency (two barriers per search
iteration), so no bandwidth or FLOP fraction is given.

Prints one JSON object; --out FILE also writes it (profiles/link_bench.json is
a run of it)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from unet_amd import _lib, link, measure  # noqa: E402
import link_oracle as LO  # noqa: E402

LOOP, SLOW_LOOP, WINDOWS, DENSE_FRAMES, DENSE_OBJECTS = 50, 5, 5, 4, 2000


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


def dense_scene(frames=DENSE_FRAMES, objects=DENSE_OBJECTS, size=324, seed=3):
    rng = np.random.default_rng(seed)
    at = rng.choice(size * size, objects, replace=False)
    y, x = at // size, at % size
    out = np.zeros((frames, size, size), np.uint16)
    for f in range(frames):
        order = rng.permutation(objects)
        for k, i in enumerate(order):          # a pixel already taken: the object is missing from this frame
            if out[f, y[i], x[i]] == 0:
                out[f, y[i], x[i]] = k + 1
        y = np.clip(y + rng.integers(-2, 3, objects), 0, size - 1)
        x = np.clip(x + rng.integers(-2, 3, objects), 0, size - 1)
    return out


def workload(labels, gate, loop):
    lib = _lib.load()
    n, h, w = labels.shape
    d16 = torch.from_numpy(labels.astype(np.uint16).view(np.int16)).cuda().view(torch.uint16)
    table, rec, off = measure.region_props(d16, keep_device=True)
    total = len(table)
    gq = link.gate_q(gate)
    prev = torch.empty(total, dtype=torch.int32, device="cuda")
    mother = torch.empty(total, dtype=torch.int32, device="cuda")
    dist = torch.empty(total, dtype=torch.int64, device="cuda")
    pair_total = torch.empty(n - 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.unet_link_ws_bytes(n, total), dtype=torch.uint8, device="cuda")
    stream = _lib.stream_of(d16.device)
    rws = torch.empty(lib.unet_region_props_ws_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    got = ctypes.c_longlong(0)

    def kernel(lds=-1):
        lib.unet_set_tuning(b"link_lds_objects", lds)
        rc = lib.unet_link_frames(rec.data_ptr(), off.data_ptr(), n, total, gq, 0, prev.data_ptr(), dist.data_ptr(),
                                  mother.data_ptr(), pair_total.data_ptr(), ws.data_ptr(), stream)
        lib.unet_set_tuning(b"link_lds_objects", -1)
        return rc

    def props():
        return lib.unet_region_props(d16.data_ptr(), None, n, h, w, off.data_ptr(), rec.data_ptr(), rec.shape[0],
                                     ctypes.byref(got), rws.data_ptr(), stream)

    variants = {"link_kernel": kernel, "link_kernel_forced_global": lambda: kernel(0), "region_props_call": props,
                "python_link_stack": lambda: link.link_stack(d16, gate=gate)}
    # the results first
    assert kernel() == 0
    dev = [v.cpu().numpy() for v in (prev, dist, mother, pair_total)]
    assert kernel(0) == 0
    same_paths = all(np.array_equal(a, v.cpu().numpy()) for a, v in zip(dev, (prev, dist, mother, pair_total)))
    t0 = time.perf_counter()
    host = link.link_table_host(table, gate)
    host_ms = (time.perf_counter() - t0) * 1e3
    res = link.link_stack(d16, gate=gate)
    t0 = time.perf_counter()
    link._assemble(lib, table, np.arange(n, dtype=np.int32), host[0], host[1], host[2], host[3], 0.5, 2, None)
    assemble_ms = (time.perf_counter() - t0) * 1e3
    cols = {k: np.asarray(getattr(table, k), np.int64) for k in ("area", "sum_y", "sum_x")}
    t0 = time.perf_counter()
    want = LO.link(table.frame_offsets, cols, gate, unique_pairs=())
    scipy_ms = (time.perf_counter() - t0) * 1e3
    per_frame = np.diff(table.frame_offsets)
    for k, fn in variants.items():     # warm-up
        window(fn, loop)
    times = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, fn in variants.items():
            times[k].append(window(fn, loop))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"frames": n, "size": [h, w], "objects": total, "objects_per_frame": [int(per_frame.min()), int(per_frame.max())],
            "gate": gate, "loop": loop, "links": int((dev[0] >= 0).sum()), "tracks": len(res.rows),
            "device_equals_host_twin": bool(all(np.array_equal(a, b) for a, b in zip(dev, host))),
            "lds_and_global_paths_equal": bool(same_paths),
            "pair_total_equals_scipy": bool(np.array_equal(dev[3], want["pair_total"])),
            "links_equal_scipy": bool(np.array_equal(dev[0], want["prev"])),
            "ms": {k: spread(v) for k, v in times.items()}, "host_twin_ms": host_ms, "host_assemble_ms": assemble_ms,
            "scipy_oracle_ms": scipy_ms,
            "kernel_share_of_link_stack": med["link_kernel"] / med["python_link_stack"],
            "region_props_share_of_link_stack": med["region_props_call"] / med["python_link_stack"]}


def main():
    if not torch.cuda.is_available():
        sys.exit("link_bench: no HIP device")
    labels = np.load(os.path.join(ROOT, "tests", "golden", "hela_postproc.npz"), allow_pickle=False)["labels"]
    out = {"windows": WINDOWS, "hela_84x324": workload(labels, 20.0, LOOP),
           "dense_4x324_2000": workload(dense_scene(), 5.0, SLOW_LOOP)}
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
