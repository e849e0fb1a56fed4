"""Times sequence inference (unet_amd.predict) on 84 synthetic uint8 frames of
512 x 512, tile_in 512 (4 tiles a frame), batch 8, in fp32 and bf16:

* frames/s of SequencePredictor with "none", "rot4" and "d4" against the
  per-frame path it replaces, a loop of TileFarm([0], 512, 4).predict(frame,
  return_mask=True) over the same frames (float frames on the host, mask back
  through the host).  The four legs run in A B A B order in one process,
  ROUNDS rounds after a warm-up round, host clock around work that ends in a
  device synchronisation;
* each new kernel alone, per symmetry code, hipEvents around LAUNCHES launches:
  at the workload's launch (8 groups, one symmetry), at the "d4" launch (1
  group, 8 symmetries) and at 64 groups (buffers beyond the caches), with the
  bytes the launch has to move (each input element once, each output element
  once) and the float4 copy ceiling of unet_peak_probe on the same GPU;
* the share of a "d4" prediction spent outside the network forwards: the
  prediction's time against the same forwards alone on the same batches.

Prints one JSON object (profiles/predict_bench.json is a run of it); --out FILE
also writes it there."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unet-segmentation_amd")]
import torch  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from unet_amd import UNet, _lib  # noqa: E402
from unet_amd.predict import SYMMETRY_SETS, SequencePredictor  # noqa: E402
from unet_amd.tiling import TileFarm, TileGeometry  # noqa: E402

T, H, W, TILE, BATCH = 84, 512, 512, 512, 8
ROUNDS, LAUNCHES = 2, 50


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def end_to_end(model, frames_u8, precision):
    model.precision = precision
    dev = frames_u8.cuda()
    host = ((frames_u8.float() / 255) - 0.5) / 0.5  # what the per-frame path is given
    farm = TileFarm(model, devices=[0], tile_in=TILE, batch=4)
    legs = {"farm_loop": lambda: [farm.predict(host[f], return_mask=True) for f in range(T)]}
    preds = {}
    for name in ("none", "rot4", "d4"):
        preds[name] = SequencePredictor(model, tile_in=TILE, batch=BATCH, symmetries=name)
        legs[name] = (lambda p: lambda: p.predict(dev, want=("mask",)))(preds[name])
    times = {k: [] for k in legs}
    for r in range(ROUNDS + 1):  # round 0 warms every shape up
        for k, fn in legs.items():
            t = timed(fn)
            if r:
                times[k].append(t)
    out = {k: {"seconds": spread(v), "frames_per_s": T / statistics.median(v)} for k, v in times.items()}
    base = statistics.median(times["farm_loop"])
    for k in ("none", "rot4", "d4"):
        out[k]["time_over_farm_loop"] = statistics.median(times[k]) / base
    out["d4"]["time_over_none"] = statistics.median(times["d4"]) / statistics.median(times["none"])
    # same masks (other batch sizes run other GEMM shapes: equal up to pixels at the threshold)
    got = preds["none"].predict(dev)["mask"][:4].cpu()
    ref = torch.stack([farm.predict(host[f], return_mask=True) for f in range(4)])
    out["none_mask_agreement_with_farm_loop"] = float((got == ref).float().mean())
    # the d4 forwards alone, on the batches the prediction ran
    p = preds["d4"]
    tiles = torch.randn((BATCH, 1, TILE, TILE), device="cuda")
    n_fwd = T * len(TileGeometry(H, W, TILE))

    def forwards():
        with torch.no_grad():
            for _ in range(n_fwd):
                p.model(tiles)
    timed(forwards)
    fw = [timed(forwards) for _ in range(ROUNDS)]
    d4 = statistics.median(times["d4"])
    out["d4_outside_forwards"] = {"forwards_s": spread(fw), "predict_s": d4,
                                  "share": 1.0 - statistics.median(fw) / d4}
    return out


def event_time(fn):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / LAUNCHES


def kernels(copy_gbs):
    lib = _lib.load()
    geo = TileGeometry(H, W, TILE)
    to, K = geo.tile_out, 2
    st = _lib.stream_of()
    out = {"copy_ceiling_gbs": copy_gbs, "gather": {}, "reduce": {}}

    def codes_c(codes):
        return (ctypes.c_int32 * len(codes))(*codes)

    for label, G, sets in (("8_groups_1_symmetry", 8, [(s,) for s in range(8)]),
                           ("1_group_d4", 1, [SYMMETRY_SETS["d4"]]),
                           ("64_groups_1_symmetry", 64, [(s,) for s in range(8)])):
        F = -(-G // len(geo))
        frames = torch.randint(0, 256, (F, 1, H, W), dtype=torch.uint8, device="cuda")
        work = torch.tensor([(g // len(geo), g % len(geo)) for g in range(G)], dtype=torch.int32, device="cuda")
        for codes in sets:
            ns = len(codes)
            tiles = torch.empty((G * ns, 1, TILE, TILE), device="cuda")
            lt = torch.randn((G * ns, K, to, to), device="cuda")
            prob = torch.empty((F, K, H, W), device="cuda")
            mask = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
            cc = codes_c(codes)
            key = "s" + "".join(map(str, codes))

            def gather():
                _lib.check(lib.unet_seq_tile_gather(frames.data_ptr(), 1, F, 1, H, W, TILE, to, geo.pads[0],
                                                    geo.pads[2], geo.nx, work.data_ptr(), G, cc, ns, tiles.data_ptr(),
                                                    st), "gather")

            def reduce():
                _lib.check(lib.unet_seq_tile_reduce(lt.data_ptr(), K, to, geo.nx, work.data_ptr(), G, cc, ns, F, H, W,
                                                    0.3, prob.data_ptr(), mask.data_ptr(), None, st), "reduce")

            # pixels of a group's output tile that lie inside the frame
            inside = sum(min(to, H - y) * min(to, W - x) for (y, x) in (geo.origins[g % len(geo)] for g in range(G)))
            for name, fn, nbytes in (("gather", gather, G * TILE * TILE * (1 + 4 * ns)),
                                     ("reduce", reduce, G * ns * K * to * to * 4 + inside * (4 * K + 1))):
                t = event_time(fn)
                out[name].setdefault(label, {})[key] = {"us": t * 1e6, "bytes": nbytes, "gbs": nbytes / t * 1e-9,
                                                        "of_copy_ceiling": nbytes / t * 1e-9 / copy_gbs}
    for name in ("gather", "reduce"):
        for label, row in out[name].items():
            if "s0" in row:
                for key, v in row.items():
                    v["time_over_identity"] = v["us"] / row["s0"]["us"]
    return out


def main():
    assert torch.cuda.is_available(), "predict_bench needs a HIP device"
    params = O.hash_init(1, 2, seed=31, bn_random=True)
    model = UNet(1, 2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    model = model.cuda().eval()
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (T, H, W), dtype=np.uint8))
    out = {"frames": T, "size": [H, W], "tile_in": TILE, "batch": BATCH, "rounds": ROUNDS, "launches": LAUNCHES,
           "device": torch.cuda.get_device_name(0), "build": _lib.build_identity()}
    for precision in ("fp32", "bf16"):
        out[precision] = end_to_end(model, frames, precision)
    v = ctypes.c_double()
    _lib.check(_lib.load().unet_peak_probe(2, 5, ctypes.byref(v), _lib.stream_of()), "unet_peak_probe")
    out["kernels"] = kernels(v.value)
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
