"""Cost of a training-tile batch (unet_tile_warp / TileAugment) next to the
whole-frame warp it extends (unet_elastic_deform / ElasticDeform), timed in
one process, interleaved A B C D A B C D ...:

    A  ElasticDeform   8 x 512^2 frames                 (2 Gaussian passes + k_warp)
    B  TileAugment     8 x 512^2 tiles, elastic field   (2 Gaussian passes + k_tile_warp)
    C  TileAugment     8 x 512^2 tiles, no field        (k_tile_warp alone)
    D  TileAugment     A's own work: identity params, "reflect", no weight plane

B and C cut their tiles out of 84 resident 512^2 frames (a DIC-C2DH-HeLa
sequence) with rotation, flips, "cover" shifts, gain / bias and a gathered
weight plane; D is the new kernel doing exactly what A does (same frames, same
outputs), which isolates the cost of the composed coordinate from the cost of
the rotated gather and the extra plane.  The noise and the params are drawn
once, outside the timed windows.  Each leg is warmed up,
then timed `--rounds` times over `--iters` calls with device events; the result
carries every leg's median and spread, the ratio B / A next to A's own spread,
and the batch's share of the fp32 train step (`--step-ms`, the ms_per_step
bench.py prints).

    python tools/tile_warp_bench.py [--step-ms 25.5] [--out profiles/tile_warp_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=84)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-ms", type=float, default=None, help="fp32 train step (bench.py ms_per_step) for the share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_warp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_warp_bench needs a HIP device (no CPU timing)")
    from unet_amd.augment import ElasticDeform, TileAugment
    n, h, nf = args.batch, args.size, args.frames
    g = np.random.default_rng(0)
    frames = torch.from_numpy(g.integers(0, 256, (nf, h, h)).astype(np.uint8)).cuda()
    labels = torch.from_numpy(g.integers(0, 12, (nf, h, h)).astype(np.uint16)).cuda()
    weights = torch.from_numpy(g.uniform(1.0, 11.0, (nf, h, h)).astype(np.float32)).cuda()
    fidx = torch.from_numpy(g.choice(nf, n, replace=False).astype(np.int32)).cuda()
    sel = fidx.long()
    img8, lab8 = frames.index_select(0, sel), labels.index_select(0, sel)
    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.rand((n, 2, h, h), dtype=torch.float64, device="cuda", generator=gen)
    kw = dict(extend="mirror", alpha=2000.0, sigma=20.0, max_rotate=180.0, flip=True, gain=0.2, bias=20.0,
              out_hw=(324, 324), seed=2)
    el = ElasticDeform(2000.0, 20.0)
    tile = TileAugment((h, h), **kw)
    plain = TileAugment((h, h), elastic=False, **kw)
    same = TileAugment((h, h), extend="reflect", alpha=2000.0, sigma=20.0)
    params = torch.from_numpy(tile.sample_params(n, (h, h))).cuda()
    ident = torch.tensor([[1.0, 0, 0, 0, 1, 0, 1, 0]] * n, dtype=torch.float64, device="cuda")
    first = torch.arange(n, dtype=torch.int32, device="cuda")
    legs = {
        "elastic_deform": lambda: el(img8, lab8, noise=noise),
        "tile_elastic": lambda: tile(frames, labels, fidx, params=params, noise=noise, weights=weights),
        "tile_plain": lambda: plain(frames, labels, fidx, params=params, weights=weights),
        "tile_identity": lambda: same(img8, lab8, first, params=ident, noise=noise),
    }
    for f in legs.values():   # code objects, workspaces, the allocator's blocks
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, f in legs.items():
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.iters)

    def stat(v):
        v = np.asarray(v)
        return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
                "max_ms": round(float(v.max()), 4), "spread": round(float((v.max() - v.min()) / np.median(v)), 4)}

    res = {k: stat(v) for k, v in ms.items()}
    a, b, c, d = (res[k]["median_ms"] for k in ("elastic_deform", "tile_elastic", "tile_plain", "tile_identity"))
    out = {
        "metric": "ms per batch of augmented training tiles (unet_tile_warp) vs the whole-frame warp",
        "config": {"batch": n, "tile": h, "frames_resident": nf, "frame": h, "alpha": 2000, "sigma": 20,
                   "iters": args.iters, "rounds": args.rounds, "order": "A B C D interleaved, one process",
                   "timed": "device events around `iters` calls (launches + the output allocations)",
                   "device": torch.cuda.get_device_name(0)},
        "legs": res,
        "tile_elastic_over_elastic_deform": round(b / a, 4),
        "elastic_deform_own_spread": res["elastic_deform"]["spread"],
        "inside_spread": bool(abs(b / a - 1.0) <= res["elastic_deform"]["spread"]),
        "tile_plain_over_elastic_deform": round(c / a, 4),
        "tile_identity_over_elastic_deform": round(d / a, 4),
        "samples_per_s": {k: round(n / (v["median_ms"] * 1e-3), 1) for k, v in res.items()},
    }
    if args.step_ms:
        out["share_of_fp32_train_step"] = {"step_ms": args.step_ms, "tile_elastic": round(b / args.step_ms, 4),
                                           "tile_plain": round(c / args.step_ms, 4),
                                           "elastic_deform": round(a / args.step_ms, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
