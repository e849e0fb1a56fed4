#!/usr/bin/env python3
"""Pixel error, Rand error and warping error of segmentation results, the three
measures the U-Net paper ranks by, over one or several sequences.

    python tools/seg_errors.py --gt data/01_GT --res data/01_RES [--gt data/02_GT --res data/02_RES ...]
                               [--radius 4] [--no-separate] [--min-size 15]

--gt   <seq>_GT:  SEG/man_seg*.tif, instance ids
--res  <seq>_RES: mask*.tif, > 0 = foreground
Frames are paired by number.  Where the result frames are smaller than the
ground truth by an even margin (512 against 324: the valid convolutions' crop)
the ground truth is centre-cropped.  Prints one JSON line per sequence with the
mean over its frames of the pixel error and the warping error (fractions of the
frame; --radius and --no-separate as unet_amd.postproc.warping_error) and of the
Rand error of the ground truth against the result's instance labelling
(components under --min-size pixels removed), then with several sequences a
line "mean" with the average of the sequences' lines.  2-D sequences only.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))

KEYS = ("pixel_error", "rand_error", "warping_error")


def evaluate(gt_dir, res_dir, radius, separate, min_size):
    import torch
    from unet_amd import postproc
    from unet_amd.ctc import _numbered, _stack
    gt = _numbered(os.path.join(gt_dir, "SEG", "man_seg*.tif"))
    res = _numbered(os.path.join(res_dir, "mask*.tif"))
    frames = sorted(set(gt) & set(res))
    if not frames:
        raise ValueError(f"no frame of {gt_dir}/SEG/man_seg*.tif has a {res_dir}/mask*.tif")
    g = _stack([gt[n] for n in frames])
    r = _stack([res[n] for n in frames])
    dh, dw = g.shape[1] - r.shape[1], g.shape[2] - r.shape[2]
    if dh < 0 or dw < 0 or dh % 2 or dw % 2:
        raise ValueError(f"the result frames {r.shape[1:]} are no centre crop of the ground truth {g.shape[1:]}")
    g = g[:, dh // 2:g.shape[1] - dh // 2, dw // 2:g.shape[2] - dw // 2]
    dev = torch.device("cuda")
    g = torch.from_numpy(g).to(dev).contiguous()
    mask = (torch.from_numpy(r).to(dev) > 0).to(torch.uint8)
    w = postproc.warping_error(g, mask, radius=radius, separate=separate)
    labels = postproc.instance_masks(mask, min_size=min_size)
    rand = [postproc.rand_index(g[i], labels[i])[1] for i in range(len(frames))]
    return {"frames": len(frames), "pixel_error": float(w.pixel_error.mean()),
            "rand_error": sum(rand) / len(rand), "warping_error": float(w.warping_error.mean()),
            "converged": bool(w.converged.all())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt", action="append", required=True, help="<seq>_GT directory (repeat per sequence)")
    ap.add_argument("--res", action="append", required=True, help="<seq>_RES directory (repeat per sequence)")
    ap.add_argument("--radius", type=int, default=4, help="warping mask radius (-1 = the whole frame)")
    ap.add_argument("--no-separate", action="store_true", help="no background ridge between touching cells")
    ap.add_argument("--min-size", type=int, default=15, help="smallest component of the result's instance labelling")
    a = ap.parse_args(argv)
    if len(a.gt) != len(a.res):
        print("seg_errors: give one --res per --gt", file=sys.stderr)
        return 2
    rows = []
    try:
        for gt_dir, res_dir in zip(a.gt, a.res):
            row = evaluate(gt_dir, res_dir, a.radius, not a.no_separate, a.min_size)
            rows.append(row)
            print(json.dumps({"sequence": os.path.basename(os.path.normpath(res_dir)), **row}))
    except (RuntimeError, ValueError) as e:
        print(f"seg_errors: {e}", file=sys.stderr)
        return 1
    if len(rows) > 1:
        mean = {k: sum(r[k] for r in rows) / len(rows) for k in KEYS}
        print(json.dumps({"sequence": "mean", "frames": sum(r["frames"] for r in rows), **mean,
                          "converged": all(r["converged"] for r in rows)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
