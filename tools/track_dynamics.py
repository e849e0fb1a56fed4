#!/usr/bin/env python3
"""Per-object measurements and track dynamics of a Cell Tracking Challenge
result sequence (the "insights into cellular dynamics" the reference's README
names, and its step 8's "Average Displacement Error").

    python tools/track_dynamics.py --res data/01_RES [--images data/01] [--gt data/01_GT]
                                   [--frame-interval MIN] [--pixel-size UM] --out DIR

--res     <seq>_RES: mask%03d.tif (pixel = track id) + res_track.txt
--images  the sequence's 8-bit images t%03d.tif: adds the intensity columns
--gt      <seq>_GT: TRA/man_track%03d.tif + TRA/man_track.txt: adds the displacement error
Writes DIR/objects.csv (one row per object per frame, sorted by track, then
frame), tracks.csv, divisions.csv and frames.csv, and prints one JSON summary
line.  Lengths are in --pixel-size units (default 1 = pixels), times in
--frame-interval units (default 1 = frames).  2-D sequences only.
"""
import argparse
import csv
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))


def write_csv(path, columns):
    """columns: dict of equally long arrays; floats are written with repr (they read back bit-equal)."""
    keys = list(columns)
    cols = [np.asarray(columns[k]).tolist() for k in keys]
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(keys)
        for row in zip(*cols):
            wr.writerow([repr(v) if isinstance(v, float) else int(v) for v in row])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--res", required=True, help="<seq>_RES directory")
    ap.add_argument("--images", help="directory of the sequence's 8-bit images (t*.tif)")
    ap.add_argument("--gt", help="<seq>_GT directory, for the displacement error")
    ap.add_argument("--frame-interval", type=float, default=1.0, help="time between frames (e.g. minutes)")
    ap.add_argument("--pixel-size", type=float, default=1.0, help="edge of a pixel (e.g. micrometres)")
    ap.add_argument("--out", required=True, help="directory for the four CSV files")
    a = ap.parse_args(argv)
    import torch
    from unet_amd import measure
    from unet_amd.ctc import _numbered, _stack, read_track_file
    try:
        res = _numbered(os.path.join(a.res, "mask*.tif"))
        if not res:
            raise ValueError(f"no mask*.tif in {a.res}")
        frames = sorted(res)
        rows = read_track_file(os.path.join(a.res, "res_track.txt"))
        dev = torch.device("cuda")
        masks = torch.from_numpy(_stack([res[f] for f in frames])).to(dev)
        images = None
        if a.images:
            img = _numbered(os.path.join(a.images, "t*.tif"))
            missing = [f for f in frames if f not in img]
            if missing:
                raise ValueError(f"{a.images} has no image for frames {missing[:8]}")
            stack = _stack([img[f] for f in frames])
            if stack.min() < 0 or stack.max() > 255:
                raise ValueError("the intensity columns are for 8-bit images")
            images = torch.from_numpy(stack.astype(np.uint8)).to(dev)
        traj = measure.trajectories(masks, frames, rows, images)
        tables = measure.dynamics(traj, rows, a.frame_interval, a.pixel_size)
        summary = {"frames": len(frames), "objects": len(traj.table), "tracks": int(len(rows)),
                   "divisions": int(len(tables["divisions"]["parent"]))}
        if a.gt:
            gt = _numbered(os.path.join(a.gt, "TRA", "man_track*.tif"))
            both = [f for f in frames if f in gt]
            if not both:
                raise ValueError(f"no man_track*.tif in {os.path.join(a.gt, 'TRA')} for the result's frames")
            pick = torch.tensor([frames.index(f) for f in both], device=dev)
            err = measure.displacement_error(torch.from_numpy(_stack([gt[f] for f in both])).to(dev),
                                             read_track_file(os.path.join(a.gt, "TRA", "man_track.txt")),
                                             masks[pick], rows, both)
            summary.update(ade=None if math.isnan(err["ade"]) else err["ade"], ade_matched=err["matched"],
                           ade_total=err["total"])
    except (RuntimeError, ValueError, OSError) as e:
        print(f"track_dynamics: {e}", file=sys.stderr)
        return 1
    os.makedirs(a.out, exist_ok=True)
    objects = {"track": traj.table.label, "frame_number": traj.frame}
    objects.update({k: v for k, v in traj.table.columns().items() if k != "label"})
    write_csv(os.path.join(a.out, "objects.csv"), objects)
    for name in ("tracks", "divisions", "frames"):
        write_csv(os.path.join(a.out, name + ".csv"), tables[name])
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
