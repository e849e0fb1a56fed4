#!/usr/bin/env python3
"""Instance masks with touching cells separated, from the binary masks
scripts/predict.py writes: the instance-mask stage of predict.py:94-112 with
unet_amd.postproc.split_instances in place of get_instance_masks.

    python tools/split_instances.py --masks data/01_RES --out data/01_RES_INST --core-radius 30 [--min-size 15]

--masks  directory of mask*.tif (> 0 = foreground), one size
--out    directory for m*.tif, uint16 instance ids (what track_sequence reads)
A cell's core is where the foreground is at least --core-radius pixels deep;
every core seeds one instance.  Prints one JSON line: frames, and per frame
the markers, the segments and the growth's depth.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--masks", required=True, help="directory of mask*.tif")
    ap.add_argument("--out", required=True, help="directory for m*.tif")
    ap.add_argument("--core-radius", type=float, required=True, help="depth of a cell's core in pixels (0 = no split)")
    ap.add_argument("--min-size", type=int, default=15, help="smallest instance kept")
    a = ap.parse_args(argv)
    import torch
    from PIL import Image
    from unet_amd import postproc
    from unet_amd.ctc import _numbered, _stack
    try:
        files = _numbered(os.path.join(a.masks, "mask*.tif"))
        if not files:
            raise ValueError(f"no mask*.tif in {a.masks}")
        frames = sorted(files)
        stack = torch.from_numpy(_stack([files[n] for n in frames])).to("cuda")
        r = postproc.split_instances(stack, core_radius=a.core_radius, min_size=a.min_size)
        if bool(r.overflow.any()):
            raise ValueError("more than 65535 markers or segments in a frame")
    except (RuntimeError, ValueError) as e:
        print(f"split_instances: {e}", file=sys.stderr)
        return 1
    os.makedirs(a.out, exist_ok=True)
    labels = r.labels.cpu().numpy()
    for i, n in enumerate(frames):
        Image.fromarray(labels[i]).save(os.path.join(a.out, f"m{n:03d}.tif"))
    info = r.info.cpu().numpy()
    print(json.dumps({"frames": len(frames), "markers": info[:, 0].tolist(), "segments": info[:, 1].tolist(),
                      "levels": info[:, 2].tolist()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
