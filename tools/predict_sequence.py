#!/usr/bin/env python3
"""Binary masks of a whole sequence from a checkpoint: scripts/predict.py's
step on full frames (overlap tiles, no centre crop), optionally averaged over
symmetries of the square, with the instance-mask stage of predict.py:94-112.

    python tools/predict_sequence.py --checkpoint CKPT --frames 01 --out 01_RES_BIN
        [--instances 01_RES_INST [--core-radius R | --min-size 15]]
        [--symmetries d4] [--tile 512] [--batch 8] [--threshold 0.5] [--probs DIR]

--checkpoint  a state_dict in the reference's schema (tools/train_hela.py --checkpoint)
--frames      directory of t*.tif, uint8, one size
--out         directory for mask%03d.tif, uint8 0 / 255, the frames' size
--instances   directory for m%03d.tif, uint16 instance ids (what track_sequence
              reads): 8-connected components, or with --core-radius the
              touching cells split (tools/split_instances.py)
--symmetries  none, flip, rot4, d4, or codes such as 0,1,4 (s = r + 4 f)
--probs       directory for p%03d.tif, float32 mean foreground probability
Prints one JSON line: frames, size, tiles, forwards, symmetries, seconds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))


def _symmetries(text):
    if text[:1].isdigit():
        return tuple(int(t) for t in text.split(","))
    return text


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True, help="state_dict of the U-Net")
    ap.add_argument("--frames", required=True, help="directory of t*.tif")
    ap.add_argument("--out", required=True, help="directory for mask*.tif")
    ap.add_argument("--instances", default=None, help="directory for m*.tif")
    ap.add_argument("--core-radius", type=float, default=None, help="split touching cells: depth of a cell's core")
    ap.add_argument("--min-size", type=int, default=15, help="smallest instance kept")
    ap.add_argument("--symmetries", type=_symmetries, default="none")
    ap.add_argument("--tile", type=int, default=512, help="input tile of the network")
    ap.add_argument("--batch", type=int, default=8, help="tiles per forward")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--probs", default=None, help="directory for p*.tif (float32)")
    ap.add_argument("--precision", default=None, choices=["fp32", "bf16", "bf16x3"])
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    from unet_amd import UNet, postproc
    from unet_amd.ctc import _numbered
    from unet_amd.predict import SequencePredictor
    try:
        files = _numbered(os.path.join(a.frames, "t*.tif"))
        if not files:
            raise ValueError(f"no t*.tif in {a.frames}")
        numbers = sorted(files)
        arrs = [np.array(Image.open(files[n])) for n in numbers]
        for n, arr in zip(numbers, arrs):
            if arr.dtype != np.uint8 or arr.ndim != 2 or arr.shape != arrs[0].shape:
                raise ValueError(f"{files[n]}: frames must be 2-D uint8 of one size, got {arr.dtype} {arr.shape}")
        state = torch.load(a.checkpoint, map_location="cpu")
        model = UNet(state["inc.double_conv.0.weight"].shape[1], state["outc.conv.weight"].shape[0])
        model.load_state_dict(state)
        model.precision = a.precision
        sp = SequencePredictor(model, tile_in=a.tile, batch=a.batch, symmetries=a.symmetries, threshold=a.threshold,
                               device="cuda")
        stack = torch.from_numpy(np.stack(arrs)).to("cuda")
        t0 = time.perf_counter()
        out = sp.predict(stack, want=("mask", "prob") if a.probs else ("mask",))
        labels = None
        if a.instances:
            if a.core_radius is not None:
                r = postproc.split_instances(out["mask"], core_radius=a.core_radius, min_size=a.min_size)
                if bool(r.overflow.any()):
                    raise ValueError("more than 65535 markers or segments in a frame")
                labels = r.labels
            else:
                labels = postproc.instance_masks(out["mask"], min_size=a.min_size)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
    except (RuntimeError, ValueError, KeyError) as e:
        print(f"predict_sequence: {e}", file=sys.stderr)
        return 1
    os.makedirs(a.out, exist_ok=True)
    mask = out["mask"].cpu().numpy()
    for i, n in enumerate(numbers):
        Image.fromarray(mask[i]).save(os.path.join(a.out, f"mask{n:03d}.tif"))
    if labels is not None:
        os.makedirs(a.instances, exist_ok=True)
        lab = labels.cpu().numpy()
        for i, n in enumerate(numbers):
            Image.fromarray(lab[i]).save(os.path.join(a.instances, f"m{n:03d}.tif"))
    if a.probs:
        os.makedirs(a.probs, exist_ok=True)
        p1 = out["prob"][:, 1].cpu().numpy()
        for i, n in enumerate(numbers):
            Image.fromarray(p1[i]).save(os.path.join(a.probs, f"p{n:03d}.tif"))
    geo, work = sp._geometry(*stack.shape)
    per = sp.batch // sp.ns
    print(json.dumps({"frames": len(numbers), "size": list(stack.shape[1:]), "tiles": int(work.shape[0]),
                      "forwards": -(-int(work.shape[0]) // per), "symmetries": list(sp.codes),
                      "seconds": round(seconds, 4)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
