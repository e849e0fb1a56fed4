"""Golden fixtures for the Cell Tracking Challenge measures, taken from the
demo set the reference ships with the evaluator
(EvaluationSoftware/testing_dataset).  Only data files are read; no code of
the reference is imported or copied.

* ``ctc_tra03.npz``: the 7 + 7 frames of ``03_GT/TRA/man_track*.tif`` and
  ``03_RES/mask*.tif`` (700x1100 uint16), both track tables
  (``man_track.txt``, ``res_track.txt``) and the text of ``03_RES/TRA_log.txt``,
  the log the evaluator itself wrote for this pair (it ends with
  ``TRA measure: 0.622980``).
* ``ctc_seg01.npz``: the 18 frames of ``01_GT/SEG/man_seg*.tif`` with the
  ``01_RES/mask*.tif`` of the same frame numbers (832x992 uint16).  No tool
  output exists for SEG.

Usage:  python tests/golden/make_golden_ctc.py <reference checkout>
"""
from __future__ import annotations

import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def read_track_file(path):
    rows = [list(map(int, ln.split())) for ln in open(path) if ln.strip()]
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def read_stack(files):
    from PIL import Image
    return np.stack([np.array(Image.open(f)) for f in files]).astype(np.uint16)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    D = os.path.join(ref, "EvaluationSoftware", "testing_dataset")
    gt = sorted(glob.glob(os.path.join(D, "03_GT", "TRA", "man_track*.tif")))
    res = sorted(glob.glob(os.path.join(D, "03_RES", "mask*.tif")))
    assert len(gt) == len(res) == 7, (len(gt), len(res))
    frames = np.array([int(os.path.basename(f)[9:12]) for f in gt], np.int32)
    assert [int(os.path.basename(f)[4:7]) for f in res] == list(frames)
    with open(os.path.join(D, "03_RES", "TRA_log.txt"), "rb") as f:
        log = np.frombuffer(f.read(), np.uint8)
    path = os.path.join(HERE, "ctc_tra03.npz")
    np.savez_compressed(path, gt=read_stack(gt), res=read_stack(res), frames=frames,
                        gt_track=read_track_file(os.path.join(D, "03_GT", "TRA", "man_track.txt")),
                        res_track=read_track_file(os.path.join(D, "03_RES", "res_track.txt")), tra_log=log)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")

    seg = sorted(glob.glob(os.path.join(D, "01_GT", "SEG", "man_seg*.tif")))
    assert len(seg) == 18, len(seg)
    frames = np.array([int(os.path.basename(f)[7:10]) for f in seg], np.int32)
    res = [os.path.join(D, "01_RES", f"mask{n:03d}.tif") for n in frames]
    path = os.path.join(HERE, "ctc_seg01.npz")
    np.savez_compressed(path, gt=read_stack(seg), res=read_stack(res), frames=frames)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
