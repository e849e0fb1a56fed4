#!/usr/bin/env python3
"""SEGMeasure, DETMeasure and TRAMeasure of the Cell Tracking Challenge in one
tool (the reference's README step 8 names them; it ships no Linux builds).

    python tools/ctc_measures.py --gt data/01_GT --res data/01_RES [--log TRA_log.txt] [--json]

--gt   <seq>_GT:  SEG/man_seg*.tif and / or TRA/man_track*.tif + TRA/man_track.txt
--res  <seq>_RES: mask*.tif + res_track.txt
Prints "SEG measure: ", "DET measure: " and "TRA measure: " lines like the
binaries' (a measure whose ground truth is absent is left out), or one JSON
object with the measures and the operation counts.  --log writes the text of
the evaluator's TRA_log.txt.  2-D sequences only.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt", required=True, help="<seq>_GT directory")
    ap.add_argument("--res", required=True, help="<seq>_RES directory")
    ap.add_argument("--log", help="write the TRA log here")
    ap.add_argument("--json", action="store_true", help="print one JSON object instead of the three lines")
    a = ap.parse_args(argv)
    from unet_amd.ctc import evaluate_sequence
    try:
        out = evaluate_sequence(a.gt, a.res)
    except (RuntimeError, ValueError) as e:
        print(f"ctc_measures: {e}", file=sys.stderr)
        return 1
    if a.log:
        with open(a.log, "w") as f:
            f.write(out["log"])
    if a.json:
        print(json.dumps({k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in out.items()
                          if k != "log"}))
    else:
        for k in ("SEG", "DET", "TRA"):
            if not math.isnan(out[k]):
                print(f"{k} measure: {out[k]:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
