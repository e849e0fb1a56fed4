#!/usr/bin/env python3
"""Tracks a directory of instance masks and writes the Cell Tracking Challenge
result sequence that tools/ctc_measures.py --res reads.

    python tools/track_sequence.py --masks 01_RES_INST --out 01_RES [--label-scope frame]
                                   [--iou-track 0.3 --iou-division 0.1 --max-children 2]
                                   [--linker distance --gate 20 --division-gate 0 --division-min-ratio 0.5]

--masks  mXXX.tif instance labelings (XXX = the frame number), as
         unet_amd.postproc.instance_masks / split_instances give them
--out    receives mask%03d.tif (uint16, pixel = track id) and res_track.txt
         ("label start end parent", parent 0 for a root track)
--linker iou (default): the reference's IoU tracker, frame by frame.
         distance: the distance-based linker (unet_amd.link.link_stack), one
         assignment launch for the sequence; --gate and --division-gate are
         centroid distances in pixels (--division-gate 0: no divisions),
         --division-min-ratio the least area ratio of two daughters.
Prints the number of tracks, the objects left without a track (only under
--label-scope shared, the reference's single label dictionary) and the rows
that hold no pixel in some frame of their span.
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "unet-segmentation_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--masks", required=True, help="directory of mXXX.tif instance masks")
    ap.add_argument("--out", required=True, help="<seq>_RES directory to write")
    ap.add_argument("--label-scope", choices=("shared", "frame"), default="shared")
    ap.add_argument("--iou-track", type=float, default=0.3)
    ap.add_argument("--iou-division", type=float, default=0.1)
    ap.add_argument("--max-children", type=int, default=2)
    ap.add_argument("--linker", choices=("iou", "distance"), default="iou")
    ap.add_argument("--gate", type=float, default=20.0)
    ap.add_argument("--division-gate", type=float, default=0.0)
    ap.add_argument("--division-min-ratio", type=float, default=0.5)
    a = ap.parse_args(argv)
    from unet_amd.track import result_stats, track_directory, write_result
    try:
        if a.linker == "distance":
            from unet_amd.link import link_directory
            got = link_directory(a.masks, gate=a.gate, division_gate=a.division_gate,
                                 division_min_ratio=a.division_min_ratio, max_children=a.max_children)
            if got is None:
                return 1
            res, frames, _ = got
            tr, rows = res.tracker(), res.rows
            write_result(rows, res.masks(), frames, a.out)
        else:
            got = track_directory(a.masks, label_scope=a.label_scope, iou_track=a.iou_track,
                                  iou_division=a.iou_division, max_children=a.max_children)
            if got is None:
                return 1
            tr, frames, stack = got
            rows = tr.tracks()
            write_result(rows, tr.relabel(stack, frames), frames, a.out)
    except (RuntimeError, ValueError) as e:
        print(f"track_sequence: {e}", file=sys.stderr)
        return 1
    st = result_stats(tr, rows)
    print(f"tracks: {st['tracks']}")
    print(f"objects without a track: {st['objects_without_track']}")
    print(f"rows absent from a frame of their span: {st['rows_with_absent_frames']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
