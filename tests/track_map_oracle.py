"""NumPy checker of the tracker's frame maps and of track-labelled masks.

TEST INFRASTRUCTURE ONLY.  A frame map is {object label: id of the track that
holds it when the frame's step ends}, i.e. oracle.track_oracle.TrackOracle's
`active` read after step(), 0 where the label holds no track.

* track_maps(masks, frames): drives TrackOracle (the reference's single
  label -> track dictionary, "shared" scope) frame by frame.
* FrameScopeOracle: the same step with per-frame label scopes: previous-frame
  look-ups and deletions go to the dictionary the previous step left,
  current-frame assignments to a fresh one that becomes "previous" when the
  step ends.  The body is TrackOracle.step's with the dictionary named on each
  line.
* relabel(masks, maps): each pixel replaced by its label's track id.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

from oracle import track_oracle as T


class FrameScopeOracle(T.TrackOracle):
    def step(self, frame, labels, areas, inter):
        labels = [int(v) for v in labels]
        prev, now = self.active, {}
        if self.first:
            for lab in labels:
                now[lab] = self._new(frame)
            self.first = False
        else:
            plabels, pareas = self.prev
            plabels = [int(v) for v in plabels]
            npv, ncv = len(plabels), len(labels)

            def iou(i, j):
                it = int(inter[i, j])
                un = int(pareas[i]) + int(areas[j]) - it
                return 0.0 if un == 0 else it / un

            mp, mc = set(), set()
            if npv > 0 and ncv > 0:
                cost = np.ones((npv, ncv)) * 1000
                for i in range(npv):
                    for j in range(ncv):
                        v = iou(i, j)
                        if v > 0:
                            cost[i, j] = 1 - v
                rows, cols = linear_sum_assignment(cost)
                for i, j in zip(rows, cols):
                    pl, cl = plabels[i], labels[j]
                    v = 1 - cost[i, j]
                    if v >= self.iou_track and pl in prev:
                        tid = prev[pl]
                        self.tracks[tid][2] = frame
                        del prev[pl]
                        now[cl] = tid
                        mp.add(i)
                        mc.add(j)
            up = [i for i in range(npv) if i not in mp]
            uc = [j for j in range(ncv) if j not in mc]
            for i in up:
                pl = plabels[i]
                if pl not in prev:
                    continue
                kids = [j for j in uc if iou(i, j) >= self.iou_div]
                if 2 <= len(kids) <= self.max_children:
                    parent = prev[pl]
                    self.tracks[parent][2] = frame - 1
                    del prev[pl]
                    for j in kids:
                        now[labels[j]] = self._new(frame, parent)
                        mc.add(j)
            for j in range(ncv):
                if j not in mc:
                    now[labels[j]] = self._new(frame)
        self.active = now
        self.prev = (np.asarray(labels, np.int64), np.asarray(areas, np.int64))


def make_oracle(scope="shared", **kw):
    return {"shared": T.TrackOracle, "frame": FrameScopeOracle}[scope](**kw)


def track_maps(masks, frames=None, scope="shared", **kw):
    """(rows, maps, steps): the res_track rows, per frame the map {label: track
    id or 0}, and per frame the (frame, labels, areas, inter) the step was given
    (what unet_tracker_step_host takes)."""
    tr = make_oracle(scope, **kw)
    maps, steps, prev_mask = [], [], None
    for t, m in enumerate(masks):
        labels, areas = T.frame_objects(m)
        inter = None
        if prev_mask is not None:
            inter = T.overlap_table(prev_mask, tr.prev[0], m, labels)
        f = int(frames[t]) if frames is not None else t
        tr.step(f, labels, areas, inter)
        maps.append({int(l): int(tr.active.get(int(l), 0)) for l in labels})
        steps.append((f, labels, areas, inter))
        prev_mask = m
    return tr.result(), maps, steps


def relabel(masks, maps):
    """(n, h, w) uint16: masks[i] through maps[i]; labels the map lacks -> 0."""
    out = np.zeros(np.shape(masks), np.uint16)
    for i, (m, mp) in enumerate(zip(masks, maps)):
        lut = np.zeros(65536, np.int64)
        for lab, tid in mp.items():
            lut[lab] = tid
        assert lut.max() <= 65535
        out[i] = lut[np.asarray(m).astype(np.int64)]
    return out


def trackless(maps):
    """[(frame index, label)] of the objects that hold no track."""
    return [(i, lab) for i, mp in enumerate(maps) for lab, tid in sorted(mp.items()) if tid == 0]
