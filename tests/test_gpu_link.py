"""unet_link_frames on the MI355X: prev / dist / mother / pair_total array-equal
to the library's host twin (which tests/test_link_cpu.py holds against the
oracle), from the LDS path and from the forced workspace path.  Records,
outputs and a workspace of exactly unet_link_ws_bytes sit inside guard bands
(tests/guarded.py).  End to end: unet_amd.link.link_stack against
tests/link_oracle.py, and tools/track_sequence.py --linker distance.
"""
import ctypes
import errno
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded
import link_cases as K
import link_oracle as LO
import region_oracle as RO

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STALE = 0x5A    # the outputs' bytes before a call: neither -1 nor a record index


@pytest.fixture(scope="module")
def lib():
    from unet_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def link():
    from unet_amd import link as m
    return m


@pytest.fixture(autouse=True)
def _buffers(lib):
    guarded.begin()
    yield
    lib.unet_set_tuning(b"link_lds_objects", -1)
    guarded.release()


def out_buf(nbytes):
    return guarded.G(nbytes, np.uint8, init=np.full(nbytes, STALE, np.uint8))


def device_link(lib, offsets, cols, gq, dq=0):
    """One guarded call: (prev, dist, mother, pair_total) as the device left them."""
    rec = K.records(cols)
    n, total = len(offsets) - 1, len(rec)
    d_rec = guarded.G(total * 128, np.uint8, init=rec.view(np.uint8))
    d_off = guarded.G((n + 1) * 4, np.uint8, init=np.ascontiguousarray(offsets, np.int32).view(np.uint8))
    prev, mother, dist = out_buf(total * 4), out_buf(total * 4), out_buf(total * 8)
    pair_total = out_buf(max(n - 1, 0) * 8)
    ws = guarded.ws_buf(lib.unet_link_ws_bytes(n, total))
    rc = lib.unet_link_frames(d_rec.ptr, d_off.ptr, n, total, gq, dq, prev.ptr, dist.ptr, mother.ptr, pair_total.ptr,
                              ws.ptr, guarded.stream())
    assert rc == 0
    got = (prev.np().view(np.int32).copy(), dist.np().view(np.int64).copy(), mother.np().view(np.int32).copy(),
           pair_total.np().view(np.int64).copy())
    np.testing.assert_array_equal(d_rec.np(), rec.view(np.uint8))     # the inputs are read only
    guarded.done()
    return got


def check(lib, table, gq, dq=0, launches=1):
    """Host twin == LDS path == workspace path == a second run, byte for byte."""
    offsets, cols = table
    rc, *want = K.host_link(lib, offsets, cols, gq, dq)
    assert rc == 0
    runs = []
    for lds in (-1, 0, -1):
        assert lib.unet_set_tuning(b"link_lds_objects", lds) == 0
        lib.unet_link_launches(1)
        runs.append(device_link(lib, offsets, cols, gq, dq))
        assert lib.unet_link_launches(0) == launches
    for got in runs:
        for name, g, w in zip(("prev", "dist", "mother", "pair_total"), got, want):
            np.testing.assert_array_equal(g, w, err_msg=name)
    return want


def empty_cols():
    return {k: np.zeros(0, np.int64) for k in RO.FIELDS}


def test_no_frame_one_frame_and_empty_frames(lib):
    check(lib, (np.zeros(1, np.int32), empty_cols()), 16, launches=0)                 # n = 0
    check(lib, (np.zeros(2, np.int32), empty_cols()), 16)                             # n = 1, no object
    prev, _, mother, total = check(lib, K.from_points([[(0, 0), (0, 16)]]), 16, 16)    # n = 1: frame 0's -1s
    assert prev.tolist() == [-1, -1] and mother.tolist() == [-1, -1] and total.size == 0
    pts = [(0, 0), (16, 16), (32, 0)]
    assert check(lib, K.from_points([[], pts]), 320, 320)[3].tolist() == [0]           # P = 0: births
    assert check(lib, K.from_points([pts, []]), 320, 320)[3].tolist() == [3 * 320 * 320]     # C = 0: private columns
    assert check(lib, K.from_points([[], []]), 320, 320)[3].tolist() == [0]
    assert check(lib, K.from_points([[], pts, [], pts, pts]), 320, 320)[0].tolist() == [-1] * 6 + [3, 4, 5]


def test_one_pixel_frames(lib):
    labels = np.array([[[7]], [[9]], [[0]], [[65535]]], np.uint16)
    prev, dist, _, total = check(lib, K.from_labels(labels, RO.direct), 1)
    assert prev.tolist() == [-1, 0, -1] and dist.tolist() == [-1, 0, -1] and total.tolist() == [0, 1, 0]


def test_one_pair_on_and_past_the_gate(lib):
    on = check(lib, K.from_points([[(0, 0)], [(0, 47)]]), 47)
    past = check(lib, K.from_points([[(0, 0)], [(1, 47)]]), 47)
    assert on[0].tolist() == [-1, 0] and on[1].tolist() == [-1, 47 * 47]
    assert past[0].tolist() == [-1, -1] and past[3].tolist() == [47 * 47]
    far = check(lib, K.from_points([[(0, 0)], [(65535, 0)]]), 65535, 65535)      # the widest gate, d = g2 near 2^32
    assert far[0].tolist() == [-1, 0] and far[1][1] == 65535 * 65535


@pytest.mark.parametrize("p,c", [(127, 128), (128, 128), (128, 129), (256, 257), (257, 256)])
def test_column_counts_around_the_workgroup(lib, p, c):
    """C + P of 255, 256, 257 and 513 columns: the reduction tails of 256 lanes."""
    table = K.from_labels(K.single_pixels([p, c], seed=p + c))
    prev, _, mother, _ = check(lib, table, 48, 80)                # 3-pixel gate on a 24 x 24 frame: links, births, mothers
    linked = int((prev >= 0).sum())
    assert 0 < linked < c and (mother >= 0).any()


def test_labels_1_and_65535_in_one_frame(lib):
    labels = np.zeros((2, 4, 9), np.uint16)
    labels[0, 1, 1], labels[0, 1, 7] = 65535, 1
    labels[1, 2, 1], labels[1, 2, 7] = 1, 65535
    prev, _, _, _ = check(lib, K.from_labels(labels, RO.direct), 32)
    assert prev.tolist() == [-1, -1, 1, 0]        # by place, not by label


def test_tie_lattice_and_equidistant_pair(lib):
    want = LO.link(*K.from_labels(K.lattice(), RO.direct), 5.0, solver="algorithm")
    prev = check(lib, K.from_labels(K.lattice(), RO.direct), 80)[0]
    np.testing.assert_array_equal(prev, want["prev"])
    assert check(lib, K.from_points([[(80, 32), (80, 128)], [(80, 80)]]), 160)[0].tolist() == [-1, -1, 1]


@pytest.mark.parametrize("reverse", [False, True])
def test_chain_of_64(lib, reverse):
    prev, _, _, total = check(lib, K.chain(reverse), 640, 640)
    assert (prev[64:] >= 0).all() and total[0] == 64 * 96 * 96


def test_argument_errors_launch_nothing(lib):
    offsets, cols = K.from_points([[(0, 0)], [(0, 16)]])
    rec = K.records(cols)
    d_rec = guarded.G(2 * 128, np.uint8, init=rec.view(np.uint8))
    d_off = guarded.G(12, np.uint8, init=offsets.view(np.uint8))
    prev, mother, dist, pt = out_buf(8), out_buf(8), out_buf(16), out_buf(8)
    ws = guarded.ws_buf(lib.unet_link_ws_bytes(2, 2))
    good = dict(rec=d_rec.ptr, off=d_off.ptr, n=2, total=2, gq=16, dq=0, prev=prev.ptr, dist=dist.ptr,
                mother=mother.ptr, pt=pt.ptr, ws=ws.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return lib.unet_link_frames(a["rec"], a["off"], a["n"], a["total"], a["gq"], a["dq"], a["prev"], a["dist"],
                                    a["mother"], a["pt"], a["ws"], guarded.stream())

    lib.unet_link_launches(1)
    for bad in (dict(n=-1), dict(gq=0), dict(gq=65536), dict(dq=-1), dict(dq=65536), dict(total=-1), dict(rec=None),
                dict(off=None), dict(prev=None), dict(dist=None), dict(mother=None), dict(pt=None), dict(ws=None),
                dict(rec=d_rec.ptr + 8), dict(off=d_off.ptr + 2), dict(prev=prev.ptr + 2), dict(dist=dist.ptr + 4),
                dict(mother=mother.ptr + 1), dict(pt=pt.ptr + 4), dict(ws=ws.ptr + 128)):
        assert call(**bad) == -errno.EINVAL, bad
    assert lib.unet_link_launches(0) == 0
    torch.cuda.synchronize()
    assert (prev.np() == STALE).all() and (pt.np() == STALE).all()
    assert call() == 0 and lib.unet_link_launches(0) == 1
    guarded.done()
    assert prev.np().view(np.int32).tolist() == [-1, 0]


# ------------------------------- end to end -----------------------------------
def u16_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)


def as_long(t):
    return t.view(torch.int16).long() & 0xFFFF


def end_to_end(lib, link, labels, frames, gate, division_gate):
    offsets, cols = K.from_labels(labels)
    want = LO.link(offsets, cols, gate, division_gate)
    assert all(want["unique"])
    rows, ids = LO.assemble(offsets, cols, frames, want["prev"], want["mother"])
    stack = u16_dev(labels)
    lib.unet_link_launches(1)
    res = link.link_stack(stack, frames, gate=gate, division_gate=division_gate)
    assert lib.unet_link_launches(0) == 1                 # one assignment launch for the sequence
    host = link.link_stack_host(labels, frames, gate=gate, division_gate=division_gate)
    for k in ("prev", "dist", "mother", "pair_total", "rows", "ids"):
        np.testing.assert_array_equal(getattr(res, k), getattr(host, k), err_msg=k)
    assert res.table.records.tobytes() == host.table.records.tobytes()
    for k in ("prev", "dist", "mother", "pair_total"):
        np.testing.assert_array_equal(getattr(res, k), want[k], err_msg=k)
    np.testing.assert_array_equal(res.rows, rows)
    np.testing.assert_array_equal(res.ids, ids)
    tr = res.tracker()
    np.testing.assert_array_equal(tr.tracks(), rows)
    lut = np.zeros((len(frames), 65536), np.int64)
    for i in range(len(frames)):
        f, lab, tid = tr.frame_map(i)
        a, b = int(offsets[i]), int(offsets[i + 1])
        assert f == frames[i]
        np.testing.assert_array_equal(lab, cols["label"][a:b])
        np.testing.assert_array_equal(tid, ids[a:b])
        lut[i, lab] = tid
    masks = res.masks()
    gathered = torch.from_numpy(lut).cuda()[torch.arange(len(frames), device="cuda")[:, None, None], as_long(stack)]
    assert masks.dtype == torch.uint16 and torch.equal(as_long(masks), gathered)
    return res


def test_link_stack_tra03_gt(lib, link):
    d = np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)
    frames = [int(f) for f in d["frames"]]
    end_to_end(lib, link, d["gt"], frames, 40.0, 0.0)
    end_to_end(lib, link, d["gt"], frames, 40.0, 60.0)


@pytest.mark.parametrize("division_gate", [0.0, 30.0])
def test_link_stack_hela_frames_0_to_5(lib, link, division_gate):
    d = np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)
    labels = d["labels"][:6]
    res = end_to_end(lib, link, labels, [int(f) for f in d["frames"][:6]], 20.0, division_gate)
    assert (res.rows[:, 3] > 0).any() == (division_gate > 0)


def test_link_stack_argument_errors(link):
    with pytest.raises(ValueError, match=r"runs on the HIP device only \(no CPU fallback\)"):
        link.link_stack(torch.zeros((2, 4, 4), dtype=torch.int32))
    z = torch.zeros((2, 4, 4), dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError, match="gate"):
        link.link_stack(z, gate=5000.0)
    with pytest.raises(ValueError, match="ascend"):
        link.link_stack(z, frames=[1, 1])
    res = link.link_stack(z)
    assert len(res.rows) == 0 and res.pair_total.tolist() == [0] and not res.masks().view(torch.int16).any().item()
    res = link.link_stack(torch.zeros((0, 4, 4), dtype=torch.uint16, device="cuda"))
    assert len(res.rows) == 0 and res.pair_total.size == 0


def test_tool_writes_a_result_that_ctc_measures_reads(tmp_path):
    from PIL import Image
    d = np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)
    frames = [int(f) for f in d["frames"][:3]]
    inst, res, gt = (str(tmp_path / n) for n in ("03_INST", "03_RES", "03_GT"))
    os.makedirs(inst)
    os.makedirs(os.path.join(gt, "TRA"))
    for f, img in zip(frames, d["gt"][:3]):
        Image.fromarray(np.ascontiguousarray(img, np.uint16)).save(os.path.join(inst, f"m{f:03d}.tif"))
        Image.fromarray(np.ascontiguousarray(img, np.uint16)).save(os.path.join(gt, "TRA", f"man_track{f:03d}.tif"))
    offsets, cols = K.from_labels(d["gt"][:3])
    want = LO.link(offsets, cols, 40.0, 60.0)
    rows, _ = LO.assemble(offsets, cols, frames, want["prev"], want["mother"])
    # the fixture's ground-truth tracks, cut to the three frames
    with open(os.path.join(gt, "TRA", "man_track.txt"), "w") as fh:
        kept = [r for r in d["gt_track"].tolist() if r[1] <= frames[-1]]
        for lab, start, end, parent in kept:
            fh.write(f"{lab} {start} {min(end, frames[-1])} {parent if parent in [k[0] for k in kept] else 0}\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "track_sequence.py"), "--masks", inst, "--out", res,
                        "--linker", "distance", "--gate", "40", "--division-gate", "60"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"tracks: {len(rows)}" in r.stdout and "objects without a track: 0" in r.stdout
    assert sorted(os.listdir(res)) == [f"mask{f:03d}.tif" for f in frames] + ["res_track.txt"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ctc_measures.py"), "--gt", gt, "--res", res,
                        "--json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["DET"] == 1.0          # every object of the masks it was given is there, once
