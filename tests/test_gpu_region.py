"""unet_region_props on the MI355X: records and frame offsets array-equal to
tests/region_oracle.py.  Outputs and a workspace of exactly
unet_region_props_ws_bytes sit inside guard bands (tests/guarded.py).
"""
import ctypes
import errno
import os

import numpy as np
import pytest
import torch

import guarded
import region_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
FILL = 0xFF     # guarded.G's payload pattern


@pytest.fixture(scope="module")
def lib():
    from unet_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def measure():
    from unet_amd import measure as m
    return m


@pytest.fixture(autouse=True)
def _buffers(lib):
    guarded.begin()
    yield
    lib.unet_set_tuning(b"region_lds_objects", -1)
    guarded.release()


def u16_dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)
    guarded._KEEP.append(t)
    return t


def run(lib, measure, labels, image=None, cap=None, total_want=None):
    """One guarded call: (rc, host_total, frame_offsets, record bytes, RegionTable or None)."""
    n, h, w = labels.shape
    lab = u16_dev(labels)
    img = None if image is None else guarded.dev(image, torch.uint8)
    cap = total_want if cap is None else cap
    off = guarded.G((n + 1) * 4, np.uint8)
    rec = guarded.G(max(cap, 1) * 128, np.uint8)
    ws = guarded.ws_buf(lib.unet_region_props_ws_bytes(n, h, w))
    total = ctypes.c_longlong(-1)
    rc = lib.unet_region_props(lab.data_ptr(), None if img is None else img.data_ptr(), n, h, w, off.ptr, rec.ptr, cap,
                               ctypes.byref(total), ws.ptr, guarded.stream())
    offsets = off.np().view(np.int32).copy()
    raw = rec.np()[:cap * 128].copy()
    guarded.done()
    table = None
    if rc == 0:
        table = measure.RegionTable(raw.view(measure.RECORD)[:total.value], offsets, (n, h, w), image is not None)
    return rc, int(total.value), offsets, raw, table


def check(lib, measure, labels, image=None, oracle=O.direct):
    want = oracle(labels, image)
    rc, total, _, _, table = run(lib, measure, labels, image, total_want=len(want[1]["frame"]))
    assert rc == 0 and total == len(want[1]["frame"])
    O.assert_equal(table, want)
    return table


def dense_case():
    rng = np.random.default_rng(5)
    return rng.integers(0, 7, (3, 5, 7)).astype(np.uint16), rng.integers(0, 256, (3, 5, 7)).astype(np.uint8)


def test_frames_off_a_16_byte_boundary_with_image(lib, measure):
    labels, image = dense_case()       # frames 1 and 2 start at bytes 70 and 140; 35 pixels: a tail of 3
    check(lib, measure, labels, image)
    check(lib, measure, labels)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (2, 9, 1)])
def test_neighbour_reads_at_every_frame_edge(lib, measure, shape):
    rng = np.random.default_rng(sum(shape))
    check(lib, measure, rng.integers(1, 3, shape).astype(np.uint16))    # no background: every neighbour counts
    check(lib, measure, rng.integers(0, 3, shape).astype(np.uint16), rng.integers(0, 256, shape).astype(np.uint8))


def test_one_run_across_threads_and_workgroups_sums_past_32_bits(lib, measure):
    labels = np.full((1, 8, 4096), 40000, np.uint16)
    t = check(lib, measure, labels, oracle=O.vectorised)
    assert t.sum_xx[0] == 8 * sum(x * x for x in range(4096)) > 1 << 37
    assert t.boundary[0] == 2 * 8 + 2 * 4096 - 4 and t.contact[0] == 0


def test_row_band_seams(lib, measure):
    labels = np.zeros((1, 300, 64), np.uint16)
    labels[0, 3:297, 1:63] = 9           # one object over five 4096-pixel pieces
    t = check(lib, measure, labels, oracle=O.vectorised)
    assert t.boundary[0] == 2 * 294 + 2 * 62 - 4


def test_more_objects_than_the_lds_table(lib, measure):
    rng = np.random.default_rng(7)
    n, h, w = 2, 37, 41
    labels = np.stack([rng.permutation(np.arange(65535 - h * w + 1, 65536)).reshape(h, w),
                       rng.permutation(np.arange(1, h * w + 1)).reshape(h, w)]).astype(np.uint16)
    assert labels.max() == 65535
    image = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    t = check(lib, measure, labels, image, oracle=O.vectorised)
    assert len(t) == 2 * h * w and (t.area == 1).all()


def test_dense_tiny_case_through_the_global_path(lib, measure):
    labels, image = dense_case()
    assert lib.unet_set_tuning(b"region_lds_objects", 2) == 0     # every frame holds more than 2 objects
    a = check(lib, measure, labels, image)
    assert lib.unet_set_tuning(b"region_lds_objects", 0) == 0
    b = check(lib, measure, labels, image)
    assert lib.unet_set_tuning(b"region_lds_objects", -1) == 0
    c = check(lib, measure, labels, image)
    assert a.records.tobytes() == b.records.tobytes() == c.records.tobytes()
    assert lib.unet_set_tuning(b"region_lds_objects", -2) == -errno.EINVAL


def test_cap_one_short_of_the_total(lib, measure):
    labels, image = dense_case()
    want = O.direct(labels, image)
    total = len(want[1]["frame"])
    lib.unet_region_props_launches(1)
    rc, got, offsets, raw, _ = run(lib, measure, labels, image, cap=total - 1)     # guards checked inside
    assert rc == -errno.ENOSPC and got == total
    np.testing.assert_array_equal(offsets, want[0])
    assert (raw == FILL).all()                      # the records still hold their fill pattern
    assert lib.unet_region_props_launches(0) == 0   # no accumulate launch
    rc, got, _, _, table = run(lib, measure, labels, image, cap=total)
    assert rc == 0 and got == total
    O.assert_equal(table, want)
    assert lib.unet_region_props_launches(0) == 1


@pytest.fixture(scope="module")
def hela():
    d = np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)
    return d["labels"]


@pytest.fixture(scope="module")
def tra03():
    return np.load(os.path.join(G, "ctc_tra03.npz"), allow_pickle=False)


def full_stack(lib, measure, labels):
    want = O.vectorised(labels)
    lib.unet_region_props_launches(1)
    rc, total, _, raw, table = run(lib, measure, labels, total_want=len(want[1]["frame"]))
    assert rc == 0 and lib.unet_region_props_launches(0) == 1     # one accumulate launch for the stack
    O.assert_equal(table, want)
    rc, _, _, again, _ = run(lib, measure, labels, total_want=len(want[1]["frame"]))
    assert rc == 0 and lib.unet_region_props_launches(0) == 2
    assert raw.tobytes() == again.tobytes()                       # bit-equal run to run
    t = measure.region_props(u16_dev(labels))                     # the Python entry: guessed cap, one retry at most
    assert t.records.tobytes() == table.records.tobytes()
    np.testing.assert_array_equal(t.frame_offsets, want[0])
    return total


def test_hela_stack(lib, measure, hela):
    assert hela.shape == (84, 324, 324)
    assert full_stack(lib, measure, hela) == 11412


def test_tra03_stacks(lib, measure, tra03):
    assert tra03["gt"].shape == (7, 700, 1100)
    assert full_stack(lib, measure, tra03["gt"]) == 25
    full_stack(lib, measure, tra03["res"])


def test_python_argument_errors(measure):
    with pytest.raises(ValueError, match=r"runs on the HIP device only \(no CPU fallback\)"):
        measure.region_props(torch.zeros((1, 4, 4), dtype=torch.int32))
    bad = torch.zeros((1, 4, 4), dtype=torch.int32, device="cuda")
    bad[0, 1, 1] = 65536
    with pytest.raises(ValueError, match="65535"):
        measure.region_props(bad)
    bad[0, 1, 1] = 65535
    t = measure.region_props(bad, torch.full((1, 4, 4), 7, dtype=torch.uint8, device="cuda"))
    assert t.label.tolist() == [65535] and t.sum_v.tolist() == [7] and t.min_v.tolist() == [7]
    empty = measure.region_props(torch.zeros((0, 4, 4), dtype=torch.uint16, device="cuda"))
    assert len(empty) == 0 and empty.frame_offsets.tolist() == [0]
