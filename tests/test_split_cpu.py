"""CPU checks of the marker-seeded instance masks (no GPU): properties and known
answers of the oracle (tests/split_oracle.py) that a wrong oracle would fail,
and the library's argument checks, which run before any launch."""
import os

import numpy as np
import pytest

import split_oracle as S

G = os.path.join(os.path.dirname(__file__), "golden")
# SEG of the three hela_real frames against their own binarised ground truth, core_d2 = 900: the plain
# labelling's value is components-that-are-one-cell / 10; tests/test_gpu_split.py compares the device's with these
HELA_SEGMENTS = [8, 9, 10]
HELA_PLAIN_COMPONENTS = [4, 7, 8]


@pytest.fixture(scope="module")
def hela():
    z = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)
    return z["segs"]


def test_core_zero_equals_the_committed_instance_masks():
    z = np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)
    t, h, w = (int(v) for v in z["mask_shape"])
    masks = np.unpackbits(z["mask_bits"], axis=-1)[..., :w]
    for i in range(t):
        r = S.split(masks[i], 0, min_size=int(z["min_size"]))
        np.testing.assert_array_equal(r["labels"], z["labels"][i])
        assert r["info"][0] == r["info"][1] and r["info"][2] == 0


@pytest.mark.parametrize("core_d2", [2, 4, 9])
def test_segments_refine_the_components(core_d2):
    extra = 0
    for k, (h, w) in enumerate(S.SHAPES):
        for density in (0.3, 0.5):
            for m in S.random_stack(1000 * k + int(density * 10), 4, h, w, density):
                seg, comp = S.split(m, core_d2, min_size=1)["labels"], S.plain(m, 1)
                assert ((seg > 0) == (m > 0)).all()
                # every segment inside exactly one component, every component covered by its segments
                pairs = np.unique(np.stack([seg[m > 0], comp[m > 0]]), axis=1)
                assert np.unique(pairs[0]).size == pairs.shape[1]
                extra += int(seg.max()) - int(comp.max())
    assert extra > 30  # the cases do split


def test_dumbbell():
    r = S.split(S.dumbbell(), 36, min_size=1)
    assert r["info"].tolist()[:2] == [2, 2] and r["info"][3] == 0
    assert np.bincount(r["labels"].ravel())[1:].tolist() == [325, 325]
    assert r["labels"][15, 26:30].tolist() == [1, 1, 2, 2]
    # second disc one column further: column 28 is equally far from both markers and takes the smaller label
    r = S.split(S.dumbbell(1), 36, min_size=1)
    assert r["info"].tolist()[:2] == [2, 2]
    assert r["labels"][15, 26:31].tolist() == [1, 1, 1, 2, 2]
    assert (r["labels"][14:17, 28] == 1).all()
    # without a core the discs stay one object
    assert S.split(S.dumbbell(), 0, min_size=1)["info"].tolist() == [1, 1, 0, 0]


def test_distance_conventions():
    m = np.ones((5, 7), np.uint8)
    assert (S.distance(m > 0) == 1 << 30).all()
    assert S.split(m, 1 << 30, min_size=1)["info"].tolist() == [1, 1, 0, 0]
    m[2, 0] = 0  # the frame's border is not background: the far corner is 2^2 + 6^2 away
    d = S.distance(m > 0)
    assert d[2, 0] == 0 and d[0, 6] == 40 and d[2, 6] == 36 and d[4, 0] == 4


def test_markers_argument_and_unmarked_components():
    m = np.zeros((9, 20), np.uint8)
    m[1:4, 1:8] = m[5:8, 2:18] = 1
    mk = np.zeros_like(m)
    mk[6, 17] = mk[6, 2] = mk[0, 0] = 1  # (0, 0) is background: ignored
    r = S.split(m, markers=mk, min_size=1)
    assert r["info"].tolist() == [2, 3, 7, 0]
    assert r["labels"][2, 3] == 1  # the unmarked box comes first in raster order
    assert r["labels"][6, 2:18].tolist() == [2] * 8 + [3] * 8  # marker 1 at x = 2 wins the tie at x = 9


def test_hela_frames_split_into_their_cells(hela):
    for f in range(3):
        gt = hela[f]
        plain = S.plain(gt > 0, 15)
        r = S.split(gt > 0, 900, min_size=15)
        assert int(plain.max()) == HELA_PLAIN_COMPONENTS[f]
        assert r["info"][1] == HELA_SEGMENTS[f] and r["info"][3] == 0
        assert S.seg_measure(gt, r["labels"]) > S.seg_measure(gt, plain)
    assert S.seg_measure(hela[2], S.split(hela[2] > 0, 900)["labels"]) > 0.99


def test_library_rejects_bad_arguments_before_any_launch():
    """-EINVAL and a workspace size of 0 (host code only: nothing is launched)."""
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()

    def call(n, h, w, core_d2=4, min_size=15, ptr=None):
        return lib.unet_split_instances(ptr, None, n, h, w, core_d2, min_size, ptr, None, ptr, ptr, None)

    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 16385, 4), (1, 4, 16385), (65536, 1, 1),
                    (8, 16384, 16384)):
        assert lib.unet_split_instances_ws_bytes(n, h, w) == 0
        assert call(n, h, w) == -22
    assert call(1, 4, 4, core_d2=-1) == -22 and call(1, 4, 4, core_d2=(1 << 30) + 1) == -22
    assert call(1, 4, 4, min_size=-1) == -22
    assert "core_d2" in _lib.last_error()
    assert call(1, 4, 4) == -22 and "null" in _lib.last_error()  # good sizes, null pointers
    assert call(1, 4, 4, ptr=128) == -22  # ws not 256-byte aligned
    assert lib.unet_set_tuning(b"split_threads", 100) == -22 and lib.unet_set_tuning(b"split_threads", 2048) == -22
    assert lib.unet_set_tuning(b"split_threads", 64) == 0 and lib.unet_set_tuning(b"split_threads", -1) == 0
