"""Host-side checks of the border-aware weight maps (no GPU call): exports,
argument validation before any launch, workspace size, the Python keywords,
the train tool's choices and the fixture's own consistency."""
import ctypes
import errno
import os
import sys

import numpy as np
import pytest

from oracle import fixtures as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G = os.path.join(ROOT, "tests", "golden")


def _lib():
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    return _lib


def test_library_exports_the_three_symbols():
    L = _lib()
    lib = L.load()
    for n in ("unet_weight_map_border_ws_bytes", "unet_weight_map_border", "unet_elastic_deform_ex"):
        assert n in L.SIGNATURES and hasattr(lib, n), n


@pytest.mark.parametrize("n,h,w", [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 16385, 8), (1, 8, 16385)])
def test_bad_shapes_are_rejected_before_any_launch(n, h, w):
    L = _lib()
    lib = L.load()
    assert lib.unet_weight_map_border_ws_bytes(n, h, w) == 0
    # host buffers stand in for device pointers: the call must return before touching them
    lab, out, ws = (ctypes.create_string_buffer(64) for _ in range(3))
    rc = lib.unet_weight_map_border(ctypes.addressof(lab), n, h, w, ctypes.c_double(10), ctypes.c_double(5),
                                    ctypes.addressof(out), None, None, None, ctypes.addressof(ws), None)
    assert rc == -errno.EINVAL
    assert "unet_weight_map_border" in L.last_error()


def test_null_pointers_are_rejected():
    L = _lib()
    lib = L.load()
    assert lib.unet_weight_map_border(None, 1, 8, 8, ctypes.c_double(10), ctypes.c_double(5), None, None, None, None,
                                      None, None) == -errno.EINVAL


def test_workspace_is_linear_in_pixels():
    lib = _lib().load()
    ws = lib.unet_weight_map_border_ws_bytes
    assert ws(1, 16384, 16384) > 0
    per_px = (ws(1, 512, 1024) - ws(1, 512, 512)) // (512 * 512)
    assert per_px == 16
    for n, h, w in ((1, 1, 1), (3, 512, 512), (5, 37, 301), (8, 1024, 1024)):
        extra = ws(n, h, w) - per_px * n * h * w      # the per-sample counts, no term in the number of objects
        assert 0 <= extra <= 16 * n, (n, h, w, extra)
    # (even n: the counts are padded to 16 bytes)
    assert ws(8, 512, 512) - ws(4, 512, 512) == 2 * (ws(4, 512, 512) - ws(2, 512, 512))


def test_unknown_mode_raises_before_touching_a_device():
    torch = pytest.importorskip("torch")
    from unet_amd.augment import weight_maps
    with pytest.raises(ValueError, match="mode"):
        weight_maps(torch.zeros((1, 4, 4), dtype=torch.int32), mode="paper")   # a CPU tensor: never reached


def test_train_tool_accepts_the_border_modes():
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_hela
    finally:
        sys.path.pop(0)
    ap = train_hela.build_parser()
    for m in ("static", "warped", "border", "border-warped"):
        assert ap.parse_args(["--npz", "x.npz", "--weights", m]).weights == m
    with pytest.raises(SystemExit):
        ap.parse_args(["--npz", "x.npz", "--weights", "paper"])


def test_fixture_is_consistent():
    sys.path.insert(0, G)
    try:
        import make_golden_border as MB
    finally:
        sys.path.pop(0)
    z = np.load(os.path.join(G, "border_weightmap.npz"), allow_pickle=False)
    assert os.path.getsize(os.path.join(G, "border_weightmap.npz")) < 2 ** 20
    segs = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)["segs"]
    cases = {f"hela{i}": segs[i] for i in range(3)}
    cases.update(F.weightmap_synthetic_cases())
    for k, lab in cases.items():
        d1, d2 = MB.squares(z, k)
        assert d1.dtype == np.int32 and d2.dtype == np.int32 and d1.shape == lab.shape == d2.shape
        nobj = len(np.unique(lab[lab > 0]))
        if nobj >= 2:
            assert (d1 <= d2).all() and (d1 >= 0).all()
            np.testing.assert_array_equal(d1 == 0, lab > 0)
            assert (d2[lab > 0] > 0).all()            # another object is at least a pixel away
        elif nobj == 1:
            assert not d2.any()
            np.testing.assert_array_equal(d1 == 0, lab > 0)
        else:
            assert not d1.any() and not d2.any()
        w = z[f"{k}/weight64_rows"] if k.startswith("hela") else z[f"{k}/weight64"]
        full = MB.weight64_from(lab, d1, d2)
        # the same numpy expression on the same integers: exp may differ by an ulp or two between numpy builds
        np.testing.assert_allclose(w, full[::MB.HELA_ROW_STEP] if k.startswith("hela") else full, rtol=1e-14, atol=0)
        assert w.dtype == np.float64 and (w >= 1).all()
