"""CPU checks of the training-tile warp: its oracle (tests/tile_warp_oracle.py)
against scipy's mode="mirror" and the inference farm's mirror rule, the host
geometry of unet_amd.augment.TileAugment (affine rows, the "cover" shift range,
the seeded draws) and the argument checks of unet_tile_warp (no device call)."""
import ctypes
import os

import numpy as np
import pytest

import tile_warp_oracle as T
from oracle import elastic_oracle as E

torch = pytest.importorskip("torch")


def _aug(*a, **k):
    from unet_amd.augment import TileAugment
    return TileAugment(*a, **k)


# ---- the oracle's extend=1 sampling against scipy ----
def _rotated_coords(h, w, seed):
    """A 33 degree rotation about the centre of an (h + 140) x (w + 140) grid
    around the frame plus sub-pixel jitter: coordinates up to ~70 px outside
    (several periods for the 1 x 9 and 2 x 2 frames)."""
    g = np.random.default_rng(seed)
    gh, gw = h + 140, w + 140
    ty, tx = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    c, s = np.cos(np.deg2rad(33.0)), np.sin(np.deg2rad(33.0))
    y, x = ty - (gh - 1) / 2.0, tx - (gw - 1) / 2.0
    cy = (c * y - s * x) + (h - 1) / 2.0 + g.uniform(-0.5, 0.5, y.shape)
    cx = (s * y + c * x) + (w - 1) / 2.0 + g.uniform(-0.5, 0.5, y.shape)
    # keep every coordinate within 70 px of the frame, as the case states
    return np.clip(cy, -70.0, h - 1 + 70.0), np.clip(cx, -70.0, w - 1 + 70.0)


@pytest.mark.parametrize("h,w,seed", [(37, 53, 1), (1, 9, 2), (2, 2, 3), (188, 190, 4)])
def test_oracle_mirror_sampling_vs_scipy(h, w, seed):
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(100 + seed)
    img = g.integers(0, 256, (h, w)).astype(np.uint8)
    lab = g.integers(0, 700, (h, w)).astype(np.uint16)
    cy, cx = _rotated_coords(h, w, seed)
    assert cy.min() < -60 and cy.max() > h + 60 and cx.min() < -60 and cx.max() > w + 60
    # order 0: equal
    got0 = T.sample(lab, cy, cx, 0, 1).astype(np.uint16)
    ref0 = ndi.map_coordinates(lab, [cy, cx], order=0, mode="mirror")
    np.testing.assert_array_equal(got0, ref0)
    # order 1: equal after the integer conversion, except where the oracle's own
    # fp64 value sits within 1e-9 of a rounding boundary (at most 0.1 % of the case)
    v = T.sample(img, cy, cx, 1, 1)
    ref64 = ndi.map_coordinates(img.astype(np.float64), [cy, cx], order=1, mode="mirror")
    print(f"{h}x{w}: max |oracle - scipy| before rounding {np.abs(v - ref64).max():.3e}")
    near = np.abs((v + 0.5) - np.round(v + 0.5)) < 1e-9
    print(f"{h}x{w}: {int(near.sum())} of {near.size} values within 1e-9 of a half-integer")
    assert near.mean() <= 1e-3
    ref1 = ndi.map_coordinates(img, [cy, cx], order=1, mode="mirror")
    got1 = E.to_uint(v, np.uint8)
    np.testing.assert_array_equal(got1[~near], ref1[~near])


@pytest.mark.parametrize("n", [1, 2, 5, 37])
def test_mirror_fold_equals_the_farm_rule(n):
    """extend=1 on integer coordinates is tiling.mirror_index (np.pad "reflect",
    repeated beyond the image), order 0 and order 1 alike."""
    from unet_amd.tiling import mirror_index
    start, count = -3 * n - 70, 6 * n + 150
    want = mirror_index(count, start, n).numpy()
    c = np.arange(start, start + count, dtype=np.float64)
    np.testing.assert_array_equal(T.mirror_coord(c, n), want.astype(np.float64))
    cy, cx, (ya, yb, xa, xb, ny, nx) = T.fold(c, c, n, n, 1)
    np.testing.assert_array_equal(ya, want)
    np.testing.assert_array_equal(ny, want)
    assert yb.max() <= n - 1 and xb.max() <= n - 1
    if n > 1:
        np.testing.assert_array_equal(np.pad(np.arange(n), (2 * n, 2 * n), mode="reflect")[n:-n],
                                      mirror_index(3 * n, -n, n).numpy())


# ---- TileAugment's host geometry ----
def test_affine_identity_quarter_turns_and_flips():
    a = _aug((33, 41))
    np.testing.assert_array_equal(a.affine(0.0, False, False, (0, 0), (33, 41)), [1, 0, 0, 0, 1, 0])
    assert not np.signbit(a.affine(0.0, False, False, (0, 0), (33, 41))).any()
    for ang, (c, s) in ((90, (0, 1)), (180, (-1, 0)), (270, (0, -1)), (-90, (0, -1)), (360, (1, 0))):
        for fh in (False, True):
            for fv in (False, True):
                r = a.affine(ang, fh, fv, (2, -3), (50, 60))
                sv, sh = (-1 if fv else 1), (-1 if fh else 1)
                np.testing.assert_array_equal(r[[0, 1, 3, 4]], [c * sv, -s * sh, s * sv, c * sh])
                assert set(np.abs(r[[0, 1, 3, 4]])) == {0.0, 1.0}
    # the documented direction on a square frame: tile[ty, tx] = frame[n - 1 - tx, ty] = rot90(frame, -1)
    sq = _aug((33, 33))
    np.testing.assert_array_equal(sq.affine(90, False, False, (0, 0), (33, 33)), [0, -1, 32, 1, 0, 0])
    np.testing.assert_array_equal(sq.affine(0, True, False, (0, 0), (33, 33)), [1, 0, 0, 0, -1, 32])
    np.testing.assert_array_equal(sq.affine(0, False, True, (0, 0), (33, 33)), [-1, 0, 32, 0, 1, 0])


@pytest.mark.parametrize("ang,fh,fv", [(0, False, False), (33, False, True), (-117.5, True, False), (90, True, True)])
def test_affine_maps_centre_to_centre(ang, fh, fv):
    a = _aug((70, 45))
    H, W, sh = 37, 53, (4.0, -7.5)
    r = a.affine(ang, fh, fv, sh, (H, W))
    cy = r[0] * 34.5 + r[1] * 22.0 + r[2]
    cx = r[3] * 34.5 + r[4] * 22.0 + r[5]
    assert abs(cy - (18.0 + 4.0)) < 1e-12 and abs(cx - (26.0 - 7.5)) < 1e-12
    # a rotation (with flips: a reflection): orthonormal columns
    A = np.array([[r[0], r[1]], [r[3], r[4]]])
    np.testing.assert_allclose(A @ A.T, np.eye(2), atol=1e-15)
    assert np.isclose(np.linalg.det(A), -1.0 if fh != fv else 1.0)


def _window(a, row, out_hw):
    """Frame rows / columns the output window of an unrotated tile covers."""
    th, tw = a.tile_hw
    oy, ox = (th - out_hw[0]) // 2, (tw - out_hw[1]) // 2
    y0, x0 = row[2] + oy, row[5] + ox
    assert y0 == np.floor(y0) and x0 == np.floor(x0)   # whole pixels: no interpolation
    return int(y0), int(y0) + out_hw[0], int(x0), int(x0) + out_hw[1]


@pytest.mark.parametrize("tile", [(24, 30), (40, 52), (25, 31), (33, 30)])
def test_cover_range_reaches_every_pixel_and_no_further(tile):
    H, W, out = 40, 52, (12, 20)
    a = _aug(tile, out_hw=out, max_shift="cover")
    (ly, hy), (lx, hx) = a.shift_range((H, W))
    if (H - tile[0]) % 2 == 0 and (tile[0] - out[0]) % 2 == 0:
        assert (ly, hy) == (-((H - out[0]) // 2), (H - out[0]) // 2)
    if (W - tile[1]) % 2 == 0 and (tile[1] - out[1]) % 2 == 0:
        assert (lx, hx) == (-((W - out[1]) // 2), (W - out[1]) // 2)
    ay, ax = a.align((H, W))
    seen = np.zeros((H, W), bool)
    for sy in range(ly, hy + 1):
        for sx in range(lx, hx + 1):
            y0, y1, x0, x1 = _window(a, a.affine(0, False, False, (sy + ay, sx + ax), (H, W)), out)
            assert 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W
            seen[y0:y1, x0:x1] = True
    assert seen.all()
    for sy, sx in ((ly - 1, lx), (hy + 1, lx), (ly, lx - 1), (ly, hx + 1)):
        y0, y1, x0, x1 = _window(a, a.affine(0, False, False, (sy + ay, sx + ax), (H, W)), out)
        assert y0 < 0 or y1 > H or x0 < 0 or x1 > W


def test_sample_params_bounds_and_seed():
    kw = dict(out_hw=(12, 20), max_rotate=25.0, flip=True, gain=0.3, bias=20.0, seed=11)
    a, b = _aug((24, 30), **kw), _aug((24, 30), **kw)
    rows, d = a.sample_params(500, (40, 52), return_draws=True)
    rows_b = b.sample_params(500, (40, 52))
    np.testing.assert_array_equal(rows, rows_b)
    assert not np.array_equal(rows, a.sample_params(500, (40, 52)))   # the stream moves on
    assert rows.shape == (500, 8) and rows.dtype == np.float64
    assert np.abs(d["angle"]).max() <= 25.0 and np.abs(d["angle"]).max() > 20.0
    assert np.abs(d["shift"][:, 0]).max() == 14 and np.abs(d["shift"][:, 1]).max() == 16
    assert d["shift"].dtype == np.int64
    assert 0.7 <= d["gain"].min() < 0.75 and 1.25 < d["gain"].max() <= 1.3
    assert -20.0 <= d["bias"].min() < -18.0 and 18.0 < d["bias"].max() <= 20.0
    for k in ("flip_h", "flip_v"):
        assert 0.4 < d[k].mean() < 0.6
    np.testing.assert_array_equal(rows[:, 6], d["gain"])
    np.testing.assert_array_equal(rows[:, 7], d["bias"])
    # the defaults draw the shift only
    rows, d = _aug((24, 30), out_hw=(12, 20)).sample_params(50, (40, 52), return_draws=True)
    np.testing.assert_array_equal(rows[:, [0, 1, 3, 4, 6, 7]], np.tile([1.0, 0, 0, 1, 1, 0], (50, 1)))
    np.testing.assert_array_equal(rows[:, 2], 8 + d["shift"][:, 0])
    # an explicit range
    _, d = _aug((24, 30), max_shift=(3, 0)).sample_params(200, (40, 52), return_draws=True)
    assert np.abs(d["shift"][:, 0]).max() == 3 and np.abs(d["shift"][:, 1]).max() == 0


def test_rejects_cpu_tensors_and_bad_arguments():
    a = _aug((8, 8), elastic=False)
    with pytest.raises(ValueError, match="no CPU fallback"):
        a(torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.int32), [0])
    for bad in (dict(extend="wrap"), dict(noise="host"), dict(max_rotate=-1.0), dict(max_shift=-2)):
        with pytest.raises(ValueError):
            _aug((8, 8), **bad)
    with pytest.raises(ValueError):
        _aug((0, 8))
    with pytest.raises(ValueError):
        _aug((8, 8), out_hw=(9, 8)).shift_range((20, 20))


def test_train_tool_takes_the_tile_options():
    import sys
    tools = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
    sys.path.insert(0, tools)
    try:
        import train_hela
    finally:
        sys.path.pop(0)
    ap = train_hela.build_parser()
    a = ap.parse_args(["--npz", "x.npz"])
    assert (a.tiles, a.rotate, a.flip, a.gain, a.bias) == ("frame", 0.0, False, 0.0, 0.0)   # today's path
    a = ap.parse_args(["--npz", "x.npz", "--tiles", "mirror", "--rotate", "180", "--flip", "--gain", "0.2",
                       "--bias", "20"])
    assert (a.tiles, a.rotate, a.flip, a.gain, a.bias) == ("mirror", 180.0, True, 0.2, 20.0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--npz", "x.npz", "--tiles", "reflect"])


# ---- the C entry points' argument checks (host only) ----
def _clib():
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_tile_warp_argument_checks_need_no_device():
    lib = _clib()
    assert lib.unet_tile_warp_ws_bytes(0, 8, 8) == 0
    assert lib.unet_tile_warp_ws_bytes(2, 0, 8) == 0 and lib.unet_tile_warp_ws_bytes(2, 8, -1) == 0
    assert lib.unet_tile_warp_ws_bytes(3, 7, 5) == lib.unet_elastic_ws_bytes(3, 7, 5) == 2 * 2 * 3 * 7 * 5 * 8
    # host buffers stand in for the device pointers: every call below must
    # return before it touches one
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(nframes=1, h=4, w=4, n=1, th=4, tw=4, extend=1, noise=None, sigma=2.0, weights=None, weight_out=None,
             frames=p, x_out=p, ws=p):
        return lib.unet_tile_warp(frames, p, weights, nframes, h, w, p, p, n, th, tw, extend, noise,
                                  ctypes.c_double(10.0), ctypes.c_double(sigma), x_out, p, None, None, weight_out,
                                  ws, None)

    assert call(extend=2) < 0 and call(extend=-1) < 0
    assert call(weight_out=p) < 0
    assert call(th=0) < 0 and call(tw=-3) < 0 and call(n=0) < 0 and call(nframes=0) < 0 and call(h=0) < 0
    assert call(frames=None) < 0 and call(x_out=None) < 0
    assert call(noise=p, sigma=0.0) < 0 and call(noise=p, sigma=200.0) < 0 and call(noise=p, sigma=float("nan")) < 0
    assert call(noise=p, ws=None) < 0 and call(noise=p, ws=p + 4) < 0
    from unet_amd import _lib
    assert "unet_tile_warp" in _lib.last_error()
