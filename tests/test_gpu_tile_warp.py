"""Training tiles on the GPU (unet_tile_warp / unet_amd.augment.TileAugment /
HeLaBatches(tiles=...)) against the existing warp, the inference farm's mirror
padding, exact symmetries and the NumPy fp64 oracle (tests/tile_warp_oracle.py).

Bar: bit-exact, every comparison.  The kernel takes each rounding decision in
fp64 in the oracle's operation order (no fma contraction), as k_warp does."""
import ctypes
import os

import numpy as np
import pytest

import tile_warp_oracle as T
from oracle import elastic_oracle as E
from oracle import fixtures as F
from oracle import weightmap_oracle as WM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")
LABEL_IDS = np.array([0, 0, 1, 7, 255, 256, 257, 512, 699, 65535], np.uint16)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(seed, nf, h, w):
    g = np.random.default_rng(seed)
    frames = g.integers(0, 256, (nf, h, w)).astype(np.uint8)
    labels = LABEL_IDS[g.integers(0, len(LABEL_IDS), (nf, h, w))]
    weights = g.uniform(0.5, 11.0, (nf, h, w)).astype(np.float32)
    return frames, labels, weights


def _run(aug, frames, labels, fidx, params, noise=None, weights=None):
    out = aug(_dev(frames), _dev(labels), fidx, params=params, noise=None if noise is None else _dev(noise),
              weights=None if weights is None else _dev(weights), return_image=True, return_ids=True)
    torch.cuda.synchronize()
    names = ("x", "target", "image", "ids") + (("w",) if weights is not None else ())
    res = {k: v.cpu().numpy() for k, v in zip(names, out)}
    assert res["x"].shape[1] == 1 and res["target"].shape[1] == 1
    res["x"], res["target"] = res["x"][:, 0], res["target"][:, 0]
    return res


def _equal(got, want):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _identity(n):
    return np.tile(np.array([1.0, 0, 0, 0, 1, 0, 1, 0]), (n, 1))


# ---- reduces to the existing path ----
@pytest.mark.parametrize("tag", ["syn", "syn_s3"])
def test_identity_equals_elastic_deform_and_the_reference(tag):
    """Identity params, extend="reflect", tile = frame: ElasticDeform's outputs
    on the same noise; for the synthetic 61 x 77 frame the reference's own."""
    from unet_amd.augment import ElasticDeform, TileAugment
    z = np.load(os.path.join(G, "elastic.npz"), allow_pickle=False)
    sigma = float(z[f"{tag}_sigma"])
    img, lab = F.elastic_synthetic_case()
    frames, labels, _ = _case(1, 2, 61, 77)
    frames[0], labels[0] = img, lab
    noise = np.random.default_rng(2).random((2, 2, 61, 77))
    noise[1] = np.stack(E.noise_from_seed(7, img.shape))
    fidx = [1, 0]   # sample 1 is the synthetic frame with the reference's noise
    got = _run(TileAugment((61, 77), extend="reflect", alpha=2000.0, sigma=sigma), frames, labels, fidx,
               _identity(2), noise)
    sel = _dev(frames[fidx]), _dev(labels[fidx])
    x, t, im, ids = ElasticDeform(alpha=2000.0, sigma=sigma)(*sel, noise=_dev(noise), return_image=True,
                                                             return_ids=True)
    _equal(got, {"x": x.cpu().numpy()[:, 0], "target": t.cpu().numpy()[:, 0], "image": im.cpu().numpy(),
                 "ids": ids.cpu().numpy()})
    np.testing.assert_array_equal(got["image"][1], z[f"{tag}_img"])
    np.testing.assert_array_equal(got["target"][1], (z[f"{tag}_mask"] > 0).astype(np.uint8))
    np.testing.assert_array_equal(got["x"][1], z[f"{tag}_img"].astype(np.float32) / np.float32(255))


def test_identity_equals_elastic_deform_single_row():
    from unet_amd.augment import ElasticDeform, TileAugment
    frames, labels, _ = _case(3, 1, 1, 64)
    noise = np.random.default_rng(4).random((1, 2, 1, 64))
    got = _run(TileAugment((1, 64), extend="reflect", alpha=50.0, sigma=2.0), frames, labels, [0], _identity(1), noise)
    x, t, im, ids = ElasticDeform(alpha=50.0, sigma=2.0)(_dev(frames), _dev(labels), noise=_dev(noise),
                                                         return_image=True, return_ids=True)
    _equal(got, {"x": x.cpu().numpy()[:, 0], "target": t.cpu().numpy()[:, 0], "image": im.cpu().numpy(),
                 "ids": ids.cpu().numpy()})
    assert (got["image"] != frames).any()   # the field moved something


# ---- ties training to inference ----
def test_shifted_tiles_are_crops_of_the_farms_mirror_padding():
    """No elastic field, angle 0, whole-pixel shifts: the tile is the crop of
    tiling.mirror_pad(frame) at its origin (tiles that hang over two sides
    of the frame), image and instance ids alike."""
    from unet_amd.augment import TileAugment
    from unet_amd.tiling import mirror_pad
    frames, labels, _ = _case(5, 2, 37, 53)
    assert (labels == 256).any() and (labels > 256).any()
    th, tw, P = 48, 40, 80
    aug = TileAugment((th, tw), extend="mirror", elastic=False)
    ay, ax = aug.align((37, 53))
    shifts, fidx = [(-9, 14), (30, -41)], [1, 0]
    params = np.stack([np.concatenate([aug.affine(0.0, False, False, (sy + ay, sx + ax), (37, 53)), [1.0, 0.0]])
                       for sy, sx in shifts])
    got = _run(aug, frames, labels, fidx, params)
    for s, f in enumerate(fidx):
        oy, ox = params[s, 2], params[s, 5]
        assert oy == np.floor(oy) and ox == np.floor(ox)
        oy, ox = int(oy) + P, int(ox) + P
        assert min(oy, ox) >= 0 and oy + th <= 37 + 2 * P and ox + tw <= 53 + 2 * P
        pim = mirror_pad(torch.from_numpy(frames[f]), (P, P, P, P)).numpy()[oy:oy + th, ox:ox + tw]
        pid = mirror_pad(torch.from_numpy(labels[f].astype(np.int32)), (P, P, P, P)).numpy()[oy:oy + th, ox:ox + tw]
        np.testing.assert_array_equal(got["image"][s], pim)
        np.testing.assert_array_equal(got["ids"][s], np.where((pid & 0xff) != 0, pid, 0).astype(np.uint16))
        np.testing.assert_array_equal(got["target"][s], ((pid & 0xff) != 0).astype(np.uint8))
        np.testing.assert_array_equal(got["x"][s], pim.astype(np.float32) / np.float32(255))
    assert tuple(params[:, 2]) == (-15.0, 24.0) and tuple(params[:, 5]) == (20.0, -35.0)


# ---- exact symmetries ----
def test_quarter_turn_and_flips_are_exact():
    from unet_amd.augment import TileAugment
    frames, labels, weights = _case(6, 1, 33, 33)
    aug = TileAugment((33, 33), extend="mirror", elastic=False)
    combos = [(90, False, False), (0, True, False), (0, False, True), (90, True, False), (180, False, False),
              (270, True, True)]
    params = np.stack([np.concatenate([aug.affine(a, fh, fv, (0, 0), (33, 33)), [1.0, 0.0]]) for a, fh, fv in combos])
    got = _run(aug, frames, labels, [0] * len(combos), params, weights=weights)

    def turn(m, a, fh, fv):
        m = np.rot90(m, -(a // 90))   # a positive angle turns the content clockwise
        m = m[::-1] if fv else m      # the flips act on the tile, after the rotation
        return m[:, ::-1] if fh else m

    ids0 = np.where((labels[0] & 0xff) != 0, labels[0], 0)
    for s, (a, fh, fv) in enumerate(combos):
        np.testing.assert_array_equal(got["image"][s], turn(frames[0], a, fh, fv), err_msg=str(combos[s]))
        np.testing.assert_array_equal(got["ids"][s], turn(ids0, a, fh, fv), err_msg=str(combos[s]))
        np.testing.assert_array_equal(got["w"][s], turn(weights[0], a, fh, fv), err_msg=str(combos[s]))
    np.testing.assert_array_equal(got["image"][3], np.rot90(frames[0], -1)[:, ::-1])


# ---- the full case against the oracle ----
def _full_params(aug, frame_hw):
    rows = np.stack([aug.affine(33.0, False, True, (3.25, -6.5), frame_hw),
                     aug.affine(-117.5, True, False, (-11.75, 20.125), frame_hw),
                     aug.affine(180.0, True, False, (0.5, 0.0), frame_hw)])
    return np.concatenate([rows, [[0.7, -20.0], [1.3, 20.0], [1.3, -20.0]]], 1)


@pytest.mark.parametrize("extend", ["reflect", "mirror"])
def test_full_case_vs_oracle(extend):
    """Rotation + flips + sub-pixel shifts + elastic field + gain / bias (both
    clips reached) + weight plane, tiles larger than the frames."""
    from unet_amd.augment import TILE_EXTEND, TileAugment
    frames, labels, weights = _case(7, 2, 37, 53)
    aug = TileAugment((70, 45), extend=extend, alpha=300.0, sigma=5.0)
    params = _full_params(aug, (37, 53))
    assert (params[:, [2, 5]] != np.floor(params[:, [2, 5]])).any()
    noise = np.random.default_rng(8).random((3, 2, 70, 45))
    fidx = [1, 0, 1]
    got = _run(aug, frames, labels, fidx, params, noise, weights)
    want = T.tile_warp(frames, labels, fidx, params, (70, 45), TILE_EXTEND[extend], noise, 300.0, 5.0, weights)
    assert (want["x"] == 0.0).any() and (want["x"] == 1.0).any()       # both clips
    assert (want["x"] * 255 != want["image"]).any()
    _equal(got, want)
    # and without the elastic field (one launch, no workspace)
    plain = TileAugment((70, 45), extend=extend, elastic=False)
    _equal(_run(plain, frames, labels, fidx, params, None, weights),
           T.tile_warp(frames, labels, fidx, params, (70, 45), TILE_EXTEND[extend], None, weights=weights))


@pytest.mark.parametrize("extend", ["reflect", "mirror"])
def test_single_row_stack_vs_oracle(extend):
    """A length-1 axis: every row coordinate folds to 0."""
    from unet_amd.augment import TILE_EXTEND, TileAugment
    frames, labels, weights = _case(9, 2, 1, 64)
    aug = TileAugment((5, 70), extend=extend, alpha=50.0, sigma=2.0)
    params = np.stack([np.concatenate([aug.affine(12.0, False, False, (0.0, 3.5), (1, 64)), [1.1, -3.0]]),
                       np.concatenate([aug.affine(0.0, True, False, (2.0, -90.0), (1, 64)), [1.0, 0.0]])])
    noise = np.random.default_rng(10).random((2, 2, 5, 70))
    got = _run(aug, frames, labels, [1, 0], params, noise, weights)
    _equal(got, T.tile_warp(frames, labels, [1, 0], params, (5, 70), TILE_EXTEND[extend], noise, 50.0, 2.0, weights))


def test_gaussian_tile_seams_vs_oracle():
    """Tile 257 x 300 (past the 64-column / 64-row and 256-column Gaussian
    tiles by 1 / 44) from a 100 x 37 frame, non-integer sigma."""
    from unet_amd.augment import TileAugment
    frames, labels, weights = _case(11, 2, 100, 37)
    aug = TileAugment((257, 300), extend="mirror", alpha=900.0, sigma=11.3)
    params = np.stack([np.concatenate([aug.affine(-20.0, False, False, (1.5, 2.0), (100, 37)), [1.0, 0.0]]),
                       np.concatenate([aug.affine(90.0, True, False, (0.0, 0.0), (100, 37)), [0.9, 5.0]])])
    noise = np.random.default_rng(12).random((2, 2, 257, 300))
    got = _run(aug, frames, labels, [0, 1], params, noise, weights)
    _equal(got, T.tile_warp(frames, labels, [0, 1], params, (257, 300), 1, noise, 900.0, 11.3, weights))


# ---- nothing is written outside the outputs or the exactly-sized workspace ----
GUARD, PATTERN = 256, 0xA5


class Guarded:
    """`nbytes` of payload (0xFF-filled) between two 256-byte guards of 0xA5."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.raw[GUARD:GUARD + self.nbytes] = 0xFF
        self.ptr = self.raw.data_ptr() + GUARD

    def np(self, dtype, shape):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).reshape(shape)

    def intact(self):
        g = torch.cat([self.raw[:GUARD], self.raw[GUARD + self.nbytes:]])
        return bool((g == PATTERN).all())


@pytest.mark.parametrize("elastic", [True, False])
def test_guard_bands(elastic):
    from unet_amd import _lib
    from unet_amd.augment import TileAugment
    lib = _lib.load()
    frames, labels, weights = _case(13, 2, 37, 53)
    n, th, tw = 3, 70, 45
    aug = TileAugment((th, tw), alpha=300.0, sigma=5.0)
    params = _full_params(aug, (37, 53))
    noise = np.random.default_rng(14).random((n, 2, th, tw)) if elastic else None
    fidx = np.array([1, 0, 1], np.int32)
    px = n * th * tw
    need = lib.unet_tile_warp_ws_bytes(n, th, tw)
    assert need == 2 * 2 * px * 8
    bufs = {"x": Guarded(4 * px), "target": Guarded(px), "image": Guarded(px), "ids": Guarded(2 * px),
            "w": Guarded(4 * px), "ws": Guarded(need)}
    assert all(b.ptr % 8 == 0 for b in bufs.values())
    dn = _dev(noise) if elastic else None
    df, dl, dw, di, dp = _dev(frames), _dev(labels), _dev(weights), _dev(fidx), _dev(params)
    _lib.check(lib.unet_tile_warp(df.data_ptr(), dl.data_ptr(), dw.data_ptr(), 2, 37, 53, di.data_ptr(),
                                  dp.data_ptr(), n, th, tw, 1, _lib.ptr(dn), ctypes.c_double(300.0),
                                  ctypes.c_double(5.0), bufs["x"].ptr, bufs["target"].ptr, bufs["image"].ptr,
                                  bufs["ids"].ptr, bufs["w"].ptr, bufs["ws"].ptr if elastic else None,
                                  _lib.stream_of()), "unet_tile_warp")
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), f"guard of {k} overwritten"
    got = {"x": bufs["x"].np(np.float32, (n, th, tw)), "target": bufs["target"].np(np.uint8, (n, th, tw)),
           "image": bufs["image"].np(np.uint8, (n, th, tw)), "ids": bufs["ids"].np(np.uint16, (n, th, tw)),
           "w": bufs["w"].np(np.float32, (n, th, tw))}
    assert np.isfinite(got["x"]).all() and np.isfinite(got["w"]).all()   # every element written (0xFF bytes = NaN)
    _equal(got, T.tile_warp(frames, labels, fidx, params, (th, tw), 1, noise, 300.0, 5.0, weights))
    if not elastic:   # no Gaussian launch was made: the workspace was never named, let alone written
        assert (bufs["ws"].np(np.uint8, (need,)) == 0xFF).all()


def test_device_frame_indices_are_clamped():
    """frame_idx given as a device tensor is not read on the host; the kernel
    clamps it to [0, nframes)."""
    from unet_amd.augment import TileAugment
    frames, labels, _ = _case(15, 2, 9, 11)
    aug = TileAugment((9, 11), elastic=False)
    got = _run(aug, frames, labels, _dev(np.array([-3, 7], np.int32)), _identity(2))
    np.testing.assert_array_equal(got["image"], frames)
    with pytest.raises(ValueError, match="frame_idx"):
        aug(_dev(frames), _dev(labels), [0, 2])


# ---- the caller: HeLaBatches(tiles=...) ----
@pytest.fixture(scope="module")
def batches_case():
    from unet_amd.augment import TileAugment
    frames, labels, _ = _case(16, 4, 64, 80)
    # blobs rather than salt and pepper, so that the border term has cells to separate
    yy, xx = np.mgrid[:64, :80]
    labels = np.zeros((4, 64, 80), np.uint16)
    for f in range(4):
        for k, (cy, cx) in enumerate([(12 + 3 * f, 15), (30, 40 + 5 * f), (50, 20 + f), (40, 66)]):
            labels[f][(yy - cy) ** 2 + (xx - cx) ** 2 <= (7 + k) ** 2] = (1, 255, 256, 300)[k] + f
    tile, out = (44, 60), (20, 36)
    aug = TileAugment(tile, extend="mirror", alpha=120.0, sigma=4.0, max_rotate=30.0, flip=True, gain=0.2, bias=10.0,
                      out_hw=out, seed=17)
    params = aug.sample_params(3, (64, 80))
    noise = np.random.default_rng(18).random((3, 2) + tile)
    return frames, labels, tile, out, params, noise


@pytest.mark.parametrize("mode", ["static", "border", "warped", "border-warped"])
def test_hela_batches_with_tiles(batches_case, mode):
    from unet_amd.augment import TileAugment, weight_maps
    from unet_amd.pipeline import HeLaBatches
    frames, labels, tile, out, params, noise = batches_case
    idx = [3, 0, 2]
    aug = TileAugment(tile, extend="mirror", alpha=120.0, sigma=4.0)
    data = HeLaBatches(_dev(frames), _dev(labels), batch=3, out_hw=out, weights=mode, shuffle=False, tiles=aug)
    assert aug.out_hw == out
    x, t, w = data.make_batch(idx, params=params, noise=_dev(noise))
    torch.cuda.synchronize()
    assert x.shape == (3, 1) + tile and t.shape == (3,) + out == w.shape and t.dtype == torch.int64
    oy, ox = (tile[0] - out[0]) // 2, (tile[1] - out[1]) // 2
    crop = lambda a: a[:, oy:oy + out[0], ox:ox + out[1]]   # noqa: E731
    planes = None
    if mode == "static":
        planes = np.stack([WM.training_weights(l) for l in labels])
    elif mode == "border":
        planes = weight_maps(_dev(labels), mode="border").cpu().numpy()
    want = T.tile_warp(frames, labels, idx, params, tile, 1, noise, 120.0, 4.0, planes)
    np.testing.assert_array_equal(x.cpu().numpy()[:, 0], want["x"])
    np.testing.assert_array_equal(t.cpu().numpy(), crop(want["target"]).astype(np.int64))
    if mode == "warped":
        ww = np.stack([WM.training_weights(m) for m in want["target"]])
    elif mode == "border-warped":
        assert len(np.unique(want["ids"])) > 3
        ww = weight_maps(_dev(want["ids"]), mode="border").cpu().numpy()
    else:
        ww = want["w"]
    np.testing.assert_array_equal(w.cpu().numpy(), crop(ww))
    assert 0 < want["target"].mean() < 1


def test_hela_batches_without_tiles_is_unchanged(batches_case):
    from unet_amd.augment import TileAugment
    from unet_amd.pipeline import HeLaBatches
    frames, labels, tile, out, params, _ = batches_case
    noise = _dev(np.random.default_rng(19).random((2, 2, 64, 80)))
    a = HeLaBatches(_dev(frames), _dev(labels), batch=2, out_hw=out, sigma=4.0, shuffle=False)
    b = HeLaBatches(_dev(frames), _dev(labels), batch=2, out_hw=out, sigma=4.0, shuffle=False, tiles=None)
    for u, v in zip(a.make_batch([1, 3], noise=noise), b.make_batch([1, 3], noise=noise)):
        assert torch.equal(u, v)
    # the iterator draws its own params and noise
    it = HeLaBatches(_dev(frames), _dev(labels), batch=3, out_hw=out, tiles=TileAugment(tile, sigma=4.0, flip=True))
    shapes = [(x.shape, t.shape, w.shape) for x, t, w in it]
    assert shapes == [((3, 1) + tile, (3,) + out, (3,) + out), ((1, 1) + tile, (1,) + out, (1,) + out)]
    with pytest.raises(ValueError, match="out_hw"):
        HeLaBatches(_dev(frames), _dev(labels), batch=3, out_hw=out, tiles=TileAugment(tile, out_hw=(8, 8)))
    with pytest.raises(ValueError, match="TileAugment"):
        HeLaBatches(_dev(frames), _dev(labels), batch=3, out_hw=out, tiles="mirror")
