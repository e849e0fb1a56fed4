"""Sequence inference (unet_amd.predict), the parts that need no GPU: the
symmetry algebra, the work list, the argument checks, and the oracle's gather
against the existing mirror_pad + extract_tiles."""
import numpy as np
import pytest
import torch

import predict_oracle as PO


def _probe(n=5):
    # no symmetry of the square maps this array to itself
    return np.arange(n * n, dtype=np.float32).reshape(n, n) ** 2 + np.arange(n)[None]


@pytest.mark.parametrize("s", range(8))
def test_inverse_undoes_every_symmetry(s):
    from unet_amd import predict as P
    x = _probe()
    np.testing.assert_array_equal(PO.sym_inv(PO.sym(x, s), s), x)
    np.testing.assert_array_equal(PO.sym(PO.sym_inv(x, s), s), x)
    # the package's torch maps are the oracle's
    t = torch.from_numpy(x)
    np.testing.assert_array_equal(P.apply_symmetry(t, s).numpy(), PO.sym(x, s))
    np.testing.assert_array_equal(P.invert_symmetry(P.apply_symmetry(t, s), s).numpy(), x)
    # with leading axes too
    y = np.stack([x, 2 * x])[None]
    np.testing.assert_array_equal(PO.sym_inv(PO.sym(y, s), s), y)


def test_symmetries_are_distinct_and_closed():
    x = _probe()
    imgs = [PO.sym(x, s).tobytes() for s in range(8)]
    assert len(set(imgs)) == 8
    for a in range(8):
        for b in range(8):
            assert PO.sym(PO.sym(x, a), b).tobytes() in imgs
        assert PO.sym_inv(x, a).tobytes() in imgs


def test_named_sets_and_code_tuples():
    from unet_amd import predict as P
    assert P.symmetry_codes("none") == (0,) and P.symmetry_codes("flip") == (0, 4)
    assert P.symmetry_codes("rot4") == (0, 1, 2, 3) and P.symmetry_codes("d4") == tuple(range(8))
    assert P.SYMMETRY_SETS == PO.SETS
    assert P.symmetry_codes((1, 4, 7)) == (1, 4, 7)
    for bad in ("d8", (), (1, 1), (8,), (-1, 2)):
        with pytest.raises(ValueError):
            P.symmetry_codes(bad)


@pytest.mark.parametrize("F,H,W,tile", [(3, 100, 90, 220), (1, 20, 20, 204), (2, 41, 300, 220)])
def test_work_list_covers_every_frame_tile_once(F, H, W, tile):
    from unet_amd import predict as P
    from unet_amd.tiling import TileGeometry
    n = len(TileGeometry(H, W, tile))
    wl = P.work_list(F, n)
    assert wl.dtype == torch.int32 and wl.shape == (F * n, 2)
    np.testing.assert_array_equal(wl.numpy(), PO.work_list(F, n))
    assert sorted(map(tuple, wl.tolist())) == [(f, t) for f in range(F) for t in range(n)]
    assert wl[:, 0].tolist() == sorted(wl[:, 0].tolist())  # frame-major


@pytest.mark.parametrize("sym,batch", [("d4", 4), ("d4", 12), ("rot4", 6), ("flip", 3), ((1, 4, 7), 8)])
def test_symmetries_must_divide_the_batch(sym, batch):
    from unet_amd import UNet
    from unet_amd.predict import SequencePredictor
    with pytest.raises(ValueError, match="divide the batch"):
        SequencePredictor(UNet(1, 2), tile_in=204, batch=batch, symmetries=sym, device="cuda")


@pytest.mark.parametrize("C,H,W,tile", [(1, 100, 90, 220), (3, 5, 7, 220), (1, 1, 9, 204)])
def test_oracle_gather_identity_is_mirror_pad_and_extract(C, H, W, tile):
    from unet_amd.tiling import TileGeometry, extract_tiles, mirror_pad
    rng = np.random.default_rng(H * W)
    frames = rng.standard_normal((2, C, H, W)).astype(np.float32)
    geo = TileGeometry(H, W, tile)
    work = PO.work_list(2, len(geo))
    got = PO.gather(frames, tile, work, PO.SETS["none"])
    for f in range(2):
        ref = extract_tiles(mirror_pad(torch.from_numpy(frames[f]), geo.pads), geo, range(len(geo))).numpy()
        np.testing.assert_array_equal(got[f * len(geo):(f + 1) * len(geo)], ref)
    # and under a symmetry set, entry g * ns + j is S_j of that tile
    codes = (1, 4, 7)
    got3 = PO.gather(frames, tile, work[:2], codes)
    for g in range(2):
        for j, s in enumerate(codes):
            np.testing.assert_array_equal(got3[g * 3 + j], PO.sym(got[g], s))


def test_oracle_normalises_uint8_as_torch_does():
    v = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    ref = ((torch.from_numpy(v).float() / 255) - 0.5) / 0.5
    np.testing.assert_array_equal(PO.normalise(v), ref.numpy())


def test_oracle_reduce_of_equivariant_logits_is_their_softmax():
    """Logits that are S_s of one field average back to that field's softmax."""
    rng = np.random.default_rng(3)
    H = W = 20
    base = rng.standard_normal((2, 20, 20)).astype(np.float32)
    codes = PO.SETS["d4"]
    lt = np.stack([PO.sym(base, s) for s in codes])
    work = PO.work_list(1, 1)
    got = PO.reduce(lt, work, codes, 1, H, W, 204)[0]
    e = np.exp(base.astype(np.float64) - base.max(0))
    np.testing.assert_allclose(got, e / e.sum(0), rtol=0, atol=1e-15)
