"""GPU warping error and pixel error (unet_warping_error,
unet_amd.postproc.warping_error / pixel_error) against the NumPy oracle
(tests/warp_oracle.py): counts and warped planes array-equal, through both
plane storages (LDS, and the workspace the FORCE_WS flag selects)."""
import os

import numpy as np
import pytest
from scipy import ndimage

import warp_oracle as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")
STORAGES = [0, 1]  # flags: 0 = LDS where the planes fit, 1 = postproc.FORCE_WS


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import postproc
    assert postproc.FORCE_WS == 1
    return postproc


def run(pp, gt, pred, **kw):
    """(counts, warped) of a call as NumPy arrays"""
    r = pp.warping_error(torch.from_numpy(np.ascontiguousarray(gt)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(pred)).cuda(), return_warped=True, **kw)
    return r.counts.cpu().numpy(), r.warped.cpu().numpy()


def random_stack(seed, n, h, w, density):
    """gt: blobs with ids 1..3, touching; pred: the ground truth with pixels
    toggled (even frames) or unrelated noise (odd frames)."""
    g = np.random.default_rng(seed)
    gt = (ndimage.uniform_filter(g.random((n, h, w)), (0, 3, 3)) < 0.5 * density + 0.25).astype(np.uint16)
    gt *= g.integers(1, 4, (n, h, w)).astype(np.uint16)
    pred = np.where((np.arange(n) % 2 == 0)[:, None, None], (gt > 0) ^ (g.random((n, h, w)) < 0.15),
                    g.random((n, h, w)) < density)
    return gt, pred.astype(np.uint8) * 255


SHAPES = [(9, 31), (9, 32), (9, 33), (9, 63), (9, 64), (9, 65), (1, 1), (1, 70), (70, 1), (37, 45)]
_WANT = {}  # (shape index, density, radius, separate) -> the oracle's (counts, warped), shared by both storages


def oracle_stack(key, gt, pred, radius, separate):
    if key not in _WANT:
        _WANT[key] = W.evaluate_stack(gt, pred, radius=radius, separate=separate)
    return _WANT[key]


@pytest.mark.parametrize("flags", STORAGES)
@pytest.mark.parametrize("radius", [-1, 2, 4])
@pytest.mark.parametrize("density", [0.3, 0.5])
def test_shapes_vs_oracle(pp, density, radius, flags):
    for k, (h, w) in enumerate(SHAPES):
        gt, pred = random_stack(1000 * k + int(density * 10) + radius, 4, h, w, density)
        for separate in (True, False):
            counts, warped = run(pp, gt, pred, radius=radius, separate=separate, flags=flags)
            want_c, want_w = oracle_stack((k, density, radius, separate), gt, pred, radius, separate)
            np.testing.assert_array_equal(counts, want_c, err_msg=f"{h}x{w} separate={separate}")
            np.testing.assert_array_equal(warped, want_w, err_msg=f"{h}x{w} separate={separate}")
            assert (counts[:, 0] - counts[:, 1] == counts[:, 2]).all() and (counts[:, 4] == 1).all()


def snake(h, w, joined=False):
    """The serpentine of tests/test_gpu_postproc.py: 1-pixel rows every fourth
    line with a two-pixel hook at alternating ends, plus specks.  Its hooks
    stop a line short of the next row, so it is h / 4 separate pieces; `joined`
    makes the hooks three pixels: one line of about h w / 4 pixels."""
    m = np.zeros((h, w), np.uint8)
    for y in range(0, h, 4):
        m[y, :] = 1
        if y + 2 < h:
            m[y + 1:y + (4 if joined else 3), (w - 1) if (y // 4) % 2 == 0 else 0] = 1
    m[2, 3] = m[h - 2, w // 2] = 1
    return m


@pytest.fixture(scope="module", params=["pieces", "joined"])
def serpentine(request):
    gt = snake(64, 75, request.param == "joined").astype(np.uint16)
    pred = np.zeros((64, 75), np.uint8)
    pred[0, 0] = 1  # a line retracts towards this pixel, a flip or two per sweep
    return gt, pred, request.param


@pytest.mark.parametrize("flags", STORAGES)
def test_serpentine_many_sweeps(pp, serpentine, flags):
    gt, pred, kind = serpentine
    want = W.evaluate(gt, pred, radius=-1, separate=False)
    if kind == "joined":
        # one line of 16 x 75 + 15 x 3 + 2 = 1247 pixels that can only retract
        # from its free end, at most one pixel per sub-step whose parity fits:
        # two per sweep along a row, so over 500 sweeps
        assert want["counts"][3] > 500 and want["counts"][1] == 2  # the two specks stay
    counts, warped = run(pp, gt, pred, radius=-1, separate=False, flags=flags)
    np.testing.assert_array_equal(counts, want["counts"])
    np.testing.assert_array_equal(warped, want["warped"])


@pytest.mark.parametrize("max_sweeps", [1, 3, 10])
def test_max_sweeps_stops_at_the_same_sweep(pp, serpentine, max_sweeps):
    gt, pred, _ = serpentine
    want = W.evaluate(gt, pred, radius=-1, separate=False, max_sweeps=max_sweeps)
    for flags in STORAGES:
        counts, warped = run(pp, gt, pred, radius=-1, separate=False, max_sweeps=max_sweeps, flags=flags)
        np.testing.assert_array_equal(counts, want["counts"])
        np.testing.assert_array_equal(warped, want["warped"])
        assert counts[3] == max_sweeps and counts[4] == 0


@pytest.fixture(scope="module")
def hela():
    z = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)
    return np.ascontiguousarray(z["segs"][:, 94:418, 94:418]).astype(np.uint16), z["masks"]


@pytest.mark.parametrize("separate", [True, False])
def test_hela_batched_and_frame_by_frame(pp, hela, separate):
    gt, pred = hela
    want_c, want_w = W.evaluate_stack(gt, pred, radius=4, separate=separate)
    counts, warped = run(pp, gt, pred, radius=4, separate=separate)
    np.testing.assert_array_equal(counts, want_c)
    np.testing.assert_array_equal(warped, want_w)
    for i in range(gt.shape[0]):  # workgroups do not interfere
        c1, w1 = run(pp, gt[i], pred[i], radius=4, separate=separate)
        np.testing.assert_array_equal(c1, want_c[i])
        np.testing.assert_array_equal(w1, want_w[i])
    r = pp.warping_error(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), radius=4, separate=separate)
    assert r.warped is None and r.counts.is_cuda
    # the fractions: the device may divide by multiplying with 1 / (H W), two roundings of 2^-53 each
    np.testing.assert_allclose(r.warping_error.cpu().numpy(), want_c[:, 1] / (324 * 324), rtol=2.0 ** -51, atol=0)
    np.testing.assert_allclose(r.pixel_error.cpu().numpy(), want_c[:, 0] / (324 * 324), rtol=2.0 ** -51, atol=0)
    assert r.warping_error.dtype == torch.float64
    assert r.converged.all() and (r.sweeps.cpu().numpy() == want_c[:, 3]).all()
    assert (r.flips.cpu().numpy() == want_c[:, 2]).all()


def test_frame_too_large_for_lds(pp):
    """600 x 740 does not fit LDS: the same kernel on workspace planes.  Blobs
    against themselves shifted by 3 pixels keep the disagreement sparse."""
    g = np.random.default_rng(5)
    blobs = ndimage.uniform_filter(g.random((600, 740)), 25) > 0.5
    gt = ndimage.label(blobs, W.S8)[0].astype(np.uint16)
    pred = np.roll(blobs, 3, axis=1).astype(np.uint8)
    from unet_amd import _lib
    assert _lib.load().unet_warping_error_ws_bytes(1, 600, 740) > 160 * 1024
    want = W.evaluate(gt, pred, radius=4)
    counts, warped = run(pp, gt, pred, radius=4)
    np.testing.assert_array_equal(counts, want["counts"])
    np.testing.assert_array_equal(warped, want["warped"])
    assert want["counts"][2] > 0
    # the same content cropped to 512 x 512, through both storages
    cg, cp = gt[:512, :512], pred[:512, :512]
    want = W.evaluate(cg, cp, radius=4)
    for flags in STORAGES:
        counts, warped = run(pp, cg, cp, radius=4, flags=flags)
        np.testing.assert_array_equal(counts, want["counts"])
        np.testing.assert_array_equal(warped, want["warped"])


def test_pixel_error_and_argument_checks(pp, hela):
    gt, pred = hela
    for separate in (True, False):
        want = [int((W.ground_truth(g, separate) != (p > 0)).sum()) for g, p in zip(gt, pred)]
        got = pp.pixel_error(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), separate=separate)
        assert got.is_cuda and got.dtype == torch.int64 and got.tolist() == want
    one = pp.pixel_error(torch.from_numpy(gt[0]).cuda(), torch.from_numpy(pred[0]).cuda())
    assert one.dim() == 0 and int(one) == int((W.ground_truth(gt[0]) != (pred[0] > 0)).sum())
    # int32 labels go through _u16
    r = pp.warping_error(torch.from_numpy(gt[0].astype(np.int32)).cuda(), torch.from_numpy(pred[0]).cuda())
    assert r.counts.tolist() == W.evaluate(gt[0], pred[0])["counts"].tolist()
    g, p = torch.from_numpy(gt[0]), torch.from_numpy(pred[0])
    with pytest.raises(ValueError):
        pp.warping_error(g, p.cuda())
    with pytest.raises(ValueError):
        pp.warping_error(g.cuda(), p)
    with pytest.raises(ValueError):
        pp.pixel_error(g, p)
    with pytest.raises(ValueError):
        pp.warping_error(g.cuda(), p[:100].cuda())
    with pytest.raises(ValueError):
        pp.warping_error(g.cuda()[None, None], p.cuda()[None, None])
    for kw in ({"radius": -2}, {"radius": 256}, {"max_sweeps": -1}):
        with pytest.raises(RuntimeError, match="rc=-22"):
            pp.warping_error(g.cuda(), p.cuda(), **kw)


def test_seg_errors_tool(pp, hela, tmp_path, capsys):
    """tools/seg_errors.py on two tiny sequences written as TIFFs: one line per
    sequence and the average; the ground truth is centre-cropped to the
    result's size."""
    import importlib.util
    import json
    from PIL import Image
    from oracle import postproc_oracle as P
    gt, pred = hela
    gt, pred = gt[:, 100:164, 80:150], pred[:, 100:164, 80:150]
    big = np.zeros((3, 64 + 20, 70 + 20), np.uint16)
    big[:, 10:-10, 10:-10] = gt
    big[:, :10] = 7  # outside the crop: must not count
    args, want = [], []
    for s, frames in enumerate(((0, 1), (2,))):
        gd, rd = tmp_path / f"0{s + 1}_GT" / "SEG", tmp_path / f"0{s + 1}_RES"
        os.makedirs(gd)
        os.makedirs(rd)
        rows = []
        for f in frames:
            Image.fromarray(big[f]).save(gd / f"man_seg{f:03d}.tif")
            Image.fromarray(pred[f]).save(rd / f"mask{f:03d}.tif")
            c = W.evaluate(gt[f], pred[f], radius=2)["counts"]
            ri, re = P.rand_index(gt[f], P.get_instance_masks(pred[f], 1))
            rows.append((c[0] / gt[f].size, re, c[1] / gt[f].size))
        want.append(np.mean(rows, axis=0))
        args += ["--gt", str(gd.parent), "--res", str(rd)]
    spec = importlib.util.spec_from_file_location(
        "seg_errors", os.path.join(os.path.dirname(__file__), "..", "tools", "seg_errors.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(args + ["--radius", "2", "--min-size", "1"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 3 and [ln["frames"] for ln in lines] == [2, 1, 3]
    for ln, w in zip(lines[:2], want):
        assert (ln["pixel_error"], ln["rand_error"], ln["warping_error"]) == pytest.approx(tuple(w), rel=1e-12, abs=0)
    mean = np.mean(want, axis=0)
    assert lines[2]["sequence"] == "mean"
    assert (lines[2]["pixel_error"], lines[2]["rand_error"], lines[2]["warping_error"]) == \
        pytest.approx(tuple(mean), rel=1e-12, abs=0)
