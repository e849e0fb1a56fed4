"""Sequence inference with symmetry averaging on the GPU: unet_seq_tile_gather
and unet_seq_tile_reduce against tests/predict_oracle.py, their argument checks,
SequencePredictor against torch indexing + the same model forwards, against the
CPU oracle network, and tools/predict_sequence.py's round trip."""
import ctypes
import errno
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import predict_oracle as PO
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# (F, C, H, W, tile_in, tile_out): 220 = 6 * 32 + 28 leaves partial 32-blocks on
# both axes; 5 x 7 repeats the mirror far beyond the frame; a single-row frame;
# 64 / 32: whole blocks only
SHAPES = [(3, 1, 100, 90, 220, 36), (2, 3, 5, 7, 220, 36), (1, 1, 1, 9, 204, 20), (2, 2, 41, 300, 64, 32)]
CODE_SETS = [PO.SETS["d4"], (1, 4, 7)]
GUARD = 4096


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib, _lib.load()


def _guarded(shape, dtype, sentinel):
    """A tensor of `shape` inside a buffer with GUARD sentinel elements on both sides."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def _bands_intact(whole, sentinel):
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all())


def _codes_c(codes):
    return (ctypes.c_int32 * len(codes))(*codes)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(F, C, H, W, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        return rng.integers(0, 256, (F, C, H, W), dtype=np.uint8)
    return rng.standard_normal((F, C, H, W)).astype(np.float32)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("codes", CODE_SETS, ids=["d4", "s147"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seq_gather_bit_exact(shape, codes, dtype):
    L, lib = _need_gpu()
    F, C, H, W, ti, to = shape
    geo = PO.geometry(H, W, ti, to)
    frames = _frames(F, C, H, W, dtype, H * W + C)
    work = PO.work_list(F, len(geo.origins))
    ref = PO.gather(frames, ti, work, codes, to)
    dfr, dwork = torch.from_numpy(frames).cuda(), torch.from_numpy(work).cuda()
    whole, tiles = _guarded(ref.shape, torch.float32, -77.0)
    L.check(lib.unet_seq_tile_gather(dfr.data_ptr(), int(dtype == "u8"), F, C, H, W, ti, to, geo.top, geo.left, geo.nx,
                                     dwork.data_ptr(), len(work), _codes_c(codes), len(codes), tiles.data_ptr(),
                                     _stream()), "gather")
    np.testing.assert_array_equal(tiles.cpu().numpy(), ref)
    assert _bands_intact(whole, -77.0)


def _separated_logits(G, codes, to, thresholds, seed):
    """Standard-normal logits (G * ns, 2, to, to) whose oracle mean p1 stays
    1e-4 away from every threshold: pixels nearer have their class-1 logits
    raised under every symmetry (in the mapped-back frame, so the pixel moves)."""
    ns = len(codes)
    back = np.random.default_rng(seed).standard_normal((G, ns, 2, to, to)).astype(np.float32)
    for _ in range(4):
        lt = np.stack([PO.sym(back[g, j], s) for g in range(G) for j, s in enumerate(codes)])
        p1 = PO.mean_softmax_tiles(lt, ns, codes)[:, 1]
        near = np.zeros(p1.shape, bool)
        for th in thresholds:
            near |= np.abs(p1 - th) < 1e-4
        if not near.any():
            return lt
        back[:, :, 1][np.broadcast_to(near[:, None], (G, ns, to, to))] += 1.0
    raise AssertionError("could not separate the logits from the thresholds")


@pytest.mark.parametrize("codes", CODE_SETS, ids=["d4", "s147"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seq_reduce_vs_float64_oracle(shape, codes):
    """prob within 2e-6 (16 eps of fp32 softmax + mean, doubled); mask equal on
    every pixel once none is within 1e-4 of the threshold; thresholds 0.5 and
    0.3; a partial work list leaves the other pixels' sentinel; guard bands."""
    L, lib = _need_gpu()
    F, C, H, W, ti, to = shape
    geo = PO.geometry(H, W, ti, to)
    ns = len(codes)
    full_work = PO.work_list(F, len(geo.origins))
    for work in (full_work, np.ascontiguousarray(full_work[::2])):
        G = len(work)
        lt = _separated_logits(G, codes, to, (0.5, 0.3), H + W + G)
        ref = PO.reduce(lt, work, codes, F, H, W, ti, to)
        covered = ~np.isnan(ref[:, 0])
        assert covered.all() == (G == len(full_work))
        dlt, dwork = torch.from_numpy(lt).cuda(), torch.from_numpy(work).cuda()
        for th in (0.5, 0.3):
            pw, prob = _guarded((F, 2, H, W), torch.float32, 7.0)
            mw, mask = _guarded((F, H, W), torch.uint8, 3)
            L.check(lib.unet_seq_tile_reduce(dlt.data_ptr(), 2, to, geo.nx, dwork.data_ptr(), G, _codes_c(codes), ns,
                                             F, H, W, th, prob.data_ptr(), mask.data_ptr(), None, _stream()), "reduce")
            p, m = prob.cpu().numpy(), mask.cpu().numpy()
            cov2 = np.broadcast_to(covered[:, None], p.shape)
            err = np.abs(p[cov2] - ref[cov2]).max()
            print(f"{shape} {codes} G={G} th={th}: max |prob - oracle| {err:.3e}")
            assert err <= 2e-6
            assert (p[~cov2] == 7.0).all() and (m[~covered] == 3).all()
            np.testing.assert_array_equal(m[covered], ((ref[:, 1] > th) * 255).astype(np.uint8)[covered])
            assert _bands_intact(pw, 7.0) and _bands_intact(mw, 3)
            # the mask alone (no prob) is the same mask
            mw2, mask2 = _guarded((F, H, W), torch.uint8, 3)
            L.check(lib.unet_seq_tile_reduce(dlt.data_ptr(), 2, to, geo.nx, dwork.data_ptr(), G, _codes_c(codes), ns,
                                             F, H, W, th, None, mask2.data_ptr(), None, _stream()), "reduce")
            assert torch.equal(mask2, mask) and _bands_intact(mw2, 3)


@pytest.mark.parametrize("K", [1, 3, 5])
def test_seq_reduce_other_class_counts(K):
    """The any-class kernel (two classes have their own): prob against the
    float64 oracle within the same 2e-6, logits copied under one symmetry."""
    L, lib = _need_gpu()
    F, C, H, W, ti, to = SHAPES[0]
    geo = PO.geometry(H, W, ti, to)
    work = PO.work_list(F, len(geo.origins))[1::2].copy()
    G = len(work)
    dwork = torch.from_numpy(work).cuda()
    for codes in CODE_SETS + [(3,)]:
        ns = len(codes)
        lt = np.random.default_rng(K).standard_normal((G * ns, K, to, to)).astype(np.float32)
        ref = PO.reduce(lt, work, codes, F, H, W, ti, to)
        covered = np.broadcast_to(~np.isnan(ref[:, :1]), ref.shape)
        pw, prob = _guarded((F, K, H, W), torch.float32, 7.0)
        lw, lg = _guarded((F, K, H, W), torch.float32, 7.0)
        L.check(lib.unet_seq_tile_reduce(torch.from_numpy(lt).cuda().data_ptr(), K, to, geo.nx, dwork.data_ptr(), G,
                                         _codes_c(codes), ns, F, H, W, 0.5, prob.data_ptr(), None,
                                         lg.data_ptr() if ns == 1 else None, _stream()), "reduce")
        p = prob.cpu().numpy()
        assert np.abs(p[covered] - ref[covered]).max() <= 2e-6
        assert (p[~covered] == 7.0).all() and _bands_intact(pw, 7.0) and _bands_intact(lw, 7.0)
        if ns == 1:
            back = np.full((F, K, geo.ny * to, geo.nx * to), 7.0, np.float32)
            for g, (f, t) in enumerate(work):
                y, x = geo.origins[t]
                back[f, :, y:y + to, x:x + to] = PO.sym_inv(lt[g], codes[0])
            np.testing.assert_array_equal(lg.cpu().numpy(), back[:, :, :H, :W])


@pytest.mark.parametrize("code", [0, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seq_reduce_single_symmetry_equals_tile_scatter(shape, code):
    """ns == 1: the logits output and the threshold-0.5 mask are
    unet_tile_scatter's, bit for bit, on the same (mapped-back) logits."""
    L, lib = _need_gpu()
    F, C, H, W, ti, to = shape
    geo = PO.geometry(H, W, ti, to)
    n = len(geo.origins)
    work = PO.work_list(1, n)
    back = np.random.default_rng(code + H).standard_normal((n, 2, to, to)).astype(np.float32)
    back[:, 1, ::3, ::2] = back[:, 0, ::3, ::2]  # ties: l1 > l0 is false there
    lt = np.ascontiguousarray(PO.sym(back, code))
    dback, dlt, dwork = torch.from_numpy(back).cuda(), torch.from_numpy(lt).cuda(), torch.from_numpy(work).cuda()
    full = torch.full((2, H, W), 7.0, device="cuda")
    mask = torch.full((H, W), 3, dtype=torch.uint8, device="cuda")
    L.check(lib.unet_tile_scatter(dback.data_ptr(), 2, to, geo.nx, 0, 1, n, H, W, full.data_ptr(), mask.data_ptr(),
                                  _stream()), "scatter")
    lw, lg = _guarded((1, 2, H, W), torch.float32, 7.0)
    mw, mk = _guarded((1, H, W), torch.uint8, 3)
    pw, pr = _guarded((1, 2, H, W), torch.float32, 7.0)
    L.check(lib.unet_seq_tile_reduce(dlt.data_ptr(), 2, to, geo.nx, dwork.data_ptr(), n, _codes_c((code,)), 1, 1, H, W,
                                     0.5, pr.data_ptr(), mk.data_ptr(), lg.data_ptr(), _stream()), "reduce")
    assert torch.equal(lg[0], full) and torch.equal(mk[0], mask)
    assert _bands_intact(lw, 7.0) and _bands_intact(mw, 3) and _bands_intact(pw, 7.0)
    ref = PO.reduce(lt, work, (code,), 1, H, W, ti, to)
    assert np.abs(pr.cpu().numpy() - ref).max() <= 2e-6
    # logits alone
    lw2, lg2 = _guarded((1, 2, H, W), torch.float32, 7.0)
    L.check(lib.unet_seq_tile_reduce(dlt.data_ptr(), 2, to, geo.nx, dwork.data_ptr(), n, _codes_c((code,)), 1, 1, H, W,
                                     0.5, None, None, lg2.data_ptr(), _stream()), "reduce")
    assert torch.equal(lg2, lg) and _bands_intact(lw2, 7.0)


def test_seq_kernels_reject_bad_arguments():
    """Every rejected case returns an error and launches nothing: the output
    buffers keep their sentinel."""
    L, lib = _need_gpu()
    F, C, H, W, ti, to = 1, 1, 9, 9, 40, 8
    geo = PO.geometry(H, W, ti, to)
    fr = torch.zeros((F, C, H, W), device="cuda")
    work = torch.from_numpy(PO.work_list(F, len(geo.origins))).cuda()
    G = work.shape[0]
    tiles = torch.full((G * 8, C, ti, ti), -77.0, device="cuda")
    lt = torch.zeros((G * 8, 3, to, to), device="cuda")
    prob = torch.full((F, 3, H, W), 7.0, device="cuda")
    mask = torch.full((F, H, W), 3, dtype=torch.uint8, device="cuda")

    def gather(ti=ti, to=to, codes=(0, 1), ns=None, F=F, C=C, H=H, W=W, nx=geo.nx, G=G):
        return lib.unet_seq_tile_gather(fr.data_ptr(), 0, F, C, H, W, ti, to, geo.top, geo.left, nx, work.data_ptr(), G,
                                        _codes_c(codes or (0,)), len(codes) if ns is None else ns, tiles.data_ptr(),
                                        _stream())

    def reduce(k=2, to=to, codes=(0, 1), ns=None, F=F, H=H, W=W, nx=geo.nx, G=G, p=True, m=True, lg=False):
        return lib.unet_seq_tile_reduce(lt.data_ptr(), k, to, nx, work.data_ptr(), G, _codes_c(codes or (0,)),
                                        len(codes) if ns is None else ns, F, H, W, 0.5, prob.data_ptr() if p else None,
                                        mask.data_ptr() if m else None, prob.data_ptr() if lg else None, _stream())

    bad = [gather(ti=7), gather(codes=(0, 8)), gather(codes=(-1,)), gather(ns=0), gather(codes=(0,) * 9),
           gather(ti=0), gather(to=0), gather(F=0), gather(C=0), gather(H=0), gather(W=-1), gather(nx=0), gather(G=0),
           reduce(codes=(0, 8)), reduce(codes=(2, -3)), reduce(ns=0), reduce(codes=(0,) * 9), reduce(k=3),
           reduce(p=False, m=False), reduce(k=0, m=False), reduce(to=0), reduce(F=0), reduce(H=0), reduce(W=0),
           reduce(nx=0), reduce(G=-1), reduce(lg=True, m=False)]
    torch.cuda.synchronize()
    assert all(rc == -errno.EINVAL for rc in bad), bad
    assert bool((tiles == -77.0).all()) and bool((prob == 7.0).all()) and bool((mask == 3).all())
    # NULL required pointers
    assert lib.unet_seq_tile_gather(None, 0, F, C, H, W, ti, to, 0, 0, 1, work.data_ptr(), G, _codes_c((0,)), 1,
                                    tiles.data_ptr(), _stream()) != 0
    assert lib.unet_seq_tile_reduce(lt.data_ptr(), 2, to, 1, None, G, _codes_c((0,)), 1, F, H, W, 0.5, prob.data_ptr(),
                                    None, None, _stream()) != 0
    # and the good calls pass
    assert gather() == 0 and reduce() == 0 and reduce(k=3, m=False) == 0
    torch.cuda.synchronize()


def _model(seed=31):
    from unet_amd import UNet
    params = O.hash_init(1, 2, seed=seed, bn_random=True)
    rng = np.random.default_rng(0)
    for k in params:  # plausible running statistics, as test_tile_farm_vs_oracle
        if k.endswith("running_mean"):
            params[k] = (0.2 * rng.standard_normal(params[k].shape)).astype(np.float32)
        if k.endswith("running_var"):
            params[k] = (0.5 + rng.uniform(size=params[k].shape)).astype(np.float32)
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return m, params


@pytest.fixture(scope="module")
def model():
    _need_gpu()
    m, params = _model()
    return m.cuda().eval(), params


def test_predictor_d4_vs_torch_indexing_and_same_forwards(model):
    """2 uint8 frames of 50 x 45, tile 204, batch 8, "d4": tiles from
    mirror_pad / extract_tiles / flip / rot90, the same model forward in the
    same batches of 8, float64 softmax and mean.  prob within 2e-6, mask equal
    where |mean p1 - 0.5| > 1e-5, and a second call gives the same bits."""
    from unet_amd.predict import SequencePredictor, apply_symmetry, invert_symmetry
    from unet_amd.tiling import TileGeometry, extract_tiles, mirror_pad
    m, _ = model
    frames = torch.from_numpy(_frames(2, 1, 50, 45, "u8", 5)[:, 0]).cuda()
    sp = SequencePredictor(m, tile_in=204, batch=8, symmetries="d4")
    out = sp.predict(frames, want=("mask", "prob"))
    again = sp.predict(frames, want=("mask", "prob"))
    assert torch.equal(out["prob"], again["prob"]) and torch.equal(out["mask"], again["mask"])
    assert out["prob"].shape == (2, 2, 50, 45) and out["mask"].shape == (2, 50, 45)
    assert out["prob"].is_cuda and out["mask"].dtype == torch.uint8
    geo = TileGeometry(50, 45, 204)
    to = geo.tile_out
    x = ((frames.float() / 255) - 0.5) / 0.5
    ref = torch.zeros((2, 2, geo.ny * to, geo.nx * to), dtype=torch.float64, device="cuda")
    with torch.no_grad():
        for f in range(2):
            tiles = extract_tiles(mirror_pad(x[f][None], geo.pads), geo, range(len(geo)))
            for t, (y, xx) in enumerate(geo.origins):
                batch = torch.stack([apply_symmetry(tiles[t], s) for s in range(8)]).contiguous()
                p = torch.softmax(m(batch).double(), 1)
                ref[f, :, y:y + to, xx:xx + to] = torch.stack([invert_symmetry(p[s], s) for s in range(8)]).mean(0)
    ref = ref[:, :, :50, :45]
    err = float((out["prob"].double() - ref).abs().max())
    print(f"d4 composition: max |prob - reference| {err:.3e}")
    assert err <= 2e-6
    sure = (ref[:, 1] - 0.5).abs() > 1e-5
    assert torch.equal(out["mask"][sure], ((ref[:, 1] > 0.5).to(torch.uint8) * 255)[sure])


def test_predictor_identity_equals_tile_farm(model):
    """"none", float32 frames, batch 4: mask and logits equal
    TileFarm(model, [0], 204, 4).predict of each frame bit for bit.  Each frame
    goes through predict on its own, so that the forwards hold the same tiles
    as the farm's (9 tiles: 4 + 4 + 1)."""
    from unet_amd.predict import SequencePredictor
    from unet_amd.tiling import TileFarm
    m, _ = model
    frames = torch.from_numpy(_frames(2, 1, 50, 45, "f32", 6)[:, 0])
    sp = SequencePredictor(m, tile_in=204, batch=4, symmetries="none")
    farm = TileFarm(m, devices=[0], tile_in=204, batch=4)
    dev = frames.cuda()
    for f in range(2):
        out = sp.predict(dev[f:f + 1], want=("mask", "logits"))
        assert torch.equal(out["logits"][0].cpu(), farm.predict(frames[f]))
        assert torch.equal(out["mask"][0].cpu(), farm.predict(frames[f], return_mask=True))
    with pytest.raises(ValueError):
        SequencePredictor(m, tile_in=204, batch=8, symmetries="flip").predict(dev, want=("logits",))


def test_predictor_rot4_vs_oracle_network(model):
    """1 uint8 frame of 20 x 20, tile 204 (one tile), "rot4": four
    O.UNetOracle eval forwards on the CPU.  prob within 5e-4 (the project's
    1e-3 logit bar moves l1 - l0 by at most 2e-3, a two-class softmax's slope
    is at most 1/4); mask equal where the oracle's |mean p1 - 0.5| > 5e-4,
    which may exclude at most 5 % of the pixels.  Seeds (model 31, frame 11)
    chosen on the CPU with the oracle alone: 2 of 400 pixels (0.5 %) excluded,
    63 % foreground, mean p1 between 0.08 and 0.76."""
    from unet_amd.predict import SequencePredictor
    m, params = model
    frame = _frames(1, 1, 20, 20, "u8", 11)
    tile = PO.gather(frame, 204, PO.work_list(1, 1), PO.SETS["rot4"])
    net = O.UNetOracle(params)
    lt = np.concatenate([net.forward(tile[j:j + 1].astype(np.float64), train=False)[0] for j in range(4)])
    ref = PO.reduce(lt, PO.work_list(1, 1), PO.SETS["rot4"], 1, 20, 20, 204)
    out = SequencePredictor(m, tile_in=204, batch=4, symmetries="rot4").predict(torch.from_numpy(frame),
                                                                               want=("mask", "prob"))
    err = np.abs(out["prob"].cpu().numpy() - ref).max()
    unsure = np.abs(ref[:, 1] - 0.5) <= 5e-4
    print(f"rot4 vs oracle network: max |prob - oracle| {err:.3e}, excluded {unsure.mean():.2%}")
    assert err <= 5e-4
    assert unsure.mean() <= 0.05
    np.testing.assert_array_equal(out["mask"].cpu().numpy()[~unsure], ((ref[:, 1] > 0.5) * 255).astype(np.uint8)[~unsure])


def test_predict_sequence_tool_round_trip(model, tmp_path):
    """tools/predict_sequence.py in a fresh process, with --instances: the files
    equal SequencePredictor + instance_masks in-process and have the frames' size."""
    from PIL import Image
    from unet_amd import postproc
    from unet_amd.predict import SequencePredictor
    m, _ = model
    frames = _frames(3, 1, 44, 37, "u8", 9)[:, 0]
    src, res, inst = tmp_path / "01", tmp_path / "01_RES_BIN", tmp_path / "01_RES_INST"
    src.mkdir()
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(src / f"t{i:03d}.tif")
    ckpt = tmp_path / "ckpt.pth"
    torch.save(m.state_dict(), ckpt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict_sequence.py"), "--checkpoint", str(ckpt),
                        "--frames", str(src), "--out", str(res), "--instances", str(inst), "--symmetries", "flip",
                        "--tile", "204", "--batch", "8", "--min-size", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = SequencePredictor(m, tile_in=204, batch=8, symmetries="flip").predict(torch.from_numpy(frames).cuda())
    labels = postproc.instance_masks(out["mask"], min_size=3).cpu().numpy()
    mask = out["mask"].cpu().numpy()
    assert sorted(os.listdir(res)) == [f"mask{i:03d}.tif" for i in range(3)]
    assert sorted(os.listdir(inst)) == [f"m{i:03d}.tif" for i in range(3)]
    for i in range(3):
        got = np.array(Image.open(res / f"mask{i:03d}.tif"))
        assert got.dtype == np.uint8 and got.shape == frames[i].shape and set(np.unique(got)) <= {0, 255}
        np.testing.assert_array_equal(got, mask[i])
        gl = np.array(Image.open(inst / f"m{i:03d}.tif"))
        assert gl.dtype == np.uint16 and gl.shape == frames[i].shape
        np.testing.assert_array_equal(gl, labels[i])
