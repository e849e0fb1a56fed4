"""The unfused fp32 Winograd tiles' batched point GEMMs on the LDS-DMA ring
(k_igemm_plane, unet_set_tuning "igemm_plane") against the register-staged
kernel they replace (k_igemm).

Conv2d forward and input gradient (reference models/unet_model.py:11,15) as
Winograd F(4x4) / F(2x2) (igemm tiles 71 / 70): M[p] = U[p] V[p]^T per
transform point p.  k_igemm_plane keeps k_igemm's grid, tile and per-element
MFMA chain, so for one point-GEMM tile the output must be bit-identical with
the knob on and off.  unet_set_tuning("wino_point_tile", id) picks that tile
(1, 2, 3, 8, 9 have a ring kernel); unet_igemm_plane_launches() proves the
ring kernel ran.

(Cg, N) = (64, 128) / (128, 64) / (192, 256): the GEMM K is 64, 128, 192 --
4 / 8 / 12 K-steps at BK = 16 and 2 / 4 / 6 at BK = 32, below, at and above what
the rings hold (3 sub-slots of 16 k at BK = 16; 5 or 6 at BK = 32) -- and N is
64, 128, 256.  Forward: Cg = Ci, N = Co; input gradient: Cg = Co, N = Ci.
Input grids 1x10x10, 1x46x46, 2x50x46 give the forward 4 / 121 / 264 F(4x4)
tiles per point (16 / 484 / 1056 at F(2x2)): one row tile with 4 valid rows,
fewer rows than BM, and a ragged last row tile (2 x 128 + 8)."""
import ctypes

import numpy as np
import pytest

from oracle import unet_oracle as O
from oracle import fixtures as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAIRS = [(64, 128), (128, 64), (192, 256)]          # (Cg, N) of the point GEMMs
GRIDS = [(1, 10, 10), (1, 46, 46), (2, 50, 46)]     # (n, h, w) of the input
TILES = {1: (128, 16), 2: (128, 16), 3: (128, 32), 8: (64, 16), 9: (128, 32)}  # id -> (BN, BK)
KNOBS = ((b"igemm_variant", -1), (b"wino_point_tile", -1), (b"igemm_plane", 1))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib.load()


_CASES = {}


def _case(n, h, w, ci, co):
    """Inputs (shared by the tests of a shape, never modified) and the fp64
    convolution / input gradient, computed once."""
    key = (n, h, w, ci, co)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * h + ci + co)
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        wt = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float32)
        b = rng.standard_normal(co).astype(np.float32)
        dy = rng.standard_normal((n, h - 2, w - 2, co)).astype(np.float32)
        x64, w64, dy64 = (a.astype(np.float64) for a in (x, wt, dy))
        ry = O.conv_valid_fwd(x64, w64, b.astype(np.float64))
        rdx, _, _ = O.conv_valid_bwd(x64, w64, dy64)
        _CASES[key] = (x, wt, b, dy, ry, rdx)
    return _CASES[key]


def _run(lib, op, case, variant, tile, plane):
    """One forward / input gradient with the Winograd tile `variant`, its point
    GEMMs on `tile`, on k_igemm_plane (plane 1) or k_igemm (0); the output and
    the ring kernel's launches."""
    from unet_amd import _lib
    x, wt, b, dy, _, _ = case
    n, h, w, ci = x.shape
    co = wt.shape[0]
    ws = torch.empty(lib.unet_conv_ws_bytes(n, h, w, ci, co), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wd = torch.from_numpy(wt).cuda()
    lib.unet_set_tuning(b"igemm_variant", variant)
    lib.unet_set_tuning(b"wino_point_tile", tile)
    lib.unet_set_tuning(b"igemm_plane", plane)
    lib.unet_igemm_plane_launches(1)
    try:
        if op == "fwd":
            out = torch.empty((n, h - 2, w - 2, co), device="cuda")
            xd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
            _lib.check(lib.unet_conv3x3_fwd(xd.data_ptr(), n, h, w, ci, wd.data_ptr(), bd.data_ptr(), co, None, None,
                                            out.data_ptr(), ws.data_ptr(), st), "fwd")
        else:
            out = torch.empty((n, h, w, ci), device="cuda")
            dyd = torch.from_numpy(dy).cuda()
            _lib.check(lib.unet_conv3x3_dgrad(dyd.data_ptr(), n, h, w, ci, wd.data_ptr(), co, out.data_ptr(),
                                              ws.data_ptr(), st), "dgrad")
        torch.cuda.synchronize()
    finally:
        for k, v in KNOBS:
            lib.unet_set_tuning(k, v)
    return out.cpu(), lib.unet_igemm_plane_launches(1)


def _rel(a, ref):
    return float(np.abs(a.double().numpy() - ref).max() / np.abs(ref).max())


def _params():
    for op in ("fwd", "dgrad"):
        for variant in (71, 70):
            for cg, nn in PAIRS:
                if op == "fwd" and variant == 71 and cg < 128:
                    continue  # wino4_fwd_min_cg: the plan's forwards take F(4x4) from 128 channels on
                for grid in GRIDS:
                    yield pytest.param(op, variant, cg, nn, *grid, id=f"{op}-{variant}-K{cg}-N{nn}-{'x'.join(map(str, grid))}")


@pytest.mark.parametrize("op,variant,cg,nn,n,h,w", list(_params()))
def test_igemm_plane_bit_identical(lib, op, variant, cg, nn, n, h, w):
    """Every point-GEMM tile with a ring kernel that fits the shape: the ring
    kernel ran, and its output equals k_igemm's bit for bit."""
    ci, co = (cg, nn) if op == "fwd" else (nn, cg)
    case = _case(n, h, w, ci, co)
    ref = case[4] if op == "fwd" else case[5]
    tiles = [t for t, (bn, bk) in TILES.items() if nn % bn == 0 and cg % bk == 0]
    assert tiles
    for tile in tiles:
        old, n_old = _run(lib, op, case, variant, tile, 0)
        new, n_new = _run(lib, op, case, variant, tile, 1)
        assert n_old == 0 and n_new > 0, (tile, n_old, n_new)
        assert _rel(old, ref) < 1e-3, tile  # sanity only: a wrong kernel is off by O(1)
        assert torch.equal(old, new), f"tile {tile}: max |diff| {float((old - new).abs().max()):.3e}"


def _step(params, x, tgt, wmap):
    from unet_amd import UNet, WeightedCrossEntropyLoss
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.cuda().train()
    logits = m(torch.from_numpy(x).cuda())
    loss = WeightedCrossEntropyLoss()(logits, torch.from_numpy(tgt).cuda(), torch.from_numpy(wmap).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().cpu(), loss.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}


def test_train_step_bit_identical(lib):
    """One 2 x 188^2 fp32 train step in deterministic mode with every 3x3
    forward / input gradient that admits it forced to F(4x4) (tile 71): on
    k_igemm and on k_igemm_plane the loss, the logits and every parameter
    gradient are bit-equal."""
    params = O.hash_init(1, 2, seed=53, bn_random=True)
    x, tgt, wmap = F.make_inputs(53, 2, 1, 188, 188)
    runs, launches = [], []
    lib.unet_tuning_reset()
    lib.unet_set_tuning(b"autotune", 0)
    lib.unet_set_tuning(b"deterministic", 1)
    lib.unet_set_tuning(b"force_tile", 71)
    try:
        for plane in (0, 1):
            lib.unet_set_tuning(b"igemm_plane", plane)
            lib.unet_igemm_plane_launches(1)
            lib.unet_nondeterministic_sites(1)
            runs.append(_step(params, x, tgt, wmap))
            launches.append(lib.unet_igemm_plane_launches(1))
            assert lib.unet_nondeterministic_sites(1) == 0
    finally:
        lib.unet_set_tuning(b"igemm_plane", 1)
        lib.unet_set_tuning(b"force_tile", 0)
        lib.unet_set_tuning(b"deterministic", 0)
        lib.unet_set_tuning(b"autotune", 1)
        lib.unet_tuning_reset()
    assert launches[0] == 0 and launches[1] > 0, launches
    (l0, s0, g0), (l1, s1, g1) = runs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"{k}: k_igemm_plane and k_igemm gradients differ"
