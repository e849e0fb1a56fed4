"""The persistent form of the fused fp32 Winograd tiles 76 (F(4x4), k_wino4f64p)
and 75 (F(2x2), k_wino2f64<64>) against their plain form
(unet_set_tuning "wino_persist" 1 / 0).

Conv2d forward and input gradient (reference models/unet_model.py:11,15).  In
the persistent form min(groups, CUs) workgroups claim tile groups (32 tiles x
64 channels at F(4x4), 64 x 64 at F(2x2)) through counters in the workspace
and load the next group's first operands under the current group's output
stage.  A group keeps the plain form's column block, tile base, statistics slot
and per-tile MFMA chain, so every output must be bit-identical with the knob on
and off, whatever the number of workgroups ("wino_persist_wgs": 1 = one
workgroup walks every group, 3 = several groups each, -1 = one per CU);
unet_wino_persist_launches() proves which form ran.  Each output is also held
to the fp64 oracle, so two kernels wrong in the same way do not pass.

(Cg, N): (16, 64) gives F(4x4) two 8-channel chunks, the shortest loop whose
last chunk -- the one that carries the next group's transfers -- is not also
the first; (8, 64) gives F(2x2) one chunk; (64, 128) two column blocks, so the
column block changes between a workgroup's consecutive groups; (128, 64).
Forward: Cg = Ci, N = Co; input gradient: Cg = Co, N = Ci.  Input grids 1x10x10
(one ragged group), 1x46x46 (forward: 121 F(4x4) tiles = 4 groups, the last with
25) and 2x50x46 (264 tiles = 9 groups, the last with 8; 1056 F(2x2) tiles = 17
groups; edge tiles partly outside in both directions, a group spanning the
image boundary)."""
import ctypes

import numpy as np
import pytest

from oracle import unet_oracle as O
from oracle import fixtures as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRIDS = [(1, 10, 10), (1, 46, 46), (2, 50, 46)]     # (n, h, w) of the input
PAIRS = {76: [(16, 64), (64, 128), (128, 64)], 75: [(8, 64), (16, 64), (64, 128), (128, 64)]}  # tile -> (Cg, N)
WGS = (1, 3, -1)
KNOBS = ((b"igemm_variant", -1), (b"wino_persist", 1), (b"wino_persist_wgs", -1))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib.load()


_CASES = {}


def _case(n, h, w, ci, co):
    """Inputs (shared by the tests of a shape, never modified) and the fp64
    convolution (plain and behind the producer's BN + ReLU) / input gradient,
    computed once."""
    key = (n, h, w, ci, co)
    if key not in _CASES:
        rng = np.random.default_rng(2000 * h + ci + co)
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        wt = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float32)
        b = rng.standard_normal(co).astype(np.float32)
        sc = rng.uniform(-0.5, 1.5, ci).astype(np.float32)
        sh = (rng.standard_normal(ci) * 0.3).astype(np.float32)
        dy = rng.standard_normal((n, h - 2, w - 2, co)).astype(np.float32)
        x64, w64, dy64, b64 = (a.astype(np.float64) for a in (x, wt, dy, b))
        ry = O.conv_valid_fwd(x64, w64, b64)
        rybn = O.conv_valid_fwd(np.maximum(x64 * sc.astype(np.float64) + sh.astype(np.float64), 0), w64, b64)
        rdx, _, _ = O.conv_valid_bwd(x64, w64, dy64)
        _CASES[key] = dict(x=x, wt=wt, b=b, sc=sc, sh=sh, dy=dy, fwd=ry, fwdbn=rybn, dgrad=rdx)
    return _CASES[key]


def _run(lib, op, c, tile, persist, wgs):
    """One forward ("fwd"; "fwdbn": with the producer's BN + ReLU on load) /
    input gradient on `tile`, persistent form on or off; the output and the
    persistent launches."""
    from unet_amd import _lib
    n, h, w, ci = c["x"].shape
    co = c["wt"].shape[0]
    ws = torch.empty(lib.unet_conv_ws_bytes(n, h, w, ci, co), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wd = torch.from_numpy(c["wt"]).cuda()
    lib.unet_set_tuning(b"igemm_variant", tile)
    lib.unet_set_tuning(b"wino_persist", persist)
    lib.unet_set_tuning(b"wino_persist_wgs", wgs)
    lib.unet_wino_persist_launches(1)
    try:
        if op == "dgrad":
            out = torch.empty((n, h, w, ci), device="cuda")
            dyd = torch.from_numpy(c["dy"]).cuda()
            _lib.check(lib.unet_conv3x3_dgrad(dyd.data_ptr(), n, h, w, ci, wd.data_ptr(), co, out.data_ptr(),
                                              ws.data_ptr(), st), "dgrad")
        else:
            out = torch.empty((n, h - 2, w - 2, co), device="cuda")
            xd, bd = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["b"]).cuda()
            scd, shd = torch.from_numpy(c["sc"]).cuda(), torch.from_numpy(c["sh"]).cuda()
            bn = op == "fwdbn"
            _lib.check(lib.unet_conv3x3_fwd(xd.data_ptr(), n, h, w, ci, wd.data_ptr(), bd.data_ptr(), co,
                                            scd.data_ptr() if bn else None, shd.data_ptr() if bn else None,
                                            out.data_ptr(), ws.data_ptr(), st), op)
        torch.cuda.synchronize()
    finally:
        for k, v in KNOBS:
            lib.unet_set_tuning(k, v)
    return out.cpu(), lib.unet_wino_persist_launches(1)


def _rel(a, ref):
    return float(np.abs(a.double().numpy() - ref).max() / np.abs(ref).max())


def _params():
    for tile, pairs in PAIRS.items():
        for op in ("fwd", "fwdbn", "dgrad"):
            for cg, nn in pairs:
                for grid in GRIDS:
                    yield pytest.param(tile, op, cg, nn, *grid,
                                       id=f"{tile}-{op}-K{cg}-N{nn}-{'x'.join(map(str, grid))}")


@pytest.mark.parametrize("tile,op,cg,nn,n,h,w", list(_params()))
def test_wino_persist_bit_identical(lib, tile, op, cg, nn, n, h, w):
    """Persistent form with 1, 3 and one-per-CU workgroups: it ran, and its
    output equals the plain form's bit for bit; the plain form's output is at
    the fp64 oracle (the tolerance of test_gpu_igemm_plane.py)."""
    ci, co = (nn, cg) if op == "dgrad" else (cg, nn)
    c = _case(n, h, w, ci, co)
    old, n_old = _run(lib, op, c, tile, 0, -1)
    assert n_old == 0, n_old
    err = _rel(old, c[op])
    print(f"plain form vs fp64: {err:.2e}")
    assert err < 1e-3
    for wgs in WGS:
        new, n_new = _run(lib, op, c, tile, 1, wgs)
        assert n_new > 0, (wgs, n_new)
        assert torch.equal(old, new), f"wgs {wgs}: max |diff| {float((old - new).abs().max()):.3e}"
        assert _rel(new, c[op]) < 1e-3, wgs


def _step(params, x, tgt, wmap):
    from unet_amd import UNet, WeightedCrossEntropyLoss
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.cuda().train()
    logits = m(torch.from_numpy(x).cuda())
    loss = WeightedCrossEntropyLoss()(logits, torch.from_numpy(tgt).cuda(), torch.from_numpy(wmap).cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    bufs = {n: b.detach().cpu() for n, b in m.named_buffers()}
    return logits.detach().cpu(), loss.detach().cpu(), grads, bufs


@pytest.mark.parametrize("tile", [76, 75])
@pytest.mark.parametrize("h,w,seed", [(188, 188, 61), (204, 252, 62)])
def test_train_step_bit_identical(lib, tile, h, w, seed):
    """One fp32 train step in deterministic mode with every 3x3 forward / input
    gradient that admits it forced to the fused tile (concat sources, two
    destinations, the dgrad mask + BN-backward statistics and the statistics
    slots included): plain form against persistent form on 3 workgroups --
    loss, logits, every gradient and the updated BatchNorm running statistics
    are bit-equal."""
    params = O.hash_init(1, 2, seed=seed, bn_random=True)
    x, tgt, wmap = F.make_inputs(seed, 1, 1, h, w)
    runs, launches = [], []
    lib.unet_tuning_reset()
    lib.unet_set_tuning(b"autotune", 0)
    lib.unet_set_tuning(b"deterministic", 1)
    lib.unet_set_tuning(b"force_tile", tile)
    try:
        for persist in (0, 1):
            lib.unet_set_tuning(b"wino_persist", persist)
            lib.unet_set_tuning(b"wino_persist_wgs", 3)
            lib.unet_wino_persist_launches(1)
            lib.unet_nondeterministic_sites(1)
            runs.append(_step(params, x, tgt, wmap))
            launches.append(lib.unet_wino_persist_launches(1))
            assert lib.unet_nondeterministic_sites(1) == 0
    finally:
        lib.unet_set_tuning(b"wino_persist", 1)
        lib.unet_set_tuning(b"wino_persist_wgs", -1)
        lib.unet_set_tuning(b"force_tile", 0)
        lib.unet_set_tuning(b"deterministic", 0)
        lib.unet_set_tuning(b"autotune", 1)
        lib.unet_tuning_reset()
    print(f"persistent launches: {launches}")
    assert launches[0] == 0 and launches[1] > 0, launches
    (l0, s0, g0, b0), (l1, s1, g1, b1) = runs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"{k}: persistent and plain gradients differ"
    for k in b0:
        assert torch.equal(b0[k], b1[k]), f"{k}: persistent and plain BatchNorm statistics differ"


def test_train_step_vs_oracle(lib):
    """The persistent form under the tuned choices: a train step against the
    fp64 oracle at the fp32 bars of test_gpu_model.py."""
    import test_gpu_model as TM
    lib.unet_set_tuning(b"wino_persist", 1)
    lib.unet_wino_persist_launches(1)
    TM.test_train_step_vs_oracle(2, 188, 63, "fp32")
    print(f"persistent launches under the tuned choices: {lib.unet_wino_persist_launches(1)}")
