"""The fp32 Winograd weight gradients' batched point GEMMs on the LDS-DMA ring
(k_wgrad_plane, unet_set_tuning "wgrad_plane") against the gather kernel they
replace (k_wgrad), and the output transforms' direct OIHW store
(unet_set_tuning "wgrad_oihw") against the packed store + permute.

Conv2d's weight gradient (reference models/unet_model.py:11,15) as Winograd
F(6x6) / F(4x4): dW = G^T (sum over tiles Vd[p]^T U[p]) G.  k_wgrad_plane keeps
k_wgrad's grid, pixel split and per-element MFMA chain, so in slab mode (no
atomics) dW must be bit-identical with the knob on and off; with atomics both
paths are held to the fp64 correlation, the new one to 2x the old one's own
error on the same shape (two runs of the old kernel already differ by the order
of their atomics).

Shapes: (Co, Ci) = (64, 64) / (64, 128) / (128, 128) reach point-GEMM tiles
4 / 3 / 0 (64x64, 64x128, 128x128).  Input grids 1x14x14, 1x40x40, 2x52x46
give 4 / 49 / 144 F(6x6) tiles (9 / 100 / 286 at F(4x4)): fewer than one
16-tile K-step, and tile counts whose last split is ragged."""
import ctypes

import numpy as np
import pytest

from oracle import unet_oracle as O
from oracle import fixtures as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHANNELS = [(64, 64), (64, 128), (128, 128)]        # (Co, Ci)
GRIDS = [(1, 14, 14), (1, 40, 40), (2, 52, 46)]     # (n, h, w) of the input


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib.load()


_CASES = {}


def _case(n, h, w, ci, co):
    """Inputs (shared by the tests of a shape, never modified) and the fp64
    correlation, computed once."""
    key = (n, h, w, ci, co)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * h + ci + co)
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        dy = rng.standard_normal((n, h - 2, w - 2, co)).astype(np.float32)
        wt = np.zeros((co, ci, 3, 3))
        _, rdw, _ = O.conv_valid_bwd(x.astype(np.float64), wt, dy.astype(np.float64), need_dx=False)
        _CASES[key] = (x, dy, rdw)
    return _CASES[key]


def _wgrad(lib, x, dy, ci, co, variant, plane):
    from unet_amd import _lib
    n, h, w, _ = x.shape
    xd, dyd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    dw = torch.empty((co, ci, 3, 3), device="cuda")
    db = torch.empty(co, device="cuda")
    ws = torch.empty(lib.unet_conv_ws_bytes(n, h, w, ci, co), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.unet_set_tuning(b"wgrad_variant", variant)
    lib.unet_set_tuning(b"wgrad_plane", plane)
    try:
        _lib.check(lib.unet_conv3x3_wgrad(xd.data_ptr(), dyd.data_ptr(), n, h, w, ci, co, dw.data_ptr(),
                                          db.data_ptr(), ws.data_ptr(), st), "wgrad")
        torch.cuda.synchronize()
    finally:
        lib.unet_set_tuning(b"wgrad_plane", 1)
        lib.unet_set_tuning(b"wgrad_variant", -1)
    return dw.cpu()


def _rel(a, ref):
    return float(np.abs(a.double().numpy() - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("variant", [1074, 1071])
@pytest.mark.parametrize("n,h,w", GRIDS)
@pytest.mark.parametrize("co,ci", CHANNELS)
def test_wgrad_plane_bit_identical(lib, co, ci, n, h, w, variant):
    """Slab mode (1000 + the Winograd tile: plain-store partials, fixed-order
    reduction): the ring kernel and k_wgrad give the same bits."""
    x, dy, rdw = _case(n, h, w, ci, co)
    old = _wgrad(lib, x, dy, ci, co, variant, 0)
    new = _wgrad(lib, x, dy, ci, co, variant, 1)
    assert _rel(old, rdw) < 1e-3  # sanity only: a wrong gradient is off by O(1)
    assert torch.equal(old, new), f"max |diff| {float((old - new).abs().max()):.3e}"


@pytest.mark.parametrize("variant", [74, 71])
@pytest.mark.parametrize("n,h,w", GRIDS)
@pytest.mark.parametrize("co,ci", CHANNELS)
def test_wgrad_plane_atomic_vs_fp64(lib, co, ci, n, h, w, variant):
    """Atomic accumulation (not reproducible run to run): each path against the
    fp64 correlation; the ring kernel gets 2x the measured error of k_wgrad."""
    x, dy, rdw = _case(n, h, w, ci, co)
    e_old = _rel(_wgrad(lib, x, dy, ci, co, variant, 0), rdw)
    e_new = _rel(_wgrad(lib, x, dy, ci, co, variant, 1), rdw)
    print(f"wgrad{variant} Co={co} Ci={ci} grid={n}x{h}x{w}: rel err k_wgrad {e_old:.3e}, k_wgrad_plane {e_new:.3e}")
    assert e_old < 1e-3  # sanity only: a wrong gradient is off by O(1)
    assert e_new <= 2 * e_old


def _atomic_leaf(name):
    # weight gradients that keep fp32 atomics under wgrad_variant 1074 (the
    # ConvTranspose2d layers and inc.c0): neither is a Winograd tile, both keep
    # the permute, and two identical steps already differ in them
    return ".up.weight" in name or name == "inc.double_conv.0.weight"


def _step(params, x, tgt, wmap):
    from unet_amd import UNet, WeightedCrossEntropyLoss
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.cuda().train()
    logits = m(torch.from_numpy(x).cuda())
    loss = WeightedCrossEntropyLoss()(logits, torch.from_numpy(tgt).cuda(), torch.from_numpy(wmap).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}


def test_train_step_oihw_and_plane_bit_identical(lib):
    """One 2 x 188^2 fp32 train step with every 3x3 weight gradient forced to
    F(6x6) in slab mode (point GEMMs of up to 8 pixel splits, summed by the
    slab reduction): the packed [co][tap][ci] store followed by k_permute_slab
    on k_wgrad (wgrad_oihw 0, wgrad_plane 0; twice), the same on k_wgrad_plane,
    and the defaults (the output transform stores torch's OIHW gradient itself).
    Same values, other kernels and addresses: every parameter gradient is
    bit-equal, except that the leaves whose kernels keep atomics are held to
    the run-to-run noise of the two identical steps."""
    params = O.hash_init(1, 2, seed=51, bn_random=True)
    x, tgt, wmap = F.make_inputs(51, 2, 1, 188, 188)
    runs, sites = [], []
    lib.unet_tuning_reset()
    lib.unet_set_tuning(b"autotune", 0)
    lib.unet_set_tuning(b"wgrad_variant", 1074)
    try:
        for oihw, plane in ((0, 0), (0, 0), (0, 1), (1, 1)):
            lib.unet_set_tuning(b"wgrad_oihw", oihw)
            lib.unet_set_tuning(b"wgrad_plane", plane)
            lib.unet_wgrad_oihw_sites(1)
            runs.append(_step(params, x, tgt, wmap))
            sites.append(lib.unet_wgrad_oihw_sites(1))
    finally:
        lib.unet_set_tuning(b"wgrad_oihw", 1)
        lib.unet_set_tuning(b"wgrad_plane", 1)
        lib.unet_set_tuning(b"wgrad_variant", -1)
        lib.unet_set_tuning(b"autotune", 1)
        lib.unet_tuning_reset()
    # the direct store ran for every 3x3 layer after inc.c0 (17 layers), never when declined
    assert sites == [0, 0, 0, 17], sites
    (s0, g0), (_, g0b) = runs[:2]
    for what, (s1, g1) in (("k_wgrad_plane", runs[2]), ("k_wgrad_plane + OIHW store", runs[3])):
        assert torch.equal(s0, s1)
        for k in g0:
            if _atomic_leaf(k):
                a, b, c = (t.double() for t in (g0[k], g0b[k], g1[k]))
                nrm = a.norm().item() + 1e-30
                noise, diff = (b - a).norm().item() / nrm, (c - a).norm().item() / nrm
                assert diff <= 2 * noise + 1e-6, (what, k, diff, noise)
            else:
                assert torch.equal(g0[k], g0b[k]), f"{k}: the k_wgrad + permute step is not reproducible"
                assert torch.equal(g0[k], g1[k]), f"{k}: {what} and k_wgrad + permute gradients differ"
