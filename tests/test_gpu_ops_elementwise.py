"""Per-element parity of the memory-bound stage kernels (csrc/elementwise.hip)
through their C entry points (include/unet_hip.h), against the float64 oracle
(oracle/unet_oracle.py): error = max |got - ref| / max |ref|, at the bars the
project already uses for the same arithmetic (2e-5 direct fp32 conv; 1e-5 /
1e-4 BatchNorm; 1e-5 loss).

Every output and workspace is a slice of a larger allocation with a 256-byte
guard of 0xA5 on either side (`G`).  Outputs and workspaces start as 0xFF bytes
(a NaN as fp32 / fp64), workspaces have exactly the size the *_ws_bytes function
returns (unet_wce_fwd_bwd: the documented 64 x 8 bytes).  `done()` requires
every output element finite (it was written) and every guard intact (nothing
was written outside; the workspace size suffices).

Case -> seam of elementwise.hip it crosses

  test_conv_first_fwd
    ci 1 2 3 4                     k_conv_first_fwd<1..4>
    ci 5 / 16 / 17 / 20            k_conv_first_fwd_gen: partial chunk / full
                                   kFirstChunk / full + 1 / full + 4
    w 3 / 65 / 66 / 67 / 132       wo 1, 63, 64, 65 (2nd segment of one
                                   column), 130 (3 segments, ragged last);
                                   clamped halo loads of the last segment
  test_conv_first_bwd
    ci 1 3 4 5 7 9                 passes of <= 4 channels: 1, 3, 4, 4+1, 4+3,
                                   4+4+1 (reduce_first_slabs column offsets)
    ho 1 2 3 4 5 6                 ragged / full / full + ragged 4-row strips
    (1, 262, 3)  65 items          k_reduce_slabs: two chunks of slabs, 64 + 1
    (3, 2802, 3) 2100 items        > kFirstWgradSlabs: workgroups loop
    deterministic 0 / 1            chunked slab reduction / one pass, bit-equal
    dx / NULL                      k_conv_first_dgrad present or skipped
  test_conv1x1_fwd
    k 1 2 3 4 / 5 8 / 9 16         k_head_fwd<1,2,3,4> / <8> / <16>
    k 17 / 21 / 33 / 70            2nd pass of capacity 1 / 8, three passes
                                   (16+16+1), five passes (koff 0..64)
    pixels 15, 126, 64             16-pixel block groups, ragged and exact
  test_conv1x1_bwd
    k 1 2 31 32 / 33 70            one slice of k_head_bwd<32,0,0,0> / 2 and 3
                                   slices (koff 32, 64); k_head_bwd_dz's
                                   run-time class loop
    (1, 260, 260)                  67600 pixels > 512 blocks x 128: grid cap
    dx / NULL                      k_head_bwd_dz present or skipped
  test_bn_relu
    c 4 8 64 256 1024              256, 128, 16, 4, 1 pixels per block
                                   (k_channel_stats, k_bn_bwd_stats)
    pixels 3 / 70 / 9017           fewer than a block's slots / ragged /
                                   4 grid passes with a ragged last one
    train / eval, relu on / off    k_bn_finalize / k_bn_eval_prepare +
                                   k_bn_eval_stats; k_relu_mask; k_bnb_finalize
                                   eval
  test_bn_relu_special_channels    all-closed masks, variance 0
  test_bn_relu_rejects             -EINVAL paths
  test_wce
    k 1 2 3 4 / 5 8 / 9 16 / 17 32 k_wce<1,2,3,4> / <8> / <16> / <32>
    k 33 40                        k_wce_gen
    strides                        cropped, transposed, batch-inner views
  test_wce_large_logits            max subtraction
  test_wce_ignored_and_bad_labels  -100, [k, capacity), >= capacity, -1
  test_scale_by_device_scalar      n 1, 255, 256, 1000003 (grid-stride tail)
  test_maxpool_small               c 4 / 64, dropped row / column, first max
  test_sgd_tails                   n 1 3 4 1023: float4 body + scalar tail
"""
import ctypes
import errno

import numpy as np
import pytest

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib.load()


from guarded import G, ws_buf, done, dev, stream, begin, release, _KEEP  # noqa: E402  (the guarded buffers, shared)


@pytest.fixture(autouse=True)
def _release():
    begin()
    yield
    release()


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def ck(rc):
    from unet_amd import _lib
    _lib.check(rc, "op")


class Worst:
    """Collects error / bar ratios; asserts each, prints the worst."""

    def __init__(self):
        self.r, self.what = 0.0, ""

    def add(self, what, got, ref, bar):
        e = rel_err(got, ref)
        if e / bar >= self.r:
            self.r, self.what = e / bar, what
        assert e < bar, f"{what}: {e:.3e} >= {bar:.1e}"

    def show(self):
        print(f"worst error / bar: {self.r:.3f} ({self.what})")


def f32(a):
    """The fp32 values the device sees, as float64 for the oracle."""
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------
# first conv
# ---------------------------------------------------------------------------
S1, S63, S64, S65, S130 = (1, 3, 3), (2, 5, 65), (1, 4, 66), (3, 6, 67), (1, 7, 132)
FIRST_FWD = ([(1, s) for s in (S1, S63, S64, S65, S130)]
             + [(2, S65), (3, S130), (4, S63), (2, S64),
                (5, S1), (5, S130), (16, S63), (17, S64), (17, S130), (20, S65), (16, S1)])


@pytest.mark.parametrize("ci,shape", FIRST_FWD, ids=lambda v: str(v).replace(" ", ""))
def test_conv_first_fwd(lib, ci, shape):
    n, h, w = shape
    rng = np.random.default_rng(100 + ci)
    x = f32(rng.standard_normal((n, ci, h, w)))
    wt = f32(rng.standard_normal((64, ci, 3, 3)) / np.sqrt(9 * ci))
    b = f32(rng.standard_normal(64))
    ref = O.conv_first_fwd(x, wt, b)
    y = G((n, h - 2, w - 2, 64))
    ck(lib.unet_conv_first_fwd(dev(x).data_ptr(), n, ci, h, w, dev(wt).data_ptr(), dev(b).data_ptr(), y.ptr, stream()))
    done()
    wr = Worst()
    wr.add("y", y.f64(), ref, 2e-5)
    wr.show()


def _first_bwd(lib, x, wt, dy, with_dx):
    n, ci, h, w = x.shape
    dx = G((n, ci, h, w)) if with_dx else None
    dw = G((64, ci, 3, 3))
    db = G(64)
    ws = ws_buf(lib.unet_conv_first_ws_bytes(n, ci, h, w))
    ck(lib.unet_conv_first_bwd(dev(x).data_ptr(), dev(dy).data_ptr(), n, ci, h, w, dev(wt).data_ptr(),
                               dx.ptr if with_dx else None, dw.ptr, db.ptr, ws.ptr, stream()))
    done()
    return (dx.f64() if with_dx else None), dw.np(), db.np()


def _first_bwd_case(lib, ci, shape, det, seed):
    n, h, w = shape
    rng = np.random.default_rng(seed)
    x = f32(rng.standard_normal((n, ci, h, w)))
    wt = f32(rng.standard_normal((64, ci, 3, 3)) / np.sqrt(9 * ci))
    dy = f32(rng.standard_normal((n, h - 2, w - 2, 64)))
    rdx, rdw, rdb = O.conv_first_bwd(x, wt, dy)
    wr = Worst()
    lib.unet_set_tuning(b"deterministic", det)
    try:
        dx, dw, db = _first_bwd(lib, x, wt, dy, True)
        _, dw0, db0 = _first_bwd(lib, x, wt, dy, False)
        if det:
            _, dw1, db1 = _first_bwd(lib, x, wt, dy, True)
    finally:
        lib.unet_set_tuning(b"deterministic", 0)
    wr.add("dx", dx, rdx, 2e-5)
    for tag, a, bb in (("dx", dw, db), ("NULL", dw0, db0)):
        wr.add(f"dW ({tag})", a.astype(np.float64), rdw, 2e-5)
        wr.add(f"db ({tag})", bb.astype(np.float64), rdb, 2e-5)
    if det:  # bit-reproducible: call to call, and with or without dx
        assert np.array_equal(dw, dw1) and np.array_equal(db, db1)
        assert np.array_equal(dw, dw0) and np.array_equal(db, db0)
    wr.show()


FIRST_BWD = [(1, S1), (3, S63), (4, S64), (5, S65), (7, S130), (9, (2, 8, 5)), (1, S130), (5, S1), (9, S63),
             (3, (1, 7, 70)), (7, S64), (4, S65)]


@pytest.mark.parametrize("det", [0, 1], ids=["chunked", "det"])
@pytest.mark.parametrize("ci,shape", FIRST_BWD, ids=lambda v: str(v).replace(" ", ""))
def test_conv_first_bwd(lib, ci, shape, det):
    _first_bwd_case(lib, ci, shape, det, 200 + ci)


@pytest.mark.parametrize("det", [0, 1], ids=["chunked", "det"])
@pytest.mark.parametrize("ci,shape,items", [(5, (1, 262, 3), 65), (1, (3, 2802, 3), 2100)])
def test_conv_first_bwd_many_items(lib, ci, shape, items, det):
    """Tall, narrow images: 65 work items (slab reduction in two chunks, 64 + 1)
    and 2100 (> kFirstWgradSlabs = 2048: workgroups walk several items)."""
    n, h, w = shape
    assert n * -(-(h - 2) // 4) * -(-(w - 2) // 64) == items
    _first_bwd_case(lib, ci, shape, det, 300 + ci)


# ---------------------------------------------------------------------------
# 1x1 head
# ---------------------------------------------------------------------------
PIX = [(1, 3, 5), (2, 7, 9), (1, 8, 8)]


def _head_params(rng, k):
    # every class row distinct, O(1) apart: a logit from the wrong row, plane
    # or pass is O(1) off
    wt = f32(rng.standard_normal((k, 64)) / 8 + np.linspace(-1, 1, k)[:, None] * ((np.arange(64) % 3) - 1) / 8)
    b = f32(np.arange(k) + 1 + rng.uniform(0, 0.5, k))
    return wt, b


@pytest.mark.parametrize("shape", PIX, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16, 17, 21, 32, 33, 70])
def test_conv1x1_fwd(lib, k, shape):
    n, h, w = shape
    rng = np.random.default_rng(400 + k)
    x = f32(rng.standard_normal((n, h, w, 64)))
    wt, b = _head_params(rng, k)
    ref = O.conv1x1_fwd(x, wt, b)
    lg = G((n, k, h, w))
    ck(lib.unet_conv1x1_fwd(dev(x).data_ptr(), n, h, w, 64, dev(wt).data_ptr(), dev(b).data_ptr(), k, lg.ptr,
                            stream()))
    done()
    wr = Worst()
    wr.add("logits", lg.f64(), ref, 2e-5)
    wr.show()


@pytest.mark.parametrize("with_dx", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("k,shape", [(k, s) for k in (1, 2, 31, 32, 33, 70) for s in PIX] + [(3, (1, 260, 260))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_conv1x1_bwd(lib, k, shape, with_dx):
    n, h, w = shape
    rng = np.random.default_rng(500 + k)
    x = f32(rng.standard_normal((n, h, w, 64)))
    wt, _ = _head_params(rng, k)
    dl = f32(rng.standard_normal((n, k, h, w)))
    rdx, rdw, rdb = O.conv1x1_bwd(x, wt, dl)
    dx = G((n, h, w, 64)) if with_dx else None
    dw = G((k, 64))
    db = G(k)
    ws = ws_buf(lib.unet_conv1x1_ws_bytes(k))
    ck(lib.unet_conv1x1_bwd(dev(x).data_ptr(), dev(dl).data_ptr(), n, h, w, 64, dev(wt).data_ptr(), k,
                            dx.ptr if with_dx else None, dw.ptr, db.ptr, ws.ptr, stream()))
    done()
    wr = Worst()
    if with_dx:
        wr.add("dx", dx.f64(), rdx, 2e-5)
    wr.add("dW", dw.f64(), rdw, 2e-5)
    wr.add("db", db.f64(), rdb, 2e-5)
    wr.show()


# ---------------------------------------------------------------------------
# BatchNorm (+ ReLU)
# ---------------------------------------------------------------------------
def _stats_grid(pixels, c):
    """launch_channel_stats: blocks and pixels per grid pass."""
    ppb = 256 // (c // 4)
    grid = min(max(-(-pixels // (ppb * 4)), 1), 2048)   # grid_cap(pixels, ppb * 4, 2048)
    return grid, grid * ppb


BIG = (1, 71, 127)  # 9017 pixels
BN_CASES = [(c, s) for c in (4, 8, 64, 256, 1024) for s in ((1, 1, 3), (1, 1, 70), (2, 5, 7))] + [(4, BIG), (64, BIG)]


def _bn_run(lib, x, g, b, rm0, rv0, dy, training, relu, momentum, eps, with_nbt):
    n, h, w, c = x.shape
    ws = ws_buf(lib.unet_bn_relu_ws_bytes(n, h, w, c))
    y, sm, si = G(x.shape), G(c), G(c)
    rm, rv = G(c, init=rm0), G(c, init=rv0)
    nbt = G(1, np.int64, init=[41]) if with_nbt else None
    xd, gd = dev(x), dev(g)
    ck(lib.unet_bn_relu_fwd(xd.data_ptr(), n, h, w, c, gd.data_ptr(), dev(b).data_ptr(), rm.ptr, rv.ptr,
                            nbt.ptr if with_nbt else None, ctypes.c_float(momentum), ctypes.c_float(eps),
                            int(training), int(relu), y.ptr, sm.ptr, si.ptr, ws.ptr, stream()))
    dx, dg, dbt = G(x.shape), G(c), G(c)
    ck(lib.unet_bn_relu_bwd(xd.data_ptr(), y.ptr, dev(dy).data_ptr(), n, h, w, c, gd.data_ptr(), sm.ptr, si.ptr,
                            int(training), int(relu), dx.ptr, dg.ptr, dbt.ptr, ws.ptr, stream()))
    done()
    return dict(y=y.f64(), mean=sm.f64(), invstd=si.f64(), rm=rm.np(), rv=rv.np(),
                nbt=int(nbt.np()[0]) if with_nbt else None, dx=dx.f64(), dgamma=dg.f64(), dbeta=dbt.f64())


def _bn_compare(out, x, g, b, rm0, rv0, dy, training, relu, momentum, eps, with_nbt, wr):
    ry, cache, rmean, rinv, rrm, rrv = O.bn_relu_fwd(x, g, b, rm0, rv0, training, relu, momentum, eps)
    rdx, rdg, rdb = O.bn_relu_bwd(dy, ry, cache, g, training, relu)
    wr.add("y", out["y"], ry, 1e-5)
    wr.add("save_mean", out["mean"], rmean, 1e-5)
    wr.add("save_invstd", out["invstd"], rinv, 1e-5)
    if training:
        wr.add("running_mean", out["rm"], rrm, 1e-5)
        wr.add("running_var", out["rv"], rrv, 1e-5)
    else:  # eval leaves the buffers alone
        assert np.array_equal(out["rm"], rm0.astype(np.float32)) and np.array_equal(out["rv"], rv0.astype(np.float32))
    if with_nbt:
        assert out["nbt"] == (42 if training else 41)
    wr.add("dx", out["dx"], rdx, 1e-4)
    wr.add("dgamma", out["dgamma"], rdg, 1e-5)
    wr.add("dbeta", out["dbeta"], rdb, 1e-5)


@pytest.mark.parametrize("training,relu", [(1, 1), (1, 0), (0, 1), (0, 0)], ids=["train-relu", "train", "eval-relu", "eval"])
@pytest.mark.parametrize("c,shape", BN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bn_relu(lib, c, shape, training, relu):
    """The 3-pixel training cases are the ones that found k_channel_stats' fp32
    partial sums: with the variance formed as E[x^2] - mean^2, a channel whose
    three samples lie close together (variance 1e-3 of mean^2) had save_invstd
    3.5e-5 and y up to 5.3e-5 off (bars 1e-5).  With fp64 partials the worst
    error of this test is 0.06 of its bar."""
    n, h, w = shape
    pixels = n * h * w
    if shape == BIG:  # several grid passes of the statistics kernels, the last one ragged
        _, per_pass = _stats_grid(pixels, c)
        assert pixels > 3 * per_pass and pixels % per_pass
    custom = c in (8, 256) or shape == BIG   # momentum 0.3, eps 1e-3 (the defaults elsewhere)
    momentum, eps = (0.3, 1e-3) if custom else (0.1, 1e-5)
    with_nbt = c != 8
    rng = np.random.default_rng(600 + c + pixels)
    x = f32(rng.standard_normal((n, h, w, c)) * 2 + 1)
    g = f32(rng.uniform(0.5, 1.5, c))
    b = f32(rng.standard_normal(c))
    rm0 = f32(rng.standard_normal(c))
    rv0 = f32(rng.uniform(0.5, 2.0, c))
    dy = f32(rng.standard_normal(x.shape))
    out = _bn_run(lib, x, g, b, rm0, rv0, dy, training, relu, momentum, eps, with_nbt)
    wr = Worst()
    _bn_compare(out, x, g, b, rm0, rv0, dy, training, relu, momentum, eps, with_nbt, wr)
    wr.show()


def test_bn_relu_special_channels(lib):
    """c = 64, train, relu.  Channel 0: gamma = beta = 0 (y exactly 0, mask
    all-closed, dx exactly 0); channel 1: beta so negative that every element
    is masked; channel 2: a constant input (1.5, exact in the fp32 partial
    sums): variance 0, invstd = 1 / sqrt(eps)."""
    n, h, w, c = 2, 5, 7, 64
    eps = 1e-5
    rng = np.random.default_rng(700)
    x = f32(rng.standard_normal((n, h, w, c)) * 2 + 1)
    x[..., 2] = 1.5
    g = f32(rng.uniform(0.5, 1.5, c))
    b = f32(rng.standard_normal(c))
    g[0] = b[0] = 0.0
    b[1] = -100.0
    b[2] = 0.75
    rm0, rv0 = np.zeros(c), np.ones(c)
    dy = f32(rng.standard_normal(x.shape))
    out = _bn_run(lib, x, g, b, rm0, rv0, dy, 1, 1, 0.1, eps, True)
    wr = Worst()
    _bn_compare(out, x, g, b, rm0, rv0, dy, 1, 1, 0.1, eps, True, wr)
    for ch in (0, 1):
        assert not out["y"][..., ch].any() and not out["dx"][..., ch].any()
        assert out["dgamma"][ch] == 0 and out["dbeta"][ch] == 0
    assert out["mean"][2] == 1.5
    assert abs(out["invstd"][2] * np.sqrt(eps) - 1) < 1e-5
    assert np.ptp(out["y"][..., 2]) == 0   # one value (beta, within y's bar above)
    assert abs(out["rv"][2] - 0.9) < 1e-6
    wr.show()


def test_bn_relu_rejects(lib):
    """c = 6 (not a multiple of 4), c = 12 (256 % 3 != 0) and eval mode without
    running statistics: -EINVAL, nothing written."""
    n, h, w = 1, 2, 2
    for c, training, have_running in ((6, 1, True), (12, 1, True), (8, 0, False)):
        x = dev(np.ones((n, h, w, c)))
        g, b = dev(np.ones(c)), dev(np.zeros(c))
        rm, rv = G(c, init=np.zeros(c), output=False), G(c, init=np.ones(c), output=False)
        y, sm, si = G((n, h, w, c), output=False), G(c, output=False), G(c, output=False)
        ws = ws_buf(1 << 16)
        rc = lib.unet_bn_relu_fwd(x.data_ptr(), n, h, w, c, g.data_ptr(), b.data_ptr(),
                                  rm.ptr if have_running else None, rv.ptr if have_running else None, None,
                                  ctypes.c_float(0.1), ctypes.c_float(1e-5), training, 1, y.ptr, sm.ptr, si.ptr, ws.ptr,
                                  stream())
        assert rc == -errno.EINVAL
        if c != 8:
            dx, dg, dbt = G((n, h, w, c), output=False), G(c, output=False), G(c, output=False)
            rc = lib.unet_bn_relu_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), n, h, w, c, g.data_ptr(), sm.ptr,
                                      si.ptr, 1, 1, dx.ptr, dg.ptr, dbt.ptr, ws.ptr, stream())
            assert rc == -errno.EINVAL
        torch.cuda.synchronize()
        assert np.isnan(y.np()).all() and np.isnan(sm.np()).all()
        done()


# ---------------------------------------------------------------------------
# weighted cross-entropy
# ---------------------------------------------------------------------------
def _strided(a, kind, dtype):
    """Device copy of a (n, h, w) viewed through non-contiguous element strides.
    0: contiguous; 1: centre crop of a larger (n, h + 4, w + 6) map; 2: stored
    transposed (n, w, h); 3: stored batch-inner (h, n, w)."""
    n, h, w = a.shape
    if kind == 0:
        t = dev(a, dtype)
    elif kind == 1:
        big = np.full((n, h + 4, w + 6), 7 if a.dtype.kind == "i" else 99.0, a.dtype)
        big[:, 2:2 + h, 3:3 + w] = a
        t = dev(big, dtype)[:, 2:2 + h, 3:3 + w]
    elif kind == 2:
        t = dev(a.transpose(0, 2, 1), dtype).permute(0, 2, 1)
    else:
        t = dev(a.transpose(1, 0, 2), dtype).permute(1, 0, 2)
    assert tuple(t.shape) == (n, h, w)
    _KEEP.append(t)
    return t


def _wce_run(lib, logits, tgt, wmap, tkind, wkind, gs):
    n, k, h, w = logits.shape
    td = _strided(tgt.astype(np.int64), tkind, torch.int64)
    wd = _strided(np.asarray(wmap, np.float32), wkind, torch.float32)
    ts = (ctypes.c_int64 * 3)(*td.stride())
    wsd = (ctypes.c_int64 * 3)(*wd.stride())
    loss, dl = G(1), G(logits.shape)
    ws = G(64, np.float64, output=False)
    ck(lib.unet_wce_fwd_bwd(dev(logits).data_ptr(), td.data_ptr(), wd.data_ptr(), n, k, h, w,
                            ctypes.cast(ts, ctypes.c_void_p), ctypes.cast(wsd, ctypes.c_void_p), loss.ptr, dl.ptr,
                            ctypes.c_float(gs), ws.ptr, stream()))
    done()
    return float(loss.np()[0]), dl.f64(), ws.np()


WCE_PIX = [(1, 1, 1), (1, 15, 17), (2, 20, 23)]


@pytest.mark.parametrize("shape", WCE_PIX, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40])
def test_wce(lib, k, shape):
    n, h, w = shape
    rng = np.random.default_rng(800 + k)
    logits = f32(rng.standard_normal((n, k, h, w)) * 3)
    tgt = rng.integers(0, k, (n, h, w))
    wmap = f32(rng.uniform(1, 13, (n, h, w)))
    gs = 0.37
    rloss, rdl = O.weighted_ce(logits, tgt, wmap)
    # targets and weights through different views; (2, 3): permutations of each other's strides
    tkind, wkind = [(1, 2), (2, 1), (3, 2), (2, 3), (1, 3), (0, 1)][k % 6]
    loss, dl, ws = _wce_run(lib, logits, tgt, wmap, tkind, wkind, gs)
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    wr = Worst()
    wr.add("dlogits", dl, np.float64(np.float32(gs)) * rdl, 1e-5)
    assert ws[1] == 0
    wr.show()


@pytest.mark.parametrize("tkind,wkind", [(2, 0), (0, 2), (2, 2)])
def test_wce_permuted_strides(lib, tkind, wkind):
    """A square map: the transposed view's strides (36, 1, 6) are a permutation
    of the contiguous ones (36, 6, 1); targets and weights each follow their own."""
    n, k, h, w = 2, 3, 6, 6
    rng = np.random.default_rng(850)
    logits = f32(rng.standard_normal((n, k, h, w)) * 3)
    tgt = rng.integers(0, k, (n, h, w))
    wmap = f32(rng.uniform(1, 13, (n, h, w)))
    rloss, rdl = O.weighted_ce(logits, tgt, wmap)
    loss, dl, _ = _wce_run(lib, logits, tgt, wmap, tkind, wkind, 2.0)
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    wr = Worst()
    wr.add("dlogits", dl, 2.0 * rdl, 1e-5)
    wr.show()


@pytest.mark.parametrize("k", [3, 8, 32, 33])
def test_wce_large_logits(lib, k):
    """Logits spread over +-60: exp(60) overflows nothing only because the
    maximum is subtracted first."""
    n, h, w = 1, 15, 17
    rng = np.random.default_rng(900 + k)
    logits = f32(rng.uniform(-60, 60, (n, k, h, w)))
    logits[0, 0, 0, 0], logits[0, k - 1, 0, 1] = 60.0, -60.0
    tgt = rng.integers(0, k, (n, h, w))
    wmap = f32(rng.uniform(1, 13, (n, h, w)))
    rloss, rdl = O.weighted_ce(logits, tgt, wmap)
    loss, dl, _ = _wce_run(lib, logits, tgt, wmap, 1, 2, 1.5)
    assert np.isfinite(loss) and abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    wr = Worst()
    wr.add("dlogits", dl, 1.5 * rdl, 1e-5)
    wr.show()


@pytest.mark.parametrize("k,inside,beyond", [(5, 6, 8), (33, 35, 1 << 40)])
def test_wce_ignored_and_bad_labels(lib, k, inside, beyond):
    """-100 (ignore_index), a label in [k, capacity) (6 of 8 at k = 5; k = 33
    runs the run-time class loop, which has no capacity: k + 2), one beyond
    every capacity, and -1: no loss, no gradient, still counted in the mean's
    denominator; the bad ones raise the flag."""
    n, h, w = 2, 20, 23
    rng = np.random.default_rng(1000 + k)
    logits = f32(rng.standard_normal((n, k, h, w)) * 3)
    tgt = rng.integers(0, k, (n, h, w))
    wmap = f32(rng.uniform(1, 13, (n, h, w)))
    where = [(0, 0, 0), (0, 19, 22), (1, 7, 11), (1, 19, 0), (0, 3, 3), (1, 0, 22)]
    for planted in ([-100, -100, inside, beyond, -1, inside], [-100] * 6):
        t = tgt.copy()
        wz = wmap.copy()
        for pos, lab in zip(where, planted):
            t[pos] = lab
            wz[pos] = 0.0   # oracle: out of the sum, still in the denominator
        rloss, rdl = O.weighted_ce(logits, np.where((t >= 0) & (t < k), t, 0), wz)
        loss, dl, ws = _wce_run(lib, logits, t, wmap, 2, 1, 0.37)
        assert np.isfinite(loss) and abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
        wr = Worst()
        wr.add("dlogits", dl, np.float64(np.float32(0.37)) * rdl, 1e-5)
        for pos in where:
            assert not dl[pos[0], :, pos[1], pos[2]].any()
        bad = sorted({v for v in planted if v != -100})
        if bad:
            assert ws[1] == 1 and ws[2] in bad, ws[:3]
        else:
            assert ws[1] == 0, ws[:3]
        wr.show()


# ---------------------------------------------------------------------------
# device-scalar scaling, max-pool, SGD
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 1000003])
def test_scale_by_device_scalar(lib, n):
    rng = np.random.default_rng(1100)
    x = rng.standard_normal(n).astype(np.float32)
    s = np.float32(0.3)
    ref = x * s
    g = dev(np.array([s]))
    inplace = G(n, init=x)
    ck(lib.unet_scale_by_device_scalar(inplace.ptr, n, g.data_ptr(), stream()))
    src = G(n, init=x)
    out = G(n)
    ck(lib.unet_scale_by_device_scalar_out(src.ptr, out.ptr, n, g.data_ptr(), stream()))
    a, b, c = inplace.np(), out.np(), src.np()
    done()
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(c.view(np.uint32), x.view(np.uint32))


def _pool_inputs(shape, c):
    n, h, w = shape
    rng = np.random.default_rng(1200 + c + h)
    yield "negative", -rng.integers(1, 6, (n, h, w, c)).astype(np.float64), None
    for j in range(4):  # the first maximum at window position j, ties behind it
        x = -rng.integers(2, 6, (n, h, w, c)).astype(np.float64)   # dropped row / column: anything
        for k in range(4):
            x[:, (k >> 1):2 * (h // 2):2, (k & 1):2 * (w // 2):2, :] = -9.0 if k < j else -1.0
        yield f"tie{j}", x, j


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 3, 3), (1, 9, 6)], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("c", [4, 64])
def test_maxpool_small(lib, c, shape):
    n, h, w = shape
    ho, wo = h // 2, w // 2
    for name, x, first in _pool_inputs(shape, c):
        ref, arg = O.maxpool2_fwd(x)
        assert (ref < 0).all() and (first is None or (arg == first).all())
        dy = np.random.default_rng(5).standard_normal(ref.shape).astype(np.float32)
        rdx = O.maxpool2_bwd(dy.astype(np.float64), arg, x.shape)
        y, a, dx = G(ref.shape), G(ref.shape, np.uint8), G(x.shape)
        ck(lib.unet_maxpool2_fwd(dev(x).data_ptr(), n, h, w, c, y.ptr, a.ptr, stream()))
        ck(lib.unet_maxpool2_bwd(dev(dy).data_ptr(), a.ptr, n, h, w, c, dx.ptr, stream()))
        got_y, got_a, got_dx = y.f64(), a.np(), dx.f64()
        done()   # dx finite everywhere: every element written
        np.testing.assert_array_equal(got_y, ref, err_msg=name)
        np.testing.assert_array_equal(got_a, arg, err_msg=name)
        np.testing.assert_array_equal(got_dx, rdx, err_msg=name)   # routing only: exact
        assert not got_dx[:, 2 * ho:, :, :].any() and not got_dx[:, :, 2 * wo:, :].any(), name


@pytest.mark.parametrize("n", [1, 3, 4, 1023])
def test_sgd_tails(lib, n):
    rng = np.random.default_rng(1300 + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    p = G(n, init=p0)
    buf = G(n, init=np.zeros(n))
    rp, rbuf = p0.astype(np.float64), None
    for s in range(3):
        g32 = rng.standard_normal(n).astype(np.float32)
        g = G(n, init=g32, output=False)
        ck(lib.unet_sgd_momentum(p.ptr, g.ptr, buf.ptr, n, ctypes.c_float(1e-4), ctypes.c_float(0.99),
                                 ctypes.c_float(0.5), int(s == 0), stream()))
        rp, rbuf = O.sgd_momentum_step(rp, g32.astype(np.float64) * 0.5, rbuf, 1e-4, 0.99)
        torch.cuda.synchronize()
        np.testing.assert_allclose(p.f64(), rp, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(buf.f64(), rbuf, rtol=1e-6, atol=1e-7)
    done()
