"""The oracle helpers behind tests/test_gpu_ops_elementwise.py (first conv from
NCHW, 1x1 head, BatchNorm(+ReLU) with free eps / momentum, eval-mode BatchNorm
backward) against torch.nn.functional under autograd, float64 on the CPU, two
small shapes each, 1e-12 of the reference's scale: the GPU tests compare
against the right thing."""
import numpy as np
import pytest

from oracle import unet_oracle as O

torch = pytest.importorskip("torch")
F = torch.nn.functional

BAR = 1e-12


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a, grad=False):
    # a copy: F.batch_norm updates its running buffers in place
    return torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(grad)


@pytest.mark.parametrize("n,ci,h,w", [(2, 3, 5, 7), (1, 5, 4, 9)])
def test_conv_first_vs_torch(n, ci, h, w):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, ci, h, w))
    wt = rng.standard_normal((64, ci, 3, 3))
    b = rng.standard_normal(64)
    dy = rng.standard_normal((n, h - 2, w - 2, 64))
    xt, wtt, bt = t64(x, True), t64(wt, True), t64(b, True)
    y = F.conv2d(xt, wtt, bt)
    y.backward(t64(dy).permute(0, 3, 1, 2))
    assert rel(O.conv_first_fwd(x, wt, b), y.detach().permute(0, 2, 3, 1).numpy()) < BAR
    dx, dw, db = O.conv_first_bwd(x, wt, dy)
    assert rel(dx, xt.grad.numpy()) < BAR and rel(dw, wtt.grad.numpy()) < BAR and rel(db, bt.grad.numpy()) < BAR
    dx0, dw0, db0 = O.conv_first_bwd(x, wt, dy, need_dx=False)
    assert dx0 is None and np.array_equal(dw0, dw) and np.array_equal(db0, db)


@pytest.mark.parametrize("n,h,w,k", [(2, 3, 5, 3), (1, 4, 2, 37)])
def test_conv1x1_vs_torch(n, h, w, k):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, h, w, 64))
    wt = rng.standard_normal((k, 64))
    b = rng.standard_normal(k)
    dl = rng.standard_normal((n, k, h, w))
    xt, wtt, bt = t64(x, True), t64(wt, True), t64(b, True)
    y = F.conv2d(xt.permute(0, 3, 1, 2), wtt[:, :, None, None], bt)
    y.backward(t64(dl))
    assert rel(O.conv1x1_fwd(x, wt, b), y.detach().numpy()) < BAR
    dx, dw, db = O.conv1x1_bwd(x, wt, dl)
    assert rel(dx, xt.grad.numpy()) < BAR and rel(dw, wtt.grad.numpy()) < BAR and rel(db, bt.grad.numpy()) < BAR


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n,h,w,c,momentum,eps", [(2, 3, 5, 8, 0.3, 1e-3), (1, 1, 3, 4, 0.1, 1e-5)])
def test_bn_relu_vs_torch(n, h, w, c, momentum, eps, relu, training):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n, h, w, c)) * 2 + 1
    g = rng.uniform(0.5, 1.5, c)
    b = rng.standard_normal(c)
    rm0 = rng.standard_normal(c)
    rv0 = rng.uniform(0.5, 2.0, c)
    dy = rng.standard_normal(x.shape)
    xt, gt, bt = t64(x, True), t64(g, True), t64(b, True)
    rmt, rvt = t64(rm0), t64(rv0)
    z = F.batch_norm(xt.permute(0, 3, 1, 2), rmt, rvt, gt, bt, training=training, momentum=momentum, eps=eps)
    yt = F.relu(z) if relu else z
    yt.backward(t64(dy).permute(0, 3, 1, 2))
    y, cache, mean, invstd, rm, rv = O.bn_relu_fwd(x, g, b, rm0, rv0, training, relu, momentum, eps)
    assert rel(y, yt.detach().permute(0, 2, 3, 1).numpy()) < BAR
    assert rel(rm, rmt.numpy()) < BAR and rel(rv, rvt.numpy()) < BAR
    if training:
        xf = x.reshape(-1, c)
        assert rel(mean, xf.mean(0)) < BAR and rel(invstd, 1 / np.sqrt(xf.var(0) + eps)) < BAR
    else:
        assert np.array_equal(rm, rm0) and np.array_equal(rv, rv0) and np.array_equal(mean, rm0)
        assert rel(invstd, 1 / np.sqrt(rv0 + eps)) < BAR
    dx, dg, db = O.bn_relu_bwd(dy, y, cache, g, training, relu)
    assert rel(dx, xt.grad.numpy()) < BAR and rel(dg, gt.grad.numpy()) < BAR and rel(db, bt.grad.numpy()) < BAR


@pytest.mark.parametrize("n,h,w,c", [(2, 3, 5, 8), (1, 2, 2, 4)])
def test_bn_eval_bwd_vs_torch(n, h, w, c):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, h, w, c)) * 2 + 1
    g = rng.uniform(0.5, 1.5, c)
    rm = rng.standard_normal(c)
    rv = rng.uniform(0.5, 2.0, c)
    dz = rng.standard_normal(x.shape)
    xt, gt, bt = t64(x, True), t64(g, True), t64(np.zeros(c), True)
    z = F.batch_norm(xt.permute(0, 3, 1, 2), t64(rm), t64(rv), gt, bt, training=False, eps=1e-3)
    z.backward(t64(dz).permute(0, 3, 1, 2))
    dx, dg, db = O.bn_eval_bwd(dz, x, g, rm, rv, 1e-3)
    assert rel(dx, xt.grad.numpy()) < BAR and rel(dg, gt.grad.numpy()) < BAR and rel(db, bt.grad.numpy()) < BAR
