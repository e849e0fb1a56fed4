"""The GEMM-site oracles (oracle/unet_oracle.py site_*) equal the blocks they
restate, written out here from the primitives, and the Winograd restatement
equals the direct convolution in float64.  These are the references of
tests/test_gpu_gemm_sites.py; nothing here needs a GPU."""
import numpy as np
import pytest

from oracle import unet_oracle as O


def _rng_site(seed, n=2, h=5, w=7, ci=6, co=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h + 2, w + 2, ci))
    wt = rng.standard_normal((co, ci, 3, 3))
    b = rng.standard_normal(co)
    sc = rng.uniform(0.5, 1.5, ci) * rng.choice([-1.0, 1.0], ci)
    sh = 0.3 * rng.standard_normal(ci)
    return rng, x, wt, b, sc, sh


def test_site_f_plain_is_conv_of_relu_bn():
    _, x, wt, b, sc, sh = _rng_site(1)
    y, (s1, s2) = O.site_f_plain(x, sc, sh, wt, b)
    ref = O.conv_valid_fwd(O.relu_fwd(x * sc + sh), wt, b)
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12)
    # the sums are what bn_train_fwd's statistics are made of
    _, _, mean, var_unb = O.bn_train_fwd(ref, np.ones(5), np.zeros(5))
    m = ref.size // 5
    np.testing.assert_allclose(s1 / m, mean, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose((s2 / m - (s1 / m) ** 2) * m / (m - 1), var_unb, rtol=1e-11)
    y0, _ = O.site_f_plain(x, None, None, wt, b)
    np.testing.assert_allclose(y0, O.conv_valid_fwd(x, wt, b), rtol=0, atol=1e-12)


def test_site_f_cat_is_conv_of_cat_crop():
    rng, up, wt, b, _, _ = _rng_site(2, ci=4)
    n, hh, ww, _ = up.shape
    skip = rng.standard_normal((n, hh + 5, ww + 4, 3))
    sc = np.array([1.2, -0.7, 0.9])
    sh = np.array([0.1, 0.2, -0.4])
    wt = rng.standard_normal((5, 7, 3, 3))
    oy, ox = 2, 3
    y, (s1, s2) = O.site_f_cat(skip, sc, sh, oy, ox, up, wt, b)
    a = O.relu_fwd(skip * sc + sh)[:, oy:oy + hh, ox:ox + ww, :]
    ref = O.conv_valid_fwd(np.concatenate([a, up], -1), wt, b)
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s1, ref.reshape(-1, 5).sum(0), rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(s2, (ref ** 2).reshape(-1, 5).sum(0), rtol=1e-12)
    # a centred crop is center_crop_nhwc's
    skip2 = rng.standard_normal((n, hh + 4, ww + 6, 3))
    y2, _ = O.site_f_cat(skip2, None, None, 2, 3, up, wt, b)
    np.testing.assert_allclose(y2, O.conv_valid_fwd(np.concatenate([O.center_crop_nhwc(skip2, hh, ww), up], -1), wt, b),
                               rtol=0, atol=1e-12)
    # moving the origin by one pixel moves the result
    y3, _ = O.site_f_cat(skip, sc, sh, oy, ox - 1, up, wt, b)
    assert np.abs(y3 - y).max() > 0.1


def test_site_f_eval_is_relu_of_conv():
    _, x, wt, b, _, _ = _rng_site(3)
    np.testing.assert_allclose(O.site_f_eval(x, None, None, wt, b), O.relu_fwd(O.conv_valid_fwd(x, wt, b)),
                               rtol=0, atol=1e-12)


def test_site_d_pool_is_conv_bwd_dx():
    rng, x, wt, _, _, _ = _rng_site(4)
    n, hh, ww, _ = x.shape
    dy = rng.standard_normal((n, hh - 2, ww - 2, 5))
    dx, _, _ = O.conv_valid_bwd(x, wt, dy)
    got = O.site_d_pool(np.pad(dy, ((0, 0), (2, 2), (2, 2), (0, 0))), wt)
    np.testing.assert_allclose(got, dx, rtol=0, atol=1e-12)


def test_site_d_mask_is_relu_and_bn_backward():
    rng, x, wt, _, _, _ = _rng_site(5)
    n, hh, ww, ci = x.shape
    dy = rng.standard_normal((n, hh - 2, ww - 2, 5))
    dypad = np.pad(dy, ((0, 0), (2, 2), (2, 2), (0, 0)))
    yref = rng.standard_normal(x.shape)
    gamma, beta = rng.uniform(0.5, 1.5, ci) * np.array([1, -1, 1, 1, -1, 1]), 0.3 * rng.standard_normal(ci)
    z, cache, mean, _ = O.bn_train_fwd(yref, gamma, beta)
    invstd = cache[1]
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    dz, (b1, b2) = O.site_d_mask(dypad, wt, yref, scale, shift, mean, invstd)
    dx, _, _ = O.conv_valid_bwd(x, wt, dy)
    ref = O.relu_bwd(dx, O.relu_fwd(z))
    np.testing.assert_allclose(dz, ref, rtol=0, atol=1e-12)
    _, dgamma, dbeta = O.bn_train_bwd(ref, cache, gamma)
    np.testing.assert_allclose(b1, dbeta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b2, dgamma, rtol=1e-12, atol=1e-12)


def test_site_d_split_is_the_concat_split():
    rng, x, wt, _, _, _ = _rng_site(6)
    n, hh, ww, _ = x.shape
    dy = rng.standard_normal((n, hh - 2, ww - 2, 5))
    dx, _, _ = O.conv_valid_bwd(x, wt, dy)
    d0, d1, cs = O.site_d_split(np.pad(dy, ((0, 0), (2, 2), (2, 2), (0, 0))), wt, 2)
    np.testing.assert_allclose(d0, dx[..., :2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(d1, dx[..., 2:], rtol=0, atol=1e-12)
    # the second part's column sums: a ConvTranspose2d's bias gradient (convT2_bwd's db)
    np.testing.assert_allclose(cs, dx[..., 2:].sum((0, 1, 2)), rtol=1e-12, atol=1e-12)
    ev = np.ascontiguousarray(dx[:, :6, :8, 2:])
    np.testing.assert_allclose(O.site_d_split(np.pad(dy, ((0, 0), (2, 2), (2, 2), (0, 0)))[:, :8, :10], wt, 2)[2],
                               O.convT2_bwd(np.zeros((n, 3, 4, 3)), np.zeros((3, 4, 2, 2)), ev)[2],
                               rtol=1e-12, atol=1e-12)


def test_site_t_sites_are_convT():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3, 5, 6))
    wt = rng.standard_normal((6, 4, 2, 2))
    b = rng.standard_normal(4)
    assert np.array_equal(O.site_t_fwd(x, wt, b), O.convT2_fwd(x, wt, b))
    dy = rng.standard_normal((2, 6, 10, 4))
    yref = rng.standard_normal(x.shape)
    sc, sh = rng.uniform(0.5, 1.5, 6) * np.array([1, 1, -1, 1, -1, 1]), 0.3 * rng.standard_normal(6)
    mean, invstd = rng.standard_normal(6), rng.uniform(0.5, 2, 6)
    dz, (b1, b2) = O.site_t_mask(dy, wt, yref, sc, sh, mean, invstd)
    dx = O.convT2_bwd(x, wt, dy)[0]
    ref = O.relu_bwd(dx, O.relu_fwd(yref * sc + sh))
    assert np.array_equal(dz, ref)
    np.testing.assert_allclose(b1, ref.reshape(-1, 6).sum(0), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(b2, (ref * (yref - mean) * invstd).reshape(-1, 6).sum(0), rtol=1e-12, atol=1e-12)


def test_bn_relu_on_load_fma32_is_one_float32_rounding():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((1, 4, 4, 8)).astype(np.float32).astype(np.float64)
    sc = rng.standard_normal(8).astype(np.float32).astype(np.float64)
    sh = rng.standard_normal(8).astype(np.float32).astype(np.float64)
    got = O.bn_relu_on_load(x, sc, sh, fma32=True)
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
    assert np.abs(got - np.maximum(x * sc + sh, 0)).max() < 1e-6


# grids that are multiples of no tile size (every tile row and column overhangs),
# one that is a multiple of all, and one smaller than a tile
@pytest.mark.parametrize("m", [2, 4, 6])
@pytest.mark.parametrize("shape", [(2, 13, 19), (1, 12, 12), (3, 1, 5)])
def test_winograd_float64_equals_direct(m, shape):
    n, ho, wo = shape
    rng = np.random.default_rng(10 * m + ho)
    x = rng.standard_normal((n, ho + 2, wo + 2, 5))
    wt = rng.standard_normal((4, 5, 3, 3)) / np.sqrt(45)
    ref = O.conv_valid_fwd(x, wt, np.zeros(4))
    got = O.winograd_conv(x, wt, m, np.float64)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-12


@pytest.mark.parametrize("m", [2, 4, 6])
def test_winograd_float32_is_float32_and_close(m):
    rng = np.random.default_rng(m)
    x = rng.standard_normal((1, 9, 11, 16))
    wt = rng.standard_normal((8, 16, 3, 3)) / 12
    ref = O.conv_valid_fwd(x, wt, np.zeros(8))
    got = O.winograd_conv(x, wt, m)
    assert got.dtype == np.float32
    e = np.abs(got - ref).max() / np.abs(ref).max()
    assert 1e-9 < e < 1e-4   # fp32 rounding, not fp64 and not a wrong matrix


def test_winograd_through_a_site():
    _, x, wt, b, sc, sh = _rng_site(9)
    y, _ = O.site_f_plain(x, sc, sh, wt, b)
    yw, _ = O.site_f_plain(x, sc, sh, wt, b, conv=lambda a, w: O.winograd_conv(a, w, 4, np.float64))
    assert np.abs(y - yw).max() < 1e-11
