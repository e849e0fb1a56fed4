"""The warped instance ids (unet_elastic_deform_ex / ElasticDeform(return_ids=True))
and the border-aware weight modes of HeLaBatches ("border", "border-warped")
down to one Trainer step; the two existing modes keep their results."""
import os

import numpy as np
import pytest

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def hela():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    z = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)
    return z["images"], z["segs"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _small_case():
    """A ragged 2 x 61 x 77 batch with ids beyond one byte (256 and 512 wrap
    to background in the reference's uint8 cast)."""
    g = np.random.default_rng(9)
    img = g.integers(0, 256, (2, 61, 77)).astype(np.uint8)
    lab = np.array([0, 1, 255, 256, 257, 512, 65535], np.uint16)[g.integers(0, 7, (2, 61, 77))]
    return torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), lab


def test_ids_with_zero_displacement(hela):
    from unet_amd.augment import ElasticDeform
    img, labd, lab = _small_case()
    noise = torch.full((2, 2, 61, 77), 0.5, dtype=torch.float64, device="cuda")
    x, t, ids = ElasticDeform(alpha=2000.0, sigma=4.0)(img, labd, noise=noise, return_ids=True)
    assert ids.dtype == torch.uint16 and ids.shape == (2, 61, 77)
    np.testing.assert_array_equal(ids.cpu().numpy(), np.where((lab & 0xff) != 0, lab, 0))
    np.testing.assert_array_equal(t.cpu().numpy()[:, 0], ((lab & 0xff) != 0).astype(np.uint8))


def test_ids_with_random_noise(hela):
    from unet_amd.augment import ElasticDeform
    img, labd, lab = _small_case()
    noise = torch.rand((2, 2, 61, 77), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    aug = ElasticDeform(alpha=300.0, sigma=4.0)
    x0, t0, i0 = aug(img, labd, noise=noise, return_image=True)
    x, t, im, ids = aug(img, labd, noise=noise, return_image=True, return_ids=True)
    for a, b in ((x0, x), (t0, t), (i0, im)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    idn, tn = ids.cpu().numpy(), t.cpu().numpy()[:, 0]
    np.testing.assert_array_equal(idn != 0, tn != 0)
    assert (idn != lab).any()                      # the field moved something
    for s in range(2):
        assert set(np.unique(idn[s])) <= set(np.unique(lab[s])) | {0}
    assert (idn & 0xff != 0).sum() == (idn != 0).sum()


def test_weight_modes_of_a_batch(hela):
    from unet_amd.augment import ElasticDeform, weight_maps
    from unet_amd.pipeline import HeLaBatches, center_crop_views
    imgs, labs = _dev(hela[0][:, :200, :232]), _dev(hela[1][:, :200, :232])
    out_hw, idx = (16, 48), [2, 0]
    noise = torch.rand((2, 2, 200, 232), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    sel = torch.tensor(idx, device="cuda")
    isel, lsel = imgs.index_select(0, sel), labs.index_select(0, sel)
    x, t8, ids = ElasticDeform(alpha=2000.0, sigma=20.0)(isel, lsel, noise=noise, return_ids=True)
    assert len(np.unique(ids[0].cpu().numpy())) > 2           # instance ids, not a binary mask

    def batch(mode, augment=True):
        data = HeLaBatches(imgs, labs, batch=2, out_hw=out_hw, augment=augment, weights=mode, shuffle=False)
        return data.make_batch(idx, noise=noise if augment else None)

    crop = lambda w: center_crop_views(w.unsqueeze(1), out_hw)  # noqa: E731
    xb, tb, wb = batch("border-warped")
    assert torch.equal(xb, x) and torch.equal(tb, center_crop_views(t8.to(torch.int64), out_hw))
    assert torch.equal(wb, crop(weight_maps(ids, mode="border")))
    assert not torch.equal(wb, crop(weight_maps(ids)))                                 # the border term is there
    assert torch.equal(batch("border")[2], crop(weight_maps(lsel, mode="border")))
    assert torch.equal(batch("border-warped", augment=False)[2], crop(weight_maps(lsel, mode="border")))
    # the existing modes: the reference-mode maps of the unwarped labels / of the warped binary target
    assert torch.equal(batch("static")[2], crop(weight_maps(lsel)))
    assert torch.equal(batch("warped")[2], crop(weight_maps(t8[:, 0].to(torch.int16).view(torch.uint16))))
    with pytest.raises(ValueError, match="border-warped"):
        HeLaBatches(imgs, labs, batch=2, out_hw=out_hw, weights="paper")


def test_trainer_step_from_border_warped_batch(hela):
    from unet_amd import UNet
    from unet_amd.pipeline import HeLaBatches
    from unet_amd.train import Trainer
    imgs, labs = _dev(hela[0][:2, 100:288, 100:288]), _dev(hela[1][:2, 100:288, 100:288])
    params = O.hash_init(1, 2, seed=11, bn_random=True)
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    tr = Trainer(m.cuda().train(), 2, 188, 188, lr=1e-4, momentum=0.99)
    data = HeLaBatches(imgs, labs, batch=2, out_hw=tr.out_hw, weights="border-warped", shuffle=False,
                       generator=torch.Generator("cuda").manual_seed(2))
    x, t, w = next(iter(data))
    assert x.shape == (2, 1, 188, 188) and t.shape == (2, 4, 4) and w.shape == (2, 4, 4)
    assert np.isfinite(float(tr.step(x, t, w).item()))
