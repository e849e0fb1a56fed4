"""Golden border-aware weight maps (unet_weight_map_border), from scipy.

scipy and numpy only (no reference import): for each label map L the objects
are its distinct non-zero ids, ``dist_l = distance_transform_edt(L != l)`` the
distance to object l (0 inside it), d1 <= d2 the two smallest dist_l per pixel
(one object: d2 = 0; none: d1 = d2 = 0, scripts/preprocess_data.py:56-64), and

    weight64 = float32(wc) + w0 * exp(-(d1 + d2)^2 / (2 (sigma^2 + 1e-8)))

with wc, w0 = 10 and sigma = 5 as preprocess_data.py:14-36.  Squared
distances are integers, stored as int32 (rounded squares of the transform);
weight64 is computed from sqrt of those integers, which is what the device
does.  Maps: the three ``hela_real.npz`` label maps and the synthetic cases of
``oracle.fixtures.weightmap_synthetic_cases``.  To stay well below the size
limit of a committed file, the 512 x 512 HeLa entries hold every pixel of d1sq
and d2sq as differences along the rows (``hela{i}/d1sq_dx``; ``squares()``
undoes it) and every ``HELA_ROW_STEP``-th row of the fp64 map
(``hela{i}/weight64_rows``); the test restates the other rows from the
integers with the same numpy expression (``weight64_from``).

Usage:  python tests/golden/make_golden_border.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

W0, SIGMA = 10.0, 5.0
HELA_ROW_STEP = 4


def squares(z, case):
    """(d1sq, d2sq) int32 of a fixture entry."""
    if f"{case}/d1sq" in z:
        return z[f"{case}/d1sq"], z[f"{case}/d2sq"]
    return tuple(np.cumsum(z[f"{case}/{k}_dx"], axis=1, dtype=np.int64).astype(np.int32) for k in ("d1sq", "d2sq"))


def two_nearest_sq(lab):
    """(d1sq, d2sq) int32 of one label map, by one scipy EDT per object."""
    from scipy.ndimage import distance_transform_edt
    ids = np.unique(lab[lab > 0])
    zero = np.zeros(lab.shape, np.int32)
    if len(ids) == 0:
        return zero, zero.copy()
    sq = np.stack([np.rint(distance_transform_edt(lab != l) ** 2).astype(np.int64) for l in ids], -1)
    if len(ids) == 1:
        return sq[..., 0].astype(np.int32), zero
    part = np.partition(sq, 1, axis=-1)
    return part[..., 0].astype(np.int32), part[..., 1].astype(np.int32)


def weight64_from(lab, d1sq, d2sq, w0=W0, sigma=SIGMA):
    """The fp64 map from the integer squared distances (numpy only)."""
    fg = lab > 0
    n_fg, total = int(fg.sum()), fg.size
    n_bg = total - n_fg
    wc_bg = 1.0 / (n_bg / total) if n_bg > 0 else 0.0
    wc_fg = 1.0 / (n_fg / total) if n_fg > 0 else 0.0
    wc = np.where(fg, np.float32(wc_fg), np.float32(wc_bg)).astype(np.float32)
    d = np.sqrt(d1sq.astype(np.float64)) + np.sqrt(d2sq.astype(np.float64))
    return wc.astype(np.float64) + w0 * np.exp(-(d ** 2) / (2 * (sigma ** 2 + 1e-8)))


def main():
    from oracle.fixtures import weightmap_synthetic_cases
    z = np.load(os.path.join(HERE, "hela_real.npz"), allow_pickle=False)
    out = {}
    for i in range(3):
        lab = z["segs"][i]
        d1, d2 = two_nearest_sq(lab)
        out[f"hela{i}/d1sq_dx"] = np.diff(d1, axis=1, prepend=0).astype(np.int32)
        out[f"hela{i}/d2sq_dx"] = np.diff(d2, axis=1, prepend=0).astype(np.int32)
        out[f"hela{i}/weight64_rows"] = weight64_from(lab, d1, d2)[::HELA_ROW_STEP]
    for k, lab in weightmap_synthetic_cases().items():
        d1, d2 = two_nearest_sq(lab)
        out[f"{k}/d1sq"], out[f"{k}/d2sq"] = d1, d2
        out[f"{k}/weight64"] = weight64_from(lab, d1, d2)
    path = os.path.join(HERE, "border_weightmap.npz")
    np.savez_compressed(path, **out)
    back = np.load(path, allow_pickle=False)
    for i in range(3):
        d1, d2 = squares(back, f"hela{i}")
        assert np.array_equal((d1, d2), two_nearest_sq(z["segs"][i]))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
