"""GPU marker-seeded instance masks (unet_split_instances,
unet_amd.postproc.split_instances) against the NumPy oracle
(tests/split_oracle.py): labels, info and d2 array-equal, with and without the
distance output (the row pass stops early when only the comparison with
core_d2 is needed)."""
import os

import numpy as np
import pytest

import split_oracle as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import postproc
    return postproc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(pp, mask, want, **kw):
    """with the distance (exact row pass) and without (thresholded row pass)"""
    markers = kw.pop("markers", None)
    if markers is not None:
        kw["markers"] = dev(markers)
    r = pp.split_instances(dev(mask), return_distance=True, **kw)
    np.testing.assert_array_equal(r.d2.cpu().numpy(), want["d2"])
    np.testing.assert_array_equal(r.info.cpu().numpy(), want["info"])
    np.testing.assert_array_equal(r.labels.cpu().numpy(), want["labels"])
    assert r.labels.dtype == torch.uint16 and r.info.dtype == torch.int32 and r.d2.dtype == torch.int32
    r = pp.split_instances(dev(mask), **kw)
    assert r.d2 is None
    np.testing.assert_array_equal(r.info.cpu().numpy(), want["info"])
    np.testing.assert_array_equal(r.labels.cpu().numpy(), want["labels"])
    return r


_WANT = {}


def stack_case(k, density):
    h, w = S.SHAPES[k]
    return S.random_stack(1000 * k + int(density * 10), 4, h, w, density)


def oracle_stack(k, density, core_d2, min_size):
    key = (k, density, core_d2, min_size)
    if key not in _WANT:
        _WANT[key] = S.split_stack(stack_case(k, density), core_d2, min_size=min_size)
    return _WANT[key]


@pytest.mark.parametrize("min_size", [1, 15])
@pytest.mark.parametrize("core_d2", [0, 2, 4, 9])
@pytest.mark.parametrize("density", [0.3, 0.5])
def test_shapes_vs_oracle(pp, density, core_d2, min_size):
    for k in range(len(S.SHAPES)):
        check(pp, stack_case(k, density), oracle_stack(k, density, core_d2, min_size), core_d2=core_d2,
              min_size=min_size)


def test_the_shape_cases_do_split():
    """The oracle alone: over the cases above it makes several hundred more
    segments than there are components, so they cannot silently stop splitting."""
    extra = 0
    for k in range(len(S.SHAPES)):
        for density in (0.3, 0.5):
            comps = sum(int(S.plain(m, 1).max()) for m in stack_case(k, density))
            for core_d2 in (0, 2, 4, 9):
                extra += int(oracle_stack(k, density, core_d2, 1)["info"][:, 1].sum()) - comps
    assert extra > 100


@pytest.mark.parametrize("shift", [0, 1])
def test_dumbbell(pp, shift):
    m = S.dumbbell(shift)
    want = S.split(m, 36, min_size=1)
    r = check(pp, m, want, core_d2=36, min_size=1)
    assert (int(r.markers), int(r.segments), bool(r.overflow)) == (2, 2, False)
    lab = r.labels.cpu().numpy()
    assert lab[15, 26:30].tolist() == ([1, 1, 2, 2] if shift == 0 else [1, 1, 1, 2])
    check(pp, m, want, core_radius=6, min_size=1)  # ceil(6^2)
    check(pp, m, S.split(m, 31, min_size=1), core_radius=5.5, min_size=1)  # ceil(30.25)


@pytest.mark.parametrize("core_d2", [0, 5, 1 << 30])
def test_all_foreground_and_all_background(pp, core_d2):
    fg = np.ones((2, 33, 70), np.uint8)
    want = S.split_stack(fg, core_d2, min_size=1)
    assert (want["d2"] == 1 << 30).all() and want["info"].tolist() == [[1, 1, 0, 0]] * 2
    check(pp, fg, want, core_d2=core_d2, min_size=1)
    bg = np.zeros((2, 33, 70), np.uint8)
    want = S.split_stack(bg, core_d2, min_size=1)
    assert not want["info"].any() and not want["labels"].any()
    check(pp, bg, want, core_d2=core_d2, min_size=1)
    mixed = np.concatenate([fg[:1], bg[:1], fg[:1]])  # frames do not leak into each other
    check(pp, mixed, S.split_stack(mixed, core_d2, min_size=1), core_d2=core_d2, min_size=1)


def snake(h, w, joined=False):
    """The serpentine of tests/test_gpu_warp.py: 1-pixel rows every fourth
    line with a two-pixel hook at alternating ends, plus specks; `joined` makes
    the hooks three pixels: one line of about h w / 4 pixels."""
    m = np.zeros((h, w), np.uint8)
    for y in range(0, h, 4):
        m[y, :] = 1
        if y + 2 < h:
            m[y + 1:y + (4 if joined else 3), (w - 1) if (y // 4) % 2 == 0 else 0] = 1
    m[2, 3] = m[h - 2, w // 2] = 1
    return m


@pytest.mark.parametrize("joined", [False, True])
def test_serpentine_converges(pp, joined):
    """One marker pixel at (0, 0): the label walks the whole line, a geodesic
    distance of about h w / 4 that no sweep covers in one go."""
    m = snake(64, 75, joined)
    mk = np.zeros_like(m)
    mk[0, 0] = 1
    want = S.split(m, markers=mk, min_size=1)
    if joined:
        # the line and the two specks; diagonal steps cut the corners of the 1247-pixel line
        assert want["info"].tolist() == [1, 3, 1216, 0] and 1216 > 64 * 75 // 4
    else:
        assert want["info"].tolist() == [1, 18, 75, 0]  # the first row and its hook; 17 pieces without a marker
    r = check(pp, m, want, markers=mk, min_size=1)
    assert int(r.levels) == want["info"][2]


def test_markers_argument(pp):
    m = stack_case(9, 0.5)
    g = np.random.default_rng(7)
    mk = (g.random(m.shape) < 0.01).astype(np.uint8) * 200
    assert (mk[m == 0] > 0).any() and (mk[m > 0] > 0).any()
    want = S.split_stack(m, markers=mk, min_size=3)
    assert want["info"][:, 0].min() > 3 and (want["info"][:, 1] > want["info"][:, 0]).any()  # unmarked components too
    check(pp, m, want, markers=mk, min_size=3)
    # markers outside the foreground are ignored
    inside = np.where(m > 0, mk, 0).astype(np.uint8)
    outside = np.where(m > 0, mk, 255).astype(np.uint8)
    check(pp, m, want, markers=inside, min_size=3)
    check(pp, m, want, markers=outside, min_size=3)
    # a bool mask and an (H, W) input
    r = pp.split_instances(dev(m[1] > 0), markers=dev(mk[1] > 0), min_size=3, return_distance=True)
    assert r.labels.shape == m[1].shape and r.info.shape == (4,) and r.d2.shape == m[1].shape
    np.testing.assert_array_equal(r.labels.cpu().numpy(), want["labels"][1])
    np.testing.assert_array_equal(r.info.cpu().numpy(), want["info"][1])


@pytest.fixture(scope="module")
def golden_masks():
    z = np.load(os.path.join(G, "hela_postproc.npz"), allow_pickle=False)
    t, h, w = (int(v) for v in z["mask_shape"])
    return (np.unpackbits(z["mask_bits"], axis=-1)[..., :w] * 255).astype(np.uint8), z["labels"], int(z["min_size"])


def test_core_zero_equals_instance_masks(pp, golden_masks):
    masks, labels, min_size = golden_masks
    d = dev(masks)
    r = pp.split_instances(d, core_d2=0, min_size=min_size)
    plain = pp.instance_masks(d, min_size=min_size)
    assert torch.equal(r.labels.view(torch.int16), plain.view(torch.int16))
    np.testing.assert_array_equal(r.labels.cpu().numpy(), labels)
    info = r.info.cpu().numpy()
    assert (info[:, 0] == info[:, 1]).all() and not info[:, 2:].any()


def test_hela_frames(pp):
    from unet_amd import ctc
    from test_split_cpu import HELA_PLAIN_COMPONENTS, HELA_SEGMENTS
    gt = np.load(os.path.join(G, "hela_real.npz"), allow_pickle=False)["segs"]
    m = (gt > 0).astype(np.uint8) * 255
    want = S.split_stack(m, 900, min_size=15)
    r = check(pp, m, want, core_d2=900, min_size=15)
    assert r.segments.tolist() == HELA_SEGMENTS and r.markers.tolist() == HELA_SEGMENTS
    for f in range(3):  # workgroups do not interfere, and SEG as the CPU test has it
        one = pp.split_instances(dev(m[f]), core_radius=30, min_size=15)
        np.testing.assert_array_equal(one.labels.cpu().numpy(), want["labels"][f])
        g = dev(gt[f:f + 1])
        seg = ctc.seg_measure(g, one.labels[None])
        plain = pp.instance_masks(dev(m[f:f + 1]), 15)
        assert int(plain.cpu().numpy().max()) == HELA_PLAIN_COMPONENTS[f]
        assert seg == pytest.approx(S.seg_measure(gt[f], want["labels"][f]), rel=1e-12, abs=0)
        assert seg > ctc.seg_measure(g, plain)


def test_result_does_not_depend_on_the_workgroup_size(pp):
    from unet_amd import _lib
    lib = _lib.load()
    m = np.concatenate([stack_case(9, 0.5), np.pad(snake(64, 75, True), ((0, 33), (0, 55)))[None]])
    mk = np.zeros_like(m)
    mk[:, 0, 0] = mk[:, 50, 60] = mk[:, 96, 129] = 1
    m[:, 0, 0] = 1
    want = S.split_stack(m, markers=mk, min_size=1)
    assert want["info"][4, 2] > 1000
    try:
        for threads in (64, 192, 1024):
            assert lib.unet_set_tuning(b"split_threads", threads) == 0
            check(pp, m, want, markers=mk, min_size=1)
            check(pp, stack_case(9, 0.5), oracle_stack(9, 0.5, 9, 15), core_d2=9, min_size=15)
    finally:
        assert lib.unet_set_tuning(b"split_threads", -1) == 0


def test_overflow_flag(pp):
    """More than 65535 markers and segments in a frame raise the flag (the
    labels are then unspecified); its neighbour frame is untouched.  The keys
    hold 32 bits of distance, so there is no saturation to reach."""
    m = np.zeros((2, 514, 514), np.uint8)
    m[0, ::2, ::2] = 1  # 257^2 = 66049 isolated pixels
    m[1, 10:20, 10:30] = 1
    want = S.split_stack(m, 0, min_size=1)
    assert want["info"].tolist() == [[66049, 66049, 0, 1], [1, 1, 0, 0]]
    r = pp.split_instances(dev(m), core_d2=0, min_size=1)
    np.testing.assert_array_equal(r.info.cpu().numpy(), want["info"])
    assert r.overflow.tolist() == [True, False]
    np.testing.assert_array_equal(r.labels[1].cpu().numpy(), want["labels"][1])


GUARD, PATTERN = 256, 0xA5


class Guarded:
    """exactly nbytes of 0xFF inside [guard | payload | guard] of 0xA5"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.raw[GUARD:GUARD + self.nbytes] = 0xFF
        self.ptr = self.raw.data_ptr() + GUARD

    def np(self, dtype, shape):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).reshape(shape)

    def intact(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.nbytes:] == PATTERN).all())


@pytest.mark.parametrize("shape", [(3, 37, 45), (2, 9, 33), (1, 97, 130)])
@pytest.mark.parametrize("with_d2", [False, True])
def test_outputs_and_workspace_stay_inside_their_buffers(pp, shape, with_d2):
    from unet_amd import _lib
    lib = _lib.load()
    n, h, w = shape
    m = S.random_stack(11, n, h, w, 0.5)
    want = S.split_stack(m, 4, min_size=2)
    mask = dev(m)
    need = lib.unet_split_instances_ws_bytes(n, h, w)
    assert need > 0 and need % 256 == 0
    ws, labels, info = Guarded(need), Guarded(n * h * w * 2), Guarded(n * 16)
    d2 = Guarded(n * h * w * 4) if with_d2 else None
    rc = lib.unet_split_instances(mask.data_ptr(), None, n, h, w, 4, 2, labels.ptr, d2.ptr if d2 else None, info.ptr,
                                  ws.ptr, _lib.stream_of())
    torch.cuda.synchronize()
    assert rc == 0
    for b in (ws, labels, info) + ((d2,) if d2 else ()):
        assert b.intact()
    np.testing.assert_array_equal(labels.np(np.uint16, shape), want["labels"])
    np.testing.assert_array_equal(info.np(np.int32, (n, 4)), want["info"])
    if d2:
        np.testing.assert_array_equal(d2.np(np.int32, shape), want["d2"])


def test_argument_checks(pp):
    from unet_amd import _lib
    lib = _lib.load()
    m = dev(S.dumbbell())
    for kw in ({}, {"core_radius": 3, "core_d2": 9}, {"core_d2": 9, "markers": m}, {"core_radius": 3, "markers": m},
               {"core_d2": -1}, {"core_d2": (1 << 30) + 1}, {"core_d2": 2.5}, {"core_radius": -1.0},
               {"core_d2": 4, "min_size": -1}, {"markers": m[:10]}, {"markers": m.cpu()}):
        with pytest.raises(ValueError):
            pp.split_instances(m, **kw)
    with pytest.raises(ValueError):
        pp.split_instances(m.cpu(), core_d2=4)
    with pytest.raises(ValueError):
        pp.split_instances(m[None, None], core_d2=4)
    with pytest.raises(ValueError):
        pp.split_instances(torch.zeros((1, 16385), dtype=torch.uint8, device="cuda"), core_d2=4)
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = out.data_ptr()
    for n, h, w, core_d2, min_size in ((0, 4, 4, 4, 1), (1, 16385, 1, 4, 1), (1, 1, 16385, 4, 1), (65536, 1, 1, 4, 1),
                                       (1, 4, 4, -1, 1), (1, 4, 4, (1 << 30) + 1, 1), (1, 4, 4, 4, -1)):
        assert lib.unet_split_instances(p, None, n, h, w, core_d2, min_size, p, None, p, p, None) == -22
    assert lib.unet_split_instances(p, None, 1, 4, 4, 4, 1, p, None, p, None, None) == -22
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched


def test_split_instances_tool(pp, tmp_path, capsys):
    """tools/split_instances.py: mask*.tif in, m*.tif uint16 out, numbered alike."""
    import importlib.util
    import json
    from PIL import Image
    masks = np.stack([S.dumbbell(), S.dumbbell(1), np.zeros((31, 56), np.uint8)]) * 255
    src, dst = tmp_path / "01_RES", tmp_path / "01_RES_INST"
    os.makedirs(src)
    for f, m in zip((0, 1, 7), masks):
        Image.fromarray(m).save(src / f"mask{f:03d}.tif")
    spec = importlib.util.spec_from_file_location(
        "split_instances_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "split_instances.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(["--masks", str(src), "--out", str(dst), "--core-radius", "6", "--min-size", "1"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == 3 and line["markers"] == [2, 2, 0] and line["segments"] == [2, 2, 0]
    assert sorted(os.listdir(dst)) == ["m000.tif", "m001.tif", "m007.tif"]
    for f, m in zip((0, 1, 7), masks):
        got = np.array(Image.open(dst / f"m{f:03d}.tif"))
        assert got.dtype == np.uint16
        np.testing.assert_array_equal(got, S.split(m, 36, min_size=1)["labels"])
    assert tool.main(["--masks", str(dst), "--out", str(dst), "--core-radius", "6"]) == 1  # no mask*.tif there
