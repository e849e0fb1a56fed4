"""CPU checks of the C-ABI library and the host-side plan logic (no GPU calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import unet_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _lib():
    from unet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libunet_hip.so not built (run __graft_entry__.build())")
    return _lib


def test_library_exports_every_header_symbol():
    L = _lib()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(unet_[A-Za-z0-9_]+)\s*\(", header))
    assert len(names) >= 25
    for n in sorted(names):
        assert hasattr(lib, n), f"missing export {n}"
    # and the binding declares exactly the header's functions
    assert names == set(L.SIGNATURES), names ^ set(L.SIGNATURES)
    assert b"gfx950" in lib.unet_version()


@pytest.mark.parametrize("h,out", [(512, 324), (572, 388), (188, 4), (204, 20), (508, 324)])
def test_plan_output_size_matches_reference_rule(h, out):
    from unet_amd.plan import Plan
    _lib()
    p = Plan(2, 1, h, h, 2)
    assert (p.out_h, p.out_w) == (out, out) == (O.output_size(h),) * 2
    assert p.workspace_bytes > 0


def test_tuning_db_roundtrip(tmp_path):
    """unet_tuning_load / _save (host-only: no GPU call): a database file is
    merged into the tuner's cache, reported, written back line for line."""
    L = _lib()
    lib = L.load()
    src = tmp_path / "tune.db"
    entries = {"igemm_bf16 M=8 N=64 K=576 Cg=64 taps=3x3 s=1 grid=4x4 epi=18": (31, 1),
               "wgrad Mo=64 No=576 P=16 Cg=64 taps=3x3 s=1 grid=4x4": (74, 504)}
    src.write_text("".join(f"{k}\t{t}\t{s}\n" for k, (t, s) in entries.items()) + "malformed line\n")
    lib.unet_tuning_reset()
    try:
        assert lib.unet_tuning_load(str(src).encode()) == 2
        n = lib.unet_tuning_report(None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.unet_tuning_report(buf, n)
        assert buf.value.decode().count("tuning db") == 2, buf.value
        out = tmp_path / "out.db"
        assert lib.unet_tuning_save(str(out).encode()) == 2
        got = {}
        for line in out.read_text().splitlines():
            k, t, s = line.split("\t")
            got[k] = (int(t), int(s))
        assert got == entries
        assert lib.unet_tuning_load(str(tmp_path / "absent.db").encode()) < 0
    finally:
        lib.unet_tuning_reset()


def test_plan_rejects_too_small_input():
    from unet_amd.plan import Plan
    _lib()
    with pytest.raises(ValueError):
        Plan(1, 1, 100, 100, 2)


def test_plan_workspace_scales_with_batch():
    from unet_amd.plan import Plan
    _lib()
    a = Plan(1, 1, 512, 512, 2).workspace_bytes
    a2 = Plan(2, 1, 512, 512, 2).workspace_bytes
    b = Plan(8, 1, 512, 512, 2).workspace_bytes
    per_image = a2 - a               # activations scale with N, packed weights do not
    assert abs((b - a) - 7 * per_image) < 7 * 2**20
    assert b < 40 * 2**30  # fits easily in 288 GB HBM


def test_segments_cover_all_grads_once():
    from unet_amd.plan import Plan, N_GRADS, N_SEGMENTS
    _lib()
    p = Plan(1, 1, 188, 188, 2)
    seen = []
    for s in range(N_SEGMENTS):
        f, k = p.segment_grads(s)
        seen.extend(range(f, f + k))
    assert sorted(seen) == list(range(N_GRADS))


def test_module_state_dict_schema_matches_reference():
    import torch
    from unet_amd import UNet
    m = UNet(n_channels=1, n_classes=2)
    sd = m.state_dict()
    ref = O.param_shapes(1, 2)
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k]), k
    assert sum(p.numel() for p in m.parameters()) == 31_042_434
    names = [n for n, _ in m.named_parameters()]
    assert names == [k for k in ref if not O.is_buffer(k)]
    # scripts/train.py:54-61 init_weights works on the drop-in
    def init_weights(mod):
        if isinstance(mod, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
            if mod.bias is not None:
                torch.nn.init.constant_(mod.bias, 0)
        elif isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.constant_(mod.weight, 1)
            torch.nn.init.constant_(mod.bias, 0)
    m.apply(init_weights)
    assert float(m.inc.double_conv[0].bias.abs().sum()) == 0.0
    # the reference module path works too
    from models.unet_model import UNet as U2
    from utils.losses import WeightedCrossEntropyLoss  # noqa: F401
    assert U2 is UNet


def test_module_has_no_cpu_fallback():
    import torch
    from unet_amd import UNet, WeightedCrossEntropyLoss
    m = UNet(1, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 1, 188, 188))
    # the submodules' own forwards run on the per-op HIP blocks: no CPU path either
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.inc(torch.zeros(1, 1, 188, 188))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.up1(torch.zeros(1, 1024, 4, 4), torch.zeros(1, 512, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.outc(torch.zeros(1, 64, 4, 4))
    with pytest.raises(RuntimeError):
        WeightedCrossEntropyLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long),
                                   torch.ones(1, 4, 4))
    with pytest.raises(NotImplementedError):
        UNet(1, 2, bilinear=True)


def test_state_dict_roundtrip_with_reference_layout():
    import torch
    from unet_amd import UNet
    params = O.hash_init(1, 2, seed=5, bn_random=True)
    m = UNet(1, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    sd = m.state_dict()
    for k, v in params.items():
        np.testing.assert_array_equal(sd[k].numpy(), np.asarray(v))


def test_host_sanitizer_selftest():
    """The library's host logic under AddressSanitizer + UBSan
    (csrc/Makefile `sanitize`, built by __graft_entry__.build())."""
    import subprocess
    exe = os.path.join(os.path.dirname(__file__), "..", "build", "asan", "host_selftest")
    if not os.path.exists(exe):
        pytest.skip("host_selftest not built (make -C unet-segmentation_amd/csrc sanitize)")
    golden = os.path.join(os.path.dirname(__file__), "golden", "gemm_selection.txt")  # the GEMM variant selection
    r = subprocess.run([exe, golden], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def test_plan_takes_reference_channel_and_class_counts():
    """UNet(n_channels, n_classes) takes any counts in the reference
    (models/unet_model.py:66-85); the plan bounds both at 4096 only to keep
    its per-plan buffers in reason."""
    from unet_amd import UNet
    from unet_amd.plan import Plan
    _lib()
    for c, k in ((5, 5), (16, 32), (3, 9), (17, 2), (1, 33), (64, 150)):
        p = Plan(1, c, 188, 188, k)
        assert (p.out_h, p.out_w) == (4, 4)
        m = UNet(c, k)
        assert m.outc.conv.weight.shape == (k, 64, 1, 1) and m.inc.double_conv[0].weight.shape[1] == c
    for c, k in ((0, 2), (1, 0), (4097, 2), (1, 4097)):
        with pytest.raises(ValueError):
            Plan(1, c, 188, 188, k)
        with pytest.raises(ValueError):
            UNet(c, k)


def test_library_built_from_this_tree():
    """unet_version() carries the hash of the sources the .so was built from
    (csrc/Makefile SRC_HASH); it must equal the hash of the tree's sources."""
    L = _lib()
    ident = L.build_identity()
    assert ident["src_match"], ident



def test_pipeline_crop_views_and_cpu_rejection():
    """unet_amd.pipeline: train.py:39-51's center crop as a strided view (offset
    (H - oh) // 2, squeeze(1), no copy), and no CPU path for the frames."""
    import torch
    from unet_amd.pipeline import HeLaBatches, center_crop_views
    t = torch.arange(2 * 1 * 9 * 8).reshape(2, 1, 9, 8)
    v = center_crop_views(t, (4, 3))
    assert v.shape == (2, 4, 3) and v.data_ptr() == t[:, :, 2:6, 2:5].data_ptr()
    assert torch.equal(v, t[:, 0, 2:6, 2:5])
    with pytest.raises(ValueError):
        center_crop_views(t, (10, 3))
    with pytest.raises(ValueError):
        HeLaBatches(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.int32), 2, (4, 4))


# ---------------------------------------------------------------------------
# unet_gemm_site_* (the per-site GEMM entry point) and the igemm tile table:
# the host-only paths
# ---------------------------------------------------------------------------
def _site_desc(L, site, prec="fp32", grid="main", **kw):
    """A valid descriptor of a matrix case with stand-in pointers (never read:
    the checks below run on the host)."""
    from gemm_site_cases import Case

    class Buf:
        def __init__(self, *a, **k):
            self.ptr = 0x1000

    d = L.GemmSite()
    Case(site, grid, prec, **kw).fill(d, lambda name: 0x1000, Buf)
    return d


def _igemm_ids_in_sources():
    """Tile ids named in the sources' *_tile_rows() functions and igemm.hip's own rows."""
    csrc = os.path.join(ROOT, "unet-segmentation_amd", "csrc")
    ids = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
        blocks = re.findall(r"IgemmTileRows \w+_tile_rows\(\) \{(.*?)return tile_rows\(rows\);", text, flags=re.S)
        blocks += re.findall(r"static const IgemmTile kF32Tiles\[\] = \{(.*?)\n\};", text, flags=re.S)
        for b in blocks:
            ids += [int(m) for m in re.findall(r"\b\w*tile\w*(?:<[^<>()]*>)?\((\d+)[,)]", b)]
            ids += [int(m) for m in re.findall(r"\{(\d+), IgemmFamily::", b)]
    return ids


def test_igemm_tile_table_lists_the_rows_of_the_sources():
    L = _lib()
    table = L.igemm_tile_table()
    ids = [t["id"] for t in table]
    src = _igemm_ids_in_sources()
    assert len(src) == len(set(src)) >= 60, src
    assert sorted(ids) == sorted(src), set(ids) ^ set(src)
    assert len(ids) == len(set(ids))
    by = {t["id"]: t for t in table}
    # a few rows read off the sources
    assert by[4]["family"] == "Reg" and not by[4]["bf16"] and by[4]["ksplit"]
    assert by[21]["bf16"] and by[21]["x3"] and by[36]["family"] == "Halo" and not by[36]["x3"]
    assert [by[t]["wino_m"] for t in (70, 71, 74, 75, 76)] == [2, 4, 6, 2, 4] and not by[76]["ksplit"]
    assert by[87]["family"] == "C64" and by[99]["family"] == "GemmRing" and by[86]["family"] == "Flat"
    # a short buffer receives only what it holds
    buf = (ctypes.c_int * 12)(*([-7] * 12))
    assert L.load().unet_igemm_tile_table(buf, 1) == len(ids)
    assert buf[0] == ids[0] and list(buf[6:]) == [-7] * 6


def test_gemm_site_rejects_bad_descriptors():
    import errno
    L = _lib()
    lib = L.load()
    ok = _site_desc(L, "F_CAT")
    assert lib.unet_gemm_site_check(ctypes.byref(ok), None) == 0
    assert lib.unet_gemm_site_ws_bytes(ctypes.byref(ok)) > 0

    def refused(name, **fields):
        site = name
        d = _site_desc(L, name)
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL, (site, fields)
        assert lib.unet_gemm_site_ws_bytes(ctypes.byref(d)) == 0
        # the run refuses it before it touches ws or the device
        assert lib.unet_gemm_site_run(ctypes.byref(d), 0x1000, None) == -errno.EINVAL
        assert "unet_gemm_site" in L.last_error()

    refused("F_PLAIN", ci=124)             # channels per tap: a multiple of 8
    refused("F_PLAIN", ci=4)
    refused("F_PLAIN", co=100)             # columns: a multiple of 32
    refused("D_POOL", co=20)
    refused("T_FWD", co=12)
    refused("F_CAT", c_split=60)
    refused("F_CAT", c_split=128)          # nothing left for the second source
    refused("F_CAT", oy=6)                 # the window leaves the stored skip grid
    refused("F_CAT", ox=-1)
    refused("D_SPLIT", n_split=48)         # a multiple of 32 ...
    refused("D_SPLIT", n_split=0)
    refused("D_SPLIT", n_split=192)        # ... inside the columns
    for site, ptrs in (("F_PLAIN", ("src0", "wt", "dst0", "bias", "stats", "scale0")), ("F_CAT", ("src1",)),
                       ("D_MASK", ("yref", "bn_scale", "bn_invstd", "bstats")), ("D_SPLIT", ("dst1", "colsum1")),
                       ("T_FWD", ("bias",)), ("T_MASK", ("yref", "bn_mean"))):
        for p in ptrs:
            refused(site, **{p: None})     # scale0 alone: scale and shift come in pairs
    refused("F_PLAIN", site=8)
    refused("F_PLAIN", n=0)
    assert lib.unet_gemm_site_check(None, None) == -errno.EINVAL
    # ws: non-null, 256-byte aligned
    assert lib.unet_gemm_site_run(ctypes.byref(ok), None, None) == -errno.EINVAL
    assert lib.unet_gemm_site_run(ctypes.byref(ok), 0x1010, None) == -errno.EINVAL


def test_gemm_site_strict_forcing_and_expected_map():
    """op_strict: a forced tile or split that does not apply is -EINVAL (default:
    the built-in tile in its place).  And the map of tests/gemm_site_cases.py --
    which tile accepts which site on the main grid -- holds for every tile."""
    import errno
    from gemm_site_cases import SITES, PRECS, WINO_KNOBS, tiles_for, expected_sites
    L = _lib()
    lib = L.load()
    table = L.igemm_tile_table()
    knobs = dict(op_strict=0, op_precision=0, op_a16=0, igemm_variant=-1, wino_dgrad_max=4)
    try:
        d = _site_desc(L, "T_FWD")
        d.tile = 52   # a 3x3 halo tile at a convT site
        tile = ctypes.c_int(0)
        assert lib.unet_gemm_site_check(ctypes.byref(d), ctypes.byref(tile)) == 0 and tile.value != 52
        lib.unet_set_tuning(b"op_strict", 1)
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL
        d.tile = 12345
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL
        d.tile, d.split = 1, 3
        assert lib.unet_gemm_site_check(ctypes.byref(d), ctypes.byref(tile)) == 0 and tile.value == 1
        split_ws = lib.unet_gemm_site_ws_bytes(ctypes.byref(d))
        d.split = 1
        # the slab of an explicit K split lives in ws: 3 x M x N floats more
        assert split_ws - lib.unet_gemm_site_ws_bytes(ctypes.byref(d)) == 3 * (2 * 13 * 19) * 256 * 4
        d.split = 5   # 8 K chunks do not make 5 non-empty slices
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL
        d = _site_desc(L, "F_PLAIN")
        d.tile, d.split = 70, 3   # Winograd takes no K split
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL
        # tile -1 = the igemm_variant knob; 0 = the built-in choice whatever the knob says
        lib.unet_set_tuning(b"igemm_variant", 52)
        d.tile, d.split = -1, 1
        assert lib.unet_gemm_site_check(ctypes.byref(d), ctypes.byref(tile)) == 0 and tile.value == 52
        d.tile = 0
        assert lib.unet_gemm_site_check(ctypes.byref(d), ctypes.byref(tile)) == 0 and tile.value not in (52, -1)
        lib.unet_set_tuning(b"igemm_variant", -1)
        ran = set()
        for prec, (p, a16) in PRECS.items():
            lib.unet_set_tuning(b"op_precision", p)
            lib.unet_set_tuning(b"op_a16", a16)
            for t in table:
                if t["id"] not in tiles_for(table, prec):
                    continue
                for k, v in WINO_KNOBS.get(t["id"], [{}])[0].items():
                    lib.unet_set_tuning(k.encode(), v)
                got = []
                for site in SITES:
                    d = _site_desc(L, site, prec)
                    d.tile = t["id"]
                    if lib.unet_gemm_site_check(ctypes.byref(d), ctypes.byref(tile)) == 0:
                        assert tile.value == t["id"]
                        got.append(site)
                lib.unet_set_tuning(b"wino_dgrad_max", 4)
                assert tuple(got) == expected_sites(t, prec), (prec, t["id"], t["family"], got)
                if got:
                    ran.add(t["id"])
        # the tiles no site of the main matrix takes have a case of their own
        assert {t["id"] for t in table} - ran == {86, 87}
        lib.unet_set_tuning(b"op_precision", 1)
        lib.unet_set_tuning(b"op_a16", 1)
        d = _site_desc(L, "F_PLAIN", "bf16", cg=64, cols=64)
        d.tile = 87
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == 0
    finally:
        for k, v in knobs.items():
            lib.unet_set_tuning(k.encode(), v)
