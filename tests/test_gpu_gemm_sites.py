"""Per-element parity of every forward / input-gradient GEMM tile at the launch
sites of the network plan, through unet_gemm_site_run (include/unet_hip.h),
against the float64 site oracles (oracle/unet_oracle.py site_*).

The matrix is the full cross of: every tile id of the igemm table whose
precision flags match (plus the built-in choice), every site, two grids --
with "op_strict" on, so a cell either ran the tile under test or the entry
point refused it with -EINVAL before it launched anything.  EXPECT and
EXPECT_TILE (tests/gemm_site_cases.py) say which sites each tile must accept on
the main grid; they were read from the tiles' fits() functions.  A tile that stops accepting a site fails, a tile
that starts accepting one fails too (the map is then extended by hand, with
the cell checked), and every tile of the table must run at one site or more.

Shapes (the smallest that cross the seams)
  main grid  n 2, 13 x 19 rows: M = 494 = two 256-row workgroups, the second
             ragged; 13 and 19 are multiples of none of 2, 4, 6, 8, 16, 32, so
             every halo and Winograd tile overhangs in both directions
  tiny grid  n 3, 1 x 5 rows: M = 15, fewer rows than one wave fragment
  channels   128 per tap; 128 columns; D_SPLIT 192 columns split at 64 (C = 64
             and 128); T_FWD co 64 = 256 columns; F_CAT 64 + 64 channels, the
             skip stored 5 rows and 4 columns larger and read at (2, 3)
  other      F_PLAIN and D_POOL at 16 / 8 channels per tap (fp32), 64 -> 64 and
             256 -> 4096 (bf16: the shapes tiles 87 and 86 take)
  split-K    1 and 3 (2 where 3 does not divide the tile's K chunks)

Bars (error = max |got - ref| / max |ref| per tensor)
  fp32 direct 2e-5, bf16x3 3e-5, bf16 5e-5 on bf16-rounded operands; a bf16
  destination |got - ref| <= 2^-7 |ref| + bar * scale (one ulp for a
  rounding-boundary flip); Winograd max(2e-5, 4 e_ref) with e_ref the error of
  the float32 restatement (oracle winograd_conv) on the same inputs, printed
  with the GPU's error for every Winograd cell (profiles/gemm_site_tests.log:
  the GPU's error is 0.77 - 3.5 x e_ref, 1.4e-5 at most, and 1.0 - 1.3 x
  e_ref in the F(6x6) cells, the only ones whose bar is above 2e-5; no cell
  exceeded its bar, so the factor 4 was not put to the question).
  Statistics against fp64 sums of the GPU's OWN stored output:
  |sum_gpu - sum_own| <= 1e-5 sum |term| per column.  No element is excluded
  from the mask: pre-activations are kept >= 1e-3 away from 0 (asserted here).

Every output, statistics array and workspace is guarded (tests/guarded.py);
workspaces have exactly unet_gemm_site_ws_bytes.
"""
import ctypes
import errno

import numpy as np
import pytest

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from guarded import G, ws_buf, done, begin, release, stream  # noqa: E402
from gemm_site_cases import (SITES, GRIDS, PRECS, WINO_KNOBS, Case, tiles_for, splits_for,  # noqa: E402
                             expected_sites)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from unet_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _release():
    begin()
    yield
    release()


q = O.round_bf16
KNOBS = {"op_strict": 0, "op_precision": 0, "op_a16": 0, "igemm_variant": -1, "wino_persist": 1,
         "wino_persist_wgs": -1, "igemm_plane": 1, "wino_dgrad_max": 4}
_DEV = {}    # (case key, name) -> device tensor of an input, kept for the module
_REF = {}    # case key -> (inputs, reference outputs)
_EREF = {}   # (case key, m) -> e_ref of the float32 Winograd restatement
RAN = {}     # (precision, tile id) -> cells that ran (test_every_tile_ran reads it)
SEEN = set()  # (precision, site, grid) whose matrix ran in this process


def dev_in(key, name, a):
    k = (key, name)
    if k not in _DEV:
        _DEV[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return _DEV[k]


def reference(case):
    """Inputs and float64 reference of a case, computed once."""
    if case.key not in _REF:
        inp = case.inputs()
        _REF[case.key] = (inp, case.oracle(inp))
    return _REF[case.key]


def e_ref(case, m):
    """Error of the float32 Winograd F(m x m) restatement against float64, per
    output tensor, on the case's inputs."""
    k = (case.key, m)
    if k not in _EREF:
        inp, ref = reference(case)
        w32 = case.oracle(inp, conv=lambda x, w: O.winograd_conv(x, w, m, np.float32).astype(np.float64))
        _EREF[k] = {name: float(np.abs(w32[name] - ref[name]).max() / np.abs(ref[name]).max())
                    for name in case.outputs}
    return _EREF[k]


def run_cell(lib, case, tile, split):
    """One cell: -EINVAL (refused before any launch), or the outputs."""
    from unet_amd import _lib
    inp, _ = reference(case)
    d = _lib.GemmSite()
    bufs = case.fill(d, lambda name: dev_in(case.key, name, inp[name]).data_ptr(), G)
    d.tile, d.split = tile, split
    if lib.unet_gemm_site_check(ctypes.byref(d), None) != 0:
        assert lib.unet_gemm_site_ws_bytes(ctypes.byref(d)) == 0
        # the run refuses it as well, and before it touches anything: the
        # outputs keep their 0xFF fill (checked below), no workspace is needed
        ws = ws_buf(256)
        assert lib.unet_gemm_site_run(ctypes.byref(d), ws.ptr, stream()) == -errno.EINVAL
        torch.cuda.synchronize()
        for b in bufs.values():
            assert bool((b.bytes == 0xFF).all()), "a refused call wrote to an output"
            b.output = False
        done()
        return None
    nws = lib.unet_gemm_site_ws_bytes(ctypes.byref(d))
    assert nws > 0
    ws = ws_buf(nws)
    rc = lib.unet_gemm_site_run(ctypes.byref(d), ws.ptr, stream())
    assert rc == 0, f"unet_gemm_site_run: {rc} {_lib.last_error()}"
    done()   # every output element finite, every guard intact
    return {k: (b.f64() if b.dtype != np.float64 else b.np()) for k, b in bufs.items()}


def check_cell(case, got, tag, wino_m, log):
    inp, ref = reference(case)
    bar = case.bar
    for name in case.outputs:
        r, g = ref[name], got[name]
        scale = np.abs(r).max()
        b = bar
        if wino_m:
            er = e_ref(case, wino_m)[name]
            b = max(2e-5, 4 * er)
        if case.h16:   # a bf16 destination: one ulp for a rounding flip + the accumulation bar
            rr = q(r)
            over = np.abs(g - rr) - (2.0 ** -7 * np.abs(rr) + b * scale)
            err = float(np.abs(g - rr).max() / scale)
            ok = bool((over <= 0).all())
        else:
            err = float(np.abs(g - r).max() / scale)
            ok = err <= b
        if wino_m:
            log(f"WINO {tag} {name}: e_ref {er:.3e} gpu {err:.3e} bar {b:.3e} ratio {err / max(er, 1e-30):.2f}")
        if not ok:
            bad = np.argwhere(np.abs(g - (q(r) if case.h16 else r)) > b * scale + (2.0 ** -7 * np.abs(r) if case.h16 else 0))
            pytest.fail(f"{tag} {name}: error {err:.3e} > bar {b:.3e}; {len(bad)} elements, first at "
                        f"(n, y, x, c) = {bad[:6].tolist()}, column histogram {np.bincount(bad[:, -1] // 32).tolist()}")
    # statistics against fp64 sums of the GPU's own stored output
    for name, terms in case.stat_terms(inp, got).items():
        raw = got[name]
        sums = raw.sum(0)            # over the kStatGroups groups
        for k, t in enumerate(terms):
            own = t.reshape(-1, t.shape[-1])
            s_own, s_abs = own.sum(0), np.abs(own).sum(0)
            s_gpu = sums[:, k] if sums.ndim == 2 else sums
            worst = np.abs(s_gpu - s_own) - 1e-5 * s_abs
            assert (worst <= 0).all(), (f"{tag} {name}[{k}]: column {int(worst.argmax())}: gpu {s_gpu[worst.argmax()]:.9g} "
                                        f"own {s_own[worst.argmax()]:.9g} sum|term| {s_abs[worst.argmax()]:.6g}")


def set_knobs(lib, **kw):
    for k, v in kw.items():
        assert lib.unet_set_tuning(k.encode(), v) == 0


def matrix(lib, prec, site, grid, capsys=None):
    """All tiles of `prec` x splits at one site and grid.  Returns the cells."""
    from unet_amd import _lib
    case = Case(site, grid, prec)
    table = {t["id"]: t for t in _lib.igemm_tile_table()}
    cells = []
    lines = []
    try:
        set_knobs(lib, op_strict=1, op_precision=PRECS[prec][0], op_a16=PRECS[prec][1], igemm_variant=-1)
        for tid in [0] + tiles_for(table.values(), prec):
            t = table.get(tid)
            knob_sets = WINO_KNOBS.get(tid, [{}])
            ran_split = False
            accepted = False
            for knobs in knob_sets:
                set_knobs(lib, **{k: KNOBS[k] for k in ("wino_persist", "wino_persist_wgs", "igemm_plane", "wino_dgrad_max")})
                set_knobs(lib, **knobs)
                for split in ([1] if tid == 0 else splits_for(t)):
                    if split == 2 and ran_split:
                        continue   # 3 slices ran
                    tag = f"{prec} {site} {grid} tile {tid} split {split}" + "".join(f" {k}={v}" for k, v in knobs.items())
                    got = run_cell(lib, case, tid, split)
                    if got is None:
                        lines.append(f"REFUSED {tag}")
                        continue
                    if split == 1:
                        accepted = True
                    else:
                        ran_split = True
                    check_cell(case, got, tag, t["wino_m"] if t else 0, lines.append)
                    lines.append(f"RAN {tag}")
                    cells.append((tid, split))
                    if tid:
                        RAN.setdefault((prec, tid), []).append(f"{site}/{grid}/s{split}")
            if tid == 0:
                assert accepted, f"the built-in choice refused {site} {grid} {prec}"
                continue
            if grid == "main":
                want = site in expected_sites(t, prec)
                assert accepted == want, (f"tile {tid} ({t['family']}) {'accepts' if accepted else 'refuses'} {site} in {prec}: "
                                          f"EXPECT says it {'must' if want else 'must not'}")
            if accepted and t["ksplit"] and case.columns % 64 == 0:
                assert ran_split, f"tile {tid} has a split-K form but no split > 1 ran at {site} {grid}"
    finally:
        set_knobs(lib, **KNOBS)
        print("\n".join(lines))
    return cells


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("site", SITES)
@pytest.mark.parametrize("prec", list(PRECS))
def test_site_matrix(lib, prec, site, grid):
    cells = matrix(lib, prec, site, grid)
    assert cells
    SEEN.add((prec, site, grid))


def test_every_tile_ran(lib):
    """Every tile id of the table ran at one site or more (after the matrix)."""
    from unet_amd import _lib
    full = {(p, s, g) for p in PRECS for s in SITES for g in GRIDS}
    for p, s, g in sorted(full - SEEN):   # run alone: make up the missing cells
        matrix(lib, p, s, g)
        SEEN.add((p, s, g))
    for which in OTHER:
        if not any(c.endswith(which) for v in RAN.values() for c in v):
            other_counts(lib, "F_PLAIN", which)
    table = _lib.igemm_tile_table()
    missing = []
    for t in table:
        ran = [c for p in PRECS for c in RAN.get((p, t["id"]), [])]
        print(f"TILE {t['id']} ({t['family']}): {len(ran)} cells, e.g. {ran[:4]}")
        if not ran:
            missing.append(t["id"])
    assert not missing, f"tiles that ran at no site: {missing}"


# Channel counts the main matrix does not have.  16 and 8 channels per tap: one K
# chunk (or half of one) per tap.  64 -> 64 in bf16: the only shape the
# resident-weights tile 87 takes.  256 -> 4096 in bf16: the stream-K form of the
# flat tile (86) wants one work unit per CU or more, a (tile, column block)
# shared by four workgroups at most: 2 tiles x 32 column blocks x 4 chunks = 256.
OTHER = {"fp32-16": ("fp32", 16, None, None), "fp32-8": ("fp32", 8, None, None),
         "bf16-64x64": ("bf16", 64, 64, None), "bf16-256x4096": ("bf16", 256, 4096, [86, 85])}
_F16 = {1, 2, 4, 6, 8, 11, 12, 13, 14, 51, 52, 53, 54, 75, 77}
# (forward GEMMs take F(4x4) from wino4_fwd_min_cg = 128 channels on: 72, 73, 76 at D_POOL only)
OTHER_MUST = {("fp32-16", "F_PLAIN"): _F16, ("fp32-16", "D_POOL"): _F16 | {72, 73, 76},
              ("fp32-8", "F_PLAIN"): {75, 77}, ("fp32-8", "D_POOL"): {75, 77},
              ("bf16-64x64", "F_PLAIN"): {23, 25, 31, 63, 82, 87, 88}, ("bf16-64x64", "D_POOL"): {23, 25, 31, 63, 82, 87, 88},
              ("bf16-256x4096", "F_PLAIN"): {85, 86}, ("bf16-256x4096", "D_POOL"): {85, 86}}


def other_counts(lib, site, which):
    from unet_amd import _lib
    prec, cg, cols, only = OTHER[which]
    case = Case(site, "main", prec, cg=cg, cols=cols)
    table = {t["id"]: t for t in _lib.igemm_tile_table()}
    ran = []
    lines = []
    try:
        set_knobs(lib, op_strict=1, op_precision=PRECS[prec][0], op_a16=PRECS[prec][1], igemm_variant=-1,
                  wino_persist_wgs=3, wino_dgrad_max=6)
        for tid in only or tiles_for(table.values(), prec):
            tag = f"{prec} {site} main {which} tile {tid}"
            got = run_cell(lib, case, tid, 1)
            if got is None:
                lines.append(f"REFUSED {tag}")
                continue
            check_cell(case, got, tag, table[tid]["wino_m"], lines.append)
            lines.append(f"RAN {tag}")
            ran.append(tid)
            RAN.setdefault((prec, tid), []).append(f"{site}/{which}")
    finally:
        set_knobs(lib, **KNOBS)
        print("\n".join(lines))
    must = OTHER_MUST[which, site]
    if which == "fp32-8":   # 8-channel chunks: the fused F(2x2) tiles and nothing else
        assert set(ran) == must, ran
    assert must <= set(ran), f"{which} {site}: {sorted(must - set(ran))} refused"


@pytest.mark.parametrize("which", list(OTHER))
@pytest.mark.parametrize("site", ["F_PLAIN", "D_POOL"])
def test_other_channel_counts(lib, site, which):
    other_counts(lib, site, which)


def test_strict_off_keeps_the_fallback(lib):
    """op_strict 0 (the default): a forced tile that does not fit is replaced by
    the built-in one, as before; with it on the same call is -EINVAL."""
    from unet_amd import _lib
    case = Case("T_FWD", "tiny", "fp32")
    inp, _ = reference(case)
    d = _lib.GemmSite()
    bufs = case.fill(d, lambda name: dev_in(case.key, name, inp[name]).data_ptr(), G)
    d.tile, d.split = 52, 1   # a 3x3 halo tile at a convT site
    try:
        set_knobs(lib, op_strict=0)
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == 0
        ws = ws_buf(lib.unet_gemm_site_ws_bytes(ctypes.byref(d)))
        assert lib.unet_gemm_site_run(ctypes.byref(d), ws.ptr, stream()) == 0
        done()
        got = {k: b.f64() for k, b in bufs.items()}
        check_cell(case, got, "fallback", 0, print)
        set_knobs(lib, op_strict=1)
        assert lib.unet_gemm_site_check(ctypes.byref(d), None) == -errno.EINVAL
    finally:
        set_knobs(lib, **KNOBS)
