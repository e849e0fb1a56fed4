"""The cases of the GEMM-site matrix (tests/test_gpu_gemm_sites.py) and the map
of which tile must accept which site; no GPU needed (tests/test_clib_cpu.py
checks the map through unet_gemm_site_check).

A Case is one launch site on one grid in one precision: its shapes, its inputs
(float32 values held as float64), its float64 reference from the site oracles
(oracle/unet_oracle.py) and the descriptor that runs it."""
import numpy as np

from oracle import unet_oracle as O

SITES = ("F_PLAIN", "F_CAT", "F_EVAL", "D_POOL", "D_MASK", "D_SPLIT", "T_FWD", "T_MASK")
GRIDS = {"main": (2, 13, 19), "tiny": (3, 1, 5)}
# precision -> (op_precision, op_a16).  bf16 runs as a bf16 plan stores its
# tensors: sources, destinations and yref in bf16.
PRECS = {"fp32": (0, 0), "bf16": (1, 1), "bf16x3": (2, 0)}
BARS = {"fp32": 2e-5, "bf16": 5e-5, "bf16x3": 3e-5}
CONV = ("F_PLAIN", "F_CAT", "F_EVAL", "D_POOL", "D_MASK", "D_SPLIT")
ALL = SITES
# tiles whose two forms both run: the persistent and the plain form of the fused
# tiles 75 / 76 (three workgroups walk the groups), the point GEMMs of the
# unfused tiles on the LDS-DMA ring or not; F(6x6) input gradients are off by default
_PERSIST = [{"wino_persist": 0, "wino_persist_wgs": 3}, {"wino_persist": 1, "wino_persist_wgs": 3}]
_PLANE = [{"igemm_plane": 0}, {"igemm_plane": 1}]
WINO_KNOBS = {75: _PERSIST, 76: _PERSIST, 70: _PLANE, 71: _PLANE,
              74: [dict(k, wino_dgrad_max=6) for k in _PLANE]}

# family -> sites its tiles must accept on the main grid, read from the fits()
# functions (csrc: reg_tile_fits, halo_tile_fits, conv3_dma_fits, conv3_ring_fits,
# conv3_flat_fits, conv3_c64_fits, gemm_ring_fits, wino_applies,
# wino_fused*_applies).  "no192": the tile's bn does not divide D_SPLIT's 192
# columns.  Per-tile exceptions follow.
_NO_SPLIT = tuple(s for s in CONV if s != "D_SPLIT")
EXPECT = {
    "fp32": {
        "Reg": ALL,            # any gather; N % bn: the 128-column tiles refuse D_SPLIT (192)
        "Halo": CONV,          # 3x3 stride-1 gathers, bn 64
        "Wino": CONV,          # 3x3, linear destinations, no shuffle
        "WinoFused": CONV,
    },
    "bf16": {
        "Reg": ALL,
        "Halo": CONV,
        "Conv3Dma": CONV,      # bf16-stored sources (op_a16), bn 64
        "Ring": CONV,
        "Flat": CONV,
        "C64": (),             # N = Cg = 64 only: runs in test_small_channel_counts
        "GemmRing": ("T_FWD", "T_MASK"),
    },
    "bf16x3": {
        "Reg": ALL,
        "Halo": CONV,
    },
}
# tile id -> sites, where a tile differs from its family
_NO192 = tuple(s for s in ALL if s != "D_SPLIT")
_BF_REG = {21: _NO192, 22: _NO192, 24: _NO192,   # bn 128
           26: ("T_FWD",)}                        # bn 256: only T_FWD's 4 x 64 columns
EXPECT_TILE = {
    "fp32": {
        **{t: _NO192 for t in (4, 1, 2, 3, 9, 11, 12, 13)},  # bn 128
        # F(6x6): forward GEMMs are capped at F(4x4) (wino_max), input gradients take it with wino_dgrad_max 6
        74: ("D_POOL", "D_MASK", "D_SPLIT"),
    },
    "bf16": {
        **_BF_REG,
        34: _NO_SPLIT, 36: _NO_SPLIT,   # halo tiles of 128 columns
        68: _NO_SPLIT,                  # k_conv3_dma, 128 columns
        81: _NO_SPLIT, 83: _NO_SPLIT,   # ring tiles of 128 columns
        85: _NO_SPLIT,                  # flat tile: 128 columns
        86: (),                         # its stream-K form needs >= one work unit per CU: test_other_channel_counts
        93: ("T_FWD",), 96: ("T_FWD",), 98: ("T_FWD",),   # k_gemm_ring tiles of 256 columns
    },
    "bf16x3": dict(_BF_REG),
}


def expected_sites(t, prec):
    return tuple(EXPECT_TILE[prec].get(t["id"], EXPECT[prec].get(t["family"], ())))


def tiles_for(rows, prec):
    """Ids of the table's tiles that run in `prec`, in table order."""
    if prec == "fp32":
        return [t["id"] for t in rows if not t["bf16"]]
    if prec == "bf16":
        return [t["id"] for t in rows if t["bf16"]]
    return [t["id"] for t in rows if t["bf16"] and t["x3"]]


def splits_for(t):
    """K splits tried on a tile: 1 and 3; 2 where 3 was refused (the tile's K
    chunks do not divide into three non-empty slices)."""
    return [1, 3, 2] if t["ksplit"] else [1]


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def affine(rng, c, x, closed, negative):
    """Per-channel scale in +-U(0.5, 1.5) with mixed signs and shift 0.3 N(0, 1);
    channel `negative` has scale < 0, channel `closed` never passes the ReLU."""
    scale = rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)
    shift = 0.3 * rng.standard_normal(c)
    scale[negative] = -abs(scale[negative])
    scale[closed] = abs(scale[closed])
    scale, shift = f32(scale), f32(shift)
    shift[closed] = f32(-(np.abs(x[..., closed]).max() * scale[closed] + 1.0))
    return scale, shift


def keep_off_zero(yref, scale, shift, bf16):
    """Moves every element whose pre-activation yref * scale + shift is within
    1e-3 of 0 to +-2e-3 (yref = (+-2e-3 - shift) / scale), so that the mask's
    sign is the same in fp32 fmaf and in float64.  A bf16 yref is re-rounded; where
    the rounding step exceeds the margin the target doubles until it holds."""
    rnd = O.round_bf16 if bf16 else f32
    y = rnd(yref)
    pre = y * scale + shift
    near = np.abs(pre) < 1e-3
    sign = np.where(pre < 0, -1.0, 1.0)
    target = 2e-3
    while near.any():
        cand = rnd((sign * target - shift) / scale)
        y = np.where(near, cand, y)
        near = np.abs(y * scale + shift) < 1e-3
        target *= 2
        assert target < 64, "no representable yref keeps the pre-activation off zero"
    return y


class Case:
    def __init__(self, site, grid, prec, cg=None, cols=None):
        self.site, self.grid, self.prec = site, grid, prec
        self.n, self.h, self.w = GRIDS[grid]
        self.h16 = prec == "bf16"
        self.bar = BARS[prec]
        self.fwd = site.startswith("F_")
        self.dgrad = site.startswith("D_")
        c = cg or 128
        # (ci, co) of the layer's weight; Cg = channels per tap, columns = GEMM N
        if self.fwd:
            self.ci, self.co = c, cols or 128
        elif site == "D_SPLIT":
            self.ci, self.co = 192, c
        elif self.dgrad or site == "T_MASK":
            self.ci, self.co = cols or 128, c
        else:  # T_FWD: 4 co columns
            self.ci, self.co = c, 64
        self.columns = self.co if self.fwd else 4 * self.co if site == "T_FWD" else self.ci
        self.c_split = 64 if site == "F_CAT" else 0
        self.n_split = 64 if site == "D_SPLIT" else 0
        self.skip_h, self.skip_w, self.oy, self.ox = (self.h + 2 + 5, self.w + 2 + 4, 2, 3) if site == "F_CAT" else (0, 0, 0, 0)
        self.mask = site in ("D_MASK", "T_MASK")
        self.outputs = ("dst0", "dst1") if site == "D_SPLIT" else ("dst0",)
        self.key = (site, grid, "bf16" if self.h16 else "f32", c, self.columns)

    # ---- inputs: float32 values (as float64) ----
    def inputs(self):
        n, h, w, ci, co = self.n, self.h, self.w, self.ci, self.co
        rng = np.random.default_rng(1000 + 17 * SITES.index(self.site) + (0 if self.grid == "main" else 7) + ci + co)
        d = {}
        if self.fwd:
            if self.site == "F_CAT":
                cs = self.c_split
                d["src0"] = f32(rng.standard_normal((n, self.skip_h, self.skip_w, cs)))
                d["src1"] = f32(np.maximum(rng.standard_normal((n, h + 2, w + 2, ci - cs)), 0))
                d["scale0"], d["shift0"] = affine(rng, cs, d["src0"], closed=5, negative=3)
            else:
                d["src0"] = f32(rng.standard_normal((n, h + 2, w + 2, ci)))
                d["scale0"], d["shift0"] = affine(rng, ci, d["src0"], closed=5, negative=3)
            d["wt"] = f32(rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci))
            d["bias"] = f32(rng.standard_normal(co))
        elif self.dgrad:
            d["src0"] = f32(rng.standard_normal((n, h + 2, w + 2, co)))
            d["wt"] = f32(rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * co))
        elif self.site == "T_FWD":
            d["src0"] = f32(np.maximum(rng.standard_normal((n, h, w, ci)), 0))
            d["wt"] = f32(rng.standard_normal((ci, co, 2, 2)) / np.sqrt(ci))
            d["bias"] = f32(rng.standard_normal(co))
        else:
            d["src0"] = f32(rng.standard_normal((n, 2 * h, 2 * w, co)))
            d["wt"] = f32(rng.standard_normal((ci, co, 2, 2)) / np.sqrt(4 * co))
        if self.mask:
            y = f32(rng.standard_normal((n, h, w, ci)))
            d["bn_scale"], d["bn_shift"] = affine(rng, ci, y, closed=5, negative=3)
            d["bn_mean"] = f32(0.2 * rng.standard_normal(ci))
            d["bn_invstd"] = f32(rng.uniform(0.5, 2.0, ci))
            d["yref"] = keep_off_zero(y, d["bn_scale"], d["bn_shift"], self.h16)
            # the margin holds on the values the kernel reads, before any GPU call
            assert np.abs(d["yref"] * d["bn_scale"] + d["bn_shift"]).min() >= 1e-3
            assert np.array_equal(d["yref"], O.round_bf16(d["yref"]) if self.h16 else f32(d["yref"]))
        return d

    # ---- float64 reference ----
    def oracle(self, d, conv=None):
        kw = {} if conv is None else {"conv": conv}
        bf = self.h16
        qa = O.round_bf16 if self.prec == "bf16" else (lambda a: a)   # operands as the GEMM sees them
        wt = qa(d["wt"])

        def load(x, sc, sh):  # a bf16-stored source, its transform in one fp32 fma, the staged operand
            return qa(O.bn_relu_on_load(qa(x), sc, sh, fma32=bf))
        out = {}
        if self.site == "F_PLAIN":
            out["dst0"], _ = O.site_f_plain(load(d["src0"], d["scale0"], d["shift0"]), None, None, wt, d["bias"], **kw)
        elif self.site == "F_EVAL":
            out["dst0"] = O.site_f_eval(load(d["src0"], d["scale0"], d["shift0"]), None, None, wt, d["bias"], **kw)
        elif self.site == "F_CAT":
            out["dst0"], _ = O.site_f_cat(load(d["src0"], d["scale0"], d["shift0"]), None, None, self.oy, self.ox,
                                          qa(d["src1"]), wt, d["bias"], **kw)
        elif self.site == "D_POOL":
            out["dst0"] = O.site_d_pool(qa(d["src0"]), wt, **kw)
        elif self.site == "D_MASK":
            out["dst0"], _ = O.site_d_mask(qa(d["src0"]), wt, d["yref"], d["bn_scale"], d["bn_shift"], d["bn_mean"],
                                           d["bn_invstd"], **kw)
        elif self.site == "D_SPLIT":
            out["dst0"], out["dst1"], _ = O.site_d_split(qa(d["src0"]), wt, self.n_split, **kw)
        elif self.site == "T_FWD":
            out["dst0"] = O.site_t_fwd(qa(d["src0"]), wt, d["bias"])
        else:
            out["dst0"], _ = O.site_t_mask(qa(d["src0"]), wt, d["yref"], d["bn_scale"], d["bn_shift"], d["bn_mean"],
                                           d["bn_invstd"])
        return {k: np.ascontiguousarray(v) for k, v in out.items()}

    # ---- descriptor ----
    def fill(self, d, ptr_of, G):
        """Fills descriptor d (unet_amd._lib.GemmSite); ptr_of(name) gives an
        input's device pointer, G(shape, dtype, bf16=) a guarded output buffer.
        Returns the output buffers by name."""
        d.site = SITES.index(self.site)
        d.n, d.h, d.w, d.ci, d.co = self.n, self.h, self.w, self.ci, self.co
        d.c_split, d.n_split = self.c_split, self.n_split
        d.skip_h, d.skip_w, d.oy, d.ox = self.skip_h, self.skip_w, self.oy, self.ox
        d.tile, d.split = 0, 1
        names = ["src0", "wt"]
        if self.fwd:
            names += ["scale0", "shift0", "bias"] + (["src1"] if self.site == "F_CAT" else [])
        if self.site == "T_FWD":
            names += ["bias"]
        if self.mask:
            names += ["yref", "bn_scale", "bn_shift", "bn_mean", "bn_invstd"]
        for k in names:
            setattr(d, k, ptr_of(k))
        n, h, w = self.n, self.h, self.w
        dt = dict(dtype=np.uint16, bf16=True) if self.h16 else dict(dtype=np.float32)
        bufs = {}
        if self.site == "T_FWD":
            bufs["dst0"] = G((n, 2 * h, 2 * w, self.co), **dt)
        elif self.site == "D_SPLIT":
            bufs["dst0"] = G((n, h, w, self.n_split), **dt)
            bufs["dst1"] = G((n, h, w, self.columns - self.n_split), **dt)
            bufs["colsum1"] = G((64, self.columns - self.n_split), dtype=np.float64)
        else:
            bufs["dst0"] = G((n, h, w, self.columns), **dt)
        if self.site in ("F_PLAIN", "F_CAT"):
            bufs["stats"] = G((64, self.columns, 2), dtype=np.float64)
        if self.mask:
            bufs["bstats"] = G((64, self.columns, 2), dtype=np.float64)
        for k, b in bufs.items():
            setattr(d, k, b.ptr)
        return bufs

    def stat_terms(self, d, got):
        """name of a statistics array -> the per-element terms whose column sums
        it holds, from the GPU's own stored output."""
        if self.site in ("F_PLAIN", "F_CAT"):
            y = got["dst0"]
            return {"stats": [y, y * y]}
        if self.mask:
            dz = got["dst0"]
            return {"bstats": [dz, dz * ((d["yref"] - d["bn_mean"]) * d["bn_invstd"])]}
        if self.site == "D_SPLIT":
            return {"colsum1": [got["dst1"]]}
        return {}
