"""Whole-sequence inference with symmetry averaging (scripts/predict.py's step,
on full frames): a device-resident stack of frames in, foreground
probabilities / masks of every full frame out.

    sp = SequencePredictor(model, tile_in=512, batch=8, symmetries="d4")
    out = sp.predict(frames, want=("mask", "prob"))   # device tensors

Tiles are batched across frames: the (frame, tile) work list is built once per
geometry, frame-major, and every forward takes ``batch // ns`` groups of it,
each under the ``ns`` chosen symmetries of the square.  unet_seq_tile_gather
reads the tiles from the unpadded frames (mirror folded into the index,
predict.py's uint8 -> Normalize(0.5, 0.5) fused), the eval-mode network runs on
the batch, and unet_seq_tile_reduce maps every symmetry's output back, averages
the softmaxes in a fixed order and writes each frame pixel exactly once: no
atomics, the same bits on every run.

Symmetry code s = r + 4 f: S_s(x) = rot90(flip_f(x), r) with r quarter turns as
torch.rot90(x, r, (-2, -1)) and f = 1 a torch.flip(x, (-1,)) before them.  The
network sees S_s(tile); its output is mapped back with S_s^-1 before averaging
(the U-Net paper's submissions average over rotated inputs).

One device; callers deal frames over devices themselves.
"""
from __future__ import annotations

import copy
import ctypes

import torch

from . import _lib
from .tiling import TileGeometry

SYMMETRY_SETS = {"none": (0,), "flip": (0, 4), "rot4": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
OUTPUTS = ("mask", "prob", "logits")


def symmetry_codes(symmetries) -> tuple:
    """The codes of a named set or of a tuple of distinct codes 0..7."""
    if isinstance(symmetries, str):
        if symmetries not in SYMMETRY_SETS:
            raise ValueError(f"symmetries must be one of {sorted(SYMMETRY_SETS)} or a tuple of codes, "
                             f"got {symmetries!r}")
        return SYMMETRY_SETS[symmetries]
    codes = tuple(int(s) for s in symmetries)
    if not codes or len(set(codes)) != len(codes) or any(not 0 <= s <= 7 for s in codes):
        raise ValueError(f"symmetry codes must be distinct and within 0..7, got {symmetries!r}")
    return codes


def apply_symmetry(x: torch.Tensor, s: int) -> torch.Tensor:
    """S_s on the last two (square) axes."""
    return torch.rot90(torch.flip(x, (-1,)) if s >= 4 else x, s & 3, (-2, -1))


def invert_symmetry(y: torch.Tensor, s: int) -> torch.Tensor:
    """S_s^-1 on the last two (square) axes."""
    x = torch.rot90(y, -(s & 3), (-2, -1))
    return torch.flip(x, (-1,)) if s >= 4 else x


def work_list(n_frames: int, n_tiles: int) -> torch.Tensor:
    """(n_frames * n_tiles, 2) int32 (frame, tile), frame-major."""
    f = torch.arange(n_frames, dtype=torch.int32).repeat_interleave(n_tiles)
    t = torch.arange(n_tiles, dtype=torch.int32).repeat(n_frames)
    return torch.stack([f, t], 1).contiguous()


class SequencePredictor:
    def __init__(self, model, tile_in=512, batch=8, symmetries="none", threshold=0.5, device=None):
        self.codes = symmetry_codes(symmetries)
        self.ns = len(self.codes)
        if batch < 1 or batch % self.ns:
            raise ValueError(f"the {self.ns} symmetries must divide the batch, got batch {batch}")
        self.tile_in, self.batch, self.threshold = int(tile_in), int(batch), float(threshold)
        self.tile_out = TileGeometry(1, 1, self.tile_in).tile_out  # raises for a tile the network cannot take
        if device is None:
            p = next(model.parameters())
            device = p.device if p.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SequencePredictor runs on the HIP device only (no CPU fallback)")
        self.model = copy.deepcopy(model).to(self.device).eval()  # the caller's model keeps its mode
        self.n_classes = model.n_classes
        self._codes_c = (ctypes.c_int32 * self.ns)(*self.codes)
        self._work = {}   # (F, H, W) -> (geometry, device work list)
        self._tiles = {}  # C -> the gather's batch buffer

    def _geometry(self, F, H, W):
        key = (F, H, W)
        if key not in self._work:
            geo = TileGeometry(H, W, self.tile_in)
            self._work[key] = (geo, work_list(F, len(geo)).to(self.device))
        return self._work[key]

    @torch.no_grad()
    def predict(self, frames, want=("mask",)) -> dict:
        """frames (F, H, W) or (F, C, H, W), uint8 (normalised as predict.py
        does, ((v / 255) - 0.5) / 0.5) or float32 (used as they are); a stack on
        the device is used in place, a host stack is uploaded once.  Returns
        device tensors for the names in `want`: "mask" (F, H, W) uint8 =
        255 * (mean p1 > threshold), "prob" (F, K, H, W) fp32 mean softmax,
        "logits" (F, K, H, W), single symmetry only."""
        want = tuple(want)
        if not want or any(n not in OUTPUTS for n in want):
            raise ValueError(f"want must name some of {OUTPUTS}, got {want!r}")
        if "logits" in want and self.ns != 1:
            raise ValueError("logits are returned for a single symmetry only")
        if "mask" in want and self.n_classes != 2:
            raise ValueError("the mask needs 2 classes")
        if frames.dim() == 3:
            frames = frames[:, None]
        if frames.dim() != 4 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError("frames must be (F, H, W) or (F, C, H, W), uint8 or float32")
        frames = frames.to(self.device).contiguous()
        F, C, H, W = frames.shape
        if F < 1:
            raise ValueError("no frames")
        geo, work = self._geometry(F, H, W)
        K, ti, to, ns = self.n_classes, geo.tile_in, geo.tile_out, self.ns
        dev = self.device
        out = {}
        if "mask" in want:
            out["mask"] = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
        if "prob" in want:
            out["prob"] = torch.zeros((F, K, H, W), dtype=torch.float32, device=dev)
        if "logits" in want:
            out["logits"] = torch.zeros((F, K, H, W), dtype=torch.float32, device=dev)
        tiles = self._tiles.get(C)
        if tiles is None:
            tiles = self._tiles[C] = torch.empty((self.batch, C, ti, ti), dtype=torch.float32, device=dev)
        lib = _lib.load()
        per = self.batch // ns
        total = work.shape[0]
        with torch.cuda.device(dev):
            for s in range(0, total, per):
                ng = min(per, total - s)
                st = _lib.stream_of(dev)
                wp = work.data_ptr() + 8 * s
                _lib.check(lib.unet_seq_tile_gather(frames.data_ptr(), 1 if frames.dtype == torch.uint8 else 0, F, C,
                                                    H, W, ti, to, geo.pads[0], geo.pads[2], geo.nx, wp, ng,
                                                    self._codes_c, ns, tiles.data_ptr(), st), "unet_seq_tile_gather")
                logits = self.model(tiles[:ng * ns]).float().contiguous()
                _lib.check(lib.unet_seq_tile_reduce(logits.data_ptr(), K, to, geo.nx, wp, ng, self._codes_c, ns, F, H,
                                                    W, self.threshold, _lib.ptr(out.get("prob")),
                                                    _lib.ptr(out.get("mask")), _lib.ptr(out.get("logits")), st),
                           "unet_seq_tile_reduce")
        return out
