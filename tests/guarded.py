"""Guarded device buffers shared by the per-element GPU tests
(test_gpu_ops_elementwise.py, test_gpu_gemm_sites.py).

Every output and workspace is a slice of a larger allocation with a 256-byte
guard of 0xA5 on either side (`G`).  Outputs and workspaces start as 0xFF bytes
(a NaN as fp32 / fp64 / bf16).  `done()` requires every output element finite (it
was written) and every guard intact (nothing was written outside; a workspace
of exactly the *_ws_bytes size suffices)."""
import ctypes

import numpy as np
import torch

GUARD = 256      # bytes on either side; keeps the slice 256-byte aligned
PATTERN = 0xA5
_KEEP = []
_GUARDED = []
# (np.uint16 holds bf16 bit patterns; torch addresses them as int16)
_NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
         np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16}


def bf16_bits_to_f64(bits):
    """bf16 bit patterns (uint16) -> their values as float64."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


class G:
    """A device buffer of exactly `shape` x dtype inside a larger allocation:
    [guard | payload | guard].  The payload starts as 0xFF bytes (NaN for fp32 /
    fp64, all-ones for integers) unless `init` gives its contents.  bf16=True
    (dtype uint16): the payload holds bf16 values and is an output like a float."""

    def __init__(self, shape, dtype=np.float32, init=None, output=True, bf16=False):
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        self.dtype = np.dtype(dtype)
        self.bf16 = bf16
        assert not bf16 or self.dtype == np.dtype(np.uint16)
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * self.dtype.itemsize
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.bytes = self.raw[GUARD:GUARD + self.nbytes]
        self.bytes.fill_(0xFF)
        self.t = self.bytes.view(_NP2T[self.dtype]).view(shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=self.dtype)))
        # a float output must end up finite everywhere: it was written
        self.output = output and (self.dtype.kind == "f" or bf16)
        _GUARDED.append(self)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy().view(self.dtype)

    def f64(self):
        return bf16_bits_to_f64(self.np()) if self.bf16 else self.np().astype(np.float64)

    def check(self):
        for name, g in (("front", self.raw[:GUARD]), ("back", self.raw[GUARD + self.nbytes:])):
            bad = (g != PATTERN).nonzero().flatten().cpu().numpy()
            assert bad.size == 0, f"{name} guard of a {self.nbytes}-byte buffer overwritten at bytes {bad[:8]}"
        if self.output:
            a = self.f64() if self.bf16 else self.np()
            assert np.isfinite(a).all(), f"{int((~np.isfinite(a)).sum())} of {a.size} output elements not written"


def ws_buf(nbytes):
    """Workspace of exactly nbytes (0xFF-filled, guarded)."""
    return G(int(nbytes), np.uint8)


def done():
    """Synchronise, then check every guarded buffer of this test."""
    torch.cuda.synchronize()
    for g in _GUARDED:
        g.check()
    _GUARDED.clear()


def dev(a, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)
    _KEEP.append(t)
    return t


def begin():
    """Start of a test: no guarded buffer of an earlier one is pending."""
    _GUARDED.clear()


def release():
    """End of a test: drop the device tensors it kept alive."""
    torch.cuda.synchronize()
    _KEEP.clear()
    _GUARDED.clear()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
