"""Helpers shared by the exact GPU tests (tests/test_wgrad_exact_gpu.py, tests/test_conv_exact_gpu.py): tensors between NaN guard
bands, and a launch through the C ABI that ends the session on a GPU fault."""
import ctypes as C

import pytest
import torch

from stlpose_amd import capi

GUARD = 64 * 1024   # bytes of NaN on each side of a tensor
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(fn, params):
    """Launch, synchronise and check both return codes.  A GPU fault ends the whole session: nothing more is started on a
    device that has faulted."""
    rc = getattr(capi.lib(), fn)(C.byref(params), stream())
    err = capi.lib().stl_last_error().decode() if rc else ""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in {fn} ({capi.lib().stl_last_kernel().decode()}): {e}", returncode=3)
    if "illegal" in err or "fault" in err:
        pytest.exit(f"GPU fault in {fn}: {err}", returncode=3)
    return rc, err


class Guarded:
    """n elements between two NaN bands of GUARD bytes."""

    def __init__(self, n, dtype, data=None):
        self.gel = GUARD // torch.empty((), dtype=dtype).element_size()
        self.whole = torch.full((n + 2 * self.gel,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.whole[self.gel:self.gel + n]
        self.bits = _BITS[self.whole.element_size()]
        self.nan = self.whole[:1].view(self.bits).clone()
        if data is not None:
            self.t.copy_(data.reshape(-1).to(dtype))
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def bands_intact(self):
        lo, hi = self.whole[:self.gel].view(self.bits), self.whole[self.gel + self.t.numel():].view(self.bits)
        return bool((lo == self.nan).all()) and bool((hi == self.nan).all())
