"""nw_batch_signers_stats of the C ABI (include/narwhal_amd.h): exported by the library, declared
in the header and for ctypes, and, like every other entry, failing with NW_E_NO_DEVICE when no
gfx950 device is visible."""
import ctypes
import os

import pytest

from narwhal_amd import _lib
from narwhal_amd import crypto as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    L = _lib.lib()
    assert hasattr(L, "nw_batch_signers_stats")
    assert "nw_batch_signers_stats" in _lib.header_symbols()
    with open(os.path.join(ROOT, "include", "narwhal_amd.h")) as f:
        assert "int nw_batch_signers_stats(uint64_t out[4]);" in f.read()
    assert L.nw_batch_signers_stats.restype is ctypes.c_int
    assert "batch_signers_stats" in C.__all__


def test_no_device():
    L = _lib.lib()
    out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert L.nw_batch_signers_stats(out) == -2            # NW_E_NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert list(out) == [7, 7, 7, 7]
    with pytest.raises(_lib.EngineError):
        C.batch_signers_stats()
