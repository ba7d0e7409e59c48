"""nw_batch_signers_vote_stats of the C ABI (include/narwhal_amd.h): exported by the library,
declared in the header and for ctypes, wrapped by crypto.batch_signers_vote_stats, and, like
every other entry, failing with NW_E_NO_DEVICE when no gfx950 device is visible."""
import ctypes
import os

import pytest

from narwhal_amd import _lib
from narwhal_amd import crypto as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    L = _lib.lib()
    assert hasattr(L, "nw_batch_signers_vote_stats")
    assert "nw_batch_signers_vote_stats" in _lib.header_symbols()
    with open(os.path.join(ROOT, "include", "narwhal_amd.h")) as f:
        assert "int nw_batch_signers_vote_stats(uint64_t out[2]);" in f.read()
    assert L.nw_batch_signers_vote_stats.restype is ctypes.c_int
    assert "batch_signers_vote_stats" in C.__all__


def test_no_device():
    L = _lib.lib()
    out = (ctypes.c_uint64 * 2)(7, 7)
    assert L.nw_batch_signers_vote_stats(out) == -2            # NW_E_NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert list(out) == [7, 7]
    with pytest.raises(_lib.EngineError):
        C.batch_signers_vote_stats()
