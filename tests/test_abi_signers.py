"""The registered-signers entry points of the C ABI (include/narwhal_amd.h): exported by the
library, declared for ctypes, and, like every other entry, failing with NW_E_NO_DEVICE when no
gfx950 device is visible."""
import ctypes

import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

SYMBOLS = ("nw_strict_signers_set", "nw_strict_signers_count", "nw_dev_strict_signers_stats")


def test_symbols_exported():
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.header_symbols()
        assert getattr(L, name).restype is ctypes.c_int


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device():
    L = _lib.lib()
    keys = (ctypes.c_uint8 * 64)()
    assert L.nw_strict_signers_set(keys, 2) == -2            # NW_E_NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert L.nw_strict_signers_set(None, 0) == -2
    n = ctypes.c_uint64(7)
    assert L.nw_strict_signers_count(ctypes.byref(n)) == -2 and n.value == 7
    out = (ctypes.c_uint64 * 3)()
    assert L.nw_dev_strict_signers_stats(out, None) == -2
    with pytest.raises(_lib.EngineError):
        C.set_strict_signers([C.PublicKey(bytes(32))])
    with pytest.raises(_lib.EngineError):
        C.strict_signers_count()
    with pytest.raises(_lib.EngineError):
        C.strict_signers_stats()
