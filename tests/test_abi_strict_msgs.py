"""The entry points of the strict verification over messages of any length
(include/narwhal_amd.h): exported by the library, declared in the header and for ctypes alike,
and, like every other device entry, failing with NW_E_NO_DEVICE when no gfx950 device is
visible (the host entry needs none: tests/test_host_strict_msgs.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

# name -> number of parameters in the header
SYMBOLS = {"nw_verify_strict_msgs_many": 8, "nw_submit_verify_strict_msgs": 9,
           "nw_dev_verify_strict_msgs_many": 9, "nw_host_verify_strict_msgs_many": 7}


def test_symbols_exported_and_declared():
    L = _lib.lib()
    txt = open(_lib.HEADER).read()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.header_symbols()
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(fn.argtypes), name


def test_every_header_symbol_has_a_prototype():
    assert not set(_lib.header_symbols()) - set(_lib.prototypes())


def test_python_names():
    assert "verify_strict_msgs_many" in C.__all__ and callable(C.verify_strict_msgs_many)
    assert callable(C.Signature.verify_message)
    with pytest.raises(ValueError):
        C.verify_strict_msgs_many([b"abc", b"de"], np.zeros((1, 32), np.uint8),
                                  np.zeros((1, 64), np.uint8))
    with pytest.raises(ValueError):   # the message ends behind the data
        C.verify_strict_msgs_many((np.zeros(4, np.uint8), [2], [3]), np.zeros((1, 32), np.uint8),
                                  np.zeros((1, 64), np.uint8))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device():
    L = _lib.lib()
    off = (ctypes.c_uint64 * 1)(0)
    ln = (ctypes.c_uint64 * 1)(3)
    st = ctypes.c_int32(0)
    assert L.nw_verify_strict_msgs_many(b"abc", off, ln, b"\0" * 32, b"\0" * 64, 1,
                                        ctypes.byref(st), None) == -2   # NW_E_NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert L.nw_submit_verify_strict_msgs(b"abc", off, ln, b"\0" * 32, b"\0" * 64, 1,
                                          ctypes.byref(st), None,
                                          ctypes.byref(ctypes.c_void_p())) == -2
    assert L.nw_dev_verify_strict_msgs_many(None, None, None, None, None, 1, None, None,
                                            None) == -2
    assert L.nw_verify_strict_msgs_many(None, None, None, None, None, 0, None, None) == -2
    with pytest.raises(_lib.EngineError):
        C.verify_strict_msgs_many([b"abc"], np.zeros((1, 32), np.uint8),
                                  np.zeros((1, 64), np.uint8))
    with pytest.raises(_lib.EngineError):
        C.Signature(bytes(32), bytes(32)).verify_message(b"abc", C.PublicKey(bytes(32)))
