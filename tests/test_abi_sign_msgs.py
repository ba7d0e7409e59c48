"""The entry points of signing over messages of any length (include/narwhal_amd.h): exported by
the library, declared in the header and for ctypes alike, and, like every other device entry,
failing with NW_E_NO_DEVICE when no gfx950 device is visible."""
import ctypes
import re

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

# name -> number of parameters in the header
SYMBOLS = {"nw_sign_msgs_many": 7, "nw_dev_sign_msgs_many": 8}


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
    assert not set(_lib.header_symbols()) - set(_lib.prototypes())


def test_python_names():
    assert "sign_msgs_many" in C.__all__ and callable(C.sign_msgs_many)
    assert callable(C.Signature.new_message)
    with pytest.raises(ValueError):   # two messages, one key
        C.sign_msgs_many(np.zeros((1, 64), np.uint8), [b"abc", b"de"])
    with pytest.raises(ValueError):   # two keys, one message
        C.sign_msgs_many(np.zeros((2, 64), np.uint8), [b"abc"])
    with pytest.raises(ValueError):   # a shared key is one key
        C.sign_msgs_many(np.zeros((2, 64), np.uint8), [b"abc", b"de"], shared_key=True)
    with pytest.raises(ValueError):   # the message ends behind the data
        C.sign_msgs_many(np.zeros((1, 64), np.uint8), (np.zeros(4, np.uint8), [2], [3]))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device():
    L = _lib.lib()
    off = (ctypes.c_uint64 * 1)(0)
    ln = (ctypes.c_uint64 * 1)(3)
    out = ctypes.create_string_buffer(64)
    assert L.nw_sign_msgs_many(b"\0" * 64, 64, b"abc", off, ln, 1, out) == -2   # NW_E_NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert L.nw_dev_sign_msgs_many(None, 64, None, None, None, 1, None, None) == -2
    assert L.nw_sign_msgs_many(None, 64, None, None, None, 0, None) == -2
    assert L.nw_dev_sign_msgs_many(None, 64, None, None, None, 0, None, None) == -2
    assert L.nw_sign_msgs_many(b"\0" * 64, 7, b"abc", off, ln, 1, out) == -2   # before the checks
    assert out.raw == bytes(64)
    with pytest.raises(_lib.EngineError):
        C.sign_msgs_many(np.zeros((1, 64), np.uint8), [b"abc"])
    with pytest.raises(_lib.EngineError):
        C.Signature.new_message(b"abc", C.SecretKey(bytes(64)))
