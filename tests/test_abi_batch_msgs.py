"""The entry points of verify_batch over per-vote messages of any length
(include/narwhal_amd.h): exported by the library, declared in the header and for ctypes alike,
and, like every other device entry, failing with NW_E_NO_DEVICE when no gfx950 device is
visible (the host entry needs none: tests/test_batch_msgs_cpu.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

# name -> (result type in the header, number of parameters)
SYMBOLS = {"nw_signature_verify_batch_msgs": ("int", 8), "nw_verify_batch_msgs_many": ("int", 10),
           "nw_submit_verify_batch_msgs": ("int", 11),
           "nw_dev_verify_batch_msgs_workspace": ("size_t", 2),
           "nw_dev_verify_batch_msgs_many": ("int", 15),
           "nw_host_verify_batch_msgs_many": ("int", 10)}


def test_symbols_exported_and_declared():
    L = _lib.lib()
    txt = open(_lib.HEADER).read()
    for name, (res, nargs) in SYMBOLS.items():
        assert name in _lib.header_symbols()
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_int if res == "int" else ctypes.c_size_t)
        decl = re.search(r"\b" + res + " " + name + r"\s*\(([^;]*)\);", txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(fn.argtypes), name


def test_every_header_symbol_has_a_prototype():
    assert not set(_lib.header_symbols()) - set(_lib.prototypes())


def test_workspace_holds_the_plane():
    L = _lib.lib()
    for nb, n in ((1, 1), (7, 100), (3, 4096)):
        assert (L.nw_dev_verify_batch_msgs_workspace(nb, n)
                >= L.nw_dev_verify_batch_workspace(nb, n) + 32 * n)


def test_python_names():
    assert "verify_batch_msgs_many" in C.__all__ and callable(C.verify_batch_msgs_many)
    assert callable(C.Signature.verify_batch_messages)
    pk, sig = np.zeros((2, 32), np.uint8), np.zeros((2, 64), np.uint8)
    with pytest.raises(ValueError):   # three messages, two votes
        C.verify_batch_msgs_many([b"a", b"b", b"c"], pk, sig, [0, 2])
    with pytest.raises(ValueError):   # two keys, one signature
        C.verify_batch_msgs_many([b"a", b"b"], pk, sig[:1], [0, 2])
    with pytest.raises(ValueError):   # the batches do not cover the votes
        C.verify_batch_msgs_many([b"a", b"b"], pk, sig, [0, 1])
    with pytest.raises(ValueError):   # the second message ends behind the data
        C.verify_batch_msgs_many((np.zeros(4, np.uint8), [0, 2], [2, 3]), pk, sig, [0, 2])
    with pytest.raises(ValueError):   # a byte of a message, and no data at all
        C.verify_batch_msgs_many((np.zeros(0, np.uint8), [0], [1]), pk[:1], sig[:1], [0, 1])
    with pytest.raises(ValueError):   # offset + length wraps 64 bits
        C.verify_batch_msgs_many((np.zeros(4, np.uint8), [2**64 - 1], [2]), pk[:1], sig[:1],
                                 [0, 1])
    with pytest.raises(ValueError):   # 16 bytes of z per vote
        C.verify_batch_msgs_many([b"a", b"b"], pk, sig, [0, 2], z16=np.zeros(16, np.uint8))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device():
    L = _lib.lib()
    mo = (ctypes.c_uint64 * 1)(0)
    ml = (ctypes.c_uint64 * 1)(3)
    off = (ctypes.c_uint64 * 2)(0, 1)
    st = ctypes.c_int32(0)
    fi = ctypes.c_uint64(0)
    idx = ctypes.c_size_t(0)
    NO_DEVICE = -2
    assert L.nw_signature_verify_batch_msgs(b"abc", mo, ml, b"\0" * 32, b"\0" * 64, 1, None,
                                            ctypes.byref(idx)) == NO_DEVICE
    assert b"gfx950" in L.nw_last_error()
    assert L.nw_signature_verify_batch_msgs(None, None, None, None, None, 0, None,
                                            None) == NO_DEVICE
    assert L.nw_verify_batch_msgs_many(b"abc", mo, ml, b"\0" * 32, b"\0" * 64, off, 1, None,
                                       ctypes.byref(st), ctypes.byref(fi)) == NO_DEVICE
    assert L.nw_verify_batch_msgs_many(None, None, None, None, None, None, 0, None, None,
                                       None) == NO_DEVICE
    job = ctypes.c_void_p()
    assert L.nw_submit_verify_batch_msgs(b"abc", mo, ml, b"\0" * 32, b"\0" * 64, off, 1, None,
                                         ctypes.byref(st), ctypes.byref(fi),
                                         ctypes.byref(job)) == NO_DEVICE
    assert L.nw_submit_verify_batch_msgs(None, None, None, None, None, None, 0, None, None, None,
                                         ctypes.byref(job)) == NO_DEVICE
    assert L.nw_dev_verify_batch_msgs_many(None, None, None, None, None, None, None, 1, 1, None,
                                           None, None, None, None, None) == NO_DEVICE
    assert L.nw_dev_verify_batch_msgs_many(None, None, None, None, None, None, None, 0, 0, None,
                                           None, None, None, None, None) == NO_DEVICE
    with pytest.raises(_lib.EngineError):
        C.verify_batch_msgs_many([b"abc"], np.zeros((1, 32), np.uint8),
                                 np.zeros((1, 64), np.uint8), [0, 1])
    with pytest.raises(_lib.EngineError):
        C.Signature.verify_batch_messages(
            [(b"abc", C.PublicKey(bytes(32)), C.Signature(bytes(32), bytes(32)))])
    C.Signature.verify_batch_messages([])   # an empty iterable is Ok, device or not
