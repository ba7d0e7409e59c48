"""nw_host_verify_strict_msgs_many (narwhal_amd/csrc/nw_host.cpp: the host path's strict check
with k hashed over a message of any length) against the oracle over the corpus of
tests/strict_msgs_cases.py, and against nw_host_verify_strict_many over the golden edge corpus
of 32-byte messages. No device needed."""
import ctypes

import numpy as np

from narwhal_amd import _lib

import strict_msgs_cases as SM


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_msgs(data, offsets, lengths, pks, sigs):
    n = len(offsets)
    st = np.full(max(n, 1), -99, np.int32)
    rc = _lib.lib().nw_host_verify_strict_msgs_many(_p(data), _p(offsets), _p(lengths), _p(pks),
                                                    _p(sigs), n, _p(st))
    assert rc == 0
    return st[:n]


def test_corpus_matches_oracle():
    c = SM.corpus()
    assert 1000 <= c.n <= 1100
    st = host_msgs(c.data, c.offsets, c.lengths, c.pks, c.sigs)
    bad = np.nonzero(st != c.ref)[0]
    assert bad.size == 0, [(int(i), c.variant[i], int(c.lengths[i]), int(st[i]), int(c.ref[i]))
                           for i in bad[:8]]


def test_tiled_corpus_is_the_corpus_repeated():
    t = SM.tiled()
    c = SM.corpus()
    assert t.n == 4096 and np.array_equal(t.ref[:c.n], c.ref)
    assert len({p.tobytes() for p, v in zip(t.pks, t.variant) if v != "a_off_curve"}) == 8


def test_golden_edge_corpus_equals_the_32_byte_entry(golden):
    msgs, pks, sigs, exp = SM.golden_edge(golden)
    n = len(exp)
    data = np.ascontiguousarray(msgs).reshape(-1)
    offsets = (32 * np.arange(n)).astype(np.uint64)
    lengths = np.full(n, 32, np.uint64)
    st = host_msgs(data, offsets, lengths, pks, sigs)
    st32 = np.full(n, -99, np.int32)
    assert _lib.lib().nw_host_verify_strict_many(_p(msgs), 32, _p(pks), _p(sigs), n,
                                                 _p(st32)) == 0
    assert np.array_equal(st, exp)
    assert np.array_equal(st, st32)


def test_no_items_is_ok():
    assert _lib.lib().nw_host_verify_strict_msgs_many(None, None, None, None, None, 0, None) == 0


def test_null_pointer_is_refused():
    st = np.zeros(1, np.int32)
    assert _lib.lib().nw_host_verify_strict_msgs_many(None, None, None, None, None, 1,
                                                      _p(st)) == -1   # NW_E_INVALID_ARG
