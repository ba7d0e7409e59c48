"""verify_batch over per-vote messages of any length, without a device: the checker of
tests/batch_msgs_cases.py pinned against the oracle's verify_batch wherever the two can be
compared (every vote's message = the batch digest), then the engine's own host arithmetic
(nw_host_verify_batch_msgs_many) against the checker, exactly, over the corpus under injected
coefficients, and against nw_host_verify_batch_many on the golden batches."""
import ctypes

import numpy as np
import pytest

from narwhal_amd import _lib
from oracle import oracle as O

import batch_msgs_cases as BM
import batch_signers_cases as BS


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_msgs(c):
    st = np.full(max(c.nb, 1), -99, np.int32)
    fi = np.full(max(c.nb, 1), 2**63, np.uint64)
    data = c.data if c.data.size else np.zeros(1, np.uint8)
    rc = _lib.lib().nw_host_verify_batch_msgs_many(_p(data), _p(c.moffs), _p(c.mlens), _p(c.pks),
                                                   _p(c.sigs), _p(c.off), c.nb, _p(c.z), _p(st),
                                                   _p(fi))
    assert rc == 0
    return st[:c.nb], fi[:c.nb]


def same(c, got, what=""):
    st, fi = got
    bad = [(c.names[b], int(st[b]), int(fi[b]), int(c.ref_st[b]), int(c.ref_ix[b]))
           for b in range(c.nb) if st[b] != c.ref_st[b] or fi[b] != c.ref_ix[b]]
    assert not bad, (what, bad[:8])


# ---- the checker is pinned first ----------------------------------------------------------
def test_checker_equals_oracle_on_golden_batches(golden):
    c, dig, exp_st, exp_ix = BM.golden_call(golden)
    assert c.nb == 13
    assert {"order_A_decode_before_s_high", "torsion_residual_z_cancels",
            "torsion_residual_z_exposes"} <= set(c.names)
    o = c.off.astype(np.int64)
    for b in range(c.nb):
        ref = O.verify_batch(dig[b].tobytes(), c.pks[o[b]:o[b + 1]], c.sigs[o[b]:o[b + 1]],
                             c.z[o[b]:o[b + 1]] if o[b + 1] > o[b] else None)
        assert (int(c.ref_st[b]), int(c.ref_ix[b])) == ref == (exp_st[b], exp_ix[b]), c.names[b]


def test_checker_equals_oracle_on_mixed_order_batches():
    dig, pk, sigs, off, _, zs = BS.mixed_batches(41)
    o = off.astype(np.int64)
    seen = set()
    for z in zs:
        c = BM.digest_call(dig, pk, sigs, off, z)
        for b in range(c.nb):
            ref = O.verify_batch(dig[b].tobytes(), pk[o[b]:o[b + 1]], sigs[o[b]:o[b + 1]],
                                 z[o[b]:o[b + 1]])
            assert (int(c.ref_st[b]), int(c.ref_ix[b])) == ref, (b, ref)
            seen.add(ref[0])
    assert seen == {0, 7}   # the torsion residual: the verdict depends on z


# ---- the host entry against the checker ---------------------------------------------------
def test_host_entry_equals_checker_on_corpus():
    c = BM.corpus()
    same(c, host_msgs(c), "corpus")
    # batch by batch in reverse order: no verdict depends on a batch's place in the call
    r = c.take(range(c.nb - 1, -1, -1))
    same(r, host_msgs(r), "reversed")


def test_host_entry_empty_messages_and_empty_calls():
    c = BM.all_empty()
    same(c, host_msgs(c), "empty messages")
    L = _lib.lib()
    assert L.nw_host_verify_batch_msgs_many(None, None, None, None, None, None, 0, None, None,
                                            None) == 0
    # a call of empty batches only
    off = np.zeros(4, np.uint64)
    st = np.full(3, -99, np.int32)
    fi = np.full(3, 99, np.uint64)
    assert L.nw_host_verify_batch_msgs_many(None, None, None, None, None, _p(off), 3, None, _p(st),
                                            _p(fi)) == 0
    assert st.tolist() == [0, 0, 0] and fi.tolist() == [0, 0, 0]
    # a message without data is an argument error, not a read through a null pointer
    one = BM.corpus().take([1])
    assert L.nw_host_verify_batch_msgs_many(None, _p(one.moffs), _p(one.mlens), _p(one.pks),
                                            _p(one.sigs), _p(one.off), 1, _p(one.z), _p(st),
                                            _p(fi)) == -1


def test_host_entry_equals_digest_entry_on_golden_batches(golden):
    c, dig, exp_st, exp_ix = BM.golden_call(golden)
    st, fi = host_msgs(c)
    same(c, (st, fi), "golden")
    assert np.array_equal(st, exp_st) and np.array_equal(fi, exp_ix)
    st32 = np.full(c.nb, -99, np.int32)
    fi32 = np.full(c.nb, 99, np.uint64)
    assert _lib.lib().nw_host_verify_batch_many(_p(dig), _p(c.pks), _p(c.sigs), _p(c.off), c.nb,
                                                _p(c.z), _p(st32), _p(fi32)) == 0
    assert np.array_equal(st, st32) and np.array_equal(fi, fi32)
    by = dict(zip(c.names, st.tolist()))
    assert by["torsion_residual_z_cancels"] == 0 and by["torsion_residual_z_exposes"] == 7


def test_host_entry_random_coefficients():
    """z16 = NULL (ChaCha20 keyed by the OS CSPRNG), on the deterministic subset: an all-valid
    batch is Ok and a prime-order residual (a flipped message byte) is 7 for every z."""
    c = BM.corpus()
    pick = [b for b, nm in enumerate(c.names)
            if nm.startswith("valid_") or nm.startswith("msg_last_flipped_")]
    c = c.take(pick)
    st = np.full(c.nb, -99, np.int32)
    assert _lib.lib().nw_host_verify_batch_msgs_many(_p(c.data), _p(c.moffs), _p(c.mlens),
                                                     _p(c.pks), _p(c.sigs), _p(c.off), c.nb, None,
                                                     _p(st), None) == 0
    assert np.array_equal(st, c.ref_st) and set(st.tolist()) == {0, 7}
