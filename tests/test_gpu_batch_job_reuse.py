"""One batch job serves the digest entry and the entry over per-vote messages (nw_jobs.cpp
submit_batch), so what one call leaves in a pooled job (the done word, the fused counters, the
mapped inputs, the comb phase's counters, the section offsets) meets the next call of the other
kind. One thread, so the pool hands the same job back: a lone fused batch, a message call, the
fused batch again, a digest call and the message call under the registered signers, then both
again with the registry cleared. Every status and failing index equals the checker's
(tests/batch_msgs_cases.py, tests/batch_votes_cases.py), and nw_batch_signers_stats moves on the
registered calls only, by the counts the inputs give."""
import ctypes

import numpy as np
import pytest

from narwhal_amd import _lib
from narwhal_amd import crypto as C
from oracle import oracle as O

import batch_msgs_cases as BM
import batch_signers_cases as BS
import batch_votes_cases as BV

pytestmark = pytest.mark.gpu

FUSED_N = 2925   # the smallest lone batch that takes the fused launches (tests/test_gpu_batch.py)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _digest_call(L, dig, pk, sigs, off, z):
    nb = len(off) - 1
    st = np.full(nb, -99, np.int32)
    fi = np.full(nb, 2**64 - 1, np.uint64)
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_batch_many(_p(dig), _p(pk), _p(sigs), _p(off), nb, _p(z), _p(st),
                                       _p(fi), ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    return st.tolist(), fi.tolist()


def test_one_job_through_both_entries():
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    rng = np.random.Generator(np.random.PCG64(1801))
    # the lone batch: one vote's s damaged, so the verdict comes from the sum (7, index n)
    fdig, fpk, fsig, foff, _ = BV.honest([FUSED_N], 1802)
    fsig[1234, 40] ^= 1
    fz = rng.integers(0, 256, size=(FUSED_N, 16), dtype=np.uint8)
    fref = BV.reduced(fdig[0].tobytes(), fpk, fsig, fz, np.ones(FUSED_N, bool))
    assert fref == (7, FUSED_N)
    # 3 x 5 votes over messages of their own, one message damaged
    m = BM.sized((5, 5, 5), 1803, ((1, 2, "msg_last_flipped"),))
    assert m.ref_st.tolist() == [0, 7, 0] and m.ref_ix.tolist() == [5, 5, 5]
    # 3 x 5 votes over batch digests, one vote's s damaged; the checker's verdict is that of the
    # same votes as a message call
    ddig, dpk, dsig, doff, dkeys = BV.honest([5, 5, 5], 1804)
    dsig[12, 40] ^= 1
    dz = rng.integers(0, 256, size=(15, 16), dtype=np.uint8)
    d = BM.digest_call(ddig, dpk, dsig, doff, dz)
    assert d.ref_st.tolist() == [0, 0, 7]
    reg = np.concatenate([dkeys, np.array([np.frombuffer(pk, np.uint8) for pk, _ in O.keys(8)])])

    def fused():
        fi = ctypes.c_size_t(99)
        st = L.nw_signature_verify_batch(_p(fdig), _p(fpk), _p(fsig), FUSED_N, _p(fz),
                                         ctypes.byref(fi))
        return st, fi.value

    def msgs():
        st, fi = C.verify_batch_msgs_many((m.data, m.moffs, m.mlens), m.pks, m.sigs, m.off, m.z)
        return st.tolist(), fi.tolist()

    def digests():
        return _digest_call(L, ddig, dpk, dsig, doff, dz)

    mref = (m.ref_st.tolist(), m.ref_ix.tolist())
    dref = (d.ref_st.tolist(), d.ref_ix.tolist())
    # every signer of the message call is registered and all its votes but the damaged one are
    # valid: 14 pass, 1 does not, its batch is sent on
    mcount = (14, 1, 2, 1)
    dcount = BS.expected(ddig, dpk, dsig, doff, reg)[2]
    assert dcount == (14, 1, 2, 1)
    none = (0, 0, 0, 0)
    steps = [("fused", fused, fref, none), ("messages", msgs, mref, none),
             ("fused again", fused, fref, none),
             ("set", None, None, None),
             ("digests, registered", digests, dref, dcount),
             ("messages, registered", msgs, mref, mcount),
             ("cleared", None, None, None),
             ("fused, cleared", fused, fref, none), ("messages, cleared", msgs, mref, none),
             ("digests, cleared", digests, dref, none)]
    try:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()
        for what, run, ref, count in steps:
            if run is None:
                keys = reg if what == "set" else reg[:0]
                assert L.nw_strict_signers_set(_p(keys) if len(keys) else None, len(keys)) == 0, \
                    L.nw_last_error()
                continue
            before = C.batch_signers_stats()
            got = run()
            delta = tuple(y - x for x, y in zip(before, C.batch_signers_stats()))
            assert got == ref, (what, got, ref)
            assert delta == count, (what, delta, count)
    finally:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()
