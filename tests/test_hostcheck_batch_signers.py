"""Signature::verify_batch under the registered signers on the CPU (tools/hostcheck.hip
hc_batch_signers_many: a call as launch_batch_signers runs it: the registry's hash table, each
key's lambda (nw_strict.hpp key_lambda, the text k_key_lambda runs at registration), every vote
through batch_signers_vote, the per-batch word and the four counters). lambda against [l]A from
the oracle's point arithmetic; the settled batches against the oracle's per-vote strict
statuses and against its verify_batch under several coefficient sets."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

import irregular as IR
import batch_signers_cases as BS
from test_hostcheck import LIB, _build
from test_hostcheck_keyset import _hrams

PASS, FAIL = 0, 1    # nw_strict.hpp kVotePass, kVoteFail


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    lib.hc_batch_signers_many.restype = ctypes.c_int
    lib.hc_batch_signers_many.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [
        ctypes.c_uint32] + [ctypes.c_void_p] * 4
    lib.hc_key_lambda.restype = ctypes.c_int
    lib.hc_key_lambda.argtypes = [ctypes.c_char_p]
    return lib


def _P(a):
    return ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)


def _run(hc, dig, pk, sigs, off, reg):
    """Settled words, the registry's lambda array, the votes' final states and the counters."""
    reg = np.ascontiguousarray(reg, np.uint8).reshape(-1, 32)
    pk, sigs = np.ascontiguousarray(pk, np.uint8), np.ascontiguousarray(sigs, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    nb, n = len(off) - 1, len(pk)
    k = _hrams(BS.digests_of(dig, off), pk, sigs) if n else np.zeros((0, 32), np.uint8)
    k = np.ascontiguousarray(k, np.uint8)
    settled = np.full(nb, 77, np.uint32)
    lam = np.full(len(reg), 77, np.uint32)
    state = np.full(n, 77, np.uint32)
    stats = np.zeros(4, np.uint64)
    assert hc.hc_batch_signers_many(_P(reg), len(reg), _P(pk), _P(sigs), _P(k), _P(off), nb,
                                    _P(settled), _P(lam), _P(state), _P(stats)) == 0
    return settled, lam, state, tuple(int(x) for x in stats)


def test_lambda(hc):
    """The 8 small-order points (lambda = 5 j mod 8 for [j]T8), A = aB + T for every nonzero
    torsion point T, honest keys (0), and an undecodable key: hc_key_lambda and the registry's
    array against [l]A from the oracle."""
    rng = np.random.Generator(np.random.PCG64(1201))
    tors = IR.torsion_points()
    keys = list(tors)
    for j in range(1, 8):
        keys.append(O.point_add(O.scalarmult_base(IR._rand_scalar(rng)), tors[j]))
    keys += [O.keypair_from_seed(rng.bytes(32))[0] for _ in range(4)]
    ref = [BS.lam_ref(k) for k in keys]
    assert ref[:8] == [5 * j % 8 for j in range(8)]
    assert ref[8:15] == [5 * j % 8 for j in range(1, 8)] and ref[15:] == [0] * 4
    for k, want in zip(keys, ref):
        assert hc.hc_key_lambda(k) == want, k.hex()
    bad = IR._le(2)
    assert O.decompress(bad) is None and hc.hc_key_lambda(bad) == -1
    reg = np.array([np.frombuffer(k, np.uint8) for k in keys + [bad]])
    off = np.zeros(1, np.uint64)
    _, lam, _, stats = _run(hc, np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8),
                            np.zeros((0, 64), np.uint8), off, reg)
    assert lam.tolist() == ref + [0] and stats == (0, 0, 0, 0)


@pytest.fixture(scope="module")
def corpus():
    """200 batches of 0..12 votes under 16 keys, a third of the non-empty ones with one vote
    broken (every failure class); built once."""
    return BS.corpus(200, seed=1202)


@pytest.mark.parametrize("nreg", [16, 9, 0])
def test_settled_batches(hc, corpus, nreg):
    """With all, some and none of the keys registered: a vote passes iff the oracle's strict
    status is 0 and its key is registered (lambda 0), a batch is settled iff all its votes pass,
    the counters are those counts, and every settled batch is Ok under the oracle's verify_batch
    for 4 coefficient sets."""
    dig, pk, sigs, off, keys = corpus
    reg = keys[:nreg]
    passed, exp_settled, counts = BS.expected(dig, pk, sigs, off, reg)
    settled, lam, state, stats = _run(hc, dig, pk, sigs, off, reg)
    assert np.all(lam == 0)
    assert np.array_equal(state == PASS, passed) and set(state.tolist()) <= {PASS, FAIL}
    assert np.array_equal(settled.astype(bool), exp_settled)
    assert stats == counts and stats[0] + stats[1] == len(pk) and stats[2] + stats[3] == 200
    sizes = np.diff(off.astype(np.int64))
    if nreg == 16:
        # every failure class occurs, and the broken batches are exactly those sent on
        strict = O.verify_strict_many(BS.digests_of(dig, off), pk, sigs)
        assert len(set(strict.tolist()) - {0}) == 6 and 60 < stats[2] < 200
    if nreg == 0:
        assert stats[0] == 0 and np.array_equal(exp_settled, sizes == 0)
    rng = np.random.Generator(np.random.PCG64(1203))
    o = off.astype(np.int64)
    for b in np.nonzero(settled)[0]:
        a, e = o[b], o[b + 1]
        for _ in range(4):
            z = rng.integers(0, 256, size=(max(e - a, 1), 16), dtype=np.uint8)
            assert O.verify_batch(dig[b].tobytes(), pk[a:e], sigs[a:e], z)[0] == 0, b


def test_mixed_order_key_is_never_settled(hc):
    """8 six-vote batches, each holding one strict-valid vote under a registered mixed-order
    key A = aB + T: every vote's strict status is 0, yet the oracle's verify_batch says Ok under
    some coefficient sets and NW_ERR_EQUATION under others, so no such batch may be settled;
    the honest votes beside it pass."""
    dig, pk, sigs, off, keys, zs = BS.mixed_batches(seed=1204)
    strict = O.verify_strict_many(BS.digests_of(dig, off), pk, sigs)
    assert np.all(strict == 0)
    verdicts = np.array([[O.verify_batch(dig[b].tobytes(), pk[6 * b:6 * b + 6],
                                         sigs[6 * b:6 * b + 6], z[6 * b:6 * b + 6])[0]
                          for z in zs] for b in range(8)])
    assert set(verdicts.ravel().tolist()) == {0, 7}, verdicts
    assert BS.lam_ref(keys[-1].tobytes()) != 0
    settled, lam, state, stats = _run(hc, dig, pk, sigs, off, keys)
    assert not settled.any() and stats == (40, 8, 0, 8)
    assert lam[-1] == BS.lam_ref(keys[-1].tobytes()) and np.all(lam[:-1] == 0)
    mixed = np.array([p.tobytes() == keys[-1].tobytes() for p in pk])
    assert np.array_equal(state == FAIL, mixed)
    assert BS.expected(dig, pk, sigs, off, keys)[2] == stats
    # without the mixed-order key's lambda (the key left out) the votes under it fail as strangers
    assert _run(hc, dig, pk, sigs, off, keys[:-1])[3] == (40, 8, 0, 8)
