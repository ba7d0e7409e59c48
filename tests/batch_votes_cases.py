"""Inputs and expectations shared by the tests of verify_batch leaving the comb-passed votes out
of a failing batch's sum (test infrastructure, built with the oracle alone): the six counters a
call must report, taken from the input, the oracle's verdict of a batch over the votes that did
not pass with the index mapped back, and a vote under a key nobody registered."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

import batch_signers_cases as BS


def honest(sizes, seed, nkeys=16):
    """Batches of the given sizes, every vote valid under one of nkeys honest keys."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(nkeys)]
    sizes = np.asarray(sizes, np.int64)
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    dig = rng.integers(0, 256, size=(len(sizes), 32), dtype=np.uint8)
    key = rng.integers(0, nkeys, size=n)
    msgs = BS.digests_of(dig, off)
    pk = np.array([np.frombuffer(kps[k][0], np.uint8) for k in key]).reshape(n, 32).copy()
    sigs = np.array([np.frombuffer(O.sign(kps[k][1], m.tobytes()), np.uint8)
                     for k, m in zip(key, msgs)]).reshape(n, 64).copy()
    keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps])
    return dig, pk, sigs, off, keys


def stranger(rng):
    """A key pair of the caller's that no corpus registers."""
    return O.keypair_from_seed(rng.bytes(32))


def resign(pk, sigs, i, kp, digest: bytes):
    """Vote i becomes a valid vote over `digest` under the key pair kp."""
    pk[i] = np.frombuffer(kp[0], np.uint8)
    sigs[i] = np.frombuffer(O.sign(kp[1], digest), np.uint8)


def six(dig, pk, sigs, off, reg, leave_out=True):
    """The four counters of nw_batch_signers_stats (batch_signers_cases.expected) and the two of
    nw_batch_signers_vote_stats: over the batches sent on, the votes the comb check passed (left
    out of the sum) and the others (run in it); with leave_out False (NW_BATCH_SIGNERS_VOTES=0)
    nothing is left out and every vote of such a batch runs."""
    passed, settled, four = BS.expected(dig, pk, sigs, off, reg)
    sizes = np.diff(off.astype(np.int64))
    sent = np.repeat(~settled, sizes)
    left, run = int((passed & sent).sum()), int((~passed & sent).sum())
    return four, ((left, run) if leave_out else (0, left + run))


def reduced(digest: bytes, pk, sigs, z16, keep):
    """The oracle's (status, index) of one batch over the votes keep[i] alone, with their own
    coefficient rows, the index mapped back to the whole batch: a failing vote's position is its
    original one, and statuses 0 and 7 carry the batch's size."""
    pos = np.nonzero(keep)[0]
    z = z16[pos] if len(pos) else np.zeros((1, 16), np.uint8)
    st, ix = O.verify_batch(digest, pk[pos], sigs[pos], z)
    return int(st), (len(pk) if st in (0, 7) else int(pos[int(ix)]))
