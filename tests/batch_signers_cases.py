"""Inputs and expectations shared by the verify_batch-under-registered-signers tests (test
infrastructure, built with the oracle alone): a corpus of batches with every failure class, the
batches that hold one strict-valid vote under a mixed-order key, each key's torsion image
lambda from the oracle's point arithmetic, and the counts nw_batch_signers_stats must report,
taken from the input."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

import irregular as IR
from test_gpu_batch import _mutate

L_ORDER = IR.L_ORDER


def lam_ref(pk: bytes):
    """lambda with [l]A == [lambda]T8, or None when A does not decode. [l]A = [l - 1]A + A, so
    that the scalar handed to the oracle stays below l."""
    if O.decompress(pk) is None:
        return None
    lA = O.point_add(O.scalarmult(IR._le(L_ORDER - 1), pk), pk)
    # (point_add returns canonical encodings, as torsion_points does)
    hits = [j for j, t in enumerate(IR.torsion_points()) if lA == t]
    assert len(hits) == 1, pk.hex()
    return hits[0]


def digests_of(dig, off):
    """The digest each vote is signed over: its batch's."""
    sizes = np.diff(off.astype(np.int64))
    return dig[np.repeat(np.arange(len(sizes)), sizes)]


def corpus(nb, seed, max_n=12, nkeys=16, every=3):
    """nb batches of 0..max_n votes under nkeys honest keys; one vote of every `every`-th
    non-empty batch broken, the failure classes of test_gpu_batch._mutate in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(nkeys)]
    sizes = rng.integers(0, max_n + 1, size=nb)
    sizes[0] = 0
    off = np.zeros(nb + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    dig = rng.integers(0, 256, size=(nb, 32), dtype=np.uint8)
    key = rng.integers(0, nkeys, size=n)
    msgs = digests_of(dig, off)
    pk = np.array([np.frombuffer(kps[k][0], np.uint8) for k in key]).reshape(n, 32).copy()
    sigs = np.array([np.frombuffer(O.sign(kps[k][1], m.tobytes()), np.uint8)
                     for k, m in zip(key, msgs)]).reshape(n, 64).copy()
    for t, b in enumerate(np.nonzero(sizes)[0][::every]):
        _mutate(sigs, pk, int(off[b] + rng.integers(0, sizes[b])), t % 6)
    keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps])
    return dig, pk, sigs, off, keys


def mixed_vote(rng, mem, digest: bytes) -> bytes:
    """A signature over `digest` under the mixed-order member's key that dalek's verify_strict
    accepts: R = rB + T' with T' + kT == 0 (as test_hostcheck_signers.mixed_valid)."""
    tors = IR.torsion_points()
    while True:
        r = IR._rand_scalar(rng)
        Tp = tors[int(rng.integers(0, 8))]
        R = O.point_add(O.scalarmult_base(r), Tp)
        k = O.hram(R, mem.pk, digest)
        if O.point_add(Tp, O.scalarmult(k, mem.T)) == IR.IDENTITY:
            return R + O.scalar_add(r, O.scalar_mul(k, mem.a))


def mixed_batches(seed, nb=8, q=6, nz=8):
    """nb batches of q votes: q - 1 honest ones and, at a position that moves with the batch,
    one strict-valid vote under a mixed-order key A = aB + T. Returns the batches, the keys to
    register (the honest ones and A) and nz coefficient sets."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(q)]
    mem = IR.Member("mixed", rng)
    dig = rng.integers(0, 256, size=(nb, 32), dtype=np.uint8)
    pk = np.zeros((nb * q, 32), np.uint8)
    sigs = np.zeros((nb * q, 64), np.uint8)
    for b in range(nb):
        for t in range(q):
            i = b * q + t
            if t == b % q:
                pk[i] = np.frombuffer(mem.pk, np.uint8)
                sigs[i] = np.frombuffer(mixed_vote(rng, mem, dig[b].tobytes()), np.uint8)
            else:
                pk[i] = np.frombuffer(kps[t][0], np.uint8)
                sigs[i] = np.frombuffer(O.sign(kps[t][1], dig[b].tobytes()), np.uint8)
    off = (np.arange(nb + 1) * q).astype(np.uint64)
    keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps] +
                    [np.frombuffer(mem.pk, np.uint8)])
    zs = [rng.integers(0, 256, size=(nb * q, 16), dtype=np.uint8) for _ in range(nz)]
    return dig, pk, sigs, off, keys, zs


def expected(dig, pk, sigs, off, reg):
    """From the input alone: which votes the comb check passes (the oracle's strict status is 0
    and the key is registered with lambda 0), which batches it settles (all of their votes pass;
    an empty batch is settled), and the four counters: votes passed, votes not passed, batches
    settled, batches sent on."""
    reg = np.asarray(reg, np.uint8).reshape(-1, 32)
    lam0 = {bytes(k) for k in reg if lam_ref(bytes(k)) == 0}
    n = len(pk)
    strict = (O.verify_strict_many(digests_of(dig, off), pk, sigs).astype(np.int32)
              if n else np.zeros(0, np.int32))
    passed = np.array([strict[i] == 0 and pk[i].tobytes() in lam0 for i in range(n)], bool)
    o = off.astype(np.int64)
    settled = np.array([passed[o[b]:o[b + 1]].all() for b in range(len(o) - 1)], bool)
    counts = (int(passed.sum()), int(n - passed.sum()), int(settled.sum()),
              int(len(settled) - settled.sum()))
    return passed, settled, counts
