"""Config 4's two passes with the call's key set, on the CPU (tools/hostcheck.hip
hc_verify_strict_keyset_many: keyset_probe for every item, keyset_build for every slot, then
strict_triage on the slot's flags and the ladder on the slot's table). Statuses against the
golden edge corpus, the oracle, and the same entry with the key set off; with 64 slots, so
that some keys get none; and over keys that all start at one slot of the table, found from
the hash as nw_strict.hpp documents it."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

from test_hostcheck import LIB, _build

NO_SLOT = 0xFFFFFFFF
PROBES = 8


def keyset_hash(pk: np.ndarray) -> np.ndarray:
    """nw_strict.hpp keyset_hash over rows of 32 key bytes: h = 0x9e3779b9; for each of the 8
    little-endian words h = (h ^ w) * 0x85ebca6b, h ^= h >> 15; then h *= 0xc2b2ae35,
    h ^= h >> 16 (all mod 2^32)."""
    w = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32).view("<u4").astype(np.uint64)
    h = np.full(len(w), 0x9E3779B9, np.uint64)
    for t in range(8):
        h = ((h ^ w[:, t]) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
        h ^= h >> np.uint64(15)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    lib.hc_verify_strict_keyset_many.restype = ctypes.c_int
    lib.hc_verify_strict_keyset_many.argtypes = [ctypes.c_void_p] * 3 + [
        ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.hc_keyset_hash.restype = ctypes.c_uint32
    return lib


def _run(hc, pks, sigs, ks, slots, bw=-16):
    n = len(pks)
    pks, sigs, ks = (np.ascontiguousarray(a, np.uint8) for a in (pks, sigs, ks))
    st = np.full(n, -99, np.int32)
    ksl = np.zeros(n, np.uint32)
    stats = np.zeros(3, np.uint64)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert hc.hc_verify_strict_keyset_many(P(pks), P(sigs), P(ks), n, slots, bw, P(st), P(ksl),
                                           P(stats)) == 0
    return st, ksl, [int(x) for x in stats]


def _hrams(msgs, pks, sigs):
    return np.array([np.frombuffer(O.hram(s[:32].tobytes(), p.tobytes(), m.tobytes()), np.uint8)
                     for m, p, s in zip(msgs, pks, sigs)])


@pytest.fixture(scope="module")
def corpus(golden):
    """The golden edge corpus followed by 2,048 seeded items over 64 keys (half honest; the
    others with one bit of s, of R, of the key or of the message flipped), with k for every
    item and the oracle's statuses, computed once."""
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    em, ep, es = hexs("msg", 32), hexs("pk", 32), hexs("sig", 64)
    gold = np.array([i["status"] for i in items], np.int32)
    rng = np.random.Generator(np.random.PCG64(808))
    n = 2048
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(64)]
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.zeros((n, 32), np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        pk, sk = kps[i % 64]
        pks[i] = np.frombuffer(pk, np.uint8)
        sigs[i] = np.frombuffer(O.sign(sk, msgs[i].tobytes()), np.uint8)
    for i in range(1, n, 2):
        bit = np.uint8(1 << rng.integers(0, 8))
        c = i % 8
        if c == 1:
            sigs[i, 32 + rng.integers(0, 32)] ^= bit
        elif c == 3:
            sigs[i, rng.integers(0, 32)] ^= bit
        elif c == 5:
            pks[i, rng.integers(0, 32)] ^= bit
        else:
            msgs[i, rng.integers(0, 32)] ^= bit
    m, p, s = np.concatenate([em, msgs]), np.concatenate([ep, pks]), np.concatenate([es, sigs])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.array_equal(exp[:len(gold)], gold)
    return p, s, _hrams(m, p, s), exp


@pytest.mark.parametrize("bw", [-16, -24])
def test_statuses_default_slots(hc, corpus, bw):
    """Golden statuses (the corpus fixture checks them equal to the oracle's over the edge
    items), the oracle's, and the key set off; most items share a table."""
    p, s, k, exp = corpus
    off, ksl0, st0 = _run(hc, p, s, k, 0, bw)
    assert np.array_equal(off, exp)
    assert np.all(ksl0 == NO_SLOT) and st0 == [0, 0, len(p)]
    on, ksl, st = _run(hc, p, s, k, 1 << 16, bw)
    assert np.array_equal(on, exp)
    distinct = len({x.tobytes() for x in p})
    assert st == [distinct, len(p), 0] and np.all(ksl != NO_SLOT)
    # one slot per key: equal keys share it, different keys never do
    assert len({(x.tobytes(), int(q)) for x, q in zip(p, ksl)}) == distinct
    assert len(set(ksl.tolist())) == distinct


def test_statuses_64_slots(hc, corpus):
    """64 slots: inserts stop at 32 keys (one thread: no overshoot), the other keys' items
    take their own path; the statuses do not change."""
    p, s, k, exp = corpus
    on, ksl, st = _run(hc, p, s, k, 64)
    assert np.array_equal(on, exp)
    assert st[0] == 32 and st[1] > 0 and st[2] > 0 and st[1] + st[2] == len(p)
    assert int(ksl[ksl != NO_SLOT].max()) < 64


def test_colliding_keys(hc):
    """24 arbitrary 32-byte keys whose probe chains all start at slot 5 of a 128-slot table
    (brute force over the documented hash): the first 8 distinct keys fill the chain 5..12 in
    order of appearance, the other 16 get no slot. Items: each key's bytes as the public key
    of an honestly made signature of another key, so that whatever the key decodes to the
    oracle decides; statuses equal the oracle's and the set-off run's."""
    cap, start = 128, 5
    rng = np.random.Generator(np.random.PCG64(5150))
    found = []
    while len(found) < 24:
        cand = rng.integers(0, 256, size=(4096, 32), dtype=np.uint8)
        hit = cand[(keyset_hash(cand) & (cap - 1)) == start]
        found += [x for x in hit]
    keys = np.array(found[:24])
    for x in keys:   # the numpy restatement is the library's hash
        assert int(keyset_hash(x)[0]) == hc.hc_keyset_hash(ctypes.c_char_p(x.tobytes()))
    pk0, sk0 = O.keypair_from_seed(rng.bytes(32))
    n = 72
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.array([keys[i % 24] for i in range(n)])
    sigs = np.array([np.frombuffer(O.sign(sk0, m.tobytes()), np.uint8) for m in msgs])
    # and one honest item per chain position, so a pass is among the statuses
    msgs = np.concatenate([msgs, msgs[:4]])
    pks = np.concatenate([pks, np.tile(np.frombuffer(pk0, np.uint8), (4, 1))])
    sigs = np.concatenate([sigs, sigs[:4]])
    exp = O.verify_strict_many(msgs, pks, sigs).astype(np.int32)
    assert (exp[-4:] == 0).all()
    k = _hrams(msgs, pks, sigs)
    on, ksl, st = _run(hc, pks, sigs, k, cap)
    off, _, _ = _run(hc, pks, sigs, k, 0)
    assert np.array_equal(on, exp) and np.array_equal(off, exp)
    for i in range(n):
        want = start + (i % 24) if i % 24 < PROBES else NO_SLOT
        assert int(ksl[i]) == want, i
    assert st[0] == 9 and st[1] == 3 * 8 + 4 and st[2] == 3 * 16
