"""Registered signers on the CPU (tools/hostcheck.hip hc_verify_strict_signers_many: a slice as
launch_verify_strict runs it with a registry: the host-built hash table, the match of the
slice's keys, the selection over one index space, the keyed check with the registry's or the
call-local 8-bit tables, the leftovers through the triage and the ladder; hc_signers_table: the
hash build and the lookup alone). Statuses against the golden edge corpus and the oracle, the
matches and passes against counts taken from the input."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

import irregular as IR
from test_hostcheck import LIB, _build
from test_hostcheck_comb import _hot, _signed
from test_hostcheck_keyset import _hrams, keyset_hash

P_FIELD = 2**255 - 19
NO_KEY = 0xFFFFFFFF
PROBES = 8          # nw_strict.hpp kKeyProbes
SIGNERS_MAX = 8192  # NW_STRICT_SIGNERS_MAX's default


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    lib.hc_verify_strict_signers_many.restype = ctypes.c_int
    lib.hc_verify_strict_signers_many.argtypes = [ctypes.c_void_p] * 3 + [
        ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_signers_table.restype = ctypes.c_int64
    lib.hc_signers_table.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                     ctypes.c_void_p]
    return lib


def _P(a):
    return ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)


def _run(hc, pks, sigs, ks, reg, comb_min=256, comb_keys=8192, slots=1 << 16, bw=-16):
    """Statuses, comb stats (call-local tables, items checked, passed, sent on) and signers
    stats (registered keys matched, items under them, items passed under them)."""
    n = len(pks)
    pks, sigs, ks = (np.ascontiguousarray(a, np.uint8) for a in (pks, sigs, ks))
    reg = np.ascontiguousarray(reg, np.uint8).reshape(-1, 32)
    st = np.full(n, -99, np.int32)
    stats, sstats = np.zeros(4, np.uint64), np.zeros(3, np.uint64)
    assert hc.hc_verify_strict_signers_many(_P(pks), _P(sigs), _P(ks), n, slots, bw, comb_min,
                                            comb_keys, _P(reg), len(reg), _P(st), _P(stats),
                                            _P(sstats)) == 0
    return st, [int(x) for x in stats], [int(x) for x in sstats]


def _enc(y, sign=0):
    return np.frombuffer((y | (sign << 255)).to_bytes(32, "little"), np.uint8)


def _honest(rng, kps, n):
    """n honest items signed round-robin by kps."""
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.array([np.frombuffer(kps[i % len(kps)][0], np.uint8) for i in range(n)])
    sigs = np.array([np.frombuffer(O.sign(kps[i % len(kps)][1], msgs[i].tobytes()), np.uint8)
                     for i in range(n)])
    return msgs, pks, sigs


def mixed_valid(rng, n):
    """A = aB + T8 and n signatures under it that dalek's verify_strict accepts:
    R = rB + T' with T' + kT == 0 (irregular.Member's mode 2)."""
    mem = IR.Member("mixed", rng)
    tors = IR.torsion_points()
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        while True:
            r = IR._rand_scalar(rng)
            Tp = tors[int(rng.integers(0, 8))]
            R = O.point_add(O.scalarmult_base(r), Tp)
            k = O.hram(R, mem.pk, msgs[i].tobytes())
            if O.point_add(Tp, O.scalarmult(k, mem.T)) == IR.IDENTITY:
                break
        sigs[i] = np.frombuffer(R + O.scalar_add(r, O.scalar_mul(k, mem.a)), np.uint8)
    return msgs, np.tile(np.frombuffer(mem.pk, np.uint8), (n, 1)), sigs


def _under(pks, keys):
    ks = {bytes(k) for k in np.asarray(keys, np.uint8).reshape(-1, 32)}
    return np.array([p.tobytes() in ks for p in pks])


@pytest.mark.parametrize("bw", [-16, -24])
def test_below_the_threshold(hc, golden, bw):
    """The golden edge corpus followed by 2 registered keys of 20 honest signatures each, at
    comb_min = 256 (nothing is hot by count): golden statuses, both keys matched, their 40 items
    passed by the comb; with an empty registry the comb does nothing."""
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    gold = np.array([i["status"] for i in items], np.int32)
    rng = np.random.Generator(np.random.PCG64(1010))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(2)]
    msgs, pks, sigs = _honest(rng, kps, 40)
    m, p, s = (np.concatenate(x) for x in ((hexs("msg", 32), msgs), (hexs("pk", 32), pks),
                                           (hexs("sig", 64), sigs)))
    exp = np.concatenate([gold, np.zeros(40, np.int32)])
    k = _hrams(m, p, s)
    reg = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps])
    assert not _under(hexs("pk", 32), reg).any() and not _hot(p, 256)
    st, stats, ss = _run(hc, p, s, k, reg, bw=bw)
    assert np.array_equal(st, exp)
    assert ss == [2, 40, 40]
    assert stats == [0, 40, 40, len(p) - 40]
    st0, stats0, ss0 = _run(hc, p, s, k, np.zeros((0, 32), np.uint8), bw=bw)
    assert np.array_equal(st0, exp)
    assert stats0 == [0, 0, 0, len(p)] and ss0 == [0, 0, 0]


def test_special_keys(hc):
    """Four registered keys of 20 uses each: an undecodable key and a small-order key (never
    matched), the non-canonical y = p + 3 (matched, nothing passes), a mixed-order key
    A = aB + T8 with signatures dalek accepts (matched, everything passes)."""
    rng = np.random.Generator(np.random.PCG64(1011))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(3)]
    m, p, s = _honest(rng, kps, 60)
    special = [_enc(2), _enc(1), _enc(P_FIELD + 3)]
    for i in range(60):
        p[i] = special[i % 3]
    mm, mp, ms = mixed_valid(rng, 20)
    m, p, s = np.concatenate([m, mm]), np.concatenate([p, mp]), np.concatenate([s, ms])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.all(exp[60:] == 0) and {3, 5, 7} <= set(exp[:60].tolist())
    k = _hrams(m, p, s)
    reg = np.array(special + [mp[0]])
    st, stats, ss = _run(hc, p, s, k, reg)
    assert np.array_equal(st, exp)
    assert ss == [2, 40, 20] and stats == [0, 40, 20, 60]
    # each of them alone
    for key, want in zip(reg, ([0, 0, 0], [0, 0, 0], [1, 20, 0], [1, 20, 20])):
        st, _, ss = _run(hc, p, s, k, key)
        assert np.array_equal(st, exp) and ss == want


def test_registered_and_hot_by_count(hc):
    """3 keys of 200 uses each at comb_min = 64, one of them registered: two call-local tables
    are built, and the comb passes the valid items of all three."""
    rng = np.random.Generator(np.random.PCG64(1012))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(3)]
    m, p, s = _honest(rng, kps, 600)
    for i in range(0, 600, 7):
        s[i, rng.integers(0, 64)] ^= np.uint8(1 << rng.integers(0, 8))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    k = _hrams(m, p, s)
    assert len(_hot(p, 64)) == 3
    reg = np.frombuffer(kps[1][0], np.uint8)
    st, stats, ss = _run(hc, p, s, k, reg, comb_min=64)
    assert np.array_equal(st, exp)
    valid = int((exp == 0).sum())
    assert stats == [2, 600, valid, 600 - valid]
    under = _under(p, reg)
    assert ss == [1, 200, int((under & (exp == 0)).sum())]


def test_key_identity(hc):
    """The canonical encoding y = 3 is registered; the items arrive under y = p + 3, a second
    encoding of the same point: 32 other bytes, so not matched. Registering those bytes
    matches."""
    rng = np.random.Generator(np.random.PCG64(1013))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(2)]
    m, p, s = _honest(rng, kps, 40)
    assert O.decompress(_enc(3).tobytes()) is not None
    assert O.decompress(_enc(3).tobytes()) == O.decompress(_enc(P_FIELD + 3).tobytes())
    p[::2] = _enc(P_FIELD + 3)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    k = _hrams(m, p, s)
    st, stats, ss = _run(hc, p, s, k, _enc(3))
    assert np.array_equal(st, exp) and ss == [0, 0, 0] and stats == [0, 0, 0, 40]
    st, stats, ss = _run(hc, p, s, k, _enc(P_FIELD + 3))
    assert np.array_equal(st, exp) and ss == [1, 20, 0]


def _table(hc, keys, probes, max_keys=SIGNERS_MAX):
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
    probes = np.ascontiguousarray(probes, np.uint8).reshape(-1, 32)
    rows = np.full(len(probes), 12345, np.uint32)
    cap = hc.hc_signers_table(_P(keys), len(keys), max_keys, _P(probes), len(probes), _P(rows),
                              None)
    if cap <= 0:
        return cap, rows, None
    slots = np.zeros(cap, np.uint32)
    assert hc.hc_signers_table(_P(keys), len(keys), max_keys, _P(probes), len(probes), _P(rows),
                               _P(slots)) == cap
    return cap, rows, slots


def _build_py(keys):
    """nw_strict.hpp signers_hash_build restated: the smallest power of two >= max(2 n, 64) at
    which every key, inserted in row order into the first empty slot of its chain, lands within
    PROBES slots."""
    h = keyset_hash(keys).astype(np.int64) if len(keys) else np.zeros(0, np.int64)
    cap = 64
    while cap // 2 < len(keys):
        cap *= 2
    while True:
        slots = np.zeros(cap, np.uint32)
        for r, hv in enumerate(h):
            s0 = int(hv) & (cap - 1)
            for q in range(PROBES):
                if slots[(s0 + q) & (cap - 1)] == 0:
                    slots[(s0 + q) & (cap - 1)] = r + 1
                    break
            else:
                break
        else:
            return cap, slots
        cap *= 2


def test_hash_table(hc):
    """8,192 random keys plus 64 keys whose first slots coincide at the smallest capacity for
    that many keys: the capacity doubles until every key sits within kKeyProbes slots of its
    first one, every registered key is found and 10,000 other keys are not; n = 0, 1 and
    NW_STRICT_SIGNERS_MAX work, one more is refused."""
    rng = np.random.Generator(np.random.PCG64(1014))
    keys = rng.integers(0, 256, size=(SIGNERS_MAX, 32), dtype=np.uint8)
    first = 32768                       # the smallest capacity for 8,192 + 64 keys
    target = int(keyset_hash(keys[:1])[0]) & (first - 1)
    same = []
    while len(same) < 64:
        cand = rng.integers(0, 256, size=(1 << 19, 32), dtype=np.uint8)
        same += list(cand[(keyset_hash(cand) & np.uint32(first - 1)) == target])
    allk = np.concatenate([keys, np.array(same[:64])])
    strangers = rng.integers(0, 256, size=(10000, 32), dtype=np.uint8)
    for ks in (allk, keys):
        cap, rows, slots = _table(hc, ks, np.concatenate([ks, strangers]), max_keys=1 << 20)
        pcap, pslots = _build_py(ks)
        assert cap == pcap and np.array_equal(slots, pslots)
        assert np.array_equal(rows[:len(ks)], np.arange(len(ks), dtype=np.uint32))
        assert np.all(rows[len(ks):] == NO_KEY)
        # every key within PROBES slots of its first one
        pos = np.zeros(len(ks), np.int64)
        occ = np.nonzero(slots)[0]
        pos[slots[occ].astype(np.int64) - 1] = occ
        dist = (pos - (keyset_hash(ks).astype(np.int64) & (cap - 1))) & (cap - 1)
        assert len(occ) == len(ks) and dist.max() < PROBES
    assert cap >= 2 * SIGNERS_MAX
    # the 65 keys of one first slot cannot sit at the smallest capacity: it doubled
    cap65, _, _ = _table(hc, allk, allk[:1], max_keys=1 << 20)
    assert cap65 > first
    # n = 0, 1, the limit and one more
    cap, rows, _ = _table(hc, keys[:0], strangers[:100])
    assert cap == 64 and np.all(rows == NO_KEY)
    cap, rows, _ = _table(hc, keys[:1], np.concatenate([keys[:1], strangers[:100]]))
    assert cap == 64 and rows[0] == 0 and np.all(rows[1:] == NO_KEY)
    assert _table(hc, keys, keys[:1])[0] > 0
    assert _table(hc, allk[:SIGNERS_MAX + 1], keys[:1])[0] == -1


@pytest.mark.parametrize("nkeys", [1, 3, 8])
def test_random_and_tampered(hc, nkeys):
    """1,024 signatures under 1, 3 and 8 keys, half of them tampered, with all keys registered,
    with some and with none: the oracle's statuses, and passed + sent on = n."""
    rng = np.random.Generator(np.random.PCG64(1020 + nkeys))
    m, p, s = _signed(rng, 1024, nkeys)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    k = _hrams(m, p, s)
    rng2 = np.random.Generator(np.random.PCG64(1020 + nkeys))   # _signed draws its keys first
    signers = np.array([np.frombuffer(O.keypair_from_seed(rng2.bytes(32))[0], np.uint8)
                        for _ in range(nkeys)])
    assert np.array_equal(signers[0], p[0])
    for reg in (signers, signers[:(nkeys + 1) // 2], signers[:0]):
        under = _under(p, reg)
        for comb_min in (256, 2048):     # with call-local tables for the others, and without
            st, stats, ss = _run(hc, p, s, k, reg, comb_min=comb_min)
            assert np.array_equal(st, exp)
            assert ss == [len(reg), int(under.sum()), int((under & (exp == 0)).sum())]
            assert stats[2] + stats[3] == 1024 and stats[2] >= ss[2] and stats[1] >= ss[1]
            if comb_min == 2048:
                assert stats[:3] == [0] + ss[1:]
            if len(reg) == nkeys:
                assert stats[0] == 0 and stats[2] == int((under & (exp == 0)).sum()) > 400
