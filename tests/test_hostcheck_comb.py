"""The comb check of a strict launch's hot keys, on the CPU (tools/hostcheck.hip
hc_verify_strict_comb_many: the slice as launch_verify_strict runs it: probe with the sampled use
counts, hot selection, keyed_vote_check with 8-bit key combs, the leftovers through the triage
and the ladder). Statuses against the golden edge corpus and the oracle with the path on and
off; the keyed checks of test_hostcheck.py at comb width 8; k's 8-bit digits."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

from test_hostcheck import LIB, _b, _build, hc  # noqa: F401  (hc: the library fixture)
# the keyed checks' own sets (edge corpus, random / tampered, R' = -R), collected here with
# this module's keyw fixture: width 8
from test_hostcheck import test_keyed_vote_check_compressed_r, test_strict_keyed_comb  # noqa: F401
from test_hostcheck_keyset import _hrams

L_ORDER = 2**252 + 27742317777372353535851937790883648493
MIN = 64


@pytest.fixture(params=[8])
def keyw(request, hc):  # noqa: F811
    """The width of the call-local tables (nw_kernels.h keyspec_for(8): 32 tables of 129
    entries, every digit signed)."""
    hc.hc_set_key_width.restype = ctypes.c_int
    assert hc.hc_set_key_width(request.param) == 0
    yield request.param
    hc.hc_set_key_width(16)


def _run(hc, pks, sigs, ks, comb_min, comb_keys=8192, slots=1 << 16, bw=-16):  # noqa: F811
    hc.hc_verify_strict_comb_many.restype = ctypes.c_int
    hc.hc_verify_strict_comb_many.argtypes = [ctypes.c_void_p] * 3 + [
        ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_void_p, ctypes.c_void_p]
    n = len(pks)
    pks, sigs, ks = (np.ascontiguousarray(a, np.uint8) for a in (pks, sigs, ks))
    st = np.full(n, -99, np.int32)
    stats = np.zeros(4, np.uint64)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert hc.hc_verify_strict_comb_many(P(pks), P(sigs), P(ks), n, slots, bw, comb_min,
                                         comb_keys, P(st), P(stats)) == 0
    return st, [int(x) for x in stats]


def _sampled(n):
    """nw_strict.hpp comb_sampled over rows 0..n-1."""
    j = np.arange(n, dtype=np.uint64)
    return ((j * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28) == 0


def _hot(pks, min_uses):
    keys, counts = np.unique(pks[_sampled(len(pks))], axis=0, return_counts=True)
    return {k.tobytes() for k, c in zip(keys, counts)
            if 16 * c >= min_uses and O.decompress(k.tobytes()) is not None
            and not O.is_small_order(k.tobytes())}


def _signed(rng, n, nkeys):
    """n items signed round-robin by nkeys keys; every second one has one bit of s, of R, of
    the key or of the message flipped (which, drawn per item)."""
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(nkeys)]
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.zeros((n, 32), np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        pk, sk = kps[i % nkeys]
        pks[i] = np.frombuffer(pk, np.uint8)
        sigs[i] = np.frombuffer(O.sign(sk, msgs[i].tobytes()), np.uint8)
    for i in range(1, n, 2):
        bit = np.uint8(1 << rng.integers(0, 8))
        c = int(rng.integers(0, 4))
        if c == 0:
            sigs[i, 32 + rng.integers(0, 32)] ^= bit
        elif c == 1:
            sigs[i, rng.integers(0, 32)] ^= bit
        elif c == 2:
            pks[i, rng.integers(0, 32)] ^= bit
        else:
            msgs[i, rng.integers(0, 32)] ^= bit
    return msgs, pks, sigs


def test_edge_corpus_behind_hot_keys(hc, golden):  # noqa: F811
    """The golden edge corpus followed by 2 keys of 160 honest signatures: golden statuses,
    and the comb passes exactly the valid items of the hot keys."""
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    gold = np.array([i["status"] for i in items], np.int32)
    rng = np.random.Generator(np.random.PCG64(909))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(2)]
    msgs = rng.integers(0, 256, size=(320, 32), dtype=np.uint8)
    pks = np.array([np.frombuffer(kps[i & 1][0], np.uint8) for i in range(320)])
    sigs = np.array([np.frombuffer(O.sign(kps[i & 1][1], msgs[i].tobytes()), np.uint8)
                     for i in range(320)])
    m, p, s = (np.concatenate(x) for x in ((hexs("msg", 32), msgs), (hexs("pk", 32), pks),
                                           (hexs("sig", 64), sigs)))
    exp = np.concatenate([gold, np.zeros(320, np.int32)])
    k = _hrams(m, p, s)
    hot = _hot(p, MIN)
    assert {kp[0] for kp in kps} <= hot
    under = np.array([x.tobytes() in hot for x in p])
    for bw in (-16, -24):
        st, stats = _run(hc, p, s, k, MIN, bw=bw)
        assert np.array_equal(st, exp)
        assert stats == [len(hot), int(under.sum()), int((under & (exp == 0)).sum()),
                         len(p) - int((under & (exp == 0)).sum())]
        assert stats[2] >= 320
    off, stats = _run(hc, p, s, k, 0)
    assert np.array_equal(off, exp) and stats == [0, 0, 0, len(p)]


@pytest.mark.parametrize("nkeys", [1, 3, 8])
def test_random_and_tampered(hc, nkeys):  # noqa: F811
    """1,024 signatures under 1, 3 and 8 keys, half of them tampered: the oracle's statuses
    with the path on, off, and with room for one hot key only."""
    rng = np.random.Generator(np.random.PCG64(1000 + nkeys))
    m, p, s = _signed(rng, 1024, nkeys)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    k = _hrams(m, p, s)
    hot = _hot(p, MIN)
    assert 1 <= len(hot) <= nkeys
    under = np.array([x.tobytes() in hot for x in p])
    st, stats = _run(hc, p, s, k, MIN)
    assert np.array_equal(st, exp)
    assert stats[:3] == [len(hot), int(under.sum()), int((under & (exp == 0)).sum())]
    assert stats[2] > 400 and stats[2] + stats[3] == 1024
    off, stats0 = _run(hc, p, s, k, 0)
    assert np.array_equal(off, exp) and stats0 == [0, 0, 0, 1024]
    one, stats1 = _run(hc, p, s, k, MIN, comb_keys=1)
    assert np.array_equal(one, exp) and stats1[0] == 1


def test_key_digits_width_8(hc):  # noqa: F811
    """key_recode / key_digit at W = 8: 32 signed digits in [-128, 127] with
    sum d_t 2^(8 t) == k, for random k < l and for k = 0, l - 1, 2^252."""
    hc.hc_key_digits.restype = ctypes.c_int
    rng = np.random.Generator(np.random.PCG64(88))
    ks = [0, 1, L_ORDER - 1, 2**252, 2**252 - 1, int("80" * 32, 16) % L_ORDER]
    ks += [int.from_bytes(rng.bytes(32), "little") % L_ORDER for _ in range(200)]
    for k in ks:
        d = (ctypes.c_int32 * 32)()
        assert hc.hc_key_digits(_b(k.to_bytes(32, "little")), 8, d) == 32
        assert all(-128 <= x <= 127 for x in d)
        assert sum(int(x) << (8 * t) for t, x in enumerate(d)) == k
    d = (ctypes.c_int32 * 32)()
    assert hc.hc_key_digits(_b((5).to_bytes(32, "little")), 16, d) == 16
    assert hc.hc_key_digits(_b((5).to_bytes(32, "little")), 12, d) == -1
