"""The comb check's verdict carried to the triage (DESIGN.md 5 "Round 11": keyed_vote_check_ex's
kVoteDecided and k_strict_keyed_inv's parity mismatch, bit 31 of k_strict_todo_list's entries,
k_strict_triage settling such an item as NW_ERR_EQUATION or with its own status, without
k_verify_strict_pre) through nw_dev_verify_strict_many: every status and the bitmap against the
oracle, against NW_STRICT_COMB_DECIDE=0 and against NW_STRICT_COMB=0, and
nw_dev_strict_decided_stats against counts taken from the construction.

The committee-keyed branch (k_strict_keyed_list, which must list kVoteDecided like kVoteFail) has
no case here: test_gpu_messages.py's header and vote streams carry wrong signatures under
committee keys, whose statuses only k_verify_strict's list mode writes, so they fail already if
the new state is not listed."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from oracle import oracle as O

import irregular as IR
from test_gpu_strict_comb import (L_ORDER, MIN, P_FIELD, _enc, _hot_keys, _mixed_valid, _sign_rows,
                                  _under)

pytestmark = pytest.mark.gpu


def _launch(msgs, pks, sigs):
    """Statuses, verdict bits, comb statistics and decided statistics (items settled as
    equation failures by the triage, items handed to the ladder) of one launch."""
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    dev = torch.device("cuda", 0)
    n = len(msgs)
    m, p, s = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (msgs, pks, sigs))
    st = torch.full((n,), -99, dtype=torch.int32, device=dev)
    bm = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = L.nw_dev_verify_strict_many(P(m), 32, P(p), P(s), n, P(st), P(bm), stream)
    assert rc == 0, L.nw_last_error()
    stats = (ctypes.c_uint64 * 4)()
    dstats = (ctypes.c_uint64 * 2)()
    assert L.nw_dev_strict_comb_stats(stats, stream) == 0, L.nw_last_error()
    assert L.nw_dev_strict_decided_stats(dstats, stream) == 0, L.nw_last_error()
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()
    return st.cpu().numpy(), bits[:n].astype(bool), [int(x) for x in stats], [int(x) for x in dstats]


def _check(monkeypatch, m, p, s, exp, hot):
    """The launch with the decision on, off and with the comb path off: equal statuses and
    bitmaps (the oracle's), equal comb statistics on and off, and the decided statistics:
    settled = the hot keys' items whose status is 7, ladder = the triage's survivors (status 0 or
    7) that are not under a hot key."""
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
    monkeypatch.delenv("NW_STRICT_COMB", raising=False)
    monkeypatch.delenv("NW_STRICT_COMB_DECIDE", raising=False)
    under = _under(p, hot)
    settled = int((under & (exp == O.ERR_EQUATION)).sum())
    ladder = int((~under & np.isin(exp, (O.OK, O.ERR_EQUATION))).sum())
    st, bits, stats, d = _launch(m, p, s)
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]], stats, d)
    assert np.array_equal(bits, exp == 0)
    assert stats[2] == int((under & (exp == 0)).sum()) and stats[2] + stats[3] == len(m)
    assert d == [settled, ladder]
    monkeypatch.setenv("NW_STRICT_COMB_DECIDE", "0")
    st0, bits0, stats0, d0 = _launch(m, p, s)
    monkeypatch.delenv("NW_STRICT_COMB_DECIDE")
    assert np.array_equal(st0, st) and np.array_equal(bits0, bits)
    assert stats0 == stats
    assert d0 == [0, settled + ladder]
    monkeypatch.setenv("NW_STRICT_COMB", "0")
    st1, bits1, stats1, d1 = _launch(m, p, s)
    monkeypatch.delenv("NW_STRICT_COMB")
    assert np.array_equal(st1, st) and np.array_equal(bits1, bits)
    assert stats1 == [0, 0, 0, len(m)] and d1 == [0, 0]
    return stats, d


def _flip_r(sig, rng, want_decodes):
    """One bit of R's y flipped so that the encoding decodes (to a point that is not small) or
    does not, as wanted."""
    while True:
        r = bytearray(sig[:32].tobytes())
        b = int(rng.integers(0, 255))
        r[b >> 3] ^= 1 << (b & 7)
        dec = O.decompress(bytes(r)) is not None
        if dec == want_decodes and not (dec and O.is_small_order(bytes(r))):
            return np.frombuffer(bytes(r), np.uint8)


PER = 8   # items of each class


@pytest.fixture(scope="module")
def mixed_corpus():
    """Two hot keys with 210 honest items each and PER items of every class of failure under
    them, a hot non-canonical key y = p + 3, a hot mixed-order key with accepted and tampered
    signatures, and a cold key; the oracle's statuses, computed once."""
    rng = np.random.Generator(np.random.PCG64(1111))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(3)]
    m, p, s = _sign_rows(rng, kps, [i % 2 for i in range(420)])
    classes = ["msg", "s_low", "r_decodes", "r_undecodable", "r_sign", "r_x0", "r_big",
               "r_small", "s_plus_l", "s_high"]
    cm, cp, cs = _sign_rows(rng, kps, [i % 2 for i in range(PER * len(classes))])
    small = IR.small_order_encodings()
    for i in range(len(cm)):
        c, t = classes[i // PER], i % PER
        if c == "msg":
            cm[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == "s_low":
            cs[i, 32 + rng.integers(0, 31)] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == "r_decodes":
            cs[i, :32] = _flip_r(cs[i], rng, True)
        elif c == "r_undecodable":
            cs[i, :32] = _flip_r(cs[i], rng, False)
        elif c == "r_sign":
            cs[i, 31] ^= np.uint8(0x80)
        elif c == "r_x0":
            cs[i, :32] = _enc([1, P_FIELD - 1][t % 2], 1)
        elif c == "r_big":
            cs[i, :32] = _enc(P_FIELD + [0, 1, 3, 4, 18, 5, 9, 10][t], t & 1)
        elif c == "r_small":
            cs[i, :32] = np.frombuffer(small[t % len(small)], np.uint8)
        elif c == "s_plus_l":
            v = int.from_bytes(cs[i, 32:].tobytes(), "little") + L_ORDER
            cs[i, 32:] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        else:
            cs[i, 63] |= np.uint8(0x80 >> (t % 3))
    # the hot non-canonical key: 200 signatures of kps[0] relabelled
    nm, np_, ns = _sign_rows(rng, kps, [0] * 200)
    np_[:] = _enc(P_FIELD + 3, 0)
    # the mixed-order key: 200 accepted signatures, every tenth with a flipped message
    xm, xp, xs = _mixed_valid(rng, 200)
    xm[::10, 5] ^= 1
    # the cold key: 6 items, half with a flipped message
    km, kp, ks = _sign_rows(rng, kps, [2] * 6)
    km[::2, 7] ^= 1
    m, p, s = (np.concatenate(x) for x in ((m, cm, nm, xm, km), (p, cp, np_, xp, kp),
                                           (s, cs, ns, xs, ks)))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    hot = _hot_keys(p)
    assert hot == {kps[0][0], kps[1][0], _enc(P_FIELD + 3, 0).tobytes(), xp[0].tobytes()}
    c0 = 420
    cls = lambda name: exp[c0 + PER * classes.index(name):c0 + PER * (classes.index(name) + 1)]
    for name in ("msg", "s_low", "r_decodes", "r_sign"):
        assert np.all(cls(name) == O.ERR_EQUATION), name
    assert np.all(cls("r_undecodable") == O.ERR_R_DECODE)
    assert np.all(cls("r_small") == O.ERR_R_SMALL_ORDER)
    assert np.all(cls("s_plus_l") == O.ERR_S_NONCANONICAL)
    assert np.all(cls("s_high") == O.ERR_S_HIGH_BITS)
    n0 = c0 + len(cm)
    assert np.all(exp[n0:n0 + 200] == O.ERR_EQUATION)
    assert (exp[n0 + 200:n0 + 400] == 0).sum() == 180 and (exp[n0 + 200:n0 + 400] == 7).sum() == 20
    assert exp[n0 + 400:].tolist() == [7, 0, 7, 0, 7, 0]
    return {"kps": kps, "items": (m, p, s), "exp": exp, "hot": hot}


def test_every_class_under_hot_keys(mixed_corpus, monkeypatch):
    """Every branch that sets the flag, and every one that must not: the oracle's statuses, the
    same with the decision off and the path off, and the counts."""
    m, p, s = mixed_corpus["items"]
    stats, d = _check(monkeypatch, m, p, s, mixed_corpus["exp"], mixed_corpus["hot"])
    assert stats[0] == 4
    assert d[0] >= 4 * PER + 200 + 20 and d[1] == 6


def test_several_slices(monkeypatch):
    """NW_TRIAGE_SLICE=1024 over 4,096 items under 8 keys (slice q holds keys 2q and 2q + 1),
    every fifth item tampered, and three honest items of a cold key per slice: each slice has
    its own flags, and the counts sum over the slices."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "1024")
    rng = np.random.Generator(np.random.PCG64(6))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(12)]
    key_of = [2 * (i // 1024) + (i & 1) for i in range(4096)]
    for q in range(4):
        for r in (101, 502, 903):
            key_of[1024 * q + r] = 8 + q
    m, p, s = _sign_rows(rng, kps, key_of)
    for i in range(0, 4096, 5):
        if i % 3 == 0:
            m[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        else:
            s[i, rng.integers(0, 64)] ^= np.uint8(1 << rng.integers(0, 8))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    hot = set()
    for a in range(0, 4096, 1024):
        h = _hot_keys(p[a:a + 1024])
        assert len(h) == 2
        hot |= h
    assert hot == {kp[0] for kp in kps[:8]}
    stats, d = _check(monkeypatch, m, p, s, exp, hot)
    assert stats[0] == 8 and d[0] > 400 and d[1] == 12


def test_no_hot_key(monkeypatch):
    """320 items under 64 keys, half of them with a flipped message: no key is hot, the triage
    takes the whole slice without the to-do list, nothing is settled."""
    rng = np.random.Generator(np.random.PCG64(8))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(64)]
    m, p, s = _sign_rows(rng, kps, [i % 64 for i in range(320)])
    m[::2, 9] ^= 1
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert _hot_keys(p) == set() and (exp == 7).sum() == 160
    stats, d = _check(monkeypatch, m, p, s, exp, set())
    assert stats == [0, 0, 0, 320] and d == [0, 320]


def test_registered_signers(mixed_corpus, monkeypatch):
    """The corpus of the first test with its two ordinary hot keys registered, so that
    k_strict_keyed_signers runs the check (strict_keyed_item, shared with k_strict_keyed): the
    same statuses and counts."""
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "1")
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in mixed_corpus["kps"][:2]])
    m, p, s = mixed_corpus["items"]
    try:
        assert L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data), 2) == 0, L.nw_last_error()
        monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
        sstats = (ctypes.c_uint64 * 3)()
        stats, d = _check(monkeypatch, m, p, s, mixed_corpus["exp"], mixed_corpus["hot"])
        # the last launch of _check ran with the path off; one more with it on for the registry's
        # own statistics: both keys matched
        st, _, stats2, d2 = _launch(m, p, s)
        stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
        assert L.nw_dev_strict_signers_stats(sstats, stream) == 0, L.nw_last_error()
        assert int(sstats[0]) == 2 and stats2[0] == 2   # two call-local tables beside them
        assert np.array_equal(st, mixed_corpus["exp"]) and d2 == d
    finally:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()
