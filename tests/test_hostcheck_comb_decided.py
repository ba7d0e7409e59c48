"""The comb check's verdict carried to the triage, on the CPU (tools/hostcheck.hip
hc_verify_strict_decided_many: the slice as launch_verify_strict runs it since DESIGN.md 5
"Round 11": an item whose comb sum ran and gave R' != decode(R) is settled by the triage, without
the ladder). Statuses against the golden edge corpus and the oracle with the decision on and off,
and where each status came from."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

from test_hostcheck import hc  # noqa: F401  (hc: the library fixture)
from test_hostcheck_comb import MIN, _hot, _signed
from test_hostcheck_keyset import _hrams

COMB, SETTLED, LADDER, TRIAGE = 0, 1, 2, 3   # path_out & 3
HOT, SUMMED = 16, 32                         # path_out's flags


def _run(hc, pks, sigs, ks, decide, comb_min=MIN, bw=-16):  # noqa: F811
    f = hc.hc_verify_strict_decided_many
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 3 + [
        ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_int] + [ctypes.c_void_p] * 4
    n = len(pks)
    pks, sigs, ks = (np.ascontiguousarray(a, np.uint8) for a in (pks, sigs, ks))
    st = np.full(n, -99, np.int32)
    path = np.full(n, 255, np.uint8)
    stats = np.zeros(4, np.uint64)
    dstats = np.zeros(2, np.uint64)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert f(P(pks), P(sigs), P(ks), n, 1 << 16, bw, comb_min, 8192, decide, P(st), P(path),
             P(stats), P(dstats)) == 0
    return st, path, [int(x) for x in stats], [int(x) for x in dstats]


def _check(hc, m, p, s, exp):  # noqa: F811
    """Both settings against exp; returns the paths with the decision on."""
    k = _hrams(m, p, s)
    hot = _hot(p, MIN)
    under = np.array([x.tobytes() in hot for x in p])
    on, path, stats, d = _run(hc, p, s, k, 1)
    off, path0, stats0, d0 = _run(hc, p, s, k, 0)
    assert np.array_equal(on, exp)
    assert np.array_equal(off, on)
    # the comb's own statistics do not depend on the decision
    assert stats == stats0
    assert stats == [len(hot), int(under.sum()), int((under & (exp == 0)).sum()),
                     len(p) - int((under & (exp == 0)).sum())]
    where = path & 3
    assert np.array_equal((path & HOT) != 0, under)
    assert np.array_equal(where == COMB, under & (exp == 0))
    # nothing that is under a hot key and past the comb sum takes the ladder
    assert not np.any((where == LADDER) & ((path & (HOT | SUMMED)) == (HOT | SUMMED)))
    # every item past the sum is passed or settled, and a settled item is 7 or 4
    summed = (path & SUMMED) != 0
    assert np.array_equal(summed & (where != COMB), where == SETTLED)
    assert np.all(np.isin(on[where == SETTLED], (O.ERR_EQUATION, O.ERR_R_DECODE)))
    assert d == [int(((where == SETTLED) & (on == O.ERR_EQUATION)).sum()),
                 int((where == LADDER).sum())]
    # off: nothing is settled, and what was settled as an equation failure takes the ladder
    assert not np.any((path0 & 3) == SETTLED)
    assert d0 == [0, d[0] + d[1]]
    return path


def test_edge_corpus_behind_hot_keys(hc, golden):  # noqa: F811
    """The golden edge corpus followed by 2 keys of 160 honest signatures."""
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
    # a few of the hot keys' own items with a flipped message: decided by the comb
    msgs[5:25, 3] ^= 1
    m, p, s = (np.concatenate(x) for x in ((hexs("msg", 32), msgs), (hexs("pk", 32), pks),
                                           (hexs("sig", 64), sigs)))
    exp = np.concatenate([gold, np.zeros(320, np.int32)])
    exp[len(gold) + 5:len(gold) + 25] = O.ERR_EQUATION
    assert np.array_equal(exp, O.verify_strict_many(m, p, s).astype(np.int32))
    path = _check(hc, m, p, s, exp)
    assert np.all((path[len(gold) + 5:len(gold) + 25] & 3) == SETTLED)


@pytest.mark.parametrize("nkeys", [1, 3, 8])
def test_random_and_tampered(hc, nkeys):  # noqa: F811
    """1,024 signatures under 1, 3 and 8 keys, half of them tampered."""
    rng = np.random.Generator(np.random.PCG64(1000 + nkeys))
    m, p, s = _signed(rng, 1024, nkeys)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    path = _check(hc, m, p, s, exp)
    where = path & 3
    # all four origins occur: passes, wrong messages (settled), flipped keys (cold: the ladder)
    assert (where == COMB).sum() > 400 and (where == SETTLED).sum() > 100
    assert (where == LADDER).sum() > 20
