"""Config 4's two-pass strict verification (k_strict_triage with the scalar phase, then
k_verify_strict_pre's ladder from the stored points and digit words) through
nw_dev_verify_strict_many: statuses and bitmap against the oracle at the sizes where the
launch changes shape: below, at and above a wave; more than one block; no survivor at
all; every item a survivor; more survivors than the persistent ladder kernel's resident
lanes (a second, ragged round); several triage slices with a ragged last one."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _launch(msgs, pks, sigs):
    """Statuses and verdict bits of one nw_dev_verify_strict_many launch."""
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    dev = torch.device("cuda", 0)
    n = len(msgs)
    m, p, s = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (msgs, pks, sigs))
    st = torch.full((n,), -99, dtype=torch.int32, device=dev)
    bm = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream(dev)
    rc = L.nw_dev_verify_strict_many(P(m), 32, P(p), P(s), n, P(st), P(bm),
                                     ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, L.nw_last_error()
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()
    return st.cpu().numpy(), bits[:n].astype(bool)


def _check(msgs, pks, sigs, exp):
    st, bits = _launch(msgs, pks, sigs)
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]])
    assert np.array_equal(bits, exp == 0)


@pytest.fixture(scope="module")
def corpus(golden):
    """The 4,096-item seeded set (half honest; the others with one bit of s, of R, of the key
    or of the message flipped), the golden edge corpus, and the oracle's statuses."""
    rng = np.random.Generator(np.random.PCG64(4096))
    n = 4096
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
    exp = O.verify_strict_many(msgs, pks, sigs).astype(np.int32)
    assert (exp == 0).sum() == n // 2
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    edge = (hexs("msg", 32), hexs("pk", 32), hexs("sig", 64),
            np.array([i["status"] for i in items], np.int32))
    return {"rand": (msgs, pks, sigs, exp), "edge": edge}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_sizes(corpus, n):
    """n items drawn (seeded) from the edge corpus followed by the random set."""
    pool = [np.concatenate([e, r]) for e, r in zip(corpus["edge"], corpus["rand"])]
    ne = len(corpus["edge"][0])
    rng = np.random.Generator(np.random.PCG64(n))
    # edge items first while they last (every class at n = 257), then random ones
    idx = np.concatenate([rng.permutation(ne), ne + rng.permutation(4096)])[:n]
    if n == 1:
        idx = np.array([ne])   # one honest signature
    m, p, s, e = (a[idx] for a in pool)
    _check(m, p, s, e)


def test_no_survivor(corpus):
    """Every item fails the triage (s with high bits; or an undecodable or small-order
    point, from the edge corpus): the ladder kernel runs over an empty list."""
    m, p, s, _ = (a[:300].copy() for a in corpus["rand"])
    s[:, 63] |= 0xE0
    em, ep, es, ee = corpus["edge"]
    pre = np.isin(ee, [1, 2, 3, 4, 5, 6])
    m, p, s = np.concatenate([m, em[pre]]), np.concatenate([p, ep[pre]]), np.concatenate([s, es[pre]])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.all(exp[:300] == 1) and np.all(np.isin(exp, [1, 2, 3, 4, 5, 6]))
    _check(m, p, s, exp)


def test_all_valid(corpus):
    m, p, s, e = corpus["rand"]
    ok = e == 0
    _check(m[ok], p[ok], s[ok], e[ok])


# Lanes of the persistent ladder kernel when 3 blocks of 256 are resident on each of 256 CUs
# (its occupancy on gfx950); fewer blocks per CU only make it loop sooner.
RESIDENT_LANES = 3 * 256 * 256


def _tiled(corpus, n):
    return tuple(np.resize(a, (n,) + a.shape[1:]) for a in corpus["rand"])


def test_resident_lanes_plus_65_items(corpus):
    """196,608 + 65 items (the 4,096 set tiled): one item per resident lane of the ladder
    kernel and a ragged tail at the input's size. The ladder runs over the survivors only
    (about 87 % of the set), so at this size they still fit one round; the next test sizes
    the list itself past the resident lanes."""
    m, p, s, e = _tiled(corpus, RESIDENT_LANES + 65)
    _check(m, p, s, e)


def test_two_rounds_ragged(corpus):
    """2 x 196,608 + 65 items (the 4,096 set tiled): the survivors of the triage (statuses 0
    and 7, counted from the oracle) outnumber the ladder kernel's resident lanes, so its
    persistent loop runs a second time over the same LDS digit words and per-lane tables,
    with a partly filled last block and a partly filled last wave."""
    m, p, s, e = _tiled(corpus, 2 * RESIDENT_LANES + 65)
    survivors = int(np.isin(e, [0, 7]).sum())
    assert RESIDENT_LANES < survivors < 2 * RESIDENT_LANES
    assert survivors % 256 != 0 and survivors % 64 != 0
    _check(m, p, s, e)


def test_three_slices_ragged(corpus, monkeypatch):
    """NW_TRIAGE_SLICE=1500, which the launcher rounds up to a slice limit of 1,536 items:
    4,096 items then run as three equal slices of 1,366, 1,366 and 1,364 (the launcher's
    ceil(n / limit) slices of ceil(n / slices) items), each with its own list, count and
    planes in the shared region."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "1500")
    m, p, s, e = corpus["rand"]
    _check(m, p, s, e)
