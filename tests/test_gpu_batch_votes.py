"""Signature::verify_batch under the registered signers, a batch that is sent on running over
the votes that did not pass the comb check only (k_batch_signers_count's list, k_bv_items_listed,
k_bv_live_chunks, k_bv_chunks<true>, k_pip_points<true>): in every test the status and the
failing index equal the oracle's under injected coefficients, and the deltas of
nw_batch_signers_stats and nw_batch_signers_vote_stats equal counts taken from the input."""
import numpy as np
import pytest

from narwhal_amd import _lib
from narwhal_amd import crypto as C

import batch_signers_cases as BS
import batch_votes_cases as BV
from test_gpu_batch import _corpus_sizes, _mutate
from test_gpu_batch_signers import NONE, _call, _keys_of, _oracle, _set

pytestmark = pytest.mark.gpu

KNOBS = ("NW_BATCH_SIGNERS", "NW_BATCH_SIGNERS_VOTES", "NW_BATCH_SIGNERS_MIN_VOTES",
         "NW_BATCH_PIPPENGER_MIN", "NW_BATCH_CHUNK", "NW_BATCH_SLICE_UNITS", "NW_FANOUT_PARTS")


@pytest.fixture(autouse=True)
def _registry_cleared(monkeypatch):
    """The registry is process state: every test leaves it empty, and starts without knobs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield
    L = _lib.lib()
    if L.nw_device_count() > 0:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()


def _stats():
    return C.batch_signers_stats() + C.batch_signers_vote_stats()


def _delta(fn):
    a = _stats()
    out = fn()
    return out, tuple(y - x for x, y in zip(a, _stats()))


def _check(dig, pk, sigs, off, z16, reg, ref=None, leave_out=True, want=None):
    """One call under `reg` (left set): the oracle's statuses and failing indices, and the six
    counters moved by the input's counts. Returns the statuses."""
    ost, oix = ref if ref is not None else _oracle(dig, pk, sigs, off, z16)
    _set(reg)
    (st, fi), d = _delta(lambda: _call(dig, pk, sigs, off, z16))
    bad = np.nonzero(st != ost)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], ost[bad[:8]], d)
    assert np.array_equal(fi[ost != 0], oix[ost != 0]), np.nonzero(fi != oix)[0][:8]
    if want is None:
        four, two = BV.six(dig, pk, sigs, off, reg, leave_out)
        want = four + two
    assert d == want, (d, want)
    return st


# ---- 3: the corpus, every failure class, under both plans -------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """60 batches of 0..12 votes under 16 keys, every other non-empty one with a broken vote
    (every failure class); 3 coefficient sets and the oracle's verdicts under each, computed once."""
    dig, pk, sigs, off, keys = BS.corpus(60, 1410, max_n=12, every=2)
    rng = np.random.Generator(np.random.PCG64(1411))
    zs = [rng.integers(0, 256, size=(len(pk), 16), dtype=np.uint8) for _ in range(3)]
    refs = [_oracle(dig, pk, sigs, off, z) for z in zs]
    other = np.frombuffer(BV.stranger(rng)[0], np.uint8).reshape(1, 32)
    return {"in": (dig, pk, sigs, off), "keys": keys, "zs": zs, "refs": refs, "other": other}


@pytest.mark.parametrize("hooks", [("", ""), ("3", "97")])
@pytest.mark.parametrize("which", ["all", "half", "none"])
def test_corpus(monkeypatch, corpus, which, hooks):
    """All, half and none of the corpus' keys registered (none: the registry holds a key that
    signs nothing here, so the path runs and passes no vote). NW_BATCH_CHUNK=3 with slices of 97
    units: batches of several chunks, chunks wholly passed and wholly not, several slices."""
    monkeypatch.setenv("NW_BATCH_CHUNK", hooks[0])
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", hooks[1])
    dig, pk, sigs, off = corpus["in"]
    reg = {"all": corpus["keys"], "half": corpus["keys"][::2], "none": corpus["other"]}[which]
    want = sum(BV.six(dig, pk, sigs, off, reg), ())
    assert (want[4] > 0) == (which != "none") and want[5] > 0
    seen = set()
    for z, ref in zip(corpus["zs"], corpus["refs"]):
        seen |= set(_check(dig, pk, sigs, off, z, reg, ref, want=want).tolist())
    assert seen >= {0, 1, 2, 3, 4, 7}


# ---- 4: every position of a batch of three chunks ---------------------------------------------
@pytest.fixture(scope="module")
def seven():
    dig, pk, sigs, off, keys = BV.honest([7], 1420)
    rng = np.random.Generator(np.random.PCG64(1421))
    return dig, pk, sigs, off, keys, rng.integers(0, 256, size=(7, 16), dtype=np.uint8)


@pytest.mark.parametrize("p", range(7))
def test_positions(monkeypatch, seven, p):
    """One 7-vote batch in chunks of 2, 2 and 3 votes; the only vote that does not pass sits at
    p: valid under a key nobody registered (Ok, 6 left out, 1 run), then broken in each class."""
    monkeypatch.setenv("NW_BATCH_CHUNK", "3")
    dig, pk0, sigs0, off, keys, z = seven
    rng = np.random.Generator(np.random.PCG64(1422 + p))
    pk, sigs = pk0.copy(), sigs0.copy()
    BV.resign(pk, sigs, p, BV.stranger(rng), dig[0].tobytes())
    st = _check(dig, pk, sigs, off, z, keys, want=(6, 1, 0, 1, 6, 1))
    assert st[0] == 0
    for c in range(6):
        pk, sigs = pk0.copy(), sigs0.copy()
        _mutate(sigs, pk, p, c)
        st = _check(dig, pk, sigs, off, z, keys, want=(6, 1, 0, 1, 6, 1))
        assert st[0] != 0


@pytest.mark.parametrize("pq", [(0, 3), (1, 6), (5, 2), (6, 0)])
def test_two_votes_in_different_chunks(monkeypatch, seven, pq):
    """A valid vote of an unregistered key at p and a broken vote at q, in different chunks: the
    third chunk writes the identity, the combine names the broken vote."""
    monkeypatch.setenv("NW_BATCH_CHUNK", "3")
    dig, pk0, sigs0, off, keys, z = seven
    rng = np.random.Generator(np.random.PCG64(1430 + pq[0]))
    for c in range(6):
        pk, sigs = pk0.copy(), sigs0.copy()
        BV.resign(pk, sigs, pq[0], BV.stranger(rng), dig[0].tobytes())
        _mutate(sigs, pk, pq[1], c)
        st = _check(dig, pk, sigs, off, z, keys, want=(5, 2, 0, 1, 5, 2))
        assert st[0] != 0


# ---- 5: a mixed-order key ----------------------------------------------------------------------
@pytest.mark.parametrize("registered", [True, False])
def test_mixed_order_key(registered):
    """The verdict depends on the coefficients, and equals the oracle's under each of 8 sets with
    the five honest votes of every batch left out."""
    dig, pk, sigs, off, keys, zs = BS.mixed_batches(1440, nb=8, q=6, nz=8)
    seen = set()
    for z in zs:
        st = _check(dig, pk, sigs, off, z, keys if registered else keys[:-1],
                    want=(40, 8, 0, 8, 40, 8))
        seen |= set(st.tolist())
    assert seen == {0, 7}


# ---- 6: batches of Pippenger size --------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    """Twelve batches of 400 and 401 votes whose only vote that does not pass sits at position
    0, 63, 64 or n - 1 and is valid under an unregistered key or broken by class 0 or 3, one batch
    of 400 with all but 3 of its votes under unregistered keys, and a 5-vote batch between them."""
    cases = [(p, kind) for kind in ("valid", 0, 3) for p in (0, 63, 64, -1)]
    sizes = [400 + (t & 1) for t in range(len(cases))]
    sizes = np.array(sizes[:6] + [5] + sizes[6:] + [400], np.int64)
    rng = np.random.Generator(np.random.PCG64(1450))
    dig, pk, sigs, off, z16 = _corpus_sizes(sizes, rng, every=0)
    keys = _keys_of(pk)
    o = off.astype(np.int64)
    big = [b for b in range(len(sizes) - 1) if sizes[b] >= 400]
    for b, (p, kind) in zip(big, cases):
        i = int(o[b] + (p if p >= 0 else sizes[b] - 1))
        if kind == "valid":
            BV.resign(pk, sigs, i, BV.stranger(rng), dig[b].tobytes())
        else:
            _mutate(sigs, pk, i, kind)
    last = len(sizes) - 1
    strangers = [BV.stranger(rng) for _ in range(8)]
    for t in range(400):
        if t not in (7, 64, 399):
            BV.resign(pk, sigs, int(o[last]) + t, strangers[t % 8], dig[last].tobytes())
    _mutate(sigs, pk, int(o[6]) + 2, 0)   # the 5-vote batch: one broken vote
    return {"in": (dig, pk, sigs, off, z16), "keys": keys, "ref": _oracle(dig, pk, sigs, off, z16)}


@pytest.mark.parametrize("slice_units", ["", "2600"])
def test_pippenger_sizes(monkeypatch, large, slice_units):
    monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", slice_units)
    dig, pk, sigs, off, z16 = large["in"]
    st = _check(dig, pk, sigs, off, z16, large["keys"], large["ref"])
    assert (st == 0).sum() == 5 and (st == 7).sum() == 5 and (st != 0).sum() == 9
    d = BV.six(dig, pk, sigs, off, large["keys"])
    assert d[0][2:] == (0, 14) and d[1] == (int(off[-1]) - 12 - 1 - 397, 12 + 1 + 397)


# ---- 7: drawn coefficients ---------------------------------------------------------------------
def test_drawn_coefficients(corpus):
    """z16 = None. The corpus' statuses and indices do not depend on the coefficients (asserted
    first from the oracle under two injected sets): a batch whose votes that did not pass are
    all valid is Ok, a batch with a broken vote carries the oracle's status and index."""
    dig, pk, sigs, off = corpus["in"]
    (s0, i0), (s1, i1) = corpus["refs"][:2]
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    for reg in (corpus["keys"], corpus["keys"][::2]):
        _check(dig, pk, sigs, off, None, reg, (s0, i0))


# ---- 8: the knobs ------------------------------------------------------------------------------
def test_knobs(monkeypatch, corpus):
    dig, pk, sigs, off = corpus["in"]
    reg = corpus["keys"][::2]
    monkeypatch.setenv("NW_BATCH_SIGNERS_VOTES", "0")
    four, two = BV.six(dig, pk, sigs, off, reg, leave_out=False)
    assert two[0] == 0 and two[1] > four[1]
    _check(dig, pk, sigs, off, corpus["zs"][0], reg, corpus["refs"][0], leave_out=False)
    monkeypatch.delenv("NW_BATCH_SIGNERS_VOTES")
    _check(dig, pk, sigs, off, corpus["zs"][0], reg, corpus["refs"][0])
    monkeypatch.setenv("NW_BATCH_SIGNERS", "0")
    _check(dig, pk, sigs, off, corpus["zs"][0], reg, corpus["refs"][0], want=(0,) * 6)
    # an empty registry: nothing moves either
    monkeypatch.delenv("NW_BATCH_SIGNERS")
    _check(dig, pk, sigs, off, corpus["zs"][0], NONE, corpus["refs"][0], want=(0,) * 6)


# ---- 9: the service's requests and a fan-out ---------------------------------------------------
def test_service_requests(corpus):
    """The corpus' non-empty batches as verify_batch requests through the native service with the
    hedge off: the oracle's verdicts (drawn coefficients: see test_drawn_coefficients), and the
    jobs behind them count every vote and batch once."""
    from narwhal_amd import service as S
    dig, pk, sigs, off = corpus["in"]
    ost, _ = corpus["refs"][0]
    o = off.astype(np.int64)
    pick = [b for b in range(len(o) - 1) if o[b + 1] > o[b]]
    sub_off = np.zeros(len(pick) + 1, np.uint64)
    sub_off[1:] = np.cumsum([o[b + 1] - o[b] for b in pick])
    rows = np.concatenate([np.arange(o[b], o[b + 1]) for b in pick])
    reg = corpus["keys"][::2]
    want = sum(BV.six(dig[pick], pk[rows], sigs[rows], sub_off, reg), ())
    _set(reg)
    got = [None] * len(pick)

    def run():
        svc = S.NativeService(None, max_items=1 << 16, max_delay=0.001, hedge=0)
        for t, b in enumerate(pick):
            votes = [(pk[i].tobytes(), sigs[i].tobytes()) for i in range(o[b], o[b + 1])]
            svc.submit_verify_batch(dig[b].tobytes(), votes,
                                    lambda stt, ix, t=t: got.__setitem__(t, int(stt)))
        svc.drain()
        svc.close()

    _, d = _delta(run)
    assert got == ost[pick].tolist()
    assert d == want, (d, want)


def test_fanout_parts(monkeypatch, corpus):
    """NW_FANOUT_PARTS=3 under NW_ALL_DEVICES: every part leaves its own passed votes out, and
    the parts' counts add up to the call's."""
    L = _lib.lib()
    assert L.nw_init() > 0
    dig, pk, sigs, off = corpus["in"]
    monkeypatch.setenv("NW_FANOUT_PARTS", "3")
    assert L.nw_set_device(-1) == 0    # NW_ALL_DEVICES
    try:
        _check(dig, pk, sigs, off, corpus["zs"][0], corpus["keys"][::2], corpus["refs"][0])
        _set(NONE)
    finally:
        assert L.nw_set_device(0) == 0
