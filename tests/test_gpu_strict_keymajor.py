"""Key-major order of the strict launch's comb check (k_km_hist / k_km_scan / k_km_scatter, then
the comb kernels, k_strict_keyed_inv, k_strict_signers_count and k_strict_todo_list in position
space) through nw_dev_verify_strict_many and nw_dev_verify_strict_msgs_many with
NW_STRICT_COMB_MIN=64: every status and the bitmap against the oracle and against the same
launch with NW_STRICT_KEY_MAJOR=0, the four statistics calls equal between the two, and
nw_dev_strict_keymajor_stats showing that the sort ran (or did not, where that is the point).
Keys and signatures are made on the device, as bench.py makes them; the status array is
prefilled with -99, so an item the permutation dropped shows."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from oracle import oracle as O

import strict_msgs_cases as SM
from test_gpu_strict_comb import _hot_keys, _sampled, _under

pytestmark = pytest.mark.gpu

MIN = 64
CHUNK = 16384   # nw_strict_keymajor.hpp kKmChunk: the items one block of the sort takes
P_FIELD = 2**255 - 19
STATS = (("nw_dev_strict_comb_stats", 4), ("nw_dev_strict_decided_stats", 2),
         ("nw_dev_strict_signers_stats", 3), ("nw_dev_strict_keyset_stats", 3))


def _ready():
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    return L


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _all_stats(L):
    out = {}
    for name, k in STATS + (("nw_dev_strict_keymajor_stats", 3),):
        v = (ctypes.c_uint64 * k)()
        assert getattr(L, name)(v, _stream()) == 0, L.nw_last_error()
        out[name] = [int(x) for x in v]
    return out


def _launch(msgs, pks, sigs):
    """Statuses, verdict bits and every statistic of one nw_dev_verify_strict_many launch."""
    L = _ready()
    dev = torch.device("cuda", 0)
    n = len(msgs)
    m, p, s = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (msgs, pks, sigs))
    st = torch.full((n,), -99, dtype=torch.int32, device=dev)
    bm = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    rc = L.nw_dev_verify_strict_many(_P(m), 32, _P(p), _P(s), n, _P(st), _P(bm), _stream())
    assert rc == 0, L.nw_last_error()
    stats = _all_stats(L)
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()
    return st.cpu().numpy(), bits[:n].astype(bool), stats


def _launch_msgs(c):
    """The same through the entry over messages of any length."""
    L = _ready()
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (c.data, c.offsets.view(np.int64), c.lengths.view(np.int64), c.pks, c.sigs)]
    st = torch.full((c.n,), -99, dtype=torch.int32, device=dev)
    bm = torch.zeros((c.n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = L.nw_dev_verify_strict_msgs_many(_P(t[0]), _P(t[1]), _P(t[2]), _P(t[3]), _P(t[4]), c.n,
                                          _P(st), _P(bm), _stream())
    assert rc == 0, L.nw_last_error()
    stats = _all_stats(L)
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    return st.cpu().numpy(), bits[:c.n].astype(bool), stats


def _on_and_off(monkeypatch, launch, exp, on="1"):
    """The launch with NW_STRICT_KEY_MAJOR = `on` (None: unset) and with 0: both give the
    oracle's statuses and bitmap and the same four statistics. Returns both launches'
    statistics."""
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
    if on is None:
        monkeypatch.delenv("NW_STRICT_KEY_MAJOR", raising=False)
    else:
        monkeypatch.setenv("NW_STRICT_KEY_MAJOR", on)
    st, bits, stats = launch()
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]], stats)
    assert np.array_equal(bits, exp == 0)
    monkeypatch.setenv("NW_STRICT_KEY_MAJOR", "0")
    st0, bits0, stats0 = launch()
    assert np.array_equal(st0, st) and np.array_equal(bits0, bits)
    for name, _ in STATS:
        assert stats[name] == stats0[name], (name, stats[name], stats0[name])
    assert stats0["nw_dev_strict_keymajor_stats"] == [0, 0, 0]
    return stats, stats0


def _device_signed(rng, seeds, key_of):
    """len(key_of) items with random 32-byte messages, item i signed by key key_of[i] of the
    keys made from `seeds` on the device. Returns (msgs, pks, sigs, the keys)."""
    L = _ready()
    dev = torch.device("cuda", 0)
    n, nk = len(key_of), len(seeds)
    sd = torch.from_numpy(np.ascontiguousarray(seeds)).to(dev)
    pk = torch.empty((nk, 32), dtype=torch.uint8, device=dev)
    assert L.nw_dev_keypair_from_seed_many(_P(sd), nk, _P(pk), _stream()) == 0, L.nw_last_error()
    sks = torch.cat([sd, pk], dim=1).index_select(
        0, torch.from_numpy(np.asarray(key_of, np.int64)).to(dev)).contiguous()
    msgs = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).to(dev)
    sigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    rc = L.nw_dev_sign_many(_P(sks), 64, _P(msgs), 32, n, _P(sigs), _stream())
    assert rc == 0, L.nw_last_error()
    torch.cuda.synchronize()
    return (msgs.cpu().numpy().copy(), sks[:, 32:].cpu().numpy().copy(), sigs.cpu().numpy().copy(),
            pk.cpu().numpy().copy())


def _tamper(rng, msgs, pks, sigs, rows):
    """One flipped bit of s, of R, of the key or of the message (test_gpu_strict_comb._signed)."""
    for i in rows:
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


def _enc(y, sign):
    return np.frombuffer((y | (sign << 255)).to_bytes(32, "little"), np.uint8)


NKEYS = 48      # 40 used enough to be hot, 6 cold, and the rows of 2 go to keys that never are


@pytest.fixture(scope="module")
def corpus(golden):
    """Two sort chunks plus 37 items, then the golden edge corpus. Key 0 signs more items than a
    chunk holds (its bin spans the blocks), key 1 exactly 64 (4 of them on sampled rows, so that
    it counts as hot), keys 2..39 share the rest unevenly, keys 40..45 sign 5 items each (cold),
    the rows of keys 46 / 47 carry a key that does not decode / has small order. Every second
    item is tampered."""
    rng = np.random.Generator(np.random.PCG64(1212))
    n = 2 * CHUNK + 37
    key_of = np.full(n, -1, np.int64)
    sampled = np.nonzero(_sampled(n))[0]
    plain = np.nonzero(~_sampled(n))[0]
    # key 1: exactly 64 rows, 4 of them sampled and honest (even rows are never tampered)
    rows1 = np.concatenate([sampled[sampled % 2 == 0][10:14], plain[plain % 2 == 0][500:560]])
    key_of[rows1] = 1
    free = np.nonzero(key_of < 0)[0]
    rng.shuffle(free)
    a = CHUNK + 1000
    key_of[free[:a]] = 0
    for k in range(40, 46):
        key_of[free[a:a + 5]] = k
        a += 5
    for k in (46, 47):
        key_of[free[a:a + 200]] = k
        a += 200
    rest = free[a:]
    weights = np.arange(8, 46, dtype=np.float64)   # ~110 to ~640 items a key
    key_of[rest] = 2 + rng.choice(38, size=len(rest), p=weights / weights.sum())
    assert (key_of == 0).sum() > CHUNK and (key_of == 1).sum() == 64
    seeds = rng.integers(0, 256, size=(NKEYS, 32), dtype=np.uint8)
    m, p, s, keys = _device_signed(rng, seeds, key_of)
    p[key_of == 46] = _enc(2, 0)    # not on the curve
    p[key_of == 47] = _enc(1, 0)    # the identity: small order
    _tamper(rng, m, p, s, [i for i in range(1, n, 2) if key_of[i] != 1])
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    m, p, s = (np.concatenate([x, hexs(k, w)])
               for x, k, w in ((m, "msg", 32), (p, "pk", 32), (s, "sig", 64)))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.array_equal(exp[n:], np.array([i["status"] for i in items], np.int32))
    assert (exp[:n] == 0).sum() > n // 3 and len(set(exp[:n].tolist())) >= 4
    return {"m": m, "p": p, "s": s, "exp": exp, "keys": keys, "seeds": seeds, "key_of": key_of}


@pytest.fixture
def registry():
    """Sets the device's registered signers; always cleared afterwards."""
    L = _ready()

    def put(keys):
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        rc = L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data if len(keys) else None),
                                     len(keys))
        assert rc == 0, L.nw_last_error()
    try:
        put(np.zeros((0, 32), np.uint8))
        yield put
    finally:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()


def test_sort_chunks(corpus, monkeypatch, registry):
    """One slice of two full sort chunks and a ragged third, forced on."""
    c = corpus
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(c["m"], c["p"], c["s"]), c["exp"])
    comb, km = stats["nw_dev_strict_comb_stats"], stats["nw_dev_strict_keymajor_stats"]
    # keys 0 and 1 and (nearly) all of 2..39 are hot; every item under a hot key was checked
    # by the comb and placed by the sort, in one bin per hot key (fewer than 1,023 live keys:
    # groups of one)
    hot = _hot_keys(c["p"])
    assert {c["keys"][0].tobytes(), c["keys"][1].tobytes()} <= hot and 36 <= len(hot)
    assert comb[:2] == [len(hot), int(_under(c["p"], hot).sum())], comb
    assert km == [comb[1], comb[0], 1], (km, comb)


def test_several_slices(corpus, monkeypatch, registry):
    """The same corpus in three slices with a ragged last one: the histogram is left clean for
    the next slice, the cursors and the order are rebuilt for each."""
    c = corpus
    n = len(c["exp"])
    per = -(-n // 3)
    assert n % 3 != 0 and per % 64 != 0 and per < CHUNK
    monkeypatch.setenv("NW_TRIAGE_SLICE", str(per))
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(c["m"], c["p"], c["s"]), c["exp"])
    comb, km = stats["nw_dev_strict_comb_stats"], stats["nw_dev_strict_keymajor_stats"]
    hots = [_hot_keys(c["p"][a:a + per]) for a in range(0, n, per)]
    assert comb[0] == sum(len(h) for h in hots) > 30
    assert comb[1] == sum(int(_under(c["p"][a:a + per], h).sum())
                          for a, h in zip(range(0, n, per), hots))
    assert km == [comb[1], comb[0], 3], (km, comb)


def test_registered_signers(corpus, monkeypatch, registry):
    """Half the corpus's keys registered, behind 1,100 registered keys that sign nothing: one
    index space of more than 1,023 indices, so the bins are groups of two indices; the
    registered-signers comb kernel and the counting kernel run in position space."""
    c = corpus
    rng = np.random.Generator(np.random.PCG64(77))
    filler = _device_signed(rng, rng.integers(0, 256, size=(1100, 32), dtype=np.uint8), [0])[3]
    registry(np.concatenate([filler, c["keys"][0:40:2]]))
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "1")
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(c["m"], c["p"], c["s"]), c["exp"])
    comb, km = stats["nw_dev_strict_comb_stats"], stats["nw_dev_strict_keymajor_stats"]
    sg = stats["nw_dev_strict_signers_stats"]
    assert sg[0] == 20 and sg[1] > CHUNK * 3 // 4 and 0 < sg[2] < sg[1], sg
    local = _hot_keys(c["p"]) - {k.tobytes() for k in c["keys"][0:40:2]}
    assert comb[0] == len(local) >= 18, comb   # a registered key takes no call-local table
    # adjacent rows of the registry share a bin, so do adjacent call-local tables
    assert km[0] == comb[1] and km[2] == 1 and (sg[0] + comb[0]) // 2 <= km[1] <= sg[0] + comb[0]


def test_messages_of_any_length(monkeypatch, registry):
    """The entry over messages of any length: k_strict_keyed_hot_k sorted, then
    k_strict_keyed_signers_k with four of the eight keys registered."""
    c = SM.tiled()
    stats, _ = _on_and_off(monkeypatch, lambda: _launch_msgs(c), c.ref)
    comb, km = stats["nw_dev_strict_comb_stats"], stats["nw_dev_strict_keymajor_stats"]
    assert comb[0] > 0 and km == [comb[1], comb[0], 1], (km, comb)
    keys = []
    for p, v in zip(c.pks, c.variant):
        if v != "a_off_curve" and p.tobytes() not in keys:
            keys.append(p.tobytes())
    registry(np.frombuffer(b"".join(keys[::2]), np.uint8).reshape(-1, 32))
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "1")
    stats, _ = _on_and_off(monkeypatch, lambda: _launch_msgs(c), c.ref)
    comb, km = stats["nw_dev_strict_comb_stats"], stats["nw_dev_strict_keymajor_stats"]
    assert stats["nw_dev_strict_signers_stats"][0] == 4
    assert km[0] == comb[1] and km[2] == 1, (km, comb)


def test_one_key(monkeypatch, registry):
    """Every item under one key: one bin that spans both blocks of the sort."""
    rng = np.random.Generator(np.random.PCG64(5))
    n = CHUNK + 100
    m, p, s, _ = _device_signed(rng, rng.integers(0, 256, size=(1, 32), dtype=np.uint8), [0] * n)
    _tamper(rng, m, p, s, [i for i in range(1, n, 16) if i % 8 != 5])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(m, p, s), exp)
    assert stats["nw_dev_strict_keymajor_stats"] == [n, 1, 1]


def test_no_hot_key(monkeypatch, registry):
    """A key per item: nothing is hot, the sort kernels exit, and the triage (which reads no
    order) takes the whole slice."""
    rng = np.random.Generator(np.random.PCG64(6))
    n = 2048 + 37
    m, p, s, _ = _device_signed(rng, rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
                                np.arange(n))
    _tamper(rng, m, p, s, range(1, n, 2))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(m, p, s), exp)
    assert stats["nw_dev_strict_comb_stats"] == [0, 0, 0, n]
    assert stats["nw_dev_strict_keymajor_stats"] == [0, 0, 0]


def test_below_the_automatic_threshold(corpus, monkeypatch, registry):
    """The knob unset: a slice of 33 thousand items stays in item order (the host's part of the
    automatic decision), with the same results."""
    c = corpus
    stats, _ = _on_and_off(monkeypatch, lambda: _launch(c["m"], c["p"], c["s"]), c["exp"], on=None)
    assert stats["nw_dev_strict_comb_stats"][0] == len(_hot_keys(c["p"]))
    assert stats["nw_dev_strict_keymajor_stats"] == [0, 0, 0]
