"""Registered signers (nw_strict_signers_set; k_strict_signers_match, k_strict_comb_select over
one index space, k_strict_keyed_signers, k_strict_signers_count) through
nw_dev_verify_strict_many and the host-buffer entries: every status and the bitmap against the
oracle and against the same launch with the registry cleared, and nw_dev_strict_signers_stats /
nw_dev_strict_comb_stats against counts taken from the input."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C
from oracle import oracle as O

from test_gpu_strict_comb import _hot_keys, _sign_rows, _signed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _set(keys):
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
    rc = L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data if len(keys) else None), len(keys))
    assert rc == 0, L.nw_last_error()
    assert C.strict_signers_count() == (len(np.unique(keys, axis=0)) if len(keys) else 0)


@pytest.fixture(autouse=True)
def _registry_cleared(monkeypatch):
    """The registry is process state: every test leaves it empty."""
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "1")
    monkeypatch.delenv("NW_STRICT_COMB", raising=False)
    monkeypatch.delenv("NW_STRICT_COMB_MIN", raising=False)
    yield
    L = _lib.lib()
    if L.nw_device_count() > 0:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()


def _launch(msgs, pks, sigs):
    """Statuses, verdict bits, comb stats (call-local tables, items checked, passed, sent on)
    and signers stats (keys matched, items under them, items passed under them) of one
    nw_dev_verify_strict_many launch."""
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
    sstats = (ctypes.c_uint64 * 3)()
    assert L.nw_dev_strict_comb_stats(stats, stream) == 0, L.nw_last_error()
    assert L.nw_dev_strict_signers_stats(sstats, stream) == 0, L.nw_last_error()
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()          # the padding bits
    return st.cpu().numpy(), bits[:n].astype(bool), [int(x) for x in stats], [int(x) for x in sstats]


def _under(pks, keys):
    ks = {bytes(k) for k in np.asarray(keys, np.uint8).reshape(-1, 32)}
    return np.array([p.tobytes() in ks for p in pks])


def _expected(pks, exp, reg):
    """[keys matched, items under them, valid items under them] for one slice of these rows."""
    under = _under(pks, reg)
    return [len(np.unique(pks[under], axis=0)) if under.any() else 0, int(under.sum()),
            int((under & (exp == 0)).sum())]


def _check(m, p, s, exp, reg, want=None):
    """The launch under the registered keys (oracle statuses and bitmap, signers stats from the
    input) and with the registry cleared (the same statuses, no match). Leaves `reg` set."""
    _set(np.zeros((0, 32), np.uint8))
    st0, bits0, stats0, ss0 = _launch(m, p, s)
    assert ss0 == [0, 0, 0]
    _set(reg)
    st, bits, stats, ss = _launch(m, p, s)
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]], stats, ss)
    assert np.array_equal(bits, exp == 0)
    assert np.array_equal(st0, st) and np.array_equal(bits0, bits)
    assert ss == (_expected(p, exp, reg) if want is None else want), (ss, stats)
    assert stats[2] + stats[3] == len(m) and ss[2] <= stats[2] <= stats[1] and ss[1] <= stats[1]
    return stats, ss, stats0


@pytest.fixture(scope="module")
def corpus():
    """10 keys, the first 8 of them registered by the tests, and 4,096 items signed round-robin
    with every second one tampered; the oracle's statuses, computed once."""
    rng = np.random.Generator(np.random.PCG64(1010))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(10)]
    m, p, s = _signed(rng, 4096, kps)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps])
    return {"kps": kps, "keys": keys, "reg": keys[:8], "items": (m, p, s, exp)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 4096])
def test_launch_sizes(corpus, n):
    """The first n items at the default NW_STRICT_COMB_MIN: below 256 items nothing is hot by
    count and no call-local table is built, yet the registered keys' valid items pass by the
    comb; at 4,096 the two unregistered keys are hot by count beside them."""
    m, p, s, e = (a[:n] for a in corpus["items"])
    stats, ss, stats0 = _check(m, p, s, e, corpus["reg"])
    assert ss[2] > 0 and stats[2] >= ss[2]
    if n <= 300:
        assert stats[0] == 0 and stats[1:3] == ss[1:] and stats0 == [0, 0, 0, n]
    else:
        hot = _hot_keys(p, 256) - {k.tobytes() for k in corpus["reg"]}
        assert hot == {k.tobytes() for k in corpus["keys"][8:]}
        assert stats[0] == len(hot) == 2
        assert stats[2] == int((_under(p, corpus["keys"]) & (e == 0)).sum())


def test_the_cut(corpus, monkeypatch):
    """NW_STRICT_SIGNERS_MIN_ITEMS above n: the launch ignores the registry."""
    m, p, s, e = (a[:300] for a in corpus["items"])
    _set(corpus["reg"])
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "301")
    st, bits, stats, ss = _launch(m, p, s)
    assert np.array_equal(st, e) and np.array_equal(bits, e == 0)
    assert ss == [0, 0, 0] and stats == [0, 0, 0, 300]
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "300")
    st, bits, stats, ss = _launch(m, p, s)
    assert np.array_equal(st, e) and ss == _expected(p, e, corpus["reg"])


def test_several_slices(corpus, monkeypatch):
    """NW_TRIAGE_SLICE=1024 over 4,096 items: slice q holds registered keys 2q and 2q + 1 and one
    unregistered key; the matches of a launch are summed over its slices."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "1024")
    rng = np.random.Generator(np.random.PCG64(1011))
    key_of = [[2 * (i // 1024), 2 * (i // 1024) + 1, 8 + ((i // 1024) & 1)][i % 3] for i in range(4096)]
    m, p, s = _sign_rows(rng, corpus["kps"], key_of)
    for i in range(0, 4096, 5):
        s[i, rng.integers(0, 64)] ^= np.uint8(1 << rng.integers(0, 8))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    want = np.sum([_expected(p[a:a + 1024], exp[a:a + 1024], corpus["reg"])
                   for a in range(0, 4096, 1024)], axis=0).tolist()
    assert want[0] == 8
    _check(m, p, s, exp, corpus["reg"], want)


def test_slice_without_registered_or_hot_key(corpus):
    """300 items under the two unregistered keys while 8 other keys are registered: the comb
    kernels are skipped on the device, the triage takes the whole slice."""
    rng = np.random.Generator(np.random.PCG64(1012))
    m, p, s = _signed(rng, 300, corpus["kps"][8:])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    stats, ss, _ = _check(m, p, s, exp, corpus["reg"], [0, 0, 0])
    assert stats == [0, 0, 0, 300]


_READERS = {"keyset": 3, "comb": 4, "decided": 2, "signers": 3}


def _readers(order):
    """The counters of the last launch through the four readers, called in `order`."""
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    out = {}
    for name in order:
        buf = (ctypes.c_uint64 * _READERS[name])()
        assert getattr(L, f"nw_dev_strict_{name}_stats")(buf, stream) == 0, L.nw_last_error()
        out[name] = [int(x) for x in buf]
    return out


def test_counter_readers_agree(corpus, monkeypatch):
    """200 items in four slices (NW_TRIAGE_SLICE=64) at NW_STRICT_COMB_MIN=16: two keys of 80 and
    60 uses, one registered key of 40, 20 strangers of one use each, nine broken signatures. The
    four readers project one snapshot of the launch's counters: whatever the order and however
    often they are called they give the same values, which satisfy the identities between them;
    without the comb path, and without the key set, they give the fallback tuples."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "64")
    monkeypatch.setenv("NW_STRICT_COMB_MIN", "16")
    rng = np.random.Generator(np.random.PCG64(1013))
    kps = [corpus["kps"][0], corpus["kps"][8], corpus["kps"][9]]
    kps += [O.keypair_from_seed(rng.bytes(32)) for _ in range(20)]
    n = 200
    key_of = [[1, 1, 1, 1, 2, 2, 2, 0, 0, 3 + i // 10][i % 10] for i in range(n)]
    m, p, s = _sign_rows(rng, kps, key_of)
    for i in range(0, n, 23):
        s[i, rng.integers(0, 64)] ^= np.uint8(1 << rng.integers(0, 8))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert 0 < int((exp != 0).sum()) <= 9
    _set(corpus["keys"][:1])
    st, bits, stats, ss = _launch(m, p, s)
    assert np.array_equal(st, exp) and np.array_equal(bits, exp == 0)
    fwd, rev = list(_READERS), list(_READERS)[::-1]
    got = [_readers(fwd), _readers(fwd), _readers(rev), _readers(rev)]
    print("readers:", got[0])
    assert all(g == got[0] for g in got[1:]), got
    keyset, comb, decided, signers = (got[0][k] for k in fwd)
    assert comb == stats and signers == ss
    assert comb[2] + comb[3] == n
    assert keyset[1] + keyset[2] == n
    assert decided[0] + decided[1] <= comb[3]
    assert signers[2] <= signers[1] <= comb[1]
    monkeypatch.setenv("NW_STRICT_COMB", "0")
    st, bits, _, _ = _launch(m, p, s)
    assert np.array_equal(st, exp) and np.array_equal(bits, exp == 0)
    for got in (_readers(fwd), _readers(rev)):
        assert got["comb"] == [0, 0, 0, n] and got["decided"] == [0, 0]
        assert got["signers"] == [0, 0, 0]
        assert got["keyset"] == keyset          # the key set does not depend on the comb path
    monkeypatch.delenv("NW_STRICT_COMB")
    monkeypatch.setenv("NW_STRICT_KEYS", "0")
    st, bits, _, _ = _launch(m, p, s)
    assert np.array_equal(st, exp) and np.array_equal(bits, exp == 0)
    for got in (_readers(fwd), _readers(rev)):
        assert got["keyset"] == [0, 0, n] and got["comb"] == [0, 0, 0, n]
        assert got["decided"] == [0, 0] and got["signers"] == [0, 0, 0]


def test_replacing_the_registry(corpus):
    """Set A, a disjoint set B, then none: the keys matched follow the registry each time, and
    the cleared registry is the launch sequence of before."""
    m, p, s, e = (a[:300] for a in corpus["items"])
    for reg in (corpus["keys"][:4], corpus["keys"][4:8]):
        _set(reg)
        st, bits, stats, ss = _launch(m, p, s)
        assert np.array_equal(st, e) and np.array_equal(bits, e == 0)
        assert ss == _expected(p, e, reg) and ss[0] == 4
    _set(corpus["keys"][:0])
    st, bits, stats, ss = _launch(m, p, s)
    assert np.array_equal(st, e) and ss == [0, 0, 0] and stats == [0, 0, 0, 300]


def test_regions_that_grow(corpus):
    """300 items, then 65,536 + 65 (the triage and comb regions are reallocated), then 300 again:
    the registry survives, the statuses are the oracle's each time."""
    _set(corpus["reg"])
    big = 65536 + 65
    for n in (300, big, 300):
        m, p, s, e = (np.resize(a, (n,) + a.shape[1:]) for a in corpus["items"])
        st, bits, stats, ss = _launch(m, p, s)
        assert np.array_equal(st, e) and np.array_equal(bits, e == 0)
        assert ss == _expected(p, e, corpus["reg"]) and ss[0] == 8
    assert C.strict_signers_count() == 8


def test_concurrent_launches_and_updates(corpus):
    """Two host threads on two torch streams run 20 launches of 2,048 items each while the main
    thread sets and clears the registry ten times: every launch's statuses are the oracle's
    (its stats may be of either state). The device's lease orders the three."""
    L = _lib.lib()
    assert L.nw_init() > 0
    dev = torch.device("cuda", 0)
    m, p, s, e = (a[:2048] for a in corpus["items"])
    errors = []

    def worker(t):
        try:
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                dm, dp, ds = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (m, p, s))
                P = lambda x: ctypes.c_void_p(x.data_ptr())
                for _ in range(20):
                    st = torch.full((2048,), -99, dtype=torch.int32, device=dev)
                    bm = torch.zeros(2048 // 8, dtype=torch.uint8, device=dev)
                    rc = L.nw_dev_verify_strict_many(P(dm), 32, P(dp), P(ds), 2048, P(st), P(bm),
                                                     ctypes.c_void_p(stream.cuda_stream))
                    assert rc == 0, L.nw_last_error()
                    stream.synchronize()
                    assert np.array_equal(st.cpu().numpy(), e)
        except BaseException as x:   # noqa: BLE001 (reported by the main thread)
            errors.append((t, repr(x)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for r in range(10):
        _set(corpus["reg"] if r % 2 == 0 else corpus["keys"][:0])
    for t in th:
        t.join()
    assert not errors, errors


def test_host_buffer_entries_and_service(corpus):
    """500 items through nw_verify_strict_many, through nw_submit_verify_strict + wait, and as
    500 verify requests of the native service: the oracle's verdicts, and the launch behind
    each shows the registered keys matched."""
    from narwhal_amd import service as S
    L = _lib.lib()
    m, p, s, e = (np.ascontiguousarray(a[:500]) for a in corpus["items"])
    _set(corpus["reg"])
    want = _expected(p, e, corpus["reg"])
    st, _ = C.verify_strict_many(m, p, s)
    assert np.array_equal(st, e)
    assert list(C.strict_signers_stats()) == want
    st = np.full(500, -9, np.int32)
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_strict(m.ctypes.data, 32, p.ctypes.data, s.ctypes.data, 500,
                                   st.ctypes.data, None, ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    assert np.array_equal(st, e)
    assert list(C.strict_signers_stats()) == want
    svc = S.NativeService(None, max_items=1 << 16, max_delay=0.001, hedge=0)
    got = [None] * 500
    for i in range(500):
        svc.submit_verify(m[i].tobytes(), p[i].tobytes(), s[i].tobytes(),
                          lambda stt, ix, i=i: got.__setitem__(i, int(stt)))
    svc.drain()
    svc.close()
    assert got == e.tolist()
    ss = C.strict_signers_stats()     # of the last job, which holds some of the 500
    assert 1 <= ss[0] <= 8 and 1 <= ss[2] <= ss[1] <= 500


_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import test_gpu_strict_signers as T
from narwhal_amd import _lib
from oracle import oracle as O

rng = np.random.Generator(np.random.PCG64(7))
kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(8)]
keys = np.array([np.frombuffer(kp[0], np.uint8) for kp in kps])
m, p, s = T._signed(rng, 300, kps)
exp = O.verify_strict_many(m, p, s).astype(np.int32)
T._set(keys)
for _ in range(2):
    st, bits, stats, ss = T._launch(m, p, s)
    assert np.array_equal(st, exp) and np.array_equal(bits, exp == 0), (stats, ss)
    assert ss == [0, 0, 0] and stats == [0, 0, 0, 300], (stats, ss)
os.environ["NW_STRICT_SIGNERS_MAX"] = "4"
L = _lib.lib()
assert L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data), 8) == -1    # NW_E_INVALID_ARG
assert T.C.strict_signers_count() == 8
assert L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data), 4) == 0
assert T.C.strict_signers_count() == 4
print("LIMIT_OK", stats, ss)
"""


def test_three_gb_limit():
    """Under the 3 GB allocation limit of test_gpu_memory.py registering 8 keys succeeds, the B
    comb (11.8 GB) cannot be had, so the launch runs without the path: the oracle's statuses,
    and no error is left behind for the second launch. NW_STRICT_SIGNERS_MAX=4 refuses 8 keys."""
    env = dict(os.environ, NW_DEVICE_MEM_LIMIT=str(3 * 10**9), NW_STRICT_SIGNERS_MIN_ITEMS="1")
    env.pop("NW_STRICT_COMB", None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _CHILD], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "LIMIT_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
