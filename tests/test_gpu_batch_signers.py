"""Signature::verify_batch under the registered signers (nw_strict_signers_set; k_key_lambda,
k_batch_signers, k_batch_signers_inv, k_batch_signers_count, then launch_verify_batch under the
skip list, Pippenger kernels included) through the host-buffer entries: in every test the status
and the failing index equal the oracle's and the same call's with the registry cleared, and the
deltas of nw_batch_signers_stats equal counts taken from the input with the oracle's per-vote
strict statuses."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from narwhal_amd import _lib
from narwhal_amd import crypto as C
from oracle import oracle as O

import batch_signers_cases as BS
from test_gpu_batch import _corpus, _corpus_sizes, _mutate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros((0, 32), np.uint8)


def _set(keys):
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
    rc = L.nw_strict_signers_set(ctypes.c_void_p(keys.ctypes.data if len(keys) else None), len(keys))
    assert rc == 0, L.nw_last_error()


@pytest.fixture(autouse=True)
def _registry_cleared(monkeypatch):
    """The registry is process state: every test leaves it empty, and starts without knobs."""
    for k in ("NW_BATCH_SIGNERS", "NW_BATCH_SIGNERS_MIN_VOTES", "NW_BATCH_PIPPENGER_MIN",
              "NW_BATCH_CHUNK", "NW_BATCH_SLICE_UNITS"):
        monkeypatch.delenv(k, raising=False)
    yield
    L = _lib.lib()
    if L.nw_device_count() > 0:
        assert L.nw_strict_signers_set(None, 0) == 0, L.nw_last_error()


def _call(dig, pk, sigs, off, z16, blocking=False):
    """(status, fail index) of one call: nw_submit_verify_batch_many + wait, or the blocking
    nw_verify_batch_many (status only)."""
    L = _lib.lib()
    dig, pk, sigs = (np.ascontiguousarray(a, np.uint8) for a in (dig, pk, sigs))
    off = np.ascontiguousarray(off, np.uint64)
    nb = len(off) - 1
    z = None if z16 is None else np.ascontiguousarray(z16, np.uint8)
    P = lambda a: ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)
    st = np.full(nb, -99, np.int32)
    fi = np.full(nb, 2**64 - 1, np.uint64)
    if blocking:
        assert L.nw_verify_batch_many(P(dig), P(pk), P(sigs), P(off), nb, P(z), P(st)) == 0, \
            L.nw_last_error()
        return st, None
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_batch_many(P(dig), P(pk), P(sigs), P(off), nb, P(z), P(st), P(fi),
                                       ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    return st, fi


def _delta(fn):
    a = C.batch_signers_stats()
    out = fn()
    b = C.batch_signers_stats()
    return out, tuple(y - x for x, y in zip(a, b))


def _oracle(dig, pk, sigs, off, z16):
    o = off.astype(np.int64)
    n = int(o[-1])
    z = z16 if z16 is not None else np.zeros((max(n, 1), 16), np.uint8) + 1
    ref = [O.verify_batch(dig[b].tobytes(), pk[o[b]:o[b + 1]], sigs[o[b]:o[b + 1]],
                          z[o[b]:o[b + 1]]) for b in range(len(o) - 1)]
    return np.array([r[0] for r in ref], np.int32), np.array([r[1] for r in ref], np.uint64)


def _check(dig, pk, sigs, off, z16, reg, ref=None, want=None):
    """The call with the registry cleared (no counter moves) and under `reg` (the counters move
    by the input's counts): both give the oracle's statuses and failing indices. Leaves `reg`
    set; returns the statuses and the delta."""
    ost, oix = ref if ref is not None else _oracle(dig, pk, sigs, off, z16)
    _set(NONE)
    (st0, fi0), d0 = _delta(lambda: _call(dig, pk, sigs, off, z16))
    assert d0 == (0, 0, 0, 0)
    _set(reg)
    (st, fi), d = _delta(lambda: _call(dig, pk, sigs, off, z16))
    bad = np.nonzero(st != ost)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], ost[bad[:8]], d)
    assert np.array_equal(fi[ost != 0], oix[ost != 0])
    assert np.array_equal(st0, st) and np.array_equal(fi0, fi)
    exp = BS.expected(dig, pk, sigs, off, reg)[2] if want is None else want
    assert d == exp, (d, exp)
    return st, d


def _keys_of(pk):
    """The corpus' honest keys: every key of the input but the off-curve one of _mutate."""
    ks = np.unique(pk, axis=0)
    return ks[[O.decompress(k.tobytes()) is not None for k in ks]]


@pytest.fixture(scope="module")
def small():
    """300 batches of 0..40 votes under 64 keys, one batch in four broken (every failure
    class), with injected coefficients; the oracle's verdicts computed once."""
    dig, pk, sigs, off, z16 = _corpus(300, seed=1210)
    keys = _keys_of(pk)
    assert len(keys) == 64
    return {"in": (dig, pk, sigs, off, z16), "keys": keys, "ref": _oracle(dig, pk, sigs, off, z16)}


def test_all_keys_registered(small):
    dig, pk, sigs, off, z16 = small["in"]
    st, d = _check(dig, pk, sigs, off, z16, small["keys"], small["ref"])
    assert (st != 0).any() and d[2] > 150 and d[3] > 50 and d[2] + d[3] == 300
    # settled is exactly "the verdict is Ok" here: every signer is registered with lambda 0
    assert d[2] == int((st == 0).sum())
    # the blocking entry: the same verdicts, the same counts
    (stb, _), db = _delta(lambda: _call(dig, pk, sigs, off, z16, blocking=True))
    assert np.array_equal(stb, st) and db == d


def test_half_of_the_keys_registered(small):
    dig, pk, sigs, off, z16 = small["in"]
    st, d = _check(dig, pk, sigs, off, z16, small["keys"][::2], small["ref"])
    assert 0 < d[0] < int(off[-1]) and d[2] < int((st == 0).sum())


def test_random_coefficients(small):
    dig, pk, sigs, off, _ = small["in"]
    _check(dig, pk, sigs, off, None, small["keys"], small["ref"])


def test_mixed_order_key_with_injected_coefficients():
    """The batches of test_hostcheck_batch_signers: under each of 8 coefficient sets the verdicts
    are the oracle's, Ok and NW_ERR_EQUATION both occur, and nothing is ever settled."""
    dig, pk, sigs, off, keys, zs = BS.mixed_batches(seed=1204)
    seen = set()
    for z in zs:
        st, d = _check(dig, pk, sigs, off, z, keys, want=(40, 8, 0, 8))
        seen |= set(st.tolist())
    assert seen == {0, 7}


PIP_SIZES = np.array([400, 3, 0, 1200, 17, 401, 650, 2, 399, 900], np.int64)


@pytest.mark.parametrize("slice_units", ["", "2600"])
def test_pippenger_sizes_all_valid(monkeypatch, slice_units):
    monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", slice_units)
    rng = np.random.Generator(np.random.PCG64(1220 + len(slice_units)))
    dig, pk, sigs, off, z16 = _corpus_sizes(PIP_SIZES, rng, every=0)
    st, d = _check(dig, pk, sigs, off, z16, _keys_of(pk))
    assert not st.any() and d == (int(PIP_SIZES.sum()), 0, len(PIP_SIZES), 0)


@pytest.mark.parametrize("slice_units", ["", "2600"])
def test_pippenger_sizes_broken(monkeypatch, slice_units):
    """One broken vote per non-empty batch and a later second failure in three large ones: the
    first failure is reported, only the empty batch is settled."""
    monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", slice_units)
    rng = np.random.Generator(np.random.PCG64(1230 + len(slice_units)))
    dig, pk, sigs, off, z16 = _corpus_sizes(PIP_SIZES, rng, every=1)
    for b in (3, 6, 9):
        _mutate(sigs, pk, int(off[b + 1]) - 5, 3)
    st, d = _check(dig, pk, sigs, off, z16, _keys_of(pk))
    assert (st != 0).sum() == 9 and d[2:] == (1, 9)


def test_pippenger_some_settled(monkeypatch):
    """Large and small batches, every other large one broken: the settled large batches leave
    the Pippenger list, the others keep their verdicts."""
    monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
    rng = np.random.Generator(np.random.PCG64(1240))
    dig, pk, sigs, off, z16 = _corpus_sizes(PIP_SIZES, rng, every=0)
    for t, b in enumerate((0, 5, 9)):
        _mutate(sigs, pk, int(off[b]) + 7 * t, (0, 3, 4)[t])
    st, d = _check(dig, pk, sigs, off, z16, _keys_of(pk))
    assert sorted(np.nonzero(st)[0].tolist()) == [0, 5, 9] and d[2:] == (7, 3)


@pytest.mark.parametrize("n,cls", [(2925, None), (2925, 0), (2925, 3), (10000, None), (10000, 0), (10000, 3)])
def test_lone_batch(n, cls):
    """One batch alone in the call, the sizes of the fused launches: under the registry it takes
    the separate kernels. Valid: Ok, one batch settled; broken: the oracle's status and index,
    one batch sent on."""
    rng = np.random.Generator(np.random.PCG64(1250 + n + (cls or 0)))
    dig, pk, sigs, off, z16 = _corpus_sizes(np.array([n]), rng, every=0)
    if cls is not None:
        _mutate(sigs, pk, int(rng.integers(0, n)), cls)
    st, d = _check(dig, pk, sigs, off, z16, _keys_of(pk))
    assert d == ((n, 0, 1, 0) if cls is None else (n - 1, 1, 0, 1))
    assert (st[0] == 0) == (cls is None)


def test_plan_hooks(monkeypatch, small):
    monkeypatch.setenv("NW_BATCH_CHUNK", "3")
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", "97")
    dig, pk, sigs, off, z16 = small["in"]
    _check(dig, pk, sigs, off, z16, small["keys"], small["ref"])


def test_knobs(monkeypatch, small):
    """NW_BATCH_SIGNERS=0 and a minimum above the call's votes: the path is not taken, the
    verdicts are the same."""
    dig, pk, sigs, off, z16 = small["in"]
    ost, oix = small["ref"]
    _set(small["keys"])
    for name, val in (("NW_BATCH_SIGNERS", "0"), ("NW_BATCH_SIGNERS_MIN_VOTES", str(int(off[-1]) + 1))):
        monkeypatch.setenv(name, val)
        (st, fi), d = _delta(lambda: _call(dig, pk, sigs, off, z16))
        assert d == (0, 0, 0, 0) and np.array_equal(st, ost)
        assert np.array_equal(fi[ost != 0], oix[ost != 0])
        monkeypatch.delenv(name)
    monkeypatch.setenv("NW_BATCH_SIGNERS_MIN_VOTES", str(int(off[-1])))
    (st, fi), d = _delta(lambda: _call(dig, pk, sigs, off, z16))
    assert d == BS.expected(dig, pk, sigs, off, small["keys"])[2] and np.array_equal(st, ost)


def test_service_requests(small):
    """200 verify_batch requests through the native service: the oracle's verdicts, and the
    jobs behind them count every vote and batch once."""
    from narwhal_amd import service as S
    dig, pk, sigs, off, _ = small["in"]
    ost, _ = small["ref"]
    o = off.astype(np.int64)
    pick = [b for b in range(300) if o[b + 1] > o[b]][:200]
    sub_off = np.zeros(201, np.uint64)
    sub_off[1:] = np.cumsum([o[b + 1] - o[b] for b in pick])
    rows = np.concatenate([np.arange(o[b], o[b + 1]) for b in pick])
    exp = BS.expected(dig[pick], pk[rows], sigs[rows], sub_off, small["keys"])[2]
    _set(small["keys"])
    got = [None] * 200

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
    assert d == exp, (d, exp)


def test_fanout_parts(monkeypatch, small):
    """NW_FANOUT_PARTS=3 under NW_ALL_DEVICES: the registry is set on every device, every part
    takes the path, and the parts' counts add up to the call's."""
    L = _lib.lib()
    assert L.nw_init() > 0
    dig, pk, sigs, off, z16 = small["in"]
    monkeypatch.setenv("NW_FANOUT_PARTS", "3")
    assert L.nw_set_device(-1) == 0    # NW_ALL_DEVICES
    try:
        _check(dig, pk, sigs, off, z16, small["keys"], small["ref"])
        _set(NONE)
    finally:
        assert L.nw_set_device(0) == 0


def test_concurrent_calls_and_updates():
    """Two host threads make 20 calls each of 64 batches of 32 votes while the main thread sets
    and clears the registry ten times: every call's verdicts are the oracle's (a call may run in
    either state). The registry's read lease orders the calls against the updates."""
    rng = np.random.Generator(np.random.PCG64(1260))
    dig, pk, sigs, off, z16 = _corpus_sizes(np.full(64, 32, np.int64), rng, every=4)
    ost, oix = _oracle(dig, pk, sigs, off, z16)
    keys = _keys_of(pk)
    errors = []

    def worker(t):
        try:
            for _ in range(20):
                st, fi = _call(dig, pk, sigs, off, z16)
                assert np.array_equal(st, ost) and np.array_equal(fi[ost != 0], oix[ost != 0])
        except BaseException as x:   # noqa: BLE001 (reported by the main thread)
            errors.append((t, repr(x)))

    before = C.batch_signers_stats()
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for r in range(10):
        _set(keys if r % 2 == 0 else NONE)
    for t in th:
        t.join()
    assert not errors, errors
    # whole calls only: every call that took the path counted all of its votes and batches
    d = tuple(y - x for x, y in zip(before, C.batch_signers_stats()))
    one = BS.expected(dig, pk, sigs, off, keys)[2]
    calls = d[2] // one[2]
    assert 0 <= calls <= 40 and d == tuple(calls * x for x in one)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import test_gpu_batch_signers as T

dig, pk, sigs, off, z16 = T._corpus(60, seed=1270)
ost, oix = T._oracle(dig, pk, sigs, off, z16)
T._set(T._keys_of(pk))
assert T.C.strict_signers_count() == 64
for _ in range(2):
    (st, fi), d = T._delta(lambda: T._call(dig, pk, sigs, off, z16))
    assert np.array_equal(st, ost) and np.array_equal(fi[ost != 0], oix[ost != 0]), (st, ost)
    assert d == (0, 0, 0, 0), d
print("LIMIT_OK")
"""


def test_three_gb_limit():
    """Under the 3 GB allocation limit of test_gpu_memory.py registering 64 keys succeeds, the B
    comb (11.8 GB) cannot be had, so the calls run without the path: the oracle's verdicts, no
    counter moves, and no error is left behind for the second call."""
    env = dict(os.environ, NW_DEVICE_MEM_LIMIT=str(3 * 10**9))
    for k in ("NW_BATCH_SIGNERS", "NW_BATCH_SIGNERS_MIN_VOTES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _CHILD], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "LIMIT_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
