"""verify_batch over per-vote messages of any length (k_strict_hram over the call's votes, then
the batch pipeline over the k plane with k_bv_items_k / k_bv_items_listed_k / k_pip_points_k /
k_batch_signers_k) through nw_verify_batch_msgs_many, nw_submit_verify_batch_msgs,
nw_dev_verify_batch_msgs_many, nw_host_verify_batch_msgs_many and
Signature.verify_batch_messages: every status and failing index against the checker of
tests/batch_msgs_cases.py under injected coefficients, exactly; Straus chunks and slices,
Pippenger batches, a lone large batch, the digest entry's verdicts, the registered signers,
CSPRNG coefficients, the fan-out and two streams."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

import batch_msgs_cases as BM
import batch_signers_cases as BS

pytestmark = pytest.mark.gpu


def _lib_ready():
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _data(c):
    return c.data if c.data.size else np.zeros(1, np.uint8)


def _blocking(c, z=True):
    _lib_ready()
    return C.verify_batch_msgs_many((c.data, c.moffs, c.mlens), c.pks, c.sigs, c.off,
                                    c.z if z else None)


def _submit(c):
    L = _lib_ready()
    st = np.full(max(c.nb, 1), -99, np.int32)
    fi = np.full(max(c.nb, 1), 2**63, np.uint64)
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_batch_msgs(_p(_data(c)), _p(c.moffs), _p(c.mlens), _p(c.pks),
                                       _p(c.sigs), _p(c.off), c.nb, _p(c.z), _p(st), _p(fi),
                                       ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    return st[:c.nb], fi[:c.nb]


def _host(c):
    st = np.full(max(c.nb, 1), -99, np.int32)
    fi = np.full(max(c.nb, 1), 2**63, np.uint64)
    rc = _lib.lib().nw_host_verify_batch_msgs_many(_p(_data(c)), _p(c.moffs), _p(c.mlens),
                                                   _p(c.pks), _p(c.sigs), _p(c.off), c.nb,
                                                   _p(c.z), _p(st), _p(fi))
    assert rc == 0
    return st[:c.nb], fi[:c.nb]


def _prep_dev(L, c, dev):
    """Inputs, workspace and outputs of one device launch, in place before anything is queued."""
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (_data(c), c.moffs.view(np.int64), c.mlens.view(np.int64), c.pks, c.sigs,
                   c.off.view(np.int64), c.z)]
    ws = torch.empty(L.nw_dev_verify_batch_msgs_workspace(c.nb, c.n) + 8, dtype=torch.uint8,
                     device=dev)
    st = torch.full((max(c.nb, 1),), -99, dtype=torch.int32, device=dev)
    fi = torch.full((max(c.nb, 1),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return t, ws, st, fi


def _queue_dev(L, c, run, stream):
    t, ws, st, fi = run
    rc = L.nw_dev_verify_batch_msgs_many(_P(t[0]), _P(t[1]), _P(t[2]), _P(t[3]), _P(t[4]),
                                         _P(t[5]), _p(c.off), c.nb, c.n, _P(t[6]), None, _P(ws),
                                         _P(st), _P(fi), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, L.nw_last_error()


def _read_dev(c, run):
    return run[2].cpu().numpy()[:c.nb], run[3].cpu().numpy()[:c.nb].view(np.uint64)


def _dev(c):
    L = _lib_ready()
    dev = torch.device("cuda", 0)
    run = _prep_dev(L, c, dev)
    _queue_dev(L, c, run, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    return _read_dev(c, run)


def _same(c, got, what=""):
    st, fi = got
    bad = [(c.names[b], int(st[b]), int(fi[b]), int(c.ref_st[b]), int(c.ref_ix[b]))
           for b in range(c.nb) if st[b] != c.ref_st[b] or fi[b] != c.ref_ix[b]]
    assert not bad, (what, len(bad), bad[:8])


@pytest.fixture
def registry():
    """Sets the device's registered signers; always cleared afterwards."""
    L = _lib_ready()

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


def _signer_keys():
    from oracle import oracle as O
    return np.array([np.frombuffer(pk, np.uint8) for pk, _ in O.keys(8)])


# ---- 1. the corpus through every entry ------------------------------------------------------
@pytest.mark.parametrize("entry", [_blocking, _submit, _dev, _host])
def test_corpus_matches_checker(registry, entry):
    c = BM.corpus()
    _same(c, entry(c), entry.__name__)
    e = BM.all_empty()
    _same(e, entry(e), entry.__name__ + " (empty messages)")


@pytest.mark.parametrize("entry", [_blocking, _submit, _dev])
def test_empty_batches_and_single_batches(registry, entry):
    c = BM.corpus()
    lone = c.take([c.names.index("valid_0")])
    _same(lone, entry(lone), "one empty batch")
    mix = c.take([0, c.names.index("valid_5"), 0, 0, c.names.index("s_plus_l_12_at_6"), 0])
    _same(mix, entry(mix), "empty batches among others")
    for name in ("valid_1", "msg_last_flipped_64_at_63", "a_off_curve_2_at_1"):
        one = c.take([c.names.index(name)])
        _same(one, entry(one), name)


def test_no_batches(registry):
    L = _lib_ready()
    assert L.nw_verify_batch_msgs_many(None, None, None, None, None, None, 0, None, None,
                                       None) == 0
    assert L.nw_signature_verify_batch_msgs(None, None, None, None, None, 0, None, None) == 0
    assert L.nw_dev_verify_batch_msgs_many(None, None, None, None, None, None, None, 0, 0, None,
                                           None, None, None, None, None) == 0


def test_verify_batch_messages(registry):
    _lib_ready()
    c = BM.corpus()
    C.Signature.verify_batch_messages([])
    seen = set()
    for name in ("valid_3", "valid_12", "msg_last_flipped_5_at_2", "short_length_3_at_0",
                 "byte_after_5_at_4", "s_plus_l_12_at_11", "s_high_bit_3_at_1",
                 "a_off_curve_5_at_0", "r_off_curve_12_at_6", "s_noncanonical_3_after_r_decode_1"):
        b = c.names.index(name)
        lo, hi = int(c.off[b]), int(c.off[b + 1])
        items = [(m, C.PublicKey(p.tobytes()), C.Signature.from_bytes(s.tobytes()))
                 for m, p, s in zip(c.messages(b), c.pks[lo:hi], c.sigs[lo:hi])]
        z = c.z[lo:hi].tobytes()
        if c.ref_st[b] == 0:
            C.Signature.verify_batch_messages(items, z)
        else:
            with pytest.raises(C.CryptoError) as e:
                C.Signature.verify_batch_messages(iter(items), z)
            assert (e.value.code, e.value.index) == (int(c.ref_st[b]), int(c.ref_ix[b])), name
        seen.add(int(c.ref_st[b]))
    assert seen == {0, 1, 2, 3, 4, 7}


# ---- 2. Straus: chunks, the combine step, slices --------------------------------------------
@pytest.mark.parametrize("entry", [_blocking, _dev])
def test_chunks_of_three(registry, monkeypatch, entry):
    monkeypatch.setenv("NW_BATCH_CHUNK", "3")   # 5, 12 and 64 votes: several chunks, k_bv_combine
    c = BM.corpus()
    _same(c, entry(c), "NW_BATCH_CHUNK=3")


@pytest.mark.parametrize("chunk", [None, "3"])
@pytest.mark.parametrize("entry", [_blocking, _dev])
def test_slices(registry, monkeypatch, entry, chunk):
    """Several slices: a valid batch of distinct messages in a later slice fails unless the plane
    is indexed by the call-global vote index."""
    monkeypatch.setenv("NW_BATCH_SLICE_UNITS", "97")
    if chunk:
        monkeypatch.setenv("NW_BATCH_CHUNK", chunk)
    c = BM.corpus()
    assert c.n + c.nb > 20 * 97
    late = [b for b, nm in enumerate(c.names) if nm.startswith("valid_") and c.off[b] > 97]
    assert late and all(c.ref_st[b] == 0 for b in late)
    _same(c, entry(c), "NW_BATCH_SLICE_UNITS=97")


# ---- 3. Pippenger batches among small ones ----------------------------------------------------
def _pip_call():
    # 3,300 votes: two slices of 2,600 units
    return BM.sized((3, 400, 12, 0, 401, 5, 400, 64, 401, 400, 7, 401, 400, 1, 401), 20273,
                    ((4, 400, "msg_last_flipped"), (6, 399, "s_plus_l"), (2, 7, "short_length"),
                     (14, 400, "msg_last_flipped")))


@pytest.mark.parametrize("slice_units", [None, "2600"])
@pytest.mark.parametrize("entry", [_blocking, _dev])
def test_pippenger_batches(registry, monkeypatch, entry, slice_units):
    monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
    if slice_units:
        monkeypatch.setenv("NW_BATCH_SLICE_UNITS", slice_units)
    c = _pip_call()
    assert c.ref_st.tolist() == [0, 0, 7, 0, 7, 0, 2, 0, 0, 0, 0, 0, 0, 0, 7]
    assert c.n + c.nb > 2600
    _same(c, entry(c), f"Pippenger, slice {slice_units}")


# ---- 4. a lone large batch: the unfused launches ----------------------------------------------
@pytest.mark.parametrize("broken", [(), ((0, 4000, "msg_last_flipped"),)])
def test_lone_large_batch(registry, broken):
    """4,096 votes with distinct messages, alone in the call: the digest entry would take the
    fused head here, which hashes the batch digest itself; this entry must not."""
    c = BM.sized((4096,), 20274, broken)
    assert c.ref_st.tolist() == [7 if broken else 0] and c.ref_ix.tolist() == [4096]
    for entry in (_blocking, _dev):
        _same(c, entry(c), entry.__name__)


# ---- 5. agreement with the digest entry -------------------------------------------------------
def test_golden_batches_equal_the_digest_entry(registry, golden):
    L = _lib_ready()
    c, dig, exp_st, exp_ix = BM.golden_call(golden)
    st32 = np.full(c.nb, -99, np.int32)
    fi32 = np.full(c.nb, 99, np.uint64)
    job = ctypes.c_void_p()
    assert L.nw_submit_verify_batch_many(_p(dig), _p(c.pks), _p(c.sigs), _p(c.off), c.nb, _p(c.z),
                                         _p(st32), _p(fi32), ctypes.byref(job)) == 0
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    assert np.array_equal(st32, C.verify_batch_many(dig, c.pks, c.sigs, c.off, c.z))
    for entry in (_blocking, _submit, _dev, _host):
        st, fi = entry(c)
        _same(c, (st, fi), entry.__name__)
        assert np.array_equal(st, exp_st) and np.array_equal(fi, exp_ix), entry.__name__
        assert np.array_equal(st, st32) and np.array_equal(fi, fi32), entry.__name__
    by = dict(zip(c.names, exp_st.tolist()))
    assert by["torsion_residual_z_cancels"] == 0 and by["torsion_residual_z_exposes"] == 7


# ---- 6. the registered signers -----------------------------------------------------------------
def _all_stats():
    return C.batch_signers_stats() + C.batch_signers_vote_stats()


def test_registered_signers(registry, monkeypatch):
    _lib_ready()
    c = BM.corpus()
    keys = _signer_keys()
    for part, what in ((keys, "8 registered"), (keys[::2], "4 registered")):
        registry(part)
        before = _all_stats()
        for entry in (_blocking, _submit):
            _same(c, entry(c), f"{what}, {entry.__name__}")
        d = [y - x for x, y in zip(before, _all_stats())]
        # votes passed, batches settled, batches sent on, votes left out of their sums
        assert d[0] > 0 and d[2] > 0 and d[3] > 0 and d[4] > 0, (what, d)
        assert d[0] + d[1] == 2 * c.n and d[2] + d[3] == 2 * c.nb, (what, d)
    registry(keys)
    for name in ("NW_BATCH_SIGNERS", "NW_BATCH_SIGNERS_VOTES"):
        with monkeypatch.context() as m:
            m.setenv(name, "0")
            before = _all_stats()
            _same(c, _blocking(c), f"{name}=0")
            d = [y - x for x, y in zip(before, _all_stats())]
            if name == "NW_BATCH_SIGNERS":
                assert d == [0] * 6, d
            else:
                assert d[0] > 0 and d[4] == 0 and d[5] > 0, d


@pytest.mark.parametrize("hooks", [(), (("NW_BATCH_CHUNK", "3"), ("NW_BATCH_SLICE_UNITS", "97"))])
def test_registered_signers_chunks_and_pippenger(registry, monkeypatch, hooks):
    for k, v in hooks:
        monkeypatch.setenv(k, v)
    registry(_signer_keys()[:6])   # two signers unknown: their batches are sent on
    c = BM.corpus()
    _same(c, _blocking(c), f"6 registered, {hooks}")
    if not hooks:
        monkeypatch.setenv("NW_BATCH_PIPPENGER_MIN", "400")
        p = _pip_call()
        before = _all_stats()
        _same(p, _blocking(p), "Pippenger under the registry")
        d = [y - x for x, y in zip(before, _all_stats())]
        assert d[0] > 0 and d[3] > 0 and d[4] > 0, d


def test_mixed_order_signer_is_never_settled(registry):
    """A strict-valid vote under a registered mixed-order key: its batch's verdict depends on z,
    so the comb phase must send the batch on, and the verdict is the checker's for the z used."""
    _lib_ready()
    dig, pk, sigs, off, keys, zs = BS.mixed_batches(43)
    registry(keys)
    seen = set()
    for z in zs[:4]:
        c = BM.digest_call(dig, pk, sigs, off, z)
        before = _all_stats()
        _same(c, _blocking(c), "mixed-order signer")
        d = [y - x for x, y in zip(before, _all_stats())]
        assert d[2] == 0 and d[3] == c.nb, d   # no batch settled, every batch sent on
        seen |= set(c.ref_st.tolist())
    assert seen == {0, 7}


# ---- 7. CSPRNG coefficients --------------------------------------------------------------------
@pytest.mark.parametrize("entry", [_blocking, _dev])
def test_random_coefficients(registry, entry):
    """z16 = NULL on the deterministic subset: all-valid batches are Ok, a prime-order residual
    (a flipped message byte) is 7, whatever the coefficients."""
    L = _lib_ready()
    c = BM.corpus()
    c = c.take([b for b, nm in enumerate(c.names)
                if nm.startswith("valid_") or nm.startswith("msg_last_flipped_")])
    assert set(c.ref_st.tolist()) == {0, 7}
    if entry is _blocking:
        st, fi = _blocking(c, z=False)
    else:
        dev = torch.device("cuda", 0)
        t, ws, st_d, fi_d = _prep_dev(L, c, dev)
        rc = L.nw_dev_verify_batch_msgs_many(_P(t[0]), _P(t[1]), _P(t[2]), _P(t[3]), _P(t[4]),
                                             _P(t[5]), None, c.nb, c.n, None, None, _P(ws),
                                             _P(st_d), _P(fi_d), None)
        assert rc == 0, L.nw_last_error()
        assert L.nw_synchronize() == 0, L.nw_last_error()
        torch.cuda.synchronize()
        st, fi = _read_dev(c, (t, ws, st_d, fi_d))
    _same(c, (st, fi), "random z")


# ---- 8. fan-out ----------------------------------------------------------------------------------
def test_fanout_three_parts(registry, monkeypatch):
    L = _lib_ready()
    c = BM.corpus()
    monkeypatch.setenv("NW_FANOUT_PARTS", "3")
    assert L.nw_set_device(-1) == 0   # NW_ALL_DEVICES
    try:
        got = C.verify_batch_msgs_many((c.data, c.moffs, c.mlens), c.pks, c.sigs, c.off, c.z)
        sub = _submit_all_devices(L, c)
    finally:
        assert L.nw_set_device(0) == 0
    _same(c, got, "fan-out")
    _same(c, sub, "fan-out (submit)")


def _submit_all_devices(L, c):
    st = np.full(c.nb, -99, np.int32)
    fi = np.full(c.nb, 2**63, np.uint64)
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_batch_msgs(_p(c.data), _p(c.moffs), _p(c.mlens), _p(c.pks),
                                       _p(c.sigs), _p(c.off), c.nb, _p(c.z), _p(st), _p(fi),
                                       ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    return st, fi


# ---- 9. two streams: each call has a plane of its own -------------------------------------------
def test_two_streams(registry):
    L = _lib_ready()
    dev = torch.device("cuda", 0)
    c = BM.corpus()
    half = c.nb // 2
    halves = [c.take(range(half - 1, -1, -1)), c.take(range(c.nb - 1, half - 1, -1))]
    streams = [torch.cuda.Stream(device=dev) for _ in halves]
    runs = [_prep_dev(L, h, dev) for h in halves]
    for h, run, s in zip(halves, runs, streams):
        _queue_dev(L, h, run, s)
    torch.cuda.synchronize()
    for h, run in zip(halves, runs):
        _same(h, _read_dev(h, run), "two streams")
