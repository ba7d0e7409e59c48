"""Strict verification over messages of any length (k_strict_hram, then the unkeyed two-pass
launch over the k plane with k_strict_triage_k / k_strict_keyed_hot_k / k_strict_keyed_signers_k)
through nw_verify_strict_msgs_many, nw_submit_verify_strict_msgs, nw_dev_verify_strict_msgs_many
and Signature.verify_message: every status and the bitmap against the oracle's verify_strict over
the message's own bytes, exactly, over the corpus of tests/strict_msgs_cases.py; with the call's
comb check, the registered signers, slices, the knobs that turn paths off, the fan-out and two
streams."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C

import strict_msgs_cases as SM

pytestmark = pytest.mark.gpu

MIN = 64   # NW_STRICT_COMB_MIN, as tests/test_gpu_strict_comb.py lowers it


def _lib_ready():
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    return L


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _to_dev(c, dev):
    """The corpus' arrays as device tensors (the 64-bit arrays through their int64 view)."""
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            for a in (c.data, c.offsets.view(np.int64), c.lengths.view(np.int64), c.pks, c.sigs)]


def _prep_dev(c, dev):
    """Inputs and outputs of one device launch, in place before anything is queued."""
    t = _to_dev(c, dev)
    st = torch.full((max(c.n, 1),), -99, dtype=torch.int32, device=dev)
    bm = torch.zeros((c.n + 63) // 64 * 8 + 8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return t, st, bm


def _queue_dev(L, c, run, stream):
    t, st, bm = run
    rc = L.nw_dev_verify_strict_msgs_many(_P(t[0]), _P(t[1]), _P(t[2]), _P(t[3]), _P(t[4]), c.n,
                                          _P(st), _P(bm), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, L.nw_last_error()


def _read_dev(c, st, bm):
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[c.n:(c.n + 63) // 64 * 64].any()
    return st.cpu().numpy()[:c.n], bits[:c.n].astype(bool)


def _dev(c):
    L = _lib_ready()
    dev = torch.device("cuda", 0)
    run = _prep_dev(c, dev)
    _queue_dev(L, c, run, torch.cuda.current_stream(dev))
    assert L.nw_synchronize() == 0, L.nw_last_error()   # stream 0 names the library's own
    torch.cuda.synchronize()
    return _read_dev(c, run[1], run[2])


def _host(c):
    st, bm = C.verify_strict_msgs_many((c.data, c.offsets, c.lengths), c.pks, c.sigs)
    return st, np.unpackbits(bm, bitorder="little")[:c.n].astype(bool)


def _submit(c):
    L = _lib_ready()
    st = np.full(max(c.n, 1), -99, np.int32)
    bm = np.zeros((c.n + 7) // 8 + 1, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    job = ctypes.c_void_p()
    rc = L.nw_submit_verify_strict_msgs(p(c.data), p(c.offsets), p(c.lengths), p(c.pks), p(c.sigs),
                                        c.n, p(st), p(bm), ctypes.byref(job))
    assert rc == 0, L.nw_last_error()
    assert L.nw_job_wait(job) == 0, L.nw_last_error()
    L.nw_job_release(job)
    return st[:c.n], np.unpackbits(bm, bitorder="little")[:c.n].astype(bool)


def _same(c, got, what=""):
    st, bits = got
    bad = np.nonzero(st != c.ref)[0]
    assert bad.size == 0, (what, [(int(i), c.variant[i], int(c.lengths[i]), int(c.offsets[i]) % 4,
                                   int(st[i]), int(c.ref[i])) for i in bad[:8]])
    assert np.array_equal(bits, c.ref == 0), what


def _stats(L, name, k):
    out = (ctypes.c_uint64 * k)()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert getattr(L, name)(out, stream) == 0, L.nw_last_error()
    return [int(x) for x in out]


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


def _signer_keys(c):
    keys = []
    for p, v in zip(c.pks, c.variant):
        if v != "a_off_curve" and p.tobytes() not in keys:
            keys.append(p.tobytes())
    assert len(keys) == 8
    return np.frombuffer(b"".join(keys), np.uint8).reshape(8, 32)


# ---- 3. the corpus through every entry -------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, None])
@pytest.mark.parametrize("entry", [_host, _submit, _dev])
def test_corpus_matches_oracle(registry, entry, n):
    c = SM.corpus()
    if n is not None:
        # a spread of lengths, alignments and variants, not the corpus' first rows
        c = c.take((np.arange(n) * 17) % c.n)
    _same(c, entry(c), entry.__name__)


@pytest.mark.parametrize("entry", [_host, _submit, _dev])
def test_all_messages_empty(registry, entry):
    c = SM.corpus()
    c = c.take(np.nonzero(c.lengths == 0)[0])
    assert c.n >= 24 and set(c.ref.tolist()) >= {0, 1, 2, 3, 6, 7}
    _same(c, entry(c), entry.__name__)


def test_list_of_bytes_and_verify_message(registry):
    c = SM.corpus()
    c = c.take((np.arange(40) * 29) % c.n)
    st, bm = C.verify_strict_msgs_many(c.messages(), c.pks, c.sigs)
    _same(c, (st, np.unpackbits(bm, bitorder="little")[:c.n].astype(bool)))
    seen = set()
    for msg, pk, sig, ref in zip(c.messages()[:12], c.pks, c.sigs, c.ref):
        s = C.Signature.from_bytes(sig.tobytes())
        if ref == 0:
            s.verify_message(msg, C.PublicKey(pk.tobytes()))
        else:
            with pytest.raises(C.CryptoError) as e:
                s.verify_message(msg, C.PublicKey(pk.tobytes()))
            assert e.value.code == ref
        seen.add(int(ref))
    assert 0 in seen and len(seen) >= 3


# ---- 4. 32-byte messages: the golden statuses, and the 32-byte entry's -------------------
def test_golden_edge_corpus_equals_the_32_byte_entry(registry, golden):
    msgs, pks, sigs, exp = SM.golden_edge(golden)
    n = len(exp)
    c = SM.Corpus(np.ascontiguousarray(msgs).reshape(-1), (32 * np.arange(n)).astype(np.uint64),
                  np.full(n, 32, np.uint64), pks, sigs, exp, ["edge"] * n)
    st32, bm32 = C.verify_strict_many(msgs, pks, sigs)
    for entry in (_dev, _host):
        st, bits = entry(c)
        _same(c, (st, bits), entry.__name__)
        assert np.array_equal(st, st32)
        assert np.array_equal(bits, np.unpackbits(bm32, bitorder="little")[:n].astype(bool))


# ---- 5. / 6. the call's comb check and the registered signers ---------------------------
def test_comb_and_registered_signers(registry, monkeypatch):
    L = _lib_ready()
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
    monkeypatch.setenv("NW_STRICT_SIGNERS_MIN_ITEMS", "1")
    c = SM.tiled()
    st5, bits5 = _dev(c)
    comb = _stats(L, "nw_dev_strict_comb_stats", 4)
    decided = _stats(L, "nw_dev_strict_decided_stats", 2)
    keyset = _stats(L, "nw_dev_strict_keyset_stats", 3)
    _same(c, (st5, bits5), "call-local comb")
    assert comb[0] > 0 and comb[2] > 0 and comb[2] + comb[3] == c.n, comb
    assert decided[0] > 0, decided   # the flipped-message items: the comb's sum decided them
    assert keyset[0] > 0 and keyset[1] + keyset[2] == c.n, keyset
    assert _stats(L, "nw_dev_strict_signers_stats", 3) == [0, 0, 0]
    keys = _signer_keys(c)
    for part, what in ((keys, "8 registered"), (keys[::2], "4 registered")):
        registry(part)
        st6, bits6 = _dev(c)
        sg = _stats(L, "nw_dev_strict_signers_stats", 3)
        assert np.array_equal(st6, st5) and np.array_equal(bits6, bits5), what
        assert sg[0] > 0 and sg[1] > 0 and sg[2] > 0, (what, sg)
    registry(keys)
    _same(c, _host(c), "job under the registry")


# ---- 7. / 8. slices and the knobs --------------------------------------------------------
@pytest.mark.parametrize("knob,value", [("NW_TRIAGE_SLICE", "1024"), ("NW_TRIAGE_SLICE", "1500"),
                                        ("NW_STRICT_KEYS", "0"), ("NW_STRICT_COMB", "0")])
def test_slices_and_knobs(registry, monkeypatch, knob, value):
    L = _lib_ready()
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
    monkeypatch.setenv(knob, value)
    c = SM.tiled()
    _same(c, _dev(c), f"{knob}={value}")
    comb = _stats(L, "nw_dev_strict_comb_stats", 4)
    if knob == "NW_TRIAGE_SLICE":
        assert comb[0] > 0 and comb[2] > 0, comb
    else:
        assert comb == [0, 0, 0, c.n], comb


# ---- 9. fan-out --------------------------------------------------------------------------
def test_fanout_three_parts(registry, monkeypatch):
    L = _lib_ready()
    c = SM.corpus()
    monkeypatch.setenv("NW_FANOUT_PARTS", "3")
    assert L.nw_set_device(-1) == 0   # NW_ALL_DEVICES
    try:
        got = _host(c)   # the thread's device stays NW_ALL_DEVICES
    finally:
        assert L.nw_set_device(0) == 0
    _same(c, got, "fan-out")


# ---- 10. two streams: the lease orders the shared k plane --------------------------------
def test_two_streams(registry):
    L = _lib_ready()
    dev = torch.device("cuda", 0)
    full = SM.tiled()
    halves = [full.take(np.arange(0, 2048)), full.take(np.arange(4095, 2047, -1))]
    streams = [torch.cuda.Stream(device=dev) for _ in halves]
    runs = [_prep_dev(c, dev) for c in halves]
    for c, run, s in zip(halves, runs, streams):
        _queue_dev(L, c, run, s)
    torch.cuda.synchronize()
    for c, (_, st, bm) in zip(halves, runs):
        _same(c, _read_dev(c, st, bm), "two streams")
