"""Signing over messages of any length (k_sign_msgs) through nw_sign_msgs_many,
nw_dev_sign_msgs_many, sign_msgs_many and Signature.new_message: every signature against the
oracle's (RFC 8032 signing is deterministic, so byte for byte) over the corpus of
tests/sign_msgs_cases.py, the literal RFC 8032 vectors over their raw messages, the launch
shapes, the 32-byte entry's output, a shared key, and the round trip through the verifiers over
messages."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from narwhal_amd import crypto as C
from oracle import oracle as O

import sign_msgs_cases as SG

pytestmark = pytest.mark.gpu


def _lib_ready():
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    return L


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def shuffled():
    """The corpus in a shuffled order, so that every wave holds many lengths: (corpus, order)."""
    c = SG.corpus()
    order = np.random.Generator(np.random.PCG64(7)).permutation(c.n)
    assert len({int(l) for l in c.lengths[order[:64]]}) >= 20
    return c, order


def _host_entry(c, order):
    L = _lib_ready()
    sks, offs, lens = (np.ascontiguousarray(a[order]) for a in (c.sks, c.offsets, c.lengths))
    out = np.zeros((len(order), 64), np.uint8)
    rc = L.nw_sign_msgs_many(_p(sks), 64, _p(c.data), _p(offs), _p(lens), len(order), _p(out))
    assert rc == 0, L.nw_last_error()
    return out


def _dev_entry(c, order):
    L = _lib_ready()
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (c.sks[order], c.data, c.offsets[order].view(np.int64),
                   c.lengths[order].view(np.int64))]
    out = torch.zeros((len(order), 64), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    rc = L.nw_dev_sign_msgs_many(_P(t[0]), 64, _P(t[1]), _P(t[2]), _P(t[3]), len(order), _P(out),
                                 ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, L.nw_last_error()
    stream.synchronize()
    return out.cpu().numpy()


# ---- 1. the corpus through both entries ---------------------------------------------------
@pytest.mark.parametrize("entry", [_host_entry, _dev_entry])
def test_corpus_equals_oracle(shuffled, entry):
    c, order = shuffled
    got = entry(c, order)
    bad = np.nonzero((got != c.sigs[order]).any(axis=1))[0]
    assert bad.size == 0, (entry.__name__, len(bad),
                           [(int(order[i]), int(c.lengths[order[i]]), int(c.aligns[order[i]]))
                            for i in bad[:8]])


# ---- 2. RFC 8032 section 7.1 over the raw messages ----------------------------------------
def test_rfc8032_vectors_literally(golden):
    vec = golden["keys"]["rfc8032"]
    sks = np.array([np.frombuffer(bytes.fromhex(v["seed"] + v["pk"]), np.uint8) for v in vec])
    msgs = [bytes.fromhex(v["msg"]) for v in vec]
    assert [len(m) for m in msgs] == [0, 1, 2]
    sigs = C.sign_msgs_many(sks, msgs)
    assert [s.tobytes().hex() for s in sigs] == [v["sig"] for v in vec]
    for v, m, sk in zip(vec, msgs, sks):
        assert C.Signature.new_message(m, C.SecretKey(sk.tobytes())).flatten().hex() == v["sig"]


# ---- 3. launch shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257])
def test_launch_shapes(n):
    L = _lib_ready()
    c = SG.corpus()
    idx = (np.arange(n) * 13) % c.n
    sks, offs, lens = (np.ascontiguousarray(a[idx]) for a in (c.sks, c.offsets, c.lengths))
    out = np.full((n + 2, 64), 0xCD, np.uint8)
    rc = L.nw_sign_msgs_many(_p(sks), 64, _p(c.data), _p(offs), _p(lens), n, _p(out))
    assert rc == 0, L.nw_last_error()
    assert (out[n:] == 0xCD).all()
    assert np.array_equal(out[:n], c.sigs[idx])
    if n == 0:
        assert L.nw_sign_msgs_many(None, 64, None, None, None, 0, None) == 0
        assert L.nw_dev_sign_msgs_many(None, 64, None, None, None, 0, None, None) == 0


def test_argument_checks():
    L = _lib_ready()
    c = SG.corpus()
    out = np.zeros((1, 64), np.uint8)
    args = lambda **k: [k.get("sks", _p(c.sks)), k.get("stride", 64), _p(c.data),
                        k.get("offs", _p(c.offsets)), k.get("lens", _p(c.lengths)), 1, _p(out)]
    for bad in (dict(stride=32), dict(sks=None), dict(offs=None), dict(lens=None)):
        assert L.nw_sign_msgs_many(*args(**bad)) == -1, bad   # NW_E_INVALID_ARG
        assert L.nw_dev_sign_msgs_many(*args(**bad), None) == -1, bad
    assert L.nw_set_device(-1) == 0   # NW_ALL_DEVICES
    try:
        assert L.nw_sign_msgs_many(*args()) == -1
    finally:
        assert L.nw_set_device(0) == 0
    # data may be null when every message is empty
    empty = np.nonzero(c.lengths == 0)[0][:4]
    sks, offs, lens = (np.ascontiguousarray(a[empty]) for a in (c.sks, c.offsets, c.lengths))
    out = np.zeros((4, 64), np.uint8)
    assert L.nw_sign_msgs_many(_p(sks), 64, None, _p(offs), _p(lens), 4, _p(out)) == 0
    assert np.array_equal(out, c.sigs[empty])


# ---- 4. 32-byte messages: the 32-byte entry's output --------------------------------------
def test_32_byte_messages_equal_sign_many():
    rng = np.random.Generator(np.random.PCG64(18))
    seeds = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    sks = np.concatenate([seeds, C.keypair_from_seed_many(seeds)], axis=1)
    msgs = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    a = C.sign_many(sks, msgs)
    b = C.sign_msgs_many(sks, (msgs.reshape(-1), 32 * np.arange(300), np.full(300, 32)))
    assert np.array_equal(a, b)
    assert a[7].tobytes() == O.sign(sks[7].tobytes(), msgs[7].tobytes())


# ---- 5. one key for every message ---------------------------------------------------------
def test_shared_key():
    c = SG.corpus()
    idx = (np.arange(64) * 11) % c.n
    assert len({int(l) for l in c.lengths[idx]}) >= 20
    msgs = (c.data, c.offsets[idx], c.lengths[idx])
    sk = c.sks[3]
    one = C.sign_msgs_many(sk, msgs, shared_key=True)
    rep = C.sign_msgs_many(np.tile(sk, (64, 1)), msgs)
    assert np.array_equal(one, rep)
    assert one[5].tobytes() == O.sign(sk.tobytes(), c.messages()[idx[5]])


# ---- 6. round trip through the verifiers over messages ------------------------------------
def test_round_trip(shuffled):
    c, order = shuffled
    sigs = np.zeros((c.n, 64), np.uint8)
    sigs[order] = _dev_entry(c, order)
    st, _ = C.verify_strict_msgs_many((c.data, c.offsets, c.lengths), c.pks, sigs)
    exp = np.zeros(c.n, np.int32)
    exp[c.foreign] = 7
    assert np.array_equal(st, exp), np.nonzero(st != exp)[0][:8]
    msgs = c.messages()
    C.Signature.verify_batch_messages(
        (msgs[i], C.PublicKey(c.pks[i].tobytes()), C.Signature.from_bytes(sigs[i].tobytes()))
        for i in range(c.n) if i != c.foreign)
    kps = O.keys(2)
    m = b"a transaction, not a digest" * 9
    s = C.Signature.new_message(m, C.SecretKey(kps[0][1]))
    s.verify_message(m, C.PublicKey(kps[0][0]))
    with pytest.raises(C.CryptoError):
        s.verify_message(m, C.PublicKey(kps[1][0]))
