"""The call's key set of config 4's two-pass path (k_strict_keys_probe, k_strict_keys_build,
then k_strict_triage on the slots' flags and k_verify_strict_pre on the slots' tables) through
nw_dev_verify_strict_many: statuses and bitmap against the oracle for one key, a few keys, a
key per item, keys that do not decode / have small order / are non-canonical shared by more
than a wave of items, a table too small for the keys (mixed waves), the set off, several
slices, and a second round of the persistent ladder kernel."""
import ctypes

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from oracle import oracle as O

from test_hostcheck_keyset import keyset_hash

pytestmark = pytest.mark.gpu

P_FIELD = 2**255 - 19
RESIDENT_LANES = 3 * 256 * 256   # of the persistent ladder kernel (test_gpu_strict_ladder.py)


def _launch(msgs, pks, sigs):
    """Statuses, verdict bits and key-set statistics of one nw_dev_verify_strict_many launch."""
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
    stats = (ctypes.c_uint64 * 3)()
    assert L.nw_dev_strict_keyset_stats(stats, stream) == 0, L.nw_last_error()
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()
    return st.cpu().numpy(), bits[:n].astype(bool), [int(x) for x in stats]


def _check(msgs, pks, sigs, exp):
    st, bits, stats = _launch(msgs, pks, sigs)
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]])
    assert np.array_equal(bits, exp == 0)
    assert stats[1] + stats[2] == len(msgs)
    return stats


def _signed(rng, n, kps, tamper=True):
    """n items signed round-robin by kps; with tamper every second one has one bit of s, of
    R, of the key or of the message flipped."""
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.zeros((n, 32), np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        pk, sk = kps[i % len(kps)]
        pks[i] = np.frombuffer(pk, np.uint8)
        sigs[i] = np.frombuffer(O.sign(sk, msgs[i].tobytes()), np.uint8)
    for i in range(1, n, 2) if tamper else ():
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
    return msgs, pks, sigs


def _with_oracle(m, p, s):
    return m, p, s, O.verify_strict_many(m, p, s).astype(np.int32)


@pytest.fixture(scope="module")
def corpus(golden):
    """Every set the tests use, with the oracle's statuses, computed once."""
    rng = np.random.Generator(np.random.PCG64(8192))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(300)]
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    edge = (hexs("msg", 32), hexs("pk", 32), hexs("sig", 64),
            np.array([i["status"] for i in items], np.int32))
    out = {"edge": edge,
           "k64": _with_oracle(*_signed(rng, 4096, kps[:64])),
           "k1": _with_oracle(*_signed(rng, 257, kps[:1])),
           "k3": _with_oracle(*_signed(rng, 257, kps[:3])),
           "k300": _with_oracle(*_signed(rng, 300, kps))}
    assert (out["k64"][3] == 0).sum() == 2048
    # 64 keys of which 9 start at one slot of a 64-slot table: a chain holds 8, so at least
    # one key has no slot whatever the order of the inserts (and the first insert always wins)
    pool = [O.keypair_from_seed(rng.bytes(32)) for _ in range(1500)]
    start = keyset_hash(np.array([np.frombuffer(pk, np.uint8) for pk, _ in pool])) & 63
    slot = int(np.bincount(start, minlength=64).argmax())
    same = [kp for kp, s in zip(pool, start) if s == slot][:9]
    assert len(same) == 9
    out["k64_tight"] = _with_oracle(*_signed(rng, 4096, same + kps[:55]))
    # keys that do not decode, have small order, or are a non-canonical encoding (y >= p) of
    # a large-order point, each under 65+ honestly made signatures of another key
    enc = lambda y, sign: np.frombuffer((y | (sign << 255)).to_bytes(32, "little"), np.uint8)
    special = [enc(2, 0), enc(1, 0), enc(P_FIELD + 3, 0), enc(P_FIELD - 1, 0), enc(7, 1)]
    m, p, s = _signed(rng, 5 * 70, kps[:5], tamper=False)
    for i in range(len(m)):
        p[i] = special[i % 5]
    out["special"] = _with_oracle(m, p, s)
    assert {3, 5} <= set(out["special"][3].tolist())
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_sizes(corpus, n):
    """n items drawn (seeded) from the edge corpus followed by the 64-key set."""
    pool = [np.concatenate([e, r]) for e, r in zip(corpus["edge"], corpus["k64"])]
    ne = len(corpus["edge"][0])
    rng = np.random.Generator(np.random.PCG64(n))
    idx = np.concatenate([rng.permutation(ne), ne + rng.permutation(4096)])[:n]
    if n == 1:
        idx = np.array([ne])   # one honest signature
    m, p, s, e = (a[idx] for a in pool)
    stats = _check(m, p, s, e)
    assert stats[0] == len({x.tobytes() for x in p}) and stats[2] == 0


@pytest.mark.parametrize("name,keys", [("k1", 1), ("k3", 3), ("k64", 64), ("k300", 300)])
def test_key_counts(corpus, name, keys):
    """One key for every item, 3 keys, 64 keys over 4,096 items, 300 items of 300 keys."""
    m, p, s, e = corpus[name]
    stats = _check(m, p, s, e)
    distinct = len({x.tobytes() for x in p})   # the signers and the bit-flipped keys
    assert distinct >= keys
    if keys == 300:
        # 338 keys in 2,048 slots: a key may find its 8-slot chain taken; its items then
        # run their own path
        assert stats[0] <= distinct <= stats[0] + stats[2] and stats[1] >= len(m) - 16
    else:
        assert stats == [distinct, len(m), 0]


def test_flag_only_keys(corpus):
    """Undecodable, small-order and non-canonical keys, each shared by 70 items: more than a
    wave takes its verdict from the slot's flags."""
    m, p, s, e = corpus["special"]
    stats = _check(m, p, s, e)
    assert stats == [5, len(m), 0]


def test_table_too_small(corpus, monkeypatch):
    """NW_STRICT_KEYS=64: a 64-slot table for 64 signers (plus their bit-flipped keys), of
    which 9 start at one slot: some items read a shared table and some run their own path,
    in the same waves (the keys alternate item by item)."""
    monkeypatch.setenv("NW_STRICT_KEYS", "64")
    m, p, s, e = corpus["k64_tight"]
    stats = _check(m, p, s, e)
    assert stats[1] > 0 and stats[2] > 0
    assert 1 <= stats[0] <= 64


def test_key_set_off(corpus, monkeypatch):
    """NW_STRICT_KEYS=0: the launch sequence without the key set; the default's statuses."""
    m, p, s, e = corpus["k64"]
    st_on, bits_on, _ = _launch(m, p, s)
    monkeypatch.setenv("NW_STRICT_KEYS", "0")
    st_off, bits_off, stats = _launch(m, p, s)
    assert np.array_equal(st_on, e) and np.array_equal(st_off, st_on)
    assert np.array_equal(bits_on, bits_off)
    assert stats == [0, 0, len(m)]


def test_three_slices_ragged(corpus, monkeypatch):
    """NW_TRIAGE_SLICE=1500: three slices (1,366, 1,366 and 1,364 items), the key set cleared
    and rebuilt for each: every slice tabulates the keys it holds."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "1500")
    m, p, s, e = corpus["k64"]
    stats = _check(m, p, s, e)
    per_slice = [len({x.tobytes() for x in p[a:b]}) for a, b in ((0, 1366), (1366, 2732), (2732, 4096))]
    assert stats == [sum(per_slice), len(m), 0]


def test_two_rounds(corpus):
    """2 x 196,608 + 65 items (the 64-key set tiled): the survivors outnumber the ladder
    kernel's resident lanes, so a lane of its persistent loop reads another key's shared
    table in its second round."""
    n = 2 * RESIDENT_LANES + 65
    m, p, s, e = (np.resize(a, (n,) + a.shape[1:]) for a in corpus["k64"])
    assert int(np.isin(e, [0, 7]).sum()) > RESIDENT_LANES
    stats = _check(m, p, s, e)
    assert stats[2] == 0
