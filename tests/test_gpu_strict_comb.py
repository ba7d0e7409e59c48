"""The comb check of a call's hot keys (k_strict_comb_select, k_key_base / k_key_tabs at width
8, k_strict_keyed / k_strict_keyed_inv / k_strict_keyed_list, then k_strict_triage over the
to-do list and k_verify_strict_pre) through nw_dev_verify_strict_many: every status and the
bitmap against the oracle and against NW_STRICT_COMB=0, with NW_STRICT_COMB_MIN=64 so that
small inputs turn hot, and with nw_dev_strict_comb_stats showing that the path was taken."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from narwhal_amd import _lib
from oracle import oracle as O

import irregular as IR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELD = 2**255 - 19
L_ORDER = IR.L_ORDER
MIN = 64
RESIDENT_LANES = 3 * 256 * 256   # of the persistent ladder kernel (test_gpu_strict_ladder.py)


def _launch(msgs, pks, sigs):
    """Statuses, verdict bits and comb statistics (hot keys, items checked, items passed,
    items sent on) of one nw_dev_verify_strict_many launch."""
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
    assert L.nw_dev_strict_comb_stats(stats, stream) == 0, L.nw_last_error()
    torch.cuda.synchronize()
    bits = np.unpackbits(bm.cpu().numpy(), bitorder="little")
    assert not bits[n:].any()
    return st.cpu().numpy(), bits[:n].astype(bool), [int(x) for x in stats]


def _check(monkeypatch, msgs, pks, sigs, exp, min_uses=MIN):
    """The launch with the path on (statuses, bitmap == the oracle's) and off (the same)."""
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(min_uses))
    monkeypatch.delenv("NW_STRICT_COMB", raising=False)
    st, bits, stats = _launch(msgs, pks, sigs)
    bad = np.nonzero(st != exp)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], exp[bad[:8]], stats)
    assert np.array_equal(bits, exp == 0)
    assert stats[2] + stats[3] == len(msgs) and stats[2] <= stats[1]
    monkeypatch.setenv("NW_STRICT_COMB", "0")
    st0, bits0, stats0 = _launch(msgs, pks, sigs)
    monkeypatch.delenv("NW_STRICT_COMB")
    assert np.array_equal(st0, st) and np.array_equal(bits0, bits)
    assert stats0 == [0, 0, 0, len(msgs)]
    return stats


def _sign_rows(rng, kps, key_of):
    n = len(key_of)
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pks = np.zeros((n, 32), np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i, k in enumerate(key_of):
        pk, sk = kps[k]
        pks[i] = np.frombuffer(pk, np.uint8)
        sigs[i] = np.frombuffer(O.sign(sk, msgs[i].tobytes()), np.uint8)
    return msgs, pks, sigs


def _signed(rng, n, kps, tamper=True):
    """n items signed round-robin by kps; with tamper every second one has one bit of s, of
    R, of the key or of the message flipped (as test_gpu_strict_keys._signed)."""
    msgs, pks, sigs = _sign_rows(rng, kps, [i % len(kps) for i in range(n)])
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


def _oracle(m, p, s):
    return m, p, s, O.verify_strict_many(m, p, s).astype(np.int32)


def _sampled(n):
    """Rows of an n-item slice whose key use is counted (nw_strict.hpp comb_sampled): one in
    16 by a multiplicative hash of the row, each counting for 16."""
    j = np.arange(n, dtype=np.uint64)
    return ((j * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28) == 0


def _hot_keys(pks, min_uses=MIN):
    """The keys the launch must tabulate for a slice of these rows: 16 x its sampled rows >=
    min_uses, decodable, not of small order (room for all of them)."""
    keys, counts = np.unique(pks[_sampled(len(pks))], axis=0, return_counts=True)
    return {k.tobytes() for k, c in zip(keys, counts)
            if 16 * c >= min_uses and O.decompress(k.tobytes()) is not None
            and not O.is_small_order(k.tobytes())}


def _under(pks, hot):
    return np.array([x.tobytes() in hot for x in pks])


def _enc(y, sign):
    return np.frombuffer((y | (sign << 255)).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def corpus(golden):
    rng = np.random.Generator(np.random.PCG64(9009))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(64)]
    out = {"kps": kps}
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    out["edge"] = (hexs("msg", 32), hexs("pk", 32), hexs("sig", 64),
                   np.array([i["status"] for i in items], np.int32))
    out["k8"] = _oracle(*_signed(rng, 4096, kps[:8]))
    assert (out["k8"][3] == 0).sum() == 2048
    out["k64"] = _oracle(*_signed(rng, 4096, kps))
    return out


def test_edge_under_hot_keys(corpus, monkeypatch):
    """The golden edge corpus behind 2 hot keys of 200 honest signatures each, and under those
    keys: R with x = 0 and the sign bit, R's y >= p, small-order R, undecodable R, s + l,
    s with high bits, a flipped message. The comb passes exactly the valid items of hot keys."""
    rng = np.random.Generator(np.random.PCG64(1))
    kps = corpus["kps"][:2]
    m, p, s = _sign_rows(rng, kps, [i % 2 for i in range(400)])
    cm, cp, cs = _sign_rows(rng, kps, [i % 2 for i in range(48)])
    small = IR.small_order_encodings()
    for i in range(48):
        c = i % 8
        if c == 0:     # x = 0 with the sign bit (the identity, y = 1) / y = -1 with it
            cs[i, :32] = _enc([1, P_FIELD - 1][(i // 8) % 2], 1)
        elif c == 1:   # y >= p
            cs[i, :32] = _enc(P_FIELD + [0, 1, 3, 4, 18, 5][i // 8], (i // 8) & 1)
        elif c == 2:   # small-order R
            cs[i, :32] = np.frombuffer(small[(i // 8) % len(small)], np.uint8)
        elif c == 3:   # R not on the curve
            cs[i, :32] = _enc([2, 7, 8][(i // 8) % 3], (i // 8) & 1)
        elif c == 4:   # s + l
            v = int.from_bytes(cs[i, 32:].tobytes(), "little") + L_ORDER
            cs[i, 32:] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        elif c == 5:   # s with high bits
            cs[i, 63] |= np.uint8(0x80 >> ((i // 8) % 3))
        elif c == 6:   # wrong message
            cm[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        # c == 7: honest
    em, ep, es, ee = corpus["edge"]
    m, p, s = np.concatenate([em, m, cm]), np.concatenate([ep, p, cp]), np.concatenate([es, s, cs])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.array_equal(exp[:len(ee)], ee)
    assert {1, 2, 4, 6, 7} <= set(exp[len(ee) + 400:].tolist())
    hot = _hot_keys(p)
    assert {kp[0] for kp in kps} <= hot
    stats = _check(monkeypatch, m, p, s, exp)
    under = _under(p, hot)
    assert stats[0] == len(hot) and stats[1] == int(under.sum())
    assert stats[2] == int((under & (exp == 0)).sum()) >= 406


def test_tampered(corpus, monkeypatch):
    """4,096 items of 8 keys, every second one tampered (every item of key 5 has a flipped key
    bit, so 7 keys are hot)."""
    m, p, s, e = corpus["k8"]
    stats = _check(monkeypatch, m, p, s, e)
    hot = _hot_keys(p)
    assert stats[0] == len(hot) == 7
    assert stats[2] == int((_under(p, hot) & (e == 0)).sum()) == 2048


def _mixed_valid(rng, n):
    """A = aB + T8 and n signatures under it that dalek's verify_strict accepts:
    R = rB + T' with T' + kT == 0 (irregular.Member's mode 2)."""
    mem = IR.Member("mixed", rng)
    tors = IR.torsion_points()
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        while True:
            r = IR._rand_scalar(rng)
            Tp = tors[int(rng.integers(0, 8))]
            R = O.point_add(O.scalarmult_base(r), Tp)
            k = O.hram(R, mem.pk, msgs[i].tobytes())
            if O.point_add(Tp, O.scalarmult(k, mem.T)) == IR.IDENTITY:
                break
        sigs[i] = np.frombuffer(R + O.scalar_add(r, O.scalar_mul(k, mem.a)), np.uint8)
    pks = np.tile(np.frombuffer(mem.pk, np.uint8), (n, 1))
    return msgs, pks, sigs


def test_special_keys(corpus, monkeypatch):
    """Keys used 200 times each: undecodable and small-order (never hot), a non-canonical
    large-order encoding y = p + 3 (hot, nothing passes), a mixed-order key A = aB + T8 with
    signatures dalek accepts (hot, everything passes: the comb sum is the exact [k]A)."""
    rng = np.random.Generator(np.random.PCG64(3))
    m, p, s = _signed(rng, 3 * 200, corpus["kps"][:3], tamper=False)
    special = [_enc(2, 0), _enc(1, 0), _enc(P_FIELD + 3, 0)]
    for i in range(len(m)):
        p[i] = special[i % 3]
    mm, mp, ms = _mixed_valid(rng, 200)
    m, p, s = np.concatenate([m, mm]), np.concatenate([p, mp]), np.concatenate([s, ms])
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.all(exp[600:] == 0) and {3, 5, 7} <= set(exp[:600].tolist())
    assert all(16 * c >= MIN for c in
               np.unique(p[_sampled(len(p))], axis=0, return_counts=True)[1])   # all four used enough
    stats = _check(monkeypatch, m, p, s, exp)
    assert _hot_keys(p) == {special[2].tobytes(), mp[0].tobytes()}
    assert stats[:3] == [2, 400, 200]


def test_threshold_boundary(corpus, monkeypatch):
    """The uses are estimated from the sampled rows: a key with 3 of them (48 < MIN) stays
    cold, a key with 4 (64 = MIN) is hot, whatever their other rows."""
    rng = np.random.Generator(np.random.PCG64(4))
    n = int(np.nonzero(_sampled(1000))[0][7])          # rows before the 8th sampled one
    rows = np.nonzero(_sampled(n))[0]
    assert len(rows) == 7
    key_of = [i & 1 for i in range(n)]
    for t, r in enumerate(rows):
        key_of[r] = 0 if t < 3 else 1
    m, p, s = _sign_rows(rng, corpus["kps"][:2], key_of)
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert np.all(exp == 0)
    stats = _check(monkeypatch, m, p, s, exp)
    ones = sum(key_of)
    assert stats == [1, ones, ones, n - ones]


def test_key_cap(corpus, monkeypatch):
    """NW_STRICT_COMB_KEYS=2 with 5 qualifying keys of 200 uses: two get tables (which two may
    differ from run to run), the others' items take the ladder."""
    monkeypatch.setenv("NW_STRICT_COMB_KEYS", "2")
    rng = np.random.Generator(np.random.PCG64(5))
    m, p, s = _signed(rng, 1000, corpus["kps"][:5], tamper=False)
    s[7, 3] ^= 1
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert len(_hot_keys(p)) == 5
    stats = _check(monkeypatch, m, p, s, exp)
    assert stats[0] == 2 and stats[1] == 400 and stats[2] in (399, 400)


def test_several_slices(corpus, monkeypatch):
    """NW_TRIAGE_SLICE=1024 over 4,096 items: four slices whose hot keys differ (slice q holds
    keys 2q and 2q + 1), the tables, counts and to-do list rebuilt for each."""
    monkeypatch.setenv("NW_TRIAGE_SLICE", "1024")
    rng = np.random.Generator(np.random.PCG64(6))
    m, p, s = _sign_rows(rng, corpus["kps"][:8], [2 * (i // 1024) + (i & 1) for i in range(4096)])
    for i in range(0, 4096, 5):
        s[i, rng.integers(0, 64)] ^= np.uint8(1 << rng.integers(0, 8))
    exp = O.verify_strict_many(m, p, s).astype(np.int32)
    assert all(len(_hot_keys(p[a:a + 1024])) == 2 for a in range(0, 4096, 1024))
    stats = _check(monkeypatch, m, p, s, exp)
    assert stats[0] == 8 and stats[1] == 4096 and stats[2] == int((exp == 0).sum())


def test_alternating_launches(corpus, monkeypatch):
    """Back-to-back launches on one stream with the path on, off and on again, over inputs of
    different sizes and keys: the tables, planes and lists are reused correctly."""
    monkeypatch.setenv("NW_STRICT_COMB_MIN", str(MIN))
    a, b = corpus["k8"], corpus["k64"]
    for on, (m, p, s, e), lo, hi in ((1, a, 0, 4096), (0, b, 0, 4096), (1, b, 0, 4096),
                                     (1, a, 1000, 2111), (0, a, 0, 777), (1, a, 0, 4096)):
        monkeypatch.setenv("NW_STRICT_COMB", str(on))
        st, bits, stats = _launch(m[lo:hi], p[lo:hi], s[lo:hi])
        assert np.array_equal(st, e[lo:hi]) and np.array_equal(bits, e[lo:hi] == 0)
        hot = _hot_keys(p[lo:hi]) if on else set()
        assert stats[0] == len(hot)
        assert stats[2] == int((_under(p[lo:hi], hot) & (e[lo:hi] == 0)).sum())


def test_ladder_rounds_comb_off(corpus, monkeypatch):
    """The sizes of test_gpu_strict_ladder / test_gpu_strict_keys whose tiled keys are now hot
    (so that the ladder sees only the failures): with NW_STRICT_COMB=0 the survivors still fill
    the persistent ladder kernel's resident lanes exactly once plus a tail, and twice."""
    monkeypatch.setenv("NW_STRICT_COMB", "0")
    for n in (RESIDENT_LANES + 65, 2 * RESIDENT_LANES + 65):
        m, p, s, e = (np.resize(a, (n,) + a.shape[1:]) for a in corpus["k64"])
        st, bits, stats = _launch(m, p, s)
        assert np.array_equal(st, e) and np.array_equal(bits, e == 0)
        assert stats == [0, 0, 0, n]
    assert int(np.isin(e, [0, 7]).sum()) > RESIDENT_LANES


def test_tiled_hot(corpus, monkeypatch):
    """65,536 + 65 items of the tiled 64-key set at the default threshold of 256: hot keys of
    ~1,000 uses, and bit-flipped keys tiled to a few dozen uses that stay cold."""
    n = 65536 + 65
    m, p, s, e = (np.resize(a, (n,) + a.shape[1:]) for a in corpus["k64"])
    stats = _check(monkeypatch, m, p, s, e, min_uses=256)
    hot = _hot_keys(p, 256)
    assert stats[0] == len(hot) >= 56   # 8 of the 64 signers appear only with a flipped key bit
    assert stats[2] == int((_under(p, hot) & (e == 0)).sum())


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import test_gpu_strict_comb as T
from oracle import oracle as O

rng = np.random.Generator(np.random.PCG64(7))
kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(8)]
m, p, s = T._signed(rng, 4096, kps)
exp = O.verify_strict_many(m, p, s).astype(np.int32)
for _ in range(2):
    st, bits, stats = T._launch(m, p, s)
    assert np.array_equal(st, exp) and np.array_equal(bits, exp == 0), stats
    assert stats[2] + stats[3] == 4096
print("LIMIT_OK", stats)
"""


def test_three_gb_limit():
    """4,096 items of 8 hot keys under the 3 GB allocation limit of test_gpu_memory.py: the B
    comb (11.8 GB) cannot be had, the launch runs without the path, the statuses are the
    oracle's and no error is left behind for the second launch."""
    env = dict(os.environ, NW_DEVICE_MEM_LIMIT=str(3 * 10**9), NW_STRICT_COMB_MIN=str(MIN))
    env.pop("NW_STRICT_COMB", None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _CHILD], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "LIMIT_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
