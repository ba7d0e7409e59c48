"""The branch of strict_verify_core the device runs, on the CPU (tools/hostcheck.hip): the
ladder with a prefetcher (entries requested one addition ahead, digit words through
dput / dget; a host model that poisons every slot once read, so an unmatched or stale read
gives a wrong verdict), and config 4's two passes with the scalar phase on the triage side
(hc_verify_strict_twopass_scalars: strict_triage, strict_triage_scalars, then the ladder
from the stored x, digit words, vneg and window count). Statuses against the golden edge
corpus, the oracle on random valid / tampered signatures, and constructed signatures for
injected k (k is an argument of the host entry points: for a secret a and a chosen r,
R = [r]B and S = r + k a satisfy the equation for that k whatever it is)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from oracle import oracle as O

from sc_cases import constructed_k
from test_hostcheck import LIB, L_ORDER, _adversarial_k, _b, _build, _out

BWS = [-16, -24]


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    for f in ("hc_verify_strict_half_pf", "hc_verify_strict_twopass_scalars", "hc_half_split"):
        getattr(lib, f).restype = ctypes.c_int
    return lib


def _entries(hc):
    return (hc.hc_verify_strict_half_pf, hc.hc_verify_strict_twopass_scalars)


@pytest.mark.parametrize("bw", BWS)
def test_edge_corpus(hc, golden, bw):
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        for f in _entries(hc):
            assert f(_b(pk), _b(sig), _b(k), bw) == it["status"], it["class"]


@pytest.fixture(scope="module")
def random_items():
    """2,000 valid and 2,000 tampered (one bit of s or of R flipped) signatures with the
    oracle's statuses, computed once."""
    rng = np.random.Generator(np.random.PCG64(2024))
    keys = [O.keypair_from_seed(rng.bytes(32)) for _ in range(64)]
    items = []
    for i in range(4000):
        pk, sk = keys[i % 64]
        m = rng.bytes(32)
        sig = bytearray(O.sign(sk, m))
        if i % 2 == 1:
            if i % 4 == 1:
                sig[32 + int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
            else:
                sig[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        sig = bytes(sig)
        items.append((pk, sig, O.hram(sig[:32], pk, m), O.verify_strict(m, pk, sig)))
    assert sum(1 for it in items if it[3] == 0) == 2000
    return items


@pytest.mark.parametrize("bw", BWS)
def test_random_valid_and_tampered(hc, random_items, bw):
    for f in _entries(hc):
        for pk, sig, k, want in random_items:
            assert f(_b(pk), _b(sig), _b(k), bw) == want


def _scalar_a(seed: bytes) -> int:
    h = bytearray(hashlib.sha512(seed).digest()[:32])
    h[0] &= 248
    h[31] = (h[31] & 127) | 64
    return int.from_bytes(h, "little")


def _injected_k(hc):
    """The edge k of test_hostcheck.py, random k, tests/sc_cases.py's constructed k (a partial
    quotient of 2^31 - 1 .. 2^45 at five depths of 8l / k's continued fraction), and among them
    k whose split falls back to the trivial vector (k, 1) (a ladder of up to 64 windows)."""
    rng = np.random.Generator(np.random.PCG64(77))
    ks = [k % L_ORDER for k in _adversarial_k()]
    ks += [2**129 + 5, 3 * 2**127, 2**200 + 1, (8 * L_ORDER) // 3 % L_ORDER]
    ks += [int.from_bytes(rng.bytes(32), "little") % L_ORDER for _ in range(24)]
    ks += list(constructed_k().values())
    fallback = []
    for k in ks:
        u, v = _out(32), _out(20)
        neg = hc.hc_half_split(_b(k.to_bytes(32, "little")), u, v)
        if (int.from_bytes(u.raw, "little"), int.from_bytes(v.raw, "little"), neg) == (k, 1, 0) \
                and k.bit_length() > 140:
            fallback.append(k)
    return ks, fallback


@pytest.mark.parametrize("bw", BWS)
def test_injected_k(hc, bw):
    ks, fallback = _injected_k(hc)
    assert fallback, "no k of the list takes the (k, 1) fallback"
    rng = np.random.Generator(np.random.PCG64(78))
    seed = rng.bytes(32)
    pk, _ = O.keypair_from_seed(seed)
    a = _scalar_a(seed) % L_ORDER
    for k in ks:
        r = int.from_bytes(rng.bytes(32), "little") % L_ORDER
        R = O.scalarmult_base(r.to_bytes(32, "little"))
        s = (r + k * a) % L_ORDER
        kb = k.to_bytes(32, "little")
        good = R + s.to_bytes(32, "little")
        bad = R + ((s + 1) % L_ORDER).to_bytes(32, "little")
        for f in _entries(hc):
            assert f(_b(pk), _b(good), _b(kb), bw) == 0, k
            assert f(_b(pk), _b(bad), _b(kb), bw) == 7, k
