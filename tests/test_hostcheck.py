"""The kernels' arithmetic headers (narwhal_amd/csrc/nw_*.hpp), compiled as host code into
tools/libnw_hostcheck.so (test infrastructure), against the CPU oracle on the golden
fixtures and random inputs. Catches field/point/scalar/ladder bugs without a GPU; the GPU
parity tests (test_gpu_parity.py) then check the kernels end to end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

from sc_cases import constructed_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_hostcheck.so")
L = 2**252 + 27742317777372353535851937790883648493


def _build():
    srcs = [os.path.join(ROOT, "tools", "hostcheck.hip")] + [
        os.path.join(ROOT, "narwhal_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "narwhal_amd", "csrc"))
        if f.endswith(".hpp")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in srcs):
        return
    subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "include"), srcs[0], "-o", LIB], check=True)


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    for f in ("hc_decompress", "hc_is_small_order", "hc_dsm", "hc_verify_strict",
              "hc_scalar_canonical", "hc_half_split", "hc_verify_strict_half",
              "hc_verify_strict_twopass"):
        getattr(lib, f).restype = ctypes.c_int
    return lib


def _b(x):
    return ctypes.c_char_p(bytes(x))


def _out(n=32):
    return ctypes.create_string_buffer(n)


def test_decompress_and_small_order(hc, golden):
    pts = set()
    for it in golden["edge_corpus"]["items"]:
        pts.add(bytes.fromhex(it["pk"]))
        pts.add(bytes.fromhex(it["sig"])[:32])
    rng = np.random.Generator(np.random.PCG64(1))
    pts |= {rng.bytes(32) for _ in range(200)}
    for p in pts:
        o = _out()
        ok = hc.hc_decompress(_b(p), o)
        ref = O.decompress(p)
        assert bool(ok) == (ref is not None), p.hex()
        if ok:
            assert o.raw == ref, p.hex()
        assert hc.hc_is_small_order(_b(p)) == O.is_small_order(p), p.hex()


def test_scalars(hc):
    rng = np.random.Generator(np.random.PCG64(2))
    edge = [bytes(64), (L).to_bytes(64, "little"), (L - 1).to_bytes(64, "little"),
            (2**512 - 1).to_bytes(64, "little"), (L * (2**259)).to_bytes(64, "little")]
    for x in edge + [rng.bytes(64) for _ in range(300)]:
        o = _out()
        hc.hc_reduce512(_b(x), o)
        assert o.raw == O.scalar_reduce64(x)
    for _ in range(300):
        a, b = rng.bytes(32), rng.bytes(32)
        o = _out()
        hc.hc_scalar_mul(_b(a), _b(b), o)
        assert o.raw == O.scalar_mul(a, b)
        ar = O.scalar_reduce64(a + bytes(32))
        br = O.scalar_reduce64(b + bytes(32))
        hc.hc_scalar_add(_b(ar), _b(br), o)
        assert o.raw == O.scalar_add(ar, br)
    for v in [0, 1, L - 1, L, L + 1, 2**252, 2**253, 2**256 - 1]:
        assert hc.hc_scalar_canonical(_b(v.to_bytes(32, "little"))) == (v < L)


def test_fixed_base_and_dsm(hc):
    rng = np.random.Generator(np.random.PCG64(3))
    for i in range(60):
        s = O.scalar_reduce64(rng.bytes(64))
        o = _out()
        hc.hc_fixed_base(_b(s), o)
        assert o.raw == O.scalarmult_base(s)
        a = O.scalar_reduce64(rng.bytes(64))
        P = O.scalarmult_base(O.scalar_reduce64(rng.bytes(64)))
        assert hc.hc_dsm(_b(a), _b(P), _b(s), o) == 1
        ref = O.point_add(O.scalarmult_base(s), O.scalarmult(a, P))
        assert o.raw == ref


def test_verify_strict_edge_corpus(hc, golden):
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        assert hc.hc_verify_strict(_b(pk), _b(sig), _b(k)) == it["status"], it["class"]


L_ORDER = 2**252 + 27742317777372353535851937790883648493


def _half(hc, k: int):
    u, v = _out(32), _out(20)
    neg = hc.hc_half_split(_b(k.to_bytes(32, "little")), u, v)
    vv = int.from_bytes(v.raw, "little")
    return int.from_bytes(u.raw, "little"), -vv if neg else vv


def _adversarial_k():
    """Edge k of the half-size split. Only 2**128 reaches the iteration cap (a 128-bit quotient
    at the first step); the first two entries are 125- and 128-bit numbers and, like 2**128 - 1,
    0, 1, 2 and 7, leave before the loop starts with (k, 1); l - 1 and 2**252 end after one
    step with an even cofactor and a vector too long to use. k
    with a partial quotient of a chosen size at a chosen depth are tests/sc_cases.py's
    constructed_k()."""
    n = 8 * L_ORDER
    return [(n * (2**126 + 1)) // (2**128 + 3) % L_ORDER, n // (2**127 + 1) % L_ORDER,
            (2**128 - 1), 2**128, 2**252, L_ORDER - 1, 0, 1, 2, 7]


def test_half_split_lattice(hc):
    """u = v k (mod 8l), v odd, |u|, |v| < 2^129 for random k; edge / adversarial k
    still satisfy the congruence (fallback (k, 1) allowed)."""
    n = 8 * L_ORDER
    rng = np.random.Generator(np.random.PCG64(11))
    sizes = []
    for i in range(3000):
        k = int.from_bytes(rng.bytes(32), "little") % L_ORDER
        u, v = _half(hc, k)
        assert (u - v * k) % n == 0 and v % 2 == 1 and u >= 0
        sizes.append(max(u.bit_length(), abs(v).bit_length()))
    sizes = np.array(sizes)
    # the best odd vector is <= 129 bits for ~96% of k (Python model of the same search:
    # 95.7%), and never far above
    assert (sizes > 129).mean() < 0.06 and sizes.max() <= 140
    for k in _adversarial_k():
        u, v = _half(hc, k)
        assert (u - v * k) % n == 0 and v % 2 == 1 and 0 <= u < 2**253, k


def test_half_split_lehmer_equals_one_step(hc):
    """The Lehmer rounds (Knuth Algorithm L, nw_scalar.hpp) only batch exact Euclid steps:
    the split equals the one-step loop's on random, edge and constructed k (a partial quotient
    of 2^31 - 1 .. 2^45 at depth 0, 1, 5, 20 and 50 of 8l / k's continued fraction). On this
    build a lane never waits for a wave, so the two agree in every band."""
    rng = np.random.Generator(np.random.PCG64(14))
    ks = [int.from_bytes(rng.bytes(32), "little") % L_ORDER for _ in range(4000)]
    ks += _adversarial_k() + [2**129 + 5, 3 * 2**127, 2**200 + 1, (8 * L_ORDER) // 3 % L_ORDER]
    ks += list(constructed_k().values())
    for k in ks:
        outs = []
        for f in (hc.hc_half_split, hc.hc_half_split_onestep):
            u, v = _out(32), _out(20)
            outs.append((f(_b(k.to_bytes(32, "little")), u, v), u.raw, v.raw))
        assert outs[0] == outs[1], k


@pytest.mark.parametrize("bw", [16, 8, 20, 24, -16, -24])
def test_strict_half_edge_corpus(hc, golden, bw):
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        assert hc.hc_verify_strict_half(_b(pk), _b(sig), _b(k), bw) == it["status"], it["class"]


P25519 = 2**255 - 19


def _limbs_to_int(limbs):
    """Value of 10 radix-2^25.5 limbs (limb i at bit ceil(25.5 i))."""
    return sum(int(x) << ((51 * i + 1) // 2) for i, x in enumerate(limbs))


def test_wide_btab_entries(hc):
    """The host copy of the 16-bit wide B tables (nw_consts.hpp compute_wide_btab; the device
    builds its own with k_btab_build, checked end to end by the GPU strict tests):
    entry j of half h is j * 2^(128 h) * B in affine niels form, against the oracle."""
    rng = np.random.Generator(np.random.PCG64(13))
    js = [0, 1, 2, 3, 127, 128, 129, 32767, 32768] + [int(x) for x in rng.integers(0, 32769, 24)]
    out = (ctypes.c_uint32 * 30)()
    inv2 = pow(2, P25519 - 2, P25519)
    for h in (0, 1):
        for j in js:
            hc.hc_wide_btab_entry(h, j, out)
            ypx, ymx, xy2d = (_limbs_to_int(out[10 * c:10 * c + 10]) % P25519 for c in range(3))
            y = (ypx + ymx) * inv2 % P25519
            x = (ypx - ymx) * inv2 % P25519
            enc = (y | ((x & 1) << 255)).to_bytes(32, "little")
            s = (j << (128 * h)) % L
            assert enc == O.scalarmult_base(s.to_bytes(32, "little")), (h, j)


@pytest.fixture(params=[16, 20])
def keyw(request, hc):
    """The key-comb widths the device builds (nw_api.cpp key_width: 20 bits up to 64 keys,
    otherwise 16; ntab = ceil(253 / W) tables plus a 2^128 A table when W does not divide
    128, nw_kernels.h keyspec_for)."""
    hc.hc_set_key_width.restype = ctypes.c_int
    assert hc.hc_set_key_width(request.param) == 0
    yield request.param
    hc.hc_set_key_width(16)


def test_strict_keyed_comb(hc, golden, keyw):
    """Committee-key strict path (no ladder: [s]B - [k]A from comb tables) against the
    oracle on the edge corpus and on random honest / tampered signatures."""
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        assert hc.hc_verify_strict_keyed(_b(pk), _b(sig), _b(k)) == it["status"], it["class"]
    rng = np.random.Generator(np.random.PCG64(15))
    for i in range(24):
        pk, sk = O.keypair_from_seed(rng.bytes(32))
        m = rng.bytes(32)
        sig = bytearray(O.sign(sk, m))
        if i % 3 == 1:
            sig[32 + int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
        elif i % 3 == 2:
            sig[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        k = O.hram(bytes(sig[:32]), pk, m)
        assert hc.hc_verify_strict_keyed(_b(pk), _b(bytes(sig)), _b(k)) == \
            O.verify_strict(m, pk, bytes(sig))


def _scalar_a(seed: bytes) -> int:
    import hashlib
    h = bytearray(hashlib.sha512(seed).digest()[:32])
    h[0] &= 248
    h[31] = (h[31] & 127) | 64
    return int.from_bytes(h, "little")


def test_keyed_vote_check_compressed_r(hc, golden, keyw):
    """Certificate votes' keyed check with R compared in compressed form (Y' == y_R Z' and
    the parity of X'/Z', no decompression of R): pass iff the oracle's strict verify is Ok,
    on the edge corpus (every Appendix A class), random honest / tampered signatures, and
    signatures by the key's owner with [s]B - [k]A == -R (same y, other x sign: dalek
    rejects them, so must the parity check)."""
    hc.hc_keyed_vote_check.restype = ctypes.c_int
    hc.hc_key_lambda.restype = ctypes.c_int
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        # keys with a torsion component always fail the keyed vote check (their votes take
        # the certificate's own verify_batch: a strict pass does not cancel their batch term)
        want = int(it["status"] != 0 or hc.hc_key_lambda(_b(pk)) > 0)
        assert hc.hc_keyed_vote_check(_b(pk), _b(sig), _b(k)) == want, it["class"]
    rng = np.random.Generator(np.random.PCG64(16))
    for i in range(36):
        seed = rng.bytes(32)
        pk, sk = O.keypair_from_seed(seed)
        m = rng.bytes(32)
        sig = bytearray(O.sign(sk, m))
        if i % 3 == 1:
            sig[32 + int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
        elif i % 3 == 2:
            sig[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        k = O.hram(bytes(sig[:32]), pk, m)
        want = int(O.verify_strict(m, pk, bytes(sig)) != 0)
        assert hc.hc_keyed_vote_check(_b(pk), _b(bytes(sig)), _b(k)) == want
    for i in range(12):                        # R' = -R: y matches, x sign does not
        seed = rng.bytes(32)
        pk, sk = O.keypair_from_seed(seed)
        a = _scalar_a(seed) % L_ORDER
        m = rng.bytes(32)
        r = int.from_bytes(rng.bytes(32), "little") % L_ORDER
        R = O.scalarmult_base(r.to_bytes(32, "little"))
        kk = int.from_bytes(O.hram(R, pk, m), "little")
        s = (kk * a - r) % L_ORDER
        sig = R + s.to_bytes(32, "little")
        assert O.verify_strict(m, pk, sig) != 0
        assert hc.hc_keyed_vote_check(_b(pk), _b(sig), _b(O.hram(R, pk, m))) == 1
        s_ok = (r + kk * a) % L_ORDER               # the honest s for the same R: passes
        sig = R + s_ok.to_bytes(32, "little")
        assert O.verify_strict(m, pk, sig) == 0
        assert hc.hc_keyed_vote_check(_b(pk), _b(sig), _b(O.hram(R, pk, m))) == 0


def test_key_lambda_vs_oracle(hc, golden):
    """A committee key's lambda ([l] A == [lambda] T8, k_key_base's definition) against the
    oracle's own scalar multiplication by l, for every decodable key of the edge corpus (the
    eight small-order points, mixed-order keys A = aB + T8, non-canonical encodings) and
    prime-order keys (lambda 0)."""
    hc.hc_key_lambda.restype = ctypes.c_int
    t8 = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")
    tors = [bytes.fromhex("01" + "00" * 31)]
    for _ in range(7):
        tors.append(O.point_add(tors[-1], t8))
    l_bytes = L_ORDER.to_bytes(32, "little")
    seen = set()
    pks = {bytes.fromhex(it["pk"]) for it in golden["edge_corpus"]["items"]}
    pks |= {O.keypair_from_seed(bytes([i]) * 32)[0] for i in range(4)}
    for pk in sorted(pks):
        lam = hc.hc_key_lambda(_b(pk))
        if O.decompress(pk) is None:
            assert lam == -1, pk.hex()
            continue
        lA = O.scalarmult(l_bytes, pk)
        assert lA == tors[lam], (pk.hex(), lam)
        seen.add(lam)
    assert 0 in seen and len(seen) >= 3, seen


def test_strict_half_random_and_tampered(hc):
    rng = np.random.Generator(np.random.PCG64(12))
    for i in range(120):
        seed = rng.bytes(32)
        pk, sk = O.keypair_from_seed(seed)
        m = rng.bytes(32)
        sig = bytearray(O.sign(sk, m))
        if i % 3 == 1:
            sig[32 + int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
        elif i % 3 == 2:
            sig[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        k = O.hram(bytes(sig[:32]), pk, m)
        want = O.verify_strict(m, pk, bytes(sig))
        for bw in (16, 8, 20, 24, -24):   # -24: packed per-lane table entries
            assert hc.hc_verify_strict_half(_b(pk), _b(bytes(sig)), _b(k), bw) == want


@pytest.mark.parametrize("bw", [-16, -24])
def test_strict_twopass_edge_corpus(hc, golden, bw):
    """Config 4 in two passes (k_strict_triage, then k_verify_strict_pre on the points the
    triage stored): the shared strict_triage + strict_verify_core over the stored x give the
    golden status of every edge-corpus item, as the one-pass core does."""
    for it in golden["edge_corpus"]["items"]:
        m, pk, sig = (bytes.fromhex(it[k]) for k in ("msg", "pk", "sig"))
        k = O.hram(sig[:32], pk, m)
        assert hc.hc_verify_strict_twopass(_b(pk), _b(sig), _b(k), bw) == it["status"], it["class"]


def test_strict_twopass_random_and_tampered(hc):
    rng = np.random.Generator(np.random.PCG64(15))
    for i in range(90):
        pk, sk = O.keypair_from_seed(rng.bytes(32))
        m = rng.bytes(32)
        sig = bytearray(O.sign(sk, m))
        if i % 3 == 1:
            sig[32 + int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
        elif i % 3 == 2:
            sig[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        k = O.hram(bytes(sig[:32]), pk, m)
        want = O.verify_strict(m, pk, bytes(sig))
        assert hc.hc_verify_strict_twopass(_b(pk), _b(bytes(sig)), _b(k), -24) == want
        assert hc.hc_verify_strict_half(_b(pk), _b(bytes(sig)), _b(k), -24) == want
