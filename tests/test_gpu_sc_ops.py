"""The scalar layer and the scalar phase on the MI355X (tools/libnw_lpcheck.so: k_sc_ops, one
lane per case with lane = case index, over tools/sc_ops.hpp).

On the device this code is otherwise reached only through whole verifications, where k is a
SHA-512 output. Here tests/sc_cases.py's batches run on the gfx950 build of nw_scalar.hpp and of
the scalar phase of nw_strict.hpp, at block size 64 and 256: the output must satisfy the
Python-integer expectations itself and equal the CPU build's word for word
(tests/test_sc_ops_cpu.py) — the device's floor / ldexp / f64 division and any fma contraction
of bn8_to_f64 included — except in the half-size split's in-between band, where only the
invariants apply (sc_cases.band).

The Lehmer rounds make a lane's path depend on its wave: the one-step code runs only in an
iteration where no lane made Lehmer progress (nw_any), and a waiting lane's iterations count
against the cap. test_wave_composition runs every constructed, listed, early-exit and
even-cofactor k of the exact bands in four settings and requires one result.

At their first run the two builds agreed on every case but one: for k = l - 1 (one Euclid step,
even cofactor, every candidate has u >= 2^252, so the result is the fallback (k, 1)) the device
build of strict_scalar_phase<16> and <24> returned u = l - 9, X - Y's, beside the fallback's
v = 1 and w = -s, which breaks u = v k (mod 8l); sc_half_split alone was right on the device,
and so was the CPU build. sc_half_split now writes the trivial vector before its loop instead
of after it (nw_scalar.hpp); the case stays as "regression k=l-1" in sc_cases.half_k()."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sc_cases as C
from test_sc_ops_cpu import hc, run_cpu  # noqa: F401  (the CPU build of the same text)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_lpcheck.so")
U32P = ctypes.POINTER(ctypes.c_uint32)
I32P = ctypes.POINTER(ctypes.c_int32)
BLOCKS = (64, 256)


@pytest.fixture(scope="module")
def lpc():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "lpcheck"], check=True)
    lib = ctypes.CDLL(LIB)
    lib.lpc_sc_ops.restype = ctypes.c_int
    lib.lpc_sc_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, U32P, I32P, U32P, ctypes.c_int]
    return lib


def run_words(lib, op, A, k, block):
    A = np.ascontiguousarray(A, np.uint32)
    k = np.ascontiguousarray(k, np.int32)
    out = np.full((len(A), C.OUT_WORDS), 0xdeadbeef, np.uint32)   # the entry zeroes its own copy
    rc = lib.lpc_sc_ops(op, len(A), A.ctypes.data_as(U32P), k.ctypes.data_as(I32P),
                        out.ctypes.data_as(U32P), block)
    assert rc == 0, f"lpc_sc_ops: status {rc}"
    return out


@pytest.mark.parametrize("group", C.GROUPS)
def test_sc_ops_gpu(lpc, hc, group):  # noqa: F811
    for batch in C.batches(group):
        cpu = run_cpu(hc, batch)
        A, k = batch.arrays()
        for block in BLOCKS:
            gpu = run_words(lpc, batch.op, A, k, block)
            bad = np.flatnonzero((gpu != cpu).any(axis=1) & batch.exact_rows())
            assert bad.size == 0, (block, batch.cases[bad[0]][0], gpu[bad[0]].tolist(),
                                   cpu[bad[0]].tolist())
            batch.check(gpu)


def _targets():
    """(name, k, check) of every k whose result must not depend on its wave: outside the
    in-between band, and constructed, listed, early-exit or with an even cofactor."""
    out = []
    for name, k in C.half_k():
        bnd, parity, _ = C.half_expect(k)
        if bnd != "mid" and (not name.startswith("rand") or parity == "even"):
            out.append((name, k, C._half_check(k)[0]))
    return out


def test_wave_composition(lpc):
    """Each target k in four settings: (a) replicated over a whole wave; (b) in lane 0, 31 and
    63 of a wave of 63 random k; (c) in one lane among 63 k that fall back (they run all
    400 iterations, most of them without ever making Lehmer progress); (d) in a ragged last
    wave of a 256-thread block, alone (n = 65) and with 62 other targets (n = 127). All
    outputs for the k are equal and satisfy its expectation."""
    targets = _targets()
    names = [t[0] for t in targets]
    assert sum(n.startswith("depth") for n in names) >= 30 and sum(n.startswith("rand") for n in names) > 500
    assert any(n.startswith("early") for n in names) and any(n.startswith("listed") for n in names)
    T = np.array([C.words(k, 8) + [0] * 16 for _, k, _ in targets], np.uint32)
    nt = len(T)
    rng = np.random.Generator(np.random.PCG64(43))

    def rows(ks):
        return np.array([C.words(k, 8) + [0] * 16 for k in ks], np.uint32)
    rand = rows([int.from_bytes(rng.bytes(32), "little") % C.L for _ in range(4096)])
    fall = rows([k for k in ([2**128, 2**129 + 5, 3 * 2**127, 2**200 + 1]
                             + [kk for (d, qn), kk in C.constructed_k().items() if qn == "2^45"])
                 if C.band(C.euclid(k)[0]) == "high"])
    assert len(fall) >= 8

    def launch(A, block):
        return run_words(lpc, C.HALF_SPLIT, A, np.zeros(len(A), np.int32), block)

    # (a) a whole wave of the same k
    a = launch(np.repeat(T, 64, axis=0), 64).reshape(nt, 64, C.OUT_WORDS)
    ref = a[:, 0].copy()
    assert (a == ref[:, None]).all(), "lanes of one wave holding the same k disagree"
    for (name, _, chk), row in zip(targets, ref.tolist()):
        try:
            chk(row)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None

    def differs(got, what):
        bad = np.flatnonzero((got != ref).any(axis=1))
        assert bad.size == 0, (what, names[bad[0]], got[bad[0]].tolist(), ref[bad[0]].tolist())

    # (b), (c): one lane of a wave of random k / of k that fall back
    for what, pool in (("random", rand), ("fallback", fall)):
        for lane in (0, 31, 63):
            A = pool[rng.integers(0, len(pool), size=(nt, 64))]
            A[:, lane] = T
            for block in BLOCKS if lane == 31 else (256,):
                got = launch(A.reshape(nt * 64, C.IN_WORDS), block)
                differs(got.reshape(nt, 64, C.OUT_WORDS)[:, lane], f"lane {lane} among {what} k")
    # (d) ragged last waves of a 256-thread block
    for i in range(0, nt, 63):
        chunk = T[i:i + 63]
        A = np.concatenate([rand[rng.integers(0, len(rand), size=127 - len(chunk))], chunk])
        assert len(A) == 127
        got = launch(A, 256)
        assert (got[-len(chunk):] == ref[i:i + 63]).all(), ("ragged wave of 63", names[i])
    fill = rand[:64]
    for i in range(nt):
        got = launch(np.concatenate([fill, T[i:i + 1]]), 256)
        assert (got[64] == ref[i]).all(), ("alone in the last wave", names[i])


def test_sc_bad_arguments(lpc):
    z = np.zeros((1, C.IN_WORDS), np.uint32)
    o = np.zeros((1, C.OUT_WORDS), np.uint32)
    k = np.zeros(1, np.int32)
    args = (z.ctypes.data_as(U32P), k.ctypes.data_as(I32P), o.ctypes.data_as(U32P))
    assert lpc.lpc_sc_ops(C.SC_N, 1, *args, 64) == -1
    assert lpc.lpc_sc_ops(-1, 1, *args, 64) == -1
    assert lpc.lpc_sc_ops(C.ADD, 1, *args, 96) == -1
    assert lpc.lpc_sc_ops(C.ADD, 0, *args, 64) == -1
    k[0] = 12   # a key width keyspec_for does not build: refused by the kernel's bad flag
    assert lpc.lpc_sc_ops(C.KEY_DIGITS, 1, *args, 64) == -1
