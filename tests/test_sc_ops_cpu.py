"""The scalar layer (narwhal_amd/csrc/nw_scalar.hpp: Barrett reduction, sc_mul / sc_add /
sc_neg / sc_is_canonical, sc_recode, the half-size split) and the scalar phase of a strict
verification (nw_strict.hpp strict_scalar_phase, bdigits, key_recode / key_digit) on chosen
words, compiled as host code (tools/libnw_hostcheck.so: hc_sc_ops over tools/sc_ops.hpp),
against tests/sc_cases.py's Python-integer expectations.

Every other test reaches this code with k = SHA-512(...) mod l, so none can choose a 512-bit
value, a k or a w. Here the inputs are chosen by models of the same steps, and the bucket tests
assert that they reach what they claim: both counts of Barrett's final subtraction, the 9-word
difference wrapping and not, a partial quotient of every listed size at every listed depth of
8l / k's continued fraction, the exact band, the in-between band and the fallback of the
half-size split, odd and even final cofactors. tests/test_gpu_sc_ops.py runs the same batches
on the gfx950 build.

Two final subtractions in sc_reduce512: none exists. sc_cases.TWO_SUBTRACTIONS_IMPOSSIBLE is
the proof in integers (the quotient estimate is at most one too small because
frac(2^512 / l) = 0.2249... leaves mu's truncation no room), and the seeded search of
sc_cases.search_two_subtractions (120,000 inputs aimed at the worst case) finds none. The
second sc_sub_l_if_geq9 of sc_reduce512 is therefore unreachable."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sc_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_hostcheck.so")
U32P = ctypes.POINTER(ctypes.c_uint32)
I32P = ctypes.POINTER(ctypes.c_int32)


def _build():
    csrc = os.path.join(ROOT, "narwhal_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", f) for f in ("hostcheck.hip", "limb_ops.hpp", "sc_ops.hpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in srcs):
        return
    subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "include"), srcs[0], "-o", LIB], check=True)


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    lib.hc_sc_ops.restype = ctypes.c_int
    lib.hc_sc_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, U32P, I32P, U32P]
    return lib


_cpu_out = {}


def run_cpu(lib, batch):
    """The batch through the CPU build: n x 40 output words (computed once per batch)."""
    if id(batch) not in _cpu_out:
        A, k = batch.arrays()
        out = np.full((len(A), C.OUT_WORDS), 0xdeadbeef, np.uint32)   # the entry zeroes it
        rc = lib.hc_sc_ops(batch.op, len(A), A.ctypes.data_as(U32P), k.ctypes.data_as(I32P),
                           out.ctypes.data_as(U32P))
        assert rc == 0
        out.setflags(write=False)
        _cpu_out[id(batch)] = (batch, out)
    return _cpu_out[id(batch)][1]


@pytest.mark.parametrize("group", C.GROUPS)
def test_sc_ops_cpu(hc, group):
    """barrett: sc_reduce512 and sc_mul; addneg: sc_add, sc_neg, sc_is_canonical; recode:
    sc_recode under both biases, bdigits<8/16/20/24>, key digits at every width; half:
    sc_half_split with and without the Lehmer rounds; phase: strict_scalar_phase<16/24>."""
    total = 0
    for batch in C.batches(group):
        batch.check(run_cpu(hc, batch))
        total += len(batch.cases)
    assert total > 0


def test_barrett_inputs_reach_every_class(hc):
    """The inputs of sc_reduce512, and the products sc_mul hands it, take 0 and 1 final
    subtractions, wrap and do not wrap the 9-word difference, carry and do not carry row 0 of
    q3 * l into word 8. No input takes two subtractions (module docstring); any the search did
    find would run through the build here."""
    for xs in ([x for _, x in C.reduce_inputs()], [a * b for _, a, b in C.mul_inputs()]):
        cls = [C.barrett(x)[1:] for x in xs]
        assert {c[0] for c in cls} == {0, 1}
        assert {c[1] for c in cls} == {False, True}
        assert {c[2] for c in cls} == {False, True}
        assert {(c[0], c[1]) for c in cls} == {(0, False), (0, True), (1, False), (1, True)}
    assert C.TWO_SUBTRACTIONS_IMPOSSIBLE
    found = C.search_two_subtractions()
    b = C.Batch(C.REDUCE512)
    for x in found:
        b.add(f"two subtractions {x:#x}", C.words(x, 16), 0, C._is(x % C.L))
    if found:
        b.check(run_cpu(hc, b))
    assert not found, "the proof says none exists"


def _half_rows(hc):
    lehmer, onestep = C.batches("half")
    return lehmer, run_cpu(hc, lehmer), run_cpu(hc, onestep)


def test_half_split_cases_reach_every_bucket(hc):
    """Every (depth, quotient) of the constructed k is populated (sc_cases.constructed_k confirms
    each position with the exact Euclid); the three bands, both cofactor parities and both
    outcomes (a short vector, the (k, 1) fallback) occur, the fallback also a few Lehmer rounds
    deep and an even cofactor also among the constructed k; the random k stay far below the
    iteration cap."""
    cons = C.constructed_k()
    assert set(cons) == {(d, qn) for d in C.DEPTHS for qn, _ in C.BIG_Q}
    assert len(set(cons.values())) == len(cons)
    lehmer, out, _ = _half_rows(hc)
    seen, deep_fallback, cons_parity = set(), set(), set()
    for (name, inp, _, _, _), row in zip(lehmer.cases, out.tolist()):
        k = C.val(inp[:8])
        bnd, parity, _ = C.half_expect(k)
        fallback = (C.val(row[:8]), C.val(row[8:13]), row[13]) == (k, 1, 0) and k >= 2**128
        seen.add((bnd, parity, fallback))
        if name.startswith("rand"):
            assert bnd == "low" and len(C.euclid(k)[0]) < 120
        if name.startswith("depth"):
            cons_parity.add(parity)
            if fallback and not name.startswith("depth 0,"):
                deep_fallback.add(name)
    assert {s[0] for s in seen} == {"low", "mid", "high"}
    for parity in ("odd", "even"):
        assert ("low", parity, False) in seen
    assert any(s[0] == "high" and s[2] for s in seen)
    assert cons_parity == {"odd", "even"}
    assert len(deep_fallback) >= 4
    sizes = {q.bit_length() for k in cons.values() for q in C.euclid(k)[0]}
    assert {31, 32, 33, 34, 39, 41, 46} <= sizes


def test_half_split_lehmer_equals_one_step(hc):
    """The Lehmer rounds only batch exact Euclid steps: outside the in-between band the split
    equals the one-step loop's word for word."""
    lehmer, a, b = _half_rows(hc)
    rows = lehmer.exact_rows()
    assert rows.sum() > 2000 and (~rows).sum() >= 2 * len(C.DEPTHS)
    bad = np.flatnonzero((a != b).any(axis=1) & rows)
    assert bad.size == 0, lehmer.cases[bad[0]][0]


def test_bad_arguments_are_refused(hc):
    z = np.zeros((1, C.IN_WORDS), np.uint32)
    o = np.zeros((1, C.OUT_WORDS), np.uint32)
    k = np.zeros(1, np.int32)
    args = (z.ctypes.data_as(U32P), k.ctypes.data_as(I32P), o.ctypes.data_as(U32P))
    assert hc.hc_sc_ops(C.SC_N, 1, *args) == -1
    assert hc.hc_sc_ops(-1, 1, *args) == -1
    for w in (0, 4, 12, 32):
        k[0] = w
        assert hc.hc_sc_ops(C.KEY_DIGITS, 1, *args) == -1
