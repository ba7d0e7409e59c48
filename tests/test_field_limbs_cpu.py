"""The per-lane field and point routines (narwhal_amd/csrc/nw_field.hpp, nw_point.hpp) on RAW
limbs, compiled as host code (tools/libnw_hostcheck.so: hc_fe_ops / hc_ge_ops over
tools/limb_ops.hpp), against Python integers mod p and the affine twisted-Edwards law.

Every other test enters this code through fe_frombytes, so its limbs start tight. Here the
operands come from tests/limb_cases.py AT the bounds tests/test_field_bounds.py models (T, L,
P15, S_T, S_L per operand role, one-hot pairs that leave one product term alone in its column,
non-canonical zeros, the forms fe_join leaves), and each result must (a) denote the right
value, exactly, and (b) keep every limb inside the bound the header and the model claim for
that routine: this is what ties the model's T to the code. tests/test_gpu_field_limbs.py runs
the same batches on the gfx950 build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import limb_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_hostcheck.so")
U32P = ctypes.POINTER(ctypes.c_uint32)
I32P = ctypes.POINTER(ctypes.c_int32)


def _build():
    csrc = os.path.join(ROOT, "narwhal_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", "hostcheck.hip"), os.path.join(ROOT, "tools", "limb_ops.hpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in srcs):
        return
    subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "include"), srcs[0], "-o", LIB], check=True)


@pytest.fixture(scope="module")
def hc():
    _build()
    lib = ctypes.CDLL(LIB)
    for f in (lib.hc_fe_ops, lib.hc_ge_ops):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int, ctypes.c_uint32, U32P, U32P, I32P, U32P]
    return lib


def run_cpu(lib, batch):
    """The batch through the CPU build: n x 40 output words."""
    A, B, k = batch.arrays()
    out = np.zeros_like(A)
    fn = lib.hc_fe_ops if batch.op < C.GE_DBL else lib.hc_ge_ops
    rc = fn(batch.op, len(A), A.ctypes.data_as(U32P), B.ctypes.data_as(U32P),
            k.ctypes.data_as(I32P), out.ctypes.data_as(U32P))
    assert rc == 0
    return out


@pytest.mark.parametrize("group", ["mul", "sq", "addsub", "reduce", "eq", "bytes", "pow", "ge"])
def test_limbs_cpu(hc, group):
    """mul: fe_mul over every (first, second) pair of MUL_PAIRS; sq: fe_sq / fe_sqn over
    SQ_INPUTS; addsub: fe_add, fe_sub, fe_sub_nc, fe_neg, fe_neg_nc; reduce: fe_carry,
    fe_canonical, fe_tobytes, fe_iszero, fe_isnegative over every non-canonical form; eq: fe_eq;
    bytes: fe_frombytes; pow: fe_invert, fe_pow22523; ge: ge_dbl and every addition /
    subtraction routine, against the affine law, projectively."""
    total = 0
    for batch in C.fe_batches(group):
        batch.check(run_cpu(hc, batch))
        total += len(batch.cases)
    assert total > 0


def test_unknown_operation_is_refused(hc):
    z = np.zeros((1, 40), np.uint32)
    k = np.zeros(1, np.int32)
    for fn, op in ((hc.hc_fe_ops, 31), (hc.hc_fe_ops, C.GE_DBL), (hc.hc_ge_ops, C.FE_MUL),
                   (hc.hc_ge_ops, 99)):
        assert fn(op, 1, z.ctypes.data_as(U32P), z.ctypes.data_as(U32P), k.ctypes.data_as(I32P),
                  z.ctypes.data_as(U32P)) == -1


def test_generator_forms():
    """The generator's own promises: stuffed forms keep the value and sit at the bound, the
    zero forms denote 0, the points lie on the curve."""
    for name, z in C.ZEROS.items():
        assert C.value(z) % C.P == 0 and C.value(z) != 0, name
    assert C.ZEROS["sub(a,a)"] == C.P_LIMBS      # fe_sub(a, a) leaves exactly the limbs of p
    for bn, bound in C.BOUNDS.items():
        for v in C.VALUES:
            lo, hi = C.stuff(v, bound, low=True), C.stuff(v, bound, low=False)
            for f in (lo, hi):
                assert C.fits(f, bound) and C.value(f) % C.P == v % C.P
                assert C.value(bound) - C.value(f) < C.P          # the largest multiple of p
    assert len(C.points()) >= 18 and C.ed_mul(8, C.points()[1][1]) == C.IDENTITY
    assert C.ed_mul(4, C.points()[1][1]) != C.IDENTITY
    assert C.ed_mul(C.GROUP_L, C.BASE) == C.IDENTITY
