"""The field, point and limb-parallel arithmetic on RAW limbs on the MI355X
(tools/libnw_lpcheck.so: k_fe_ops, one lane per case, and k_lp_ops, one wave per case).

k_fe_ops runs tests/limb_cases.py's per-lane batches on the device build of nw_field.hpp /
nw_point.hpp (real v_mad_u64_u32 chains behind their asm barrier): the output must equal the
CPU build's limb for limb (tests/test_field_limbs_cpu.py) and Python's mod p.

k_lp_ops runs nw_lp.hpp (DPP rotates, row_newbcast, permlane16/32_swap), which no CPU build
can check: every operand pair of the limb-parallel bounds model at its maxima, one-hot pairs
(each of the 100 product terms alone in its column, so the second rotate vector of terms
j >= 7 and the x19 of lane 0's carry stand alone), the group law against the affine law,
k_pip_final's doubling chain with the largest limb it ever holds, lanes 10..15, the neg branch
of lp_niels_component and lp_is_identity's non-canonical forms. All comparisons are exact.
Every batch runs at block size 64 and at 256 (lane = tid & 63), the product's two ways."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import limb_cases as C
from test_field_limbs_cpu import hc, run_cpu  # noqa: F401  (the CPU build of the same text)

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
    lib.lpc_fe_ops.restype = ctypes.c_int
    lib.lpc_fe_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, U32P, U32P, I32P, U32P, ctypes.c_int]
    lib.lpc_lp_ops.restype = ctypes.c_int
    lib.lpc_lp_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, U32P, I32P, U32P, ctypes.c_int]
    return lib


def run_fe(lib, batch, block):
    A, B, k = batch.arrays()
    out = np.zeros_like(A)
    rc = lib.lpc_fe_ops(batch.op, len(A), A.ctypes.data_as(U32P), B.ctypes.data_as(U32P),
                        k.ctypes.data_as(I32P), out.ctypes.data_as(U32P), block)
    assert rc == 0, f"lpc_fe_ops: status {rc}"
    return out


def run_lp(lib, batch, block, garbage=False):
    A, k = batch.arrays(garbage)
    out = np.zeros_like(A)
    rc = lib.lpc_lp_ops(batch.op, len(A), A.ctypes.data_as(U32P), k.ctypes.data_as(I32P),
                        out.ctypes.data_as(U32P), block)
    assert rc == 0, f"lpc_lp_ops: status {rc}"
    return out


@pytest.mark.parametrize("group", ["mul", "sq", "addsub", "reduce", "eq", "bytes", "pow", "ge"])
def test_fe_ops_gpu(lpc, hc, group):  # noqa: F811
    for batch in C.fe_batches(group):
        cpu = run_cpu(hc, batch)
        for block in BLOCKS:
            gpu = run_fe(lpc, batch, block)
            bad = np.flatnonzero((gpu != cpu).any(axis=1))
            assert bad.size == 0, (batch.cases[bad[0]][0], gpu[bad[0]].tolist(), cpu[bad[0]].tolist())
            batch.check(gpu)


LIVE = np.array([(lane & 15) < 10 for lane in range(64)] * 4)


@pytest.mark.parametrize("group", ["mul", "carry_sub", "moves", "points", "components",
                                   "identity", "pow", "chain"])
def test_lp_ops_gpu(lpc, group):
    """mul: lp_mul over every pair of the limb-parallel bounds model; carry_sub: lp_carry32,
    lp_sub, lp_sub_nc; moves: lp_rows_of, lp_sel, lp_identity; points: lp_dbl, lp_add,
    lp_to_cached; components: lp_cached_component, lp_niels_component (both signs); identity:
    lp_is_identity; pow: lp_sqn, lp_pow22523; chain: k doublings and one addition, k = 1, 8,
    248, with the per-lane maximum over the chain. Each check (tests/limb_cases.py): the rows'
    values or the projective point against Python, every live limb <= T_LP, lanes 10..15 zero.
    With the inputs' lanes 10..15 filled with garbage the whole output must not change for the
    operations that ignore them; the lane-wise ones (lp_rows_of, lp_sel, lp_sub_nc) pass them
    through, so their live lanes must not change (nw_lp.hpp states both)."""
    for batch in C.lp_batches(group):
        ref = run_lp(lpc, batch, 64)
        batch.check(ref)
        assert np.array_equal(run_lp(lpc, batch, 256), ref), "block size 256 differs from 64"
        for block in BLOCKS:
            dirty = run_lp(lpc, batch, block, garbage=True)
            if batch.op in C.IGNORES_DEAD:
                assert np.array_equal(dirty, ref), "lanes 10..15 of an input leak into the result"
            else:
                assert np.array_equal(dirty[:, LIVE], ref[:, LIVE]), "live lanes changed"


def test_lp_bad_arguments(lpc):
    z = np.zeros((1, 256), np.uint32)
    k = np.zeros(1, np.int32)
    args = (z.ctypes.data_as(U32P), k.ctypes.data_as(I32P), z.ctypes.data_as(U32P))
    assert lpc.lpc_lp_ops(99, 1, *args, 64) == -1
    assert lpc.lpc_lp_ops(C.LP_MUL, 1, *args, 96) == -1
    assert lpc.lpc_lp_ops(C.LP_MUL, 0, *args, 64) == -1
