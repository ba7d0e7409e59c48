"""The host side of a verify_batch call, compiled as host code into tools/libnw_batchcheck.so
(tools/batchcheck.hip) and run without a GPU: the refusal rules of nw_batch_call.hpp against a
restatement of the rules as they stood, spread over three functions, before that header; the batch
job's section plan (nw_stage.hpp plan_batch) against the 256-byte rule and section order of the
two jobs it replaced; and pack_messages against numpy."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_batchcheck.so")
SRCS = [os.path.join(ROOT, "tools", "batchcheck.hip"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_batch_call.hpp"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_stage.hpp")]
P, U64, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(scope="module")
def bc():
    if not (os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in SRCS)):
        subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), SRCS[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    lib.bc_check.argtypes = [I, I, U64, ctypes.c_double, I, I, I, I, ctypes.c_long, I, I, I, U64,
                             U64, I]
    lib.bc_check.restype = I
    lib.bc_defaults.argtypes = [P, P, P]
    lib.bc_plan.argtypes = [U64, U64, ctypes.c_longlong, I, I, U64, U64, P]
    lib.bc_pack.argtypes = [P, P, P, P, P, U64]
    lib.bc_pack.restype = U64
    return lib


# ---- the refusal rules ---------------------------------------------------------------------
def call(keys=False, skip=False, spg=0, frac=1.0, skip_pip=False, votes=False, kplane=False,
         fuse_ctr=False, gate=None, done=False, gate_ok=False, direct=False, nbatches=1, nitems=1,
         digests=True):
    return dict(keys=keys, skip=skip, spg=spg, frac=frac, skip_pip=skip_pip, votes=votes,
                kplane=kplane, fuse_ctr=fuse_ctr, gate=gate, done=done, gate_ok=gate_ok,
                direct=direct, nbatches=nbatches, nitems=nitems, digests=digests)


def check(bc, c):
    return bc.bc_check(c["keys"], c["skip"], c["spg"], c["frac"], c["skip_pip"], c["votes"],
                       c["kplane"], c["fuse_ctr"], -1 if c["gate"] is None else c["gate"],
                       c["done"], c["gate_ok"], c["direct"], c["nbatches"], c["nitems"],
                       c["digests"])


def refused_before(c):
    """The rules of the commit before nw_batch_call.hpp (8bc0cab), in its order, for a plain
    (non-group) call; line numbers are that commit's narwhal_amd/csrc/nw_batch.hip."""
    gate = c["gate"] is not None
    if c["kplane"]:
        # launch_verify_batch_msgs, the only way to a call over the plane
        if c["fuse_ctr"] or gate or c["done"]:                              # :2850
            return True
        if c["nbatches"] != 0 and c["nitems"] and not c["digests"]:         # :2851-2852 (kplane)
            return True
    # verify_batch_run
    if c["kplane"] and (c["keys"] or c["fuse_ctr"] or gate or c["done"] or c["frac"] < 1.0 or
                        (c["skip"] and not c["skip_pip"])):                 # :2674-2676
        return True
    if c["skip_pip"] and (not c["skip"] or c["fuse_ctr"] or gate or c["done"]):   # :2678
        return True
    if c["votes"] and (not c["skip_pip"] or c["spg"] != 1 or c["keys"] or c["frac"] < 1.0 or
                       c["nitems"] > 0xffffffff):                           # :2681-2683
        return True
    if gate and not c["gate_ok"]:                                           # :2686
        return True
    if gate and (c["gate"] == 0 or c["gate"] % 64 != 0):                    # :2687
        return True
    if c["done"] and not c["direct"]:                                       # :2688
        return True
    # launch_pip, group == false
    if c["kplane"] and (gate or c["done"]):                                 # :2549
        return True
    return False


def test_refusal_matrix(bc):
    tf = (False, True)
    n = 0
    for (keys, skip, spg, frac, skip_pip, votes, kplane, fuse_ctr, gate, done, gate_ok, direct,
         nitems) in itertools.product(tf, tf, (0, 1, 2), (1.0, 0.5), tf, tf, tf, tf,
                                      (None, 64, 0, 96), tf, tf, tf, (1, 2**32)):
        c = call(keys, skip, spg, frac, skip_pip, votes, kplane, fuse_ctr, gate, done, gate_ok,
                 direct, 1, nitems)
        assert check(bc, c) == (INVALID if refused_before(c) else 0), c
        n += 1
    assert n == 2**11 * 12


def test_refusal_missing_plane(bc):
    """A call over the plane without one: refused once it has a batch and a vote."""
    for kplane, nbatches, nitems, digests in itertools.product((False, True), (0, 1), (0, 5),
                                                               (False, True)):
        c = call(kplane=kplane, nbatches=nbatches, nitems=nitems, digests=digests)
        assert check(bc, c) == (INVALID if refused_before(c) else 0), c
    assert check(bc, call(kplane=True, nbatches=1, nitems=5, digests=False)) == INVALID


CALLERS = {
    # nw_jobs.cpp submit_batch
    "digest job, plain": call(nbatches=3, nitems=15),
    "digest job, fused": call(fuse_ctr=True, done=True, gate_ok=True, direct=True, nitems=10000),
    "digest job, fused, NW_BATCH_SPIN=0": call(fuse_ctr=True, direct=True, nitems=10000),
    "digest job, gated": call(fuse_ctr=True, gate=1024, done=True, gate_ok=True, direct=True,
                              nitems=10000),
    "digest job, signers, vote list": call(skip=True, spg=1, skip_pip=True, votes=True,
                                           nbatches=3, nitems=15),
    "digest job, signers, no vote list": call(skip=True, spg=1, skip_pip=True, nbatches=3,
                                              nitems=15),
    "digest job, signers, lone large batch": call(skip=True, spg=1, skip_pip=True, votes=True,
                                                  gate_ok=True, direct=True, nitems=10000),
    "message job": call(kplane=True, nbatches=3, nitems=15),
    "message job, lone large batch": call(kplane=True, gate_ok=True, direct=True, nitems=10000),
    "message job, signers, vote list": call(kplane=True, skip=True, spg=1, skip_pip=True,
                                            votes=True, nbatches=3, nitems=15),
    "message job, signers, no vote list": call(kplane=True, skip=True, spg=1, skip_pip=True,
                                               nbatches=3, nitems=15),
    # nw_api.cpp
    "nw_dev_verify_batch_many": call(nbatches=3, nitems=15),
    "nw_dev_verify_batch_many, lone large batch": call(gate_ok=True, direct=True, nitems=10000),
    "nw_dev_verify_batch_msgs_many": call(kplane=True, nbatches=3, nitems=15),
    "nw_dev_verify_batch_msgs_many, no votes": call(kplane=True, nbatches=2, nitems=0),
    "certificates, K, keyed": call(keys=True, skip=True, spg=7, frac=0.05, nbatches=100,
                                   nitems=6700),
    "certificates, K, merged groups": call(skip=True, spg=32, nbatches=100, nitems=6700),
    "certificates, K = 0": call(nbatches=100, nitems=6700),
}


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_callers_accepted(bc, name):
    assert not refused_before(CALLERS[name])
    assert check(bc, CALLERS[name]) == 0


def test_option_defaults(bc):
    """batch_call_t's options default to what the launchers' default arguments were: no keys, no
    skip list, skip_per_group 0, active_frac 1.0, no skip_pip, votes, kplane, fuse_ctr, gate, done."""
    spg, frac, flags = U64(7), ctypes.c_double(0), (I * 8)(*([1] * 8))
    bc.bc_defaults(ctypes.byref(spg), ctypes.byref(frac), flags)
    assert (spg.value, frac.value, list(flags)) == (0, 1.0, [0] * 8)


# ---- the batch job's sections --------------------------------------------------------------
SECTIONS = ["data", "mo", "ml", "d", "off", "pk", "sig", "z", "st", "fi", "dn", "ct", "ws", "kp",
            "sg", "end"]
SHAPES = [(1, 0), (1, 1), (3, 7), (1, 10000), (9000, 270000)]


def a256(x):
    return (x + 255) // 256 * 256


def plan(bc, nbatches, nitems, msg_bytes, z16, signers, ws_bytes, sg_bytes):
    out = (U64 * 16)()
    bc.bc_plan(nbatches, nitems, -1 if msg_bytes is None else msg_bytes, z16, signers, ws_bytes,
               sg_bytes, out)
    return dict(zip(SECTIONS, out))


@pytest.mark.parametrize("nbatches,nitems", SHAPES)
@pytest.mark.parametrize("z16", (False, True))
@pytest.mark.parametrize("signers", (False, True))
def test_plan_digest_call(bc, nbatches, nitems, z16, signers):
    """Every offset as submit_batch computed it before the plan function (nw_jobs.cpp:566-574 of
    8bc0cab): inputs contiguous in [0, o_st), the flags' place o_st, the done word at o_dn."""
    ws_bytes, sg_bytes = 40 * nitems + 1234567, 12 * nitems + 777
    m = nitems or 1
    o_d = 0
    o_off = o_d + a256(32 * nbatches)
    o_pk = o_off + a256(8 * (nbatches + 1))
    o_sig = o_pk + a256(32 * m)
    o_z = o_sig + a256(64 * m)
    o_st = o_z + (a256(16 * m) if z16 else 0)
    o_fi = o_st + a256(4 * nbatches)
    o_dn = o_fi + a256(8 * nbatches)
    o_ct = o_dn + 256
    o_ws = o_ct + (256 if signers else 0)
    o_sg = o_ws + a256(ws_bytes)
    end = o_sg + (a256(sg_bytes) if signers else 0)
    p = plan(bc, nbatches, nitems, None, z16, signers, ws_bytes, sg_bytes if signers else 0)
    got = {k: p[k] for k in ("d", "off", "pk", "sig", "z", "st", "fi", "dn", "ct", "ws", "sg", "end")}
    assert got == dict(d=o_d, off=o_off, pk=o_pk, sig=o_sig, z=o_z, st=o_st, fi=o_fi, dn=o_dn,
                       ct=o_ct, ws=o_ws, sg=o_sg, end=end)
    assert p["kp"] == p["sg"]   # no plane: an empty section


@pytest.mark.parametrize("nbatches,nitems", SHAPES)
@pytest.mark.parametrize("z16", (False, True))
@pytest.mark.parametrize("signers", (False, True))
@pytest.mark.parametrize("per_msg", (0, 1, 113))
def test_plan_message_call(bc, nbatches, nitems, z16, signers, per_msg):
    ws_bytes, sg_bytes = 40 * nitems + 1234567, 12 * nitems + 777
    msg_bytes = per_msg * nitems
    m = nitems or 1
    p = plan(bc, nbatches, nitems, msg_bytes, z16, signers, ws_bytes, sg_bytes if signers else 0)
    # the sections a message call has, with the bytes each must hold, in buffer order
    want = [("data", max(msg_bytes, 1)), ("mo", 8 * m), ("ml", 8 * m), ("off", 8 * (nbatches + 1)),
            ("pk", 32 * m), ("sig", 64 * m)]
    want += [("z", 16 * m)] if z16 else []
    inputs = len(want)
    want += [("st", 4 * nbatches), ("fi", 8 * nbatches)]
    want += [("ct", 8 * 6)] if signers else []
    outputs = len(want)
    want += [("ws", ws_bytes), ("kp", 32 * max(nitems, 1))]
    want += [("sg", sg_bytes)] if signers else []
    order = sorted(want, key=lambda s: p[s[0]])
    assert order == want
    assert p[want[0][0]] == 0
    for (name, nbytes), (nxt, _) in zip(want, want[1:] + [("end", 0)]):
        assert p[name] % 256 == 0
        assert p[name] + nbytes <= p[nxt], (name, nxt)        # disjoint
        assert p[nxt] - p[name] == a256(nbytes), (name, nxt)   # and no gap beyond the alignment
    # H2D = the inputs = [0, st); D2H = the outputs = [st, ws); plane and scratch device-only
    assert p[want[inputs][0]] == p["st"] and p[want[outputs][0]] == p["ws"]
    assert p["kp"] >= p["ws"] and p["sg"] >= p["kp"] + 32 * max(nitems, 1)
    assert p[want[-1][0]] == (p["sg"] if signers else p["kp"])   # the comb scratch is last
    assert p["dn"] == p["ct"]   # no done word: a message call never spins


# ---- pack_messages -------------------------------------------------------------------------
PACK_CASES = {
    "empty set": (0, [], []),
    "all empty, no data": (0, [0, 5, 9], [0, 0, 0]),
    "one run": (60, [0, 10, 30, 30], [10, 20, 0, 30]),
    "alternating gaps": (64, [0, 12, 20, 40, 63], [8, 8, 10, 3, 1]),
    "reversed": (40, [30, 20, 10, 0], [10, 10, 10, 10]),
    "overlapping": (32, [0, 4, 4, 0, 16], [16, 16, 28, 32, 16]),
}


@pytest.mark.parametrize("name", sorted(PACK_CASES))
def test_pack_messages(bc, name):
    nbytes, offsets, lengths = PACK_CASES[name]
    data = np.random.Generator(np.random.PCG64(18)).integers(0, 256, size=nbytes, dtype=np.uint8)
    offs, lens = np.array(offsets, np.uint64), np.array(lengths, np.uint64)
    want = np.concatenate([data[o:o + n] for o, n in zip(offsets, lengths)] +
                          [np.zeros(0, np.uint8)])
    want_offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if lengths else lens
    got = np.full(len(want) + 8, 0xEE, np.uint8)
    got_offs = np.full(len(offs) + 1, 2**64 - 1, np.uint64)
    total = bc.bc_pack(got.ctypes.data, got_offs.ctypes.data, data.ctypes.data if nbytes else None,
                       offs.ctypes.data, lens.ctypes.data, len(offs))
    assert total == len(want)
    assert np.array_equal(got[:total], want) and np.all(got[total:] == 0xEE)
    assert np.array_equal(got_offs[:-1], want_offs) and got_offs[-1] == 2**64 - 1


def test_pack_messages_sanitized():
    """tools/batchcheck.hip with its main under AddressSanitizer / UBSan (`make batchsan`), as a
    stand-alone program: the same cases over exactly sized buffers."""
    subprocess.run(["make", "-s", "-C", ROOT, "batchsan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "batch_san")], capture_output=True, text=True)
    assert r.returncode == 0 and "batchcheck ok" in r.stdout, r.stdout + r.stderr
