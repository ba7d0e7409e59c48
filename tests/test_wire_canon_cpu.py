"""The device canonicalisation of non-canonical Header / Certificate frames
(narwhal_amd/csrc/nw_wiredec.hpp: canon_stage / canon_mark / canon_rank and emit_lane<true>,
the text k_wire_canon and k_wire_emit run), compiled as host code into
tools/libnw_wirecheck.so, against the Python restatement of the wire format
(tests/test_wire.py, ref_decode: BTreeMap / BTreeSet re-sort, last value wins). Every case runs
at the four byte misalignments and with 1, 16, 64 and 256 lanes; the phases run for every lane
index in a loop, one phase after the other."""
import base64
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from test_wire import _corpus, _pk, ref_decode
from test_wire_device_cpu import check_frame
from cert_cases import mutated_stream, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_wirecheck.so")
SRCS = [os.path.join(ROOT, "tools", "wirecheck.hip"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_wiredec.hpp")]
CANON_MAX = 1024          # wd::kCanonMax
LANES = (1, 16, 64, 256)
NONE, DONE, OVER = 0, 1, 2


@pytest.fixture(scope="module")
def wc():
    if not (os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in SRCS)):
        subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), SRCS[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.wc_scan.argtypes = [ctypes.c_char_p, U64, U32, P]
    lib.wc_scan.restype = ctypes.c_int
    lib.wc_emit.argtypes = [ctypes.c_char_p, U64, U32, U32, P, U64, P, P, P, P, U32, P, P, P]
    lib.wc_emit.restype = ctypes.c_long
    lib.wc_canon.argtypes = [ctypes.c_char_p, U64, U32, U32, P, P, P, U32, P]
    lib.wc_canon.restype = ctypes.c_int
    lib.wc_emit_canon.argtypes = [ctypes.c_char_p, U64, U32, U32, U32, P, U64, P, P, P, P, U32, P, P]
    lib.wc_emit_canon.restype = ctypes.c_long
    return lib


@pytest.fixture(scope="module")
def rec():
    """A valid certificate record (never modified)."""
    _, s, _, _, _ = mutated_stream(N=4, copies=1, seed=11)
    return unpack(s)[0]


def frame(rec, pay, par, variant=2, votes=None):
    """rec's frame with the payload [(key, worker id)] and the parents [key] in the given wire
    order. votes: the serialised votes (count included) instead of rec's."""
    hb = rec["hb"]
    out = (struct.pack("<I", variant) + _pk(hb[:32]) + hb[32:40] + struct.pack("<Q", len(pay))
           + b"".join(k + struct.pack("<I", v) for k, v in pay)
           + struct.pack("<Q", len(par)) + b"".join(par) + rec["id"] + rec["sig"])
    if variant == 2:
        out += votes if votes is not None else (
            struct.pack("<Q", len(rec["votes"])) + b"".join(_pk(p) + s for p, s in rec["votes"]))
    return out


def entries(f):
    """Raw payload [(key, id)] and parents of a frame that decodes."""
    off = 4 + 8 + struct.unpack_from("<Q", f, 4)[0] + 8
    n = struct.unpack_from("<Q", f, off)[0]
    pay = [(f[off + 8 + 36 * i:off + 40 + 36 * i], struct.unpack_from("<I", f, off + 40 + 36 * i)[0])
           for i in range(n)]
    off += 8 + 36 * n
    m = struct.unpack_from("<Q", f, off)[0]
    return pay, [f[off + 8 + 32 * i:off + 40 + 32 * i] for i in range(m)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def check(wc, f, tag, mis=range(4), lanes=LANES, groups=(16,)):
    """One frame through wc_canon and wc_emit_canon against ref_decode. Returns the state."""
    kind, rec = ref_decode(f)
    state = None
    for m in mis:
        r8 = np.zeros(8, np.uint32)
        assert wc.wc_scan(f, len(f), m, _p(r8)) == kind, (tag, m)
        noncanon = kind in (0, 2) and not r8[1]
        for L in lanes:
            t = (tag, m, L)
            cnt, touched = np.zeros(2, np.uint32), np.zeros(1, np.uint32)
            order = np.full(CANON_MAX, 0xFFFFFFFF, np.uint32)
            st = wc.wc_canon(f, len(f), m, L, _p(cnt[0:]), _p(cnt[1:]), _p(order), order.size,
                             _p(touched))
            hb = np.full(max(len(f), 64), 0xEE, np.uint8)
            hid, sig = np.full(32, 0xEE, np.uint8), np.full(64, 0xEE, np.uint8)
            nvmax = len(f) // 72 + 1
            vpk, vsig = np.zeros((nvmax, 32), np.uint8), np.zeros((nvmax, 64), np.uint8)
            pc, off3 = np.zeros(1, np.uint32), np.zeros(3, np.uint64)
            emit = lambda g: wc.wc_emit_canon(f, len(f), m, g, L, _p(hb), hb.size, _p(hid), _p(sig),
                                              _p(vpk), _p(vsig), nvmax, _p(pc), _p(off3))
            assert state in (None, st), t
            state = st
            if not noncanon or int(r8[2]) + int(r8[3]) > CANON_MAX:
                assert st == (OVER if noncanon else NONE) and touched[0] == 0, t
                assert emit(16) == -1, t
                assert (hb == 0xEE).all() and (hid == 0xEE).all() and (sig == 0xEE).all(), t
                assert not vpk.any() and not vsig.any(), t
                continue
            assert st == DONE, t
            assert cnt.tolist() == [rec["np"], rec["nparents"]], t
            assert touched[0] == rec["np"] + rec["nparents"], t
            # the order list by its definition: output position -> the wire entry that supplies it
            pay, par = entries(f)
            last = {k: i for i, (k, _) in enumerate(pay)}
            assert order[:cnt[0]].tolist() == [last[k] for k in sorted(last)], t
            got = [par[i] for i in order[cnt[0]:cnt[0] + cnt[1]]]
            assert got == sorted(set(par)), t
            assert (order[cnt[0] + cnt[1]:] == 0xFFFFFFFF).all(), t
            for g in groups:
                hb[:] = 0xEE
                vpk[:] = 0
                vsig[:] = 0
                n = emit(g)
                assert n == len(rec["hb"]) and hb[:n].tobytes() == rec["hb"], (t, g)
                assert (hb[n:] == 0xEE).all(), (t, g)
                assert hid.tobytes() == rec["id"] and sig.tobytes() == rec["sig"], (t, g)
                nv = len(rec["votes"])
                assert pc[0] == rec["np"] and off3.tolist() == [0, n, nv], (t, g)
                assert [(vpk[j].tobytes(), vsig[j].tobytes()) for j in range(nv)] == rec["votes"], (t, g)
                assert not vpk[nv:].any() and not vsig[nv:].any(), (t, g)
    return state


A, B, C = bytes([1]) * 32, bytes([2]) * 32, bytes([3]) * 32


def parents_of(rec):
    hb = rec["hb"][40 + 36 * rec["np"]:]
    return [hb[i:i + 32] for i in range(0, len(hb), 32)]


def test_small_cases(wc, rec):
    par = parents_of(rec)
    assert len(par) >= 2 and par == sorted(par)
    z = lambda *ks: [(k, 0) for k in ks]
    cases = {
        "1 two reversed": (z(B, A), par),
        "2 equal keys, last wins": ([(A, 7), (A, 1)], par),
        "3 A B A": ([(A, 7), (B, 2), (A, 3)], par),
        "4 five equal": ([(A, v) for v in (5, 4, 9, 0, 6)], par),
        "5 equal parents": (z(A, B), [par[0], par[0]]),
        "6 parents reversed": (z(A, B), par[::-1]),
        "7 parents only": (z(A, B, C), [par[1], par[0]] + par[2:]),
        "8 payload only": (z(C, A, B), par),
    }
    for tag, (pay, pr) in cases.items():
        f = frame(rec, pay, pr)
        assert check(wc, f, tag, groups=(1, 16, 64)) == DONE, tag
    # the values that survive, spelled out (ref_decode is the reference; this pins the rule)
    assert ref_decode(frame(rec, [(A, 7), (B, 2), (A, 3)], par))[1]["hb"][40:40 + 72] == \
        A + struct.pack("<I", 3) + B + struct.pack("<I", 2)


def test_compare_is_bytewise_unsigned_big_endian(wc, rec):
    """9, 10: a little-endian word compare or a signed compare orders these wrongly."""
    def k(**at):
        b = bytearray(32)
        for i, v in at.items():
            b[int(i[1:])] = v
        return bytes(b)
    groups = [
        [k(b0=2), k(b0=1)],                        # differ only in byte 0
        [k(b31=2), k(b31=1)],                      # only in byte 31
        [k(b3=1), k(b4=1)],                        # byte 3 against byte 4 (two words)
        [k(b3=1, b0=0), k(b0=1)],                  # byte 3 against byte 0 (one word: endianness)
        [k(b0=0x80), k(b0=0x7F)],                  # signed bytes
        [k(b3=0x80), k(b3=0x7F)],                  # signed words, little-endian top byte
        [k(b4=0x80), k(b4=0x7F, b7=0xFF)],
        [k(b28=0x80), k(b31=0x80), k(b28=0x7F, b31=0xFF)],
    ]
    for i, ks in enumerate(groups):
        for order in (ks, ks[::-1], sorted(ks)[::-1]):
            pay = [(x, j) for j, x in enumerate(order)]
            if order != sorted(order):
                assert check(wc, frame(rec, pay, parents_of(rec)), ("pay", i)) == DONE
                assert check(wc, frame(rec, [], list(order)), ("par", i)) == DONE
            else:   # sorted and distinct: canonical, nothing to do
                assert check(wc, frame(rec, pay, parents_of(rec)), ("pay", i), lanes=(16,)) == NONE


@pytest.mark.parametrize("n", [65, 257, 1018])
def test_many_parents_cross_the_lane_strides(wc, rec, n):
    """11: random order; 1,018 is the largest count a frame under the default cap can hold."""
    rng = np.random.default_rng(n)
    par = [rng.bytes(32) for _ in range(n)]
    par[n // 2] = par[3]                                    # one duplicate, far apart
    f = frame(rec, [(B, 0), (A, 0)], par, variant=0)
    if n == 1018:
        # 1018 = (32768 - 176) / 32 with nothing else in the frame: an empty payload
        f = frame(rec, [], par, variant=0)
        assert len(f) <= 32768 < len(frame(rec, [], par + [A], variant=0))
    assert check(wc, f, n, groups=(64,)) == DONE


def test_over_the_bound_writes_nothing(wc, rec):
    """12: kCanonMax + 1 entries."""
    rng = np.random.default_rng(12)
    par = [rng.bytes(32) for _ in range(CANON_MAX)]
    f = frame(rec, [(A, 0)], par)
    assert ref_decode(f)[0] == 2
    assert check(wc, f, "max+1") == OVER
    # at the bound itself the device still does it
    assert check(wc, frame(rec, [(A, 0)], par[1:]), "max") == DONE
    # and split over both sections
    pay = [(rng.bytes(32), i) for i in range(500)]
    assert check(wc, frame(rec, pay, par[:524]), "500+524") == DONE
    assert check(wc, frame(rec, pay, par[:525]), "500+525") == OVER


def mixed_votes(rec):
    """Votes whose key texts differ in length (one unpadded, 43 characters): vlen == 0."""
    assert len(rec["votes"]) >= 3
    return struct.pack("<Q", len(rec["votes"])) + b"".join(
        (struct.pack("<Q", 43) + base64.b64encode(p)[:43] if j == 1 else _pk(p)) + sg
        for j, (p, sg) in enumerate(rec["votes"]))


def test_header_variant_and_walked_votes(wc, rec):
    """13."""
    par = parents_of(rec)
    pay = [(C, 1), (A, 2), (B, 3), (A, 0)]
    assert check(wc, frame(rec, pay, par[::-1] + par[:1], variant=0), "header") == DONE
    f = frame(rec, pay, par[::-1] + par[:1], votes=mixed_votes(rec))
    r8 = np.zeros(8, np.uint32)
    assert wc.wc_scan(f, len(f), 0, _p(r8)) == 2 and r8[6] == 0 and r8[4] >= 3
    assert check(wc, f, "walk", groups=(1, 16, 64)) == DONE
    assert check(wc, frame(rec, pay, par, votes=struct.pack("<Q", 0)), "nv0") == DONE


def test_every_truncation(wc, rec):
    """14: the kind is ref_decode's at every length, and nothing is emitted for kind -1."""
    par = parents_of(rec)
    f = frame(rec, [(B, 1), (A, 2), (B, 0)], par[::-1])
    assert ref_decode(f)[0] == 2
    states = [check(wc, f[:k], k) for k in range(len(f) + 1)]
    assert states[-1] == DONE and NONE in states
    # the reordered frame decodes from the end of its last vote on: those lengths, and only
    # those, are canonicalised
    first = states.index(DONE)
    assert states[first:] == [DONE] * (len(f) + 1 - first) and ref_decode(f[:first - 1])[0] == -1


def test_random_campaign(wc, rec):
    rng = np.random.default_rng(2024)
    done = 0
    for i in range(300):
        def section(n):
            pool = [rng.bytes(32) for _ in range(max(1, n - int(rng.integers(0, 4))))]
            ks = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
            if n >= 2 and rng.integers(0, 3) == 0:   # near-equal keys: one byte apart
                b = bytearray(ks[0])
                b[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
                ks[1] = bytes(b)
            return ks
        pay = [(k, int(rng.integers(0, 5))) for k in section(int(rng.integers(0, 13)))]
        par = section(int(rng.integers(0, 13)))
        f = frame(rec, pay, par, variant=(0, 2)[i % 2])
        done += check(wc, f, i, mis=(i % 4,), groups=((1, 16, 64)[i % 3],)) == DONE
    assert done >= 200


def test_scan_and_emit_unchanged(wc):
    """wc_scan / wc_emit over the existing corpus, as tests/test_wire_device_cpu.py asserts
    them: the canonical bit, the raw counts, and no emit for a non-canonical frame."""
    _, frames = _corpus(N=4, copies=2)
    out = [check_frame(wc, f, i, mis=i % 4) for i, f in enumerate(frames)]
    assert sum(k in (0, 2) and not c for k, c in out) == 1
    # that one frame (duplicate key, parents out of order) is this file's business
    i = [j for j, (k, c) in enumerate(out) if k in (0, 2) and not c][0]
    assert check(wc, frames[i], "dup") == DONE
