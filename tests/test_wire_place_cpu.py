"""The host's placement of a device-decode call's frames (narwhal_amd/csrc/nw_wireplace.hpp:
step 3 of wire_verify_device) and the frame-layout check it shares with the emit
(nw_wiredec.hpp: header_layout / vote_layout), compiled as host code into
tools/libnw_wirecheck.so. The records come from wc_scan / wc_canon over real frames of N = 4;
the rejection paths take forged records, which the scan itself never produces: one field of a
good record changed. The same forged records then go through the emit (wc_emit_rec) over
pre-filled buffers: a record that does not fit its frame writes nothing."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from test_wire import _pk, cert_frame, vote_frame
from test_wire_canon_cpu import A, B, frame, parents_of
from cert_cases import mutated_stream, unpack, votes_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_wirecheck.so")
SRCS = [os.path.join(ROOT, "tools", "wirecheck.hip"),
        os.path.join(ROOT, "tools", "wire_single.hpp"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_wiredec.hpp"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_wireplace.hpp")]
NO_SLOT = 0xFFFFFFFF               # wd::kNoSlot
OVER_CAP = -2                      # wd::kOverCap
DONE, OVER = 1, 2                  # wd::kCanonDone, kCanonOver
SERIALIZATION = 21                 # NW_DAG_SERIALIZATION
KIND, CANONICAL, NP, NQ, NV, ALEN, VLEN = range(7)   # words of wd::rec_t
DST = np.dtype([("hb_off", "<u8"), ("slot", "<u4"), ("vote0", "<u4")])   # wd::dst_t
ONES64 = 2**64 - 1


@pytest.fixture(scope="module")
def wc():
    if not (os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in SRCS)):
        subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), SRCS[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.wc_scan.argtypes = [ctypes.c_char_p, U64, U32, P]
    lib.wc_scan.restype = ctypes.c_int
    lib.wc_canon.argtypes = [ctypes.c_char_p, U64, U32, U32, P, P, P, U32, P]
    lib.wc_canon.restype = ctypes.c_int
    lib.wc_emit.argtypes = [ctypes.c_char_p, U64, U32, U32, P, U64, P, P, P, P, U32, P, P, P]
    lib.wc_emit.restype = ctypes.c_long
    lib.wc_emit_rec.argtypes = [ctypes.c_char_p, U64, U32, U32, P, P, P, U64, P, P, P, P, U32, P, P, P]
    lib.wc_emit_rec.restype = ctypes.c_long
    lib.wc_place.argtypes = [P, P, P, U64, U64, U64, P, P, P, P, P, P, P, P]
    lib.wc_place.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def frames():
    """A header, a certificate, a vote and a non-canonical certificate of N = 4 (never
    modified): the certificate's payload and parents, the latter reversed and the former with
    a duplicate key in front."""
    _, s, _, _, _ = mutated_stream(N=4, copies=1, seed=11)
    rec = unpack(s)[0]
    _, vp, _, _ = votes_case(4)
    par = parents_of(rec)
    assert len(par) >= 2 and len(rec["votes"]) >= 3
    return {"rec": rec, "header": cert_frame(rec, 0), "cert": cert_frame(rec),
            "vote": vote_frame(vp, 0), "noncanon": frame(rec, [(B, 1), (A, 2), (B, 0)], par[::-1])}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def scan(wc, f):
    r8 = np.zeros(8, np.uint32)
    wc.wc_scan(f, len(f), 0, _p(r8))
    return r8


def canon(wc, f):
    """The frame's wd::canon_t as k_wire_canon writes it: np_u, nq_u, state, 0."""
    cnt, touched = np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    order = np.zeros(1024, np.uint32)
    st = wc.wc_canon(f, len(f), 0, 64, _p(cnt[0:]), _p(cnt[1:]), _p(order), order.size, _p(touched))
    assert st >= 0
    return np.array([cnt[0], cnt[1], st, 0] if st == DONE else [0, 0, st, 0], np.uint32)


def with_(r8, **fields):
    """r8 with words replaced: with_(r, NP=5)."""
    out = r8.copy()
    for name, v in fields.items():
        out[globals()[name]] = v & 0xFFFFFFFF
    return out


def hl(np_, nq):
    return 40 + 36 * int(np_) + 32 * int(nq)


def need(r8):
    """Frame bytes a record claims (the layout functions' sums)."""
    r = [int(x) for x in r8]
    if r[KIND] == 1:
        return 124 + r[ALEN] + r[VLEN]
    return 132 + r[ALEN] + 36 * r[NP] + 32 * r[NQ] + (8 + 72 * r[NV] if r[KIND] == 2 else 0)


def place(wc, recs, lens, cans=None, total=None, vbound=None):
    """wc_place over the records; total / vbound default to what the job derives from the
    frames. kind / status / index start from values the placement never writes."""
    n = len(recs)
    R = np.ascontiguousarray(np.array(recs, np.uint32).reshape(n, 8))
    Cn = None if cans is None else np.ascontiguousarray(np.array(cans, np.uint32).reshape(n, 4))
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)   # laid end to end
    total = int(fo[-1]) if total is None else total
    vbound = total // 72 if vbound is None else vbound
    dst = np.zeros(n, DST)
    totals, cvo, host, cnt = (np.zeros(7, np.uint64), np.zeros(n + 1, np.uint64),
                              np.zeros(n, np.uint64), np.zeros(2, np.uint64))
    kind, status, index = np.full(n, 99, np.int32), np.full(n, -77, np.int32), np.full(n, ONES64, np.uint64)
    err = wc.wc_place(_p(R), _p(Cn), _p(fo), n, total, vbound, _p(dst), _p(totals), _p(cvo),
                      _p(host), _p(cnt), _p(kind), _p(status), _p(index))
    return {"err": None if err is None else err.decode(), "dst": dst,
            "totals": [int(x) for x in totals], "cvo": cvo[:int(cnt[0])].tolist(),
            "host": host[:int(cnt[1])].tolist(), "kind": kind.tolist(), "status": status.tolist(),
            "index": index.tolist()}


def test_mixed_stream(wc, frames):
    rec = frames["rec"]
    request = struct.pack("<IQ", 3, 2) + bytes(64) + _pk(rec["hb"][:32])
    fs = [frames["header"], frames["vote"], frames["cert"], request, frames["cert"][:50],
          frames["noncanon"], frames["cert"], frames["cert"]]
    recs = [scan(wc, f) for f in fs]
    recs[7] = np.array([OVER_CAP & 0xFFFFFFFF, 0, 0, 0, 0, 0, 0, 0], np.uint32)   # as k_wire_scan marks it
    assert [int(r[KIND].astype(np.int32)) for r in recs] == [0, 1, 2, 3, -1, 2, 2, OVER_CAP]
    assert [int(r[CANONICAL]) for r in recs[:7]] == [1, 1, 1, 1, 0, 0, 1]
    cans = [canon(wc, f) for f in fs]
    assert [int(c[2]) for c in cans] == [0, 0, 0, 0, 0, DONE, 0, 0]
    npp, nq, nv = rec["np"], len(parents_of(rec)), len(rec["votes"])
    assert recs[5][NP] == 3 and cans[5].tolist() == [2, nq, DONE, 0]
    full, kept = hl(npp, nq), hl(2, nq)
    lens = [len(f) for f in fs]

    on = place(wc, recs, lens, cans)
    assert on["err"] is None
    assert on["dst"]["slot"].tolist() == [0, 0, 0, NO_SLOT, NO_SLOT, 1, 2, NO_SLOT]
    assert on["dst"]["hb_off"].tolist() == [0, 0, 0, 0, 0, full, full + kept, 0]
    assert on["dst"]["vote0"].tolist() == [0, 0, 0, 0, 0, nv, 2 * nv, 0]
    assert on["totals"] == [1, 3, full, 2 * full + kept, 1, 3 * nv, 1]
    assert on["cvo"] == [0, nv, 2 * nv, 3 * nv]
    assert on["host"] == [7]
    # no device check follows for the request and the frame that does not decode: the verdict
    assert (on["kind"][3], on["status"][3], on["index"][3]) == (3, 0, 0)
    assert (on["kind"][4], on["status"][4], on["index"][4]) == (-1, SERIALIZATION, 0)
    assert on["kind"][:3] + on["kind"][5:7] == [0, 1, 2, 2, 2]
    # the host's frame is not written
    assert (on["kind"][7], on["status"][7], on["index"][7]) == (99, -77, ONES64)

    off = place(wc, recs, lens, None)
    assert off["err"] is None
    assert off["dst"]["slot"].tolist() == [0, 0, 0, NO_SLOT, NO_SLOT, NO_SLOT, 1, NO_SLOT]
    assert off["dst"]["hb_off"].tolist() == [0, 0, 0, 0, 0, 0, full, 0]
    assert off["dst"]["vote0"].tolist() == [0, 0, 0, 0, 0, 0, nv, 0]
    assert off["totals"] == [1, 2, full, 2 * full, 1, 2 * nv, 0]
    assert off["cvo"] == [0, nv, 2 * nv]
    assert off["host"] == [5, 7]
    assert (off["kind"][3], off["status"][3], off["index"][3]) == (3, 0, 0)
    assert (off["kind"][4], off["status"][4], off["index"][4]) == (-1, SERIALIZATION, 0)
    for i in (5, 7):
        assert (off["kind"][i], off["status"][i], off["index"][i]) == (99, -77, ONES64)
    # a frame over the canonicalisation's bound goes to the host like one over the cap
    cans[5] = np.array([0, 0, OVER, 0], np.uint32)
    assert place(wc, recs, lens, cans)["host"] == [5, 7]


FIT_CASES = [("header", "ALEN", 1), ("header", "NP", 36), ("header", "NQ", 32),
             ("cert", "ALEN", 1), ("cert", "NP", 36), ("cert", "NQ", 32), ("cert", "NV", 72),
             ("vote", "ALEN", 1), ("vote", "VLEN", 1)]


def forge_fit(wc, frames, which, field, step):
    """-> (frame, fits, forged): `field` of the frame's own record raised to the largest value
    that still fits the frame, and one step further, which is one byte too many. The frame is
    padded with trailing bytes (which the format allows) until exactly that holds."""
    f = frames[which]
    r = scan(wc, f)
    assert need(r) <= len(f)
    k = (len(f) - need(r)) // step + 1
    w = globals()[field]
    forged = with_(r, **{field: int(r[w]) + k})
    f = f + bytes(need(forged) - 1 - len(f))
    assert scan(wc, f).tolist() == r.tolist()           # still the same frame to the scan
    fits = with_(r, **{field: int(r[w]) + k - 1})
    assert need(fits) <= len(f) == need(forged) - 1
    return f, fits, forged


@pytest.mark.parametrize("which,field,step", FIT_CASES)
def test_forged_record_does_not_fit(wc, frames, which, field, step):
    f, fits, forged = forge_fit(wc, frames, which, field, step)
    name = "vote record" if which == "vote" else "header record"
    good = place(wc, [fits], [len(f)])
    assert good["err"] is None and good["dst"]["slot"].tolist() == [0]
    bad = place(wc, [fits, forged], [len(f), len(f)])
    assert bad["err"] == name
    assert bad["dst"]["slot"][0] == 0                   # the neighbour was placed before it
    assert place(wc, [forged], [len(f)])["err"] == name


def test_forged_canon_record(wc, frames):
    f = frames["noncanon"]
    r, c = scan(wc, f), canon(wc, f)
    npp, nq = int(r[NP]), int(r[NQ])
    assert c[2] == DONE and 0 < c[0] < npp and 0 < c[1] <= nq
    # (the good canon_t in front: the neighbour in the same call is placed, the forged one named)
    run = lambda c4: place(wc, [r, r], [len(f), len(f)], [c, np.array(c4, np.uint32)])
    good = run(c)
    assert good["err"] is None and good["totals"] == [0, 2, 0, 2 * hl(c[0], c[1]), 0, 2 * int(r[NV]), 2]
    # the kept counts may be anything from 1 to the raw count
    assert run([1, 1, DONE, 0])["err"] is None and run([npp, nq, DONE, 0])["err"] is None
    for c4 in ([c[0], c[1], 0, 0], [c[0], c[1], 3, 0],           # a state that places nothing
               [npp + 1, c[1], DONE, 0], [c[0], nq + 1, DONE, 0],   # more kept than sent
               [0, c[1], DONE, 0], [c[0], 0, DONE, 0]):             # none kept where some were sent
        bad = run(c4)
        assert bad["err"] == "canon record" and bad["dst"]["slot"][0] == 0, c4
    # none kept is right where none was sent
    f0 = frame(frames["rec"], [], parents_of(frames["rec"])[::-1])
    r0, c0 = scan(wc, f0), canon(wc, f0)
    assert r0[NP] == 0 and c0.tolist() == [0, nq, DONE, 0]
    assert place(wc, [r0], [len(f0)], [c0])["err"] is None


def test_forged_kind_and_totals(wc, frames):
    f = frames["cert"]
    r = scan(wc, f)
    for kind in (7, 4, -3):   # behind a good record, which the same call places
        bad = place(wc, [r, with_(r, KIND=kind)], [len(f), len(f)])
        assert bad["err"] == "record kind" and bad["dst"]["slot"][0] == 0, kind
    for kind in (0, 1, 2, 3, -1, OVER_CAP):
        assert place(wc, [with_(r, KIND=kind, VLEN=0)], [len(f)])["err"] is None, kind
    h, nv = hl(r[NP], r[NQ]), int(r[NV])
    assert nv > 0
    two = lambda total=2 * h, vbound=2 * nv: place(wc, [r, r], [len(f), len(f)], total=total,
                                                    vbound=vbound)
    assert two()["err"] is None and two(total=2 * h - 1)["err"] == "record totals"
    assert two(vbound=2 * nv - 1)["err"] == "record totals"
    # headers and certificates share the bound
    hf = frames["header"]
    mix = lambda total: place(wc, [scan(wc, hf), r], [len(hf), len(f)], total=total, vbound=nv)
    assert mix(2 * h)["err"] is None and mix(2 * h - 1)["err"] == "record totals"


def emit_rec(wc, f, r8, group, can=None):
    """wc_emit_rec (r8 = None: wc_emit, which scans the frame itself; can: the canon_t for the
    instance that serves canonicalised frames) over buffers filled with 0xEE; -> (return
    value, every buffer as one array, payload count, offset rows)."""
    bufs = [np.full(len(f) + 4096, 0xEE, np.uint8), np.full(32, 0xEE, np.uint8),
            np.full(64, 0xEE, np.uint8), np.full((64, 32), 0xEE, np.uint8),
            np.full((64, 64), 0xEE, np.uint8), np.full(168, 0xEE, np.uint8)]
    hb, hid, sig, vpk, vsig, v168 = bufs
    pc, off3 = np.full(1, 0xEEEEEEEE, np.uint32), np.full(3, 0xEEEEEEEEEEEEEEEE, np.uint64)
    rest = (_p(hb), hb.size, _p(hid), _p(sig), _p(vpk), _p(vsig), 64, _p(pc), _p(off3), _p(v168))
    if r8 is None:
        rc = wc.wc_emit(f, len(f), len(f) % 4, group, *rest)
    else:
        assert hl(r8[NP], r8[NQ]) <= hb.size and r8[NV] <= 64   # the capacities do not stop it
        rc = wc.wc_emit_rec(f, len(f), len(f) % 4, group, _p(r8), _p(can), *rest)
    return rc, np.concatenate([b.ravel() for b in bufs]), pc, off3


@pytest.mark.parametrize("which,field,step", FIT_CASES)
def test_forged_record_emits_nothing(wc, frames, which, field, step):
    f, _, forged = forge_fit(wc, frames, which, field, step)
    own = scan(wc, f)
    for group in (1, 16, 64):
        rc, out, pc, off3 = emit_rec(wc, f, forged, group)
        assert rc >= 0 and (out == 0xEE).all(), group
        if which != "vote":   # the offset rows and the payload count: not written either
            assert pc[0] == 0xFFFFFFFF and off3[:2].tolist() == [ONES64, ONES64], group
        # nor by the instance that serves canonicalised frames (this frame is canonical)
        rc, out, pc, off3 = emit_rec(wc, f, forged, group, canon(wc, f))
        assert rc >= 0 and (out == 0xEE).all(), group
        # the frame's own record through the same call does write: the rows wc_emit writes
        rc, out, pc, off3 = emit_rec(wc, f, own, group)
        rc2, out2, pc2, off32 = emit_rec(wc, f, None, group)
        assert rc == rc2 == (0 if which == "vote" else hl(own[NP], own[NQ])), group
        assert (out == out2).all() and (out != 0xEE).any(), group
        if which != "vote":
            assert pc[0] == pc2[0] == own[NP] and off3.tolist() == off32.tolist(), group
            assert off3[:2].tolist() == [0, rc], group


@pytest.mark.parametrize("field,step", [("ALEN", 1), ("NP", 36), ("NQ", 32), ("NV", 72)])
def test_forged_record_of_a_canonicalised_frame(wc, frames, field, step):
    """The same through the order list: the non-canonical certificate with its canon_t."""
    f, fits, forged = forge_fit(wc, frames, "noncanon", field, step)
    own, c = scan(wc, f), canon(wc, f)
    assert own[CANONICAL] == 0 and c[2] == DONE
    assert place(wc, [fits], [len(f)], [c])["err"] is None
    bad = place(wc, [fits, forged], [len(f), len(f)], [c, c])
    assert bad["err"] == "header record" and bad["dst"]["slot"][0] == 0
    for group in (1, 16, 64):
        rc, out, pc, off3 = emit_rec(wc, f, forged, group, c)
        assert rc >= 0 and (out == 0xEE).all(), group
        assert pc[0] == 0xFFFFFFFF and off3[:2].tolist() == [ONES64, ONES64], group
        # the plain instance writes nothing for a non-canonical frame, forged record or not
        assert (emit_rec(wc, f, own, group)[1] == 0xEE).all(), group
        # the frame's own record and canon_t do write: the kept counts' rows
        rc, out, pc, off3 = emit_rec(wc, f, own, group, c)
        assert (out != 0xEE).any() and pc[0] == c[0], group
        assert off3.tolist() == [0, hl(c[0], c[1]), int(own[NV])], group
