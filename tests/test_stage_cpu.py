"""The message jobs' staging layout (narwhal_amd/csrc/nw_stage.hpp: plan / fill / view of the
committee, the header stream, the certificates' votes and the Vote messages), compiled as
host code into tools/libnw_stagecheck.so and run over malloc'ed buffers. Every section offset
is pinned to the value the 256-byte rule gives for the section order of submit_small /
submit_certs / submit_votes; every staged array is read back through a view on a copy of the
staged bytes (another base than the fill's, as NW_SMALL_VRAM's copy is)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cert_cases import mutated_stream, votes_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "libnw_stagecheck.so")
SRCS = [os.path.join(ROOT, "tools", "stagecheck.hip"),
        os.path.join(ROOT, "narwhal_amd", "csrc", "nw_stage.hpp"),
        os.path.join(ROOT, "include", "narwhal_amd.h")]
HEADERS, CERTS, VOTES = 0, 1, 2
NOT_STAGED = 2**64 - 1
# the sections in the order sc_stage reports them
NAMES = ["pks", "stakes", "worker_offsets", "worker_ids",
         "header_bytes", "header_offsets", "payload_counts", "ids", "header_sigs",
         "vote_offsets", "vote_pks", "vote_sigs", "z16",
         "v_ids", "v_rounds", "v_origins", "v_authors", "v_sigs"]
P, U64 = ctypes.c_void_p, ctypes.c_uint64


class Committee(ctypes.Structure):          # nw_committee
    _fields_ = [("nauth", ctypes.c_size_t), ("pks", P), ("stakes", P), ("worker_offsets", P),
                ("worker_ids", P)]


class Certificates(ctypes.Structure):       # nw_certificates
    _fields_ = [("n", ctypes.c_size_t), ("header_bytes", P), ("header_offsets", P),
                ("payload_counts", P), ("ids", P), ("header_sigs", P), ("vote_offsets", P),
                ("vote_pks", P), ("vote_sigs", P), ("header_bytes_len", ctypes.c_size_t),
                ("nvotes", ctypes.c_size_t), ("host_vote_offsets", P)]


class VoteMsgs(ctypes.Structure):           # nw::stage::VoteMsgs
    _fields_ = [("ids", P), ("rounds", P), ("origins", P), ("authors", P), ("sigs", P),
                ("n", ctypes.c_size_t)]


@pytest.fixture(scope="module")
def sc():
    if not (os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in SRCS)):
        subprocess.run(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), SRCS[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    lib.sc_stage.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, P, P]
    lib.sc_stage.restype = P
    lib.sc_read.argtypes = [P, ctypes.c_int, P]
    lib.sc_read.restype = ctypes.c_long
    lib.sc_free.argtypes = [P]
    return lib


@pytest.fixture(scope="module")
def stream():
    """(committee, certificate stream, z16) of N = 4, never modified."""
    com, s, _, _, _ = mutated_stream(N=4, copies=1)
    z16 = np.random.Generator(np.random.PCG64(4)).integers(0, 256, size=(len(s["vote_pks"]), 16),
                                                           dtype=np.uint8)
    return com, s, z16


@pytest.fixture(scope="module")
def votes():
    com, p, _, _ = votes_case(4)
    return com, p


def _p(a):
    return None if a is None else a.ctypes.data


def a256(x):
    return (x + 255) & ~255


def packed(sizes):
    """Offsets of consecutive sections of `sizes` bytes (256-aligned, an empty one takes one
    byte's section) and the offset behind them."""
    offs, off = [], 0
    for b in sizes:
        offs.append(off)
        off += a256(b if b else 1)
    return offs, off


def expected(kind, na, nwk, n, nv=0, hlen=0, z16=False, with_vo=False):
    """{section: offset} plus o_st / o_ix / end, from the parent's section order: the
    committee; then the header stream and, for certificates, (vote offsets,) vote keys, vote
    signatures (, z16), or the Vote messages; then the statuses and the indices."""
    names = NAMES[:4]
    sizes = [32 * na, 4 * na, 8 * (na + 1), 4 * nwk]
    if kind == VOTES:
        names += NAMES[13:]
        sizes += [32 * n, 8 * n, 32 * n, 32 * n, 64 * n]
    else:
        names += NAMES[4:9]
        sizes += [hlen, 8 * (n + 1), 4 * n, 32 * n, 64 * n]
        if kind == CERTS:
            if with_vo:
                names.append("vote_offsets")
                sizes.append(8 * (n + 1))
            names += ["vote_pks", "vote_sigs"]
            sizes += [32 * nv, 64 * nv]
            if z16:
                names.append("z16")
                sizes.append(16 * nv)
    offs, _ = packed(sizes + [4 * n, 8 * n])
    exp = dict(zip(names + ["o_st", "o_ix"], offs))
    exp["end"] = offs[-1] + a256(8 * n)
    return exp, dict(zip(names, sizes))


def stage(sc, com, kind, s=None, z16=None, with_vo=False, v=None, a=0, e=None):
    """sc_stage over messages [a, e) of the stream (as a fan-out part: header offsets absolute,
    vote offsets rebased) or of the Vote messages -> ({section: offset}, {section: bytes read
    back through the view}, the part's source arrays)."""
    c = Committee(len(com["pks"]), _p(com["pks"]), _p(com["stakes"]), _p(com["worker_offsets"]),
                  _p(com["worker_ids"]))
    keep, cs, va, src = [], None, None, {k: com[k] for k in NAMES[:4]}
    if kind == VOTES:
        e = len(v["rounds"]) if e is None else e
        part = {"v_" + k: np.ascontiguousarray(v[k][a:e]) for k in ("ids", "rounds", "origins", "authors", "sigs")}
        va = VoteMsgs(*[_p(part[k]) for k in NAMES[13:]], e - a)
        src.update(part)
    else:
        e = len(s["payload_counts"]) if e is None else e
        ho, vo = s["header_offsets"], s["vote_offsets"]
        v0, v1 = int(vo[a]), int(vo[e])
        part = {"header_offsets": np.ascontiguousarray(ho[a:e + 1]),
                "payload_counts": np.ascontiguousarray(s["payload_counts"][a:e]),
                "ids": np.ascontiguousarray(s["ids"][a:e]),
                "header_sigs": np.ascontiguousarray(s["header_sigs"][a:e]),
                "vote_offsets": (vo[a:e + 1] - vo[a]).astype(np.uint64),
                "vote_pks": np.ascontiguousarray(s["vote_pks"][v0:v1]),
                "vote_sigs": np.ascontiguousarray(s["vote_sigs"][v0:v1])}
        cs = Certificates(e - a, _p(s["header_bytes"]), _p(part["header_offsets"]),
                          _p(part["payload_counts"]), _p(part["ids"]), _p(part["header_sigs"]),
                          _p(part["vote_offsets"]), _p(part["vote_pks"]), _p(part["vote_sigs"]),
                          0, 0, None)
        src.update(part)
        src["header_bytes"] = s["header_bytes"][int(ho[a]):int(ho[e])]
        src["header_offsets"] = part["header_offsets"] - ho[a]       # staged from 0
        if z16 is not None:
            src["z16"] = z16 = np.ascontiguousarray(z16[v0:v1])
    keep = [c, cs, va, part, z16]
    offs = np.zeros(len(NAMES) + 3, np.uint64)
    h = sc.sc_stage(ctypes.byref(c), kind, ctypes.byref(cs) if cs else None, _p(z16), int(with_vo),
                    ctypes.byref(va) if va else None, _p(offs))
    assert h and keep
    got = {k: int(o) for k, o in zip(NAMES + ["o_st", "o_ix", "end"], offs) if o != NOT_STAGED}
    back = {}
    buf = np.zeros(int(offs[-1]) + 1, np.uint8)
    for i, k in enumerate(NAMES):
        nb = sc.sc_read(h, i, _p(buf))
        assert (nb >= 0) == (k in got), k
        if nb >= 0:
            back[k] = buf[:nb].tobytes()
    sc.sc_free(h)
    return got, back, src


def check(got, back, src, exp, sizes):
    assert got == exp                                               # pinned offsets
    secs = [(got[k], sizes[k]) for k in sizes]
    assert all(o % 256 == 0 for o in got.values())
    assert len({o for o, _ in secs}) == len(secs)                   # distinct, also when empty
    secs.sort()
    assert all(o + b <= o2 for (o, b), (o2, _) in zip(secs, secs[1:]))   # pairwise disjoint
    assert secs[-1][0] + secs[-1][1] <= got["o_st"] < got["o_ix"] < got["end"]
    for k, b in sizes.items():                                      # round trip
        assert back[k] == np.ascontiguousarray(src[k]).tobytes()[:b] and len(back[k]) == b, k


def _counts(com, s, a=0, e=None):
    e = len(s["payload_counts"]) if e is None else e
    na, nwk = len(com["pks"]), int(com["worker_offsets"][-1])
    hlen = int(s["header_offsets"][e] - s["header_offsets"][a])
    nv = int(s["vote_offsets"][e] - s["vote_offsets"][a])
    return na, nwk, e - a, nv, hlen


@pytest.mark.parametrize("a,e", [(0, None), (3, 9)])
def test_headers(sc, stream, a, e):
    com, s, _ = stream
    na, nwk, n, _, hlen = _counts(com, s, a, e)
    assert n > 1 and hlen % 256 != 0 and (a == 0 or s["header_offsets"][a] != 0)
    got, back, src = stage(sc, com, HEADERS, s, a=a, e=e)
    check(got, back, src, *expected(HEADERS, na, nwk, n, hlen=hlen))
    assert np.frombuffer(back["header_offsets"], np.uint64)[0] == 0
    assert not set(got) & set(NAMES[9:])


@pytest.mark.parametrize("a,e", [(0, None), (3, 9)])
@pytest.mark.parametrize("with_vo", [False, True])
@pytest.mark.parametrize("with_z", [False, True])
def test_certificates(sc, stream, with_z, with_vo, a, e):
    com, s, z16 = stream
    na, nwk, n, nv, hlen = _counts(com, s, a, e)
    assert nv > n and (a == 0 or (s["header_offsets"][a] != 0 and s["vote_offsets"][a] != 0))
    got, back, src = stage(sc, com, CERTS, s, z16 if with_z else None, with_vo, a=a, e=e)
    check(got, back, src, *expected(CERTS, na, nwk, n, nv, hlen, with_z, with_vo))
    assert ("z16" in got, "vote_offsets" in got) == (with_z, with_vo)
    # the slice's header bytes, offsets from 0; the vote offsets as the part gave them
    assert np.frombuffer(back["header_offsets"], np.uint64).tolist() == \
        (s["header_offsets"][a:a + n + 1] - s["header_offsets"][a]).tolist()
    assert back["header_bytes"] == s["header_bytes"].tobytes()[int(s["header_offsets"][a]):][:hlen]
    if with_vo:
        assert np.frombuffer(back["vote_offsets"], np.uint64).tolist()[::n] == [0, nv]


@pytest.mark.parametrize("a,e", [(0, None), (5, 18)])
def test_vote_messages(sc, votes, a, e):
    com, p = votes
    n = (len(p["rounds"]) if e is None else e) - a
    got, back, src = stage(sc, com, VOTES, v=p, a=a, e=e)
    check(got, back, src, *expected(VOTES, len(com["pks"]), int(com["worker_offsets"][-1]), n))
    assert not set(got) & set(NAMES[4:13])


def test_empty_sections(sc, stream, votes):
    """No worker ids (nwk == 0) and no votes (nv == 0): the empty sections still get offsets of
    their own (the one-byte rule), in the same order."""
    com, s, z16 = stream
    bare = dict(com, worker_offsets=np.zeros(len(com["pks"]) + 1, np.uint64),
                worker_ids=np.zeros(0, np.uint32))
    na, _, n, nv, hlen = _counts(com, s)
    got, back, src = stage(sc, bare, CERTS, s, z16, True)
    exp, sizes = expected(CERTS, na, 0, n, nv, hlen, True, True)
    assert sizes["worker_ids"] == 0 and exp["header_bytes"] == exp["worker_ids"] + 256
    check(got, back, src, exp, sizes)
    novotes = dict(s, vote_offsets=np.zeros(n + 1, np.uint64))
    got, back, src = stage(sc, com, CERTS, novotes, z16[:0], True)
    exp, sizes = expected(CERTS, na, int(com["worker_offsets"][-1]), n, 0, hlen, True, True)
    assert sizes["vote_pks"] == sizes["vote_sigs"] == sizes["z16"] == 0
    assert [exp[k] - exp["vote_pks"] for k in ("vote_sigs", "z16", "o_st")] == [256, 512, 768]
    check(got, back, src, exp, sizes)
    vcom, p = votes
    vbare = dict(vcom, worker_offsets=np.zeros(len(vcom["pks"]) + 1, np.uint64),
                 worker_ids=np.zeros(0, np.uint32))
    got, back, src = stage(sc, vbare, VOTES, v=p)
    check(got, back, src, *expected(VOTES, len(vcom["pks"]), 0, len(p["rounds"])))
