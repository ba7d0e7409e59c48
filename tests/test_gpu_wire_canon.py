"""Wire ingest with NW_WIRE_DECODE_DEVICE | NW_WIRE_CANON_DEVICE: Header / Certificate frames
whose payload or parents arrive out of order or with duplicates are sorted and de-duplicated
by k_wire_canon and decided on the device. References: the host decoder (decode="host"), the
Python restatement of the wire format (tests/test_wire.py) and the oracle. nw_wire_stats pins
who decoded what: the only frames allowed a host share are the ones sent over the entry bound
on purpose. NW_WIRE_MAX_FRAME is set only in the child process of the last test."""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from narwhal_amd import _lib
from narwhal_amd import wire as WI
from narwhal_amd.messages import _p, committee_struct
from oracle import oracle as O

from cert_cases import d32, mutated_stream, pack, unpack
from test_gpu_wire_device import corpus, run, same, tiled
from test_wire import _pk, cert_frame, ref_decode

pytestmark = pytest.mark.gpu

CANON = "device-canon"


def parts(rec):
    """Payload [(key, worker id)] and parents of a record's canonical header bytes."""
    hb, n = rec["hb"], rec["np"]
    pay = [(hb[40 + 36 * i:72 + 36 * i], struct.unpack_from("<I", hb, 72 + 36 * i)[0]) for i in range(n)]
    return pay, [hb[i:i + 32] for i in range(40 + 36 * n, len(hb), 32)]


def frame(rec, pay, par, variant=2):
    """rec's frame with the payload and the parents in the given wire order."""
    hb = rec["hb"]
    out = (struct.pack("<I", variant) + _pk(hb[:32]) + hb[32:40] + struct.pack("<Q", len(pay))
           + b"".join(k + struct.pack("<I", v) for k, v in pay)
           + struct.pack("<Q", len(par)) + b"".join(par) + rec["id"] + rec["sig"])
    if variant == 2:
        out += struct.pack("<Q", len(rec["votes"])) + b"".join(_pk(p) + s for p, s in rec["votes"])
    return out


def reordered(rec, rng=None, variant=2):
    """The record's frame with payload and parents reversed (rng None) or shuffled, and a
    duplicated parent appended: it decodes to the same record."""
    pay, par = parts(rec)
    if rng is None:
        pay, par = pay[::-1], par[::-1]
    else:
        pay = [pay[i] for i in rng.permutation(len(pay))]
        par = [par[i] for i in rng.permutation(len(par))]
    f = frame(rec, pay, par + par[:1], variant)
    k, d = ref_decode(f)
    assert k == variant and d["hb"] == rec["hb"] and d["np"] == rec["np"]
    return f


_cache = {}


def certs():
    """(committee, records, oracle status, oracle index) of the mutated certificate stream,
    built once and never modified."""
    if "certs" not in _cache:
        com, s, _, _, _ = mutated_stream(N=4, copies=2, seed=11)
        ost, oix = O.certificates_verify_many(com, s)
        _cache["certs"] = (com, unpack(s), ost, oix)
    return _cache["certs"]


def signed_header(payload, parents=None):
    """A header record of the first committee member over the given canonical payload
    [(key, worker id)] (sorted, unique), signed: its id and signature hold."""
    _, recs, _, _ = certs()
    pk, sk = O.keys(4)[0]
    assert payload == sorted(payload)
    par = parts(recs[0])[1] if parents is None else parents
    hb = (pk + struct.pack("<Q", 3) + b"".join(k + struct.pack("<I", v) for k, v in payload)
          + b"".join(par))
    hid = d32(hb)
    return {"hb": hb, "np": len(payload), "id": hid, "sig": O.sign(sk, hid), "votes": []}


def header_verdict(com, rec):
    st, ix = O.certificates_verify_many(com, pack([rec]), headers_only=True)
    return int(st[0]), int(ix[0])


A, B, C = bytes([1]) * 32, bytes([2]) * 32, bytes([3]) * 32
BAD_WORKER = 7      # the committees of cert_cases give every authority worker 0 only


def variants():
    """Non-canonical frames with the verdict each must get: [(frame, kind, status, index or
    None)], built once. The reordered certificates of test 3, the headers of tests 4 and 5."""
    if "variants" not in _cache:
        com, recs, ost, oix = certs()
        rng = np.random.default_rng(5)
        out = []
        for r, st, ix in zip(recs, ost, oix):
            out.append((reordered(r), 2, int(st), int(ix)))
            out.append((reordered(r, rng), 2, int(st), int(ix)))
        h = signed_header([(A, 0), (B, 0), (C, BAD_WORKER)])
        out.append((frame(h, [(C, BAD_WORKER), (A, 0), (B, 0)], parts(h)[1], 0), 0) + header_verdict(com, h))
        h = signed_header([(A, 0), (B, 0)])
        out.append((frame(h, [(A, BAD_WORKER), (B, 0), (A, 0)], parts(h)[1], 0), 0) + header_verdict(com, h))
        _cache["variants"] = out
    return _cache["variants"]


def raw_call(com, frames, flags):
    data, offs = WI.frames_soa(frames)
    n = len(frames)
    kind, st, ix = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
    cc = committee_struct(com)
    return _lib.lib().nw_primary_messages_verify_wire_ex(ctypes.byref(cc), _p(data), _p(offs), n,
                                                         flags, _p(kind), _p(st), _p(ix))


def test_flag_validity():
    com, frames, _, _ = corpus(4)
    assert WI.WIRE_DECODE_DEVICE == 1 and WI.WIRE_CANON_DEVICE == 2
    assert raw_call(com, frames[:3], WI.WIRE_CANON_DEVICE) == -1                   # NW_E_INVALID_ARG
    assert raw_call(com, frames[:3], 1 | 2 | 4) == -1
    assert raw_call(com, frames[:3], 1 | 2 | 0x80000000) == -1
    assert raw_call(com, frames[:3], 4) == -1
    assert raw_call(com, frames[:3], 1 | 2) == 0
    assert raw_call(com, frames[:3], 1) == 0 and raw_call(com, frames[:3], 0) == 0
    with pytest.raises(ValueError):
        WI.verify_primary_messages(com, frames[:3], decode="canon")


def test_corpus_parity():
    com, frames, kinds, exp = corpus(4)
    n = len(frames)
    host = run(com, frames, "host")
    dev = run(com, frames, CANON)
    assert dev[0].tolist() == kinds.tolist() == host[0].tolist()
    bad = [(i, int(kinds[i]), int(a), int(b), int(x), int(y)) for i, (a, b, x, y) in
           enumerate(zip(dev[1], host[1], dev[2], host[2])) if a != b or x != y]
    assert not bad, bad[:10]
    bad = [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(dev[1], exp)) if a != b]
    assert not bad, bad[:10]
    assert (dev[3], dev[4]) == (n, 0)
    # the decode flag alone, in the same process: the duplicate-key frame is still the host's
    plain = run(com, frames, "device")
    assert same(plain, host) and (plain[3], plain[4]) == (n - 1, 1)


def test_valid_certificates_stay_valid():
    com, recs, ost, oix = certs()
    v = variants()[:2 * len(recs)]
    frames = [f for f, _, _, _ in v]
    assert (ost == 0).sum() >= 4 and (ost != 0).sum() >= 20
    dev = run(com, frames, CANON)
    assert dev[0].tolist() == [2] * len(frames)
    assert dev[1].tolist() == [s for _, _, s, _ in v]
    assert same(dev, run(com, frames, "host"))
    assert (dev[3], dev[4]) == (len(frames), 0)


def test_sorted_position_index():
    com = certs()[0]
    f, kind, st, ix = variants()[-2]
    assert (kind, st, ix) == (0, 18, 2)      # NW_DAG_MALFORMED_HEADER at the sorted position
    dev = run(com, [f], CANON)
    assert (int(dev[0][0]), int(dev[1][0]), int(dev[2][0])) == (0, 18, 2)
    assert same(dev, run(com, [f], "host")) and (dev[3], dev[4]) == (1, 0)


def test_dropped_value_does_not_reach_the_check():
    com = certs()[0]
    f, kind, st, ix = variants()[-1]
    assert (kind, st) == (0, 0)
    dev = run(com, [f], CANON)
    assert (int(dev[0][0]), int(dev[1][0])) == (0, 0)
    assert same(dev, run(com, [f], "host")) and (dev[3], dev[4]) == (1, 0)
    # the same entries with the unknown worker id sent last: now it is the one that counts
    h = signed_header([(A, BAD_WORKER), (B, 0)])
    g = frame(h, [(A, 0), (B, 0), (A, BAD_WORKER)], parts(h)[1], 0)
    assert header_verdict(com, h) == (18, 0)
    dev = run(com, [g], CANON)
    assert (int(dev[1][0]), int(dev[2][0])) == (18, 0) and same(dev, run(com, [g], "host"))


def mixed(seed, n=777):
    com, frames, _, _ = corpus(4)
    pool = list(frames) + [f for f, _, _, _ in variants()]
    reps = -(-n // len(pool)) + 1
    idx = np.random.default_rng(seed).permutation(np.tile(np.arange(len(pool)), reps))[:n]
    return com, [pool[i] for i in idx]


def test_mixed_tile():
    com, fr = mixed(1)
    assert len(fr) == 777 and 777 % 64 and 777 % 256
    dev = run(com, fr, CANON)
    assert same(dev, run(com, fr, "host"))
    assert (dev[3], dev[4]) == (777, 0)
    one = [variants()[1][0]]
    dev = run(com, one, CANON)
    assert same(dev, run(com, one, "host")) and (dev[3], dev[4]) == (1, 0)
    assert int(dev[1][0]) == variants()[1][2]


def test_buffer_reuse():
    """One pooled job whose buffers change size and layout from call to call: 4,000 mixed
    frames (about 1.9 MB, a third of them reordered), a 5-frame call, then a call that opens
    with frames of 1,018 shuffled parents (their order lists and canon_t entries land where
    the first call kept those of small frames, and the arrays behind them move), then other
    small frames again. Each equals its own host-decode result, with no host share."""
    com, a = mixed(2, 4000)
    _, c = mixed(3, 1500)
    _, d = mixed(4, 300)
    big = [big_header(1018, s)[1] for s in (21, 22, 23)]
    assert sum(map(len, a)) > 1 << 20 and a[:1500] != c
    for fr in (a, a[100:105], big[:2] + d + big[2:], c, big[:1]):
        dev = run(com, fr, CANON)
        assert same(dev, run(com, fr, "host")) and (dev[3], dev[4]) == (len(fr), 0)


def big_header(nparents, seed):
    rng = np.random.default_rng(seed)
    par = [rng.bytes(32) for _ in range(nparents)]
    h = signed_header([], sorted(par))
    return h, frame(h, [], par, 0)


def test_largest_frame_under_the_default_cap():
    com = certs()[0]
    h, f = big_header(1018, 8)
    assert len(f) <= 32768 and ref_decode(f)[1]["hb"] == h["hb"]
    dev = run(com, [f], CANON)
    assert (dev[3], dev[4]) == (1, 0)
    assert same(dev, run(com, [f], "host"))
    assert (int(dev[0][0]), int(dev[1][0])) == (0, header_verdict(com, h)[0])


_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r]
from narwhal_amd import wire as WI
from test_gpu_wire_canon import big_header, certs, variants
com = certs()[0]
out = []
for f in (big_header(1030, 9)[1], variants()[0][0]):
    d0, h0 = WI.stats()
    k, s, x = WI.verify_primary_messages(com, [f])        # the plain call
    d1, h1 = WI.stats()
    out.append([int(k[0]), int(s[0]), int(x[0]), d1 - d0, h1 - h0])
print("RESULT " + json.dumps(out))
"""


def test_environment_switch_and_entry_bound():
    """NW_WIRE_DECODE=device-canon makes the plain call take both flags; with the cap raised, a
    frame of more than kCanonMax entries is the host's, a small reordered one the device's."""
    com = certs()[0]
    over, small = big_header(1030, 9)[1], variants()[0][0]
    assert 32768 < len(over) < 40000
    exp = []
    for f, share in ((over, [0, 1]), (small, [1, 0])):
        h = run(com, [f], "host")
        exp.append([int(h[0][0]), int(h[1][0]), int(h[2][0])] + share)
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NW_WIRE_DECODE="device-canon", NW_WIRE_MAX_FRAME="40000")
    p = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(tests), tests)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert got == exp
