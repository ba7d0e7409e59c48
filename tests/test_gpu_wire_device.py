"""Wire ingest with the decode on the device (nw_primary_messages_verify_wire_ex with
NW_WIRE_DECODE_DEVICE; kernels in narwhal_amd/csrc/nw_wire.hip, job in nw_jobs.cpp) against
the host decoder, the Python restatement of the wire format (tests/test_wire.py) and the
oracle. nw_wire_stats pins who decoded what: a decoder that quietly sent its work to the
host would fail the split asserted here. NW_WIRE_MAX_FRAME is set nowhere in these tests."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from narwhal_amd import wire as WI
from oracle import oracle as O

from cert_cases import pack, unpack, mutated_stream, votes_case
from test_wire import _corpus, cert_frame, ref_decode, vote_frame

pytestmark = pytest.mark.gpu

_cache = {}


def corpus(N):
    """(committee, frames, ref kinds, oracle statuses), built once per N."""
    if N not in _cache:
        com, frames = _corpus(N=N, copies=2 if N == 4 else 1)
        dec = [ref_decode(f) for f in frames]
        kinds = np.array([k for k, _ in dec], np.int32)
        exp = np.where(kinds < 0, WI.DAG_SERIALIZATION, 0).astype(np.int32)
        for kind, headers_only in ((2, False), (0, True)):
            sel = [i for i, (k, _) in enumerate(dec) if k == kind]
            if sel:
                ost, _ = O.certificates_verify_many(com, pack([dec[i][1] for i in sel]),
                                                    headers_only=headers_only)
                exp[sel] = ost
        sel = [i for i, (k, _) in enumerate(dec) if k == 1]
        if sel:
            cat = lambda key, w: np.frombuffer(b"".join(dec[i][1][key] for i in sel),
                                               np.uint8).reshape(-1, w)
            vp = {"ids": cat("id", 32), "origins": cat("origin", 32), "authors": cat("author", 32),
                  "sigs": cat("sig", 64),
                  "rounds": np.array([dec[i][1]["round"] for i in sel], np.uint64)}
            exp[sel] = O.votes_verify_many(com, vp, len(sel))
        _cache[N] = (com, frames, kinds, exp)
    return _cache[N]


def run(com, frames, decode):
    """(kind, status, index, device frames, host frames) of one call."""
    d0, h0 = WI.stats()
    k, s, x = WI.verify_primary_messages(com, frames, decode=decode)
    d1, h1 = WI.stats()
    return k.copy(), s.copy(), x.copy(), d1 - d0, h1 - h0


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("N,nframes", [(4, 179), (100, 1658)])
def test_parity(N, nframes):
    com, frames, kinds, exp = corpus(N)
    assert len(frames) == nframes
    host = run(com, frames, "host")
    dev = run(com, frames, "device")
    assert dev[0].tolist() == kinds.tolist()
    bad = [(i, int(kinds[i]), int(a), int(b), int(x), int(y)) for i, (a, b, x, y) in
           enumerate(zip(dev[1], host[1], dev[2], host[2])) if a != b or x != y]
    assert not bad, bad[:10]
    assert host[0].tolist() == kinds.tolist()
    bad = [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(dev[1], exp)) if a != b]
    assert not bad, bad[:10]
    # the host's share of a device-decode call: exactly the duplicate-key frame
    assert (host[3], host[4]) == (0, nframes)
    assert (dev[3], dev[4]) == (nframes - 1, 1)
    assert kinds[-2] == 2      # (it is the last but one frame of the corpus, and it decodes)


def unpack_first(N):
    _, s, _, _, _ = mutated_stream(N=N, copies=2 if N == 4 else 1, seed=11)
    return unpack(s)[0]


def tiled(frames, seed, n=777):
    idx = np.random.default_rng(seed).permutation(np.tile(np.arange(len(frames)), 5))[:n]
    return idx, [frames[i] for i in idx]


def test_wave_and_workgroup_boundaries():
    com, frames, kinds, exp = corpus(4)
    small = run(com, frames, "device")
    idx, fr = tiled(frames, 1)
    assert len(fr) == 777 and 777 % 64 and 777 % 256
    big = run(com, fr, "device")
    assert same(big, [a[idx] for a in small[:3]])
    assert big[3] + big[4] == 777 and big[4] == int((idx == len(frames) - 2).sum())
    # n = 0, n = 1
    k, s, x, d, h = run(com, [], "device")
    assert len(k) == 0 and (d, h) == (0, 0)
    for i in (0, len(frames) - 1, int(np.flatnonzero(kinds == 1)[0]), int(np.flatnonzero(kinds == -1)[3])):
        one = run(com, [frames[i]], "device")
        assert same(one, [a[i:i + 1] for a in small[:3]]) and (one[3], one[4]) == (1, 0), i
    # only undecodable frames: all the device's, nothing to emit or verify
    junk = [b"", b"\x01", b"\x02\x00\x00", struct.pack("<I", 9) + bytes(40), frames[0][:100],
            struct.pack("<I", 1) + bytes(20)] * 20
    k, s, x, d, h = run(com, junk, "device")
    assert (k == -1).all() and (s == WI.DAG_SERIALIZATION).all() and not x.any()
    assert (d, h) == (len(junk), 0)


def test_truncations():
    com, frames, kinds, _ = corpus(4)
    rec = unpack_first(4)
    _, vp, _, _ = votes_case(4)
    cuts = [f[:k] for f in (cert_frame(rec), cert_frame(rec, 0), vote_frame(vp, 0))
            for k in range(len(f) + 1)]
    k, s, x, d, h = run(com, cuts, "device")
    assert k.tolist() == [ref_decode(c)[0] for c in cuts]
    assert (s[k < 0] == WI.DAG_SERIALIZATION).all() and (k >= 0).sum() >= 3
    assert (d, h) == (len(cuts), 0)


def test_buffer_reuse():
    """One process, one pooled job: a large call, a tiny one, another large one. Each equals
    its own host-decode result, so nothing of an earlier call's buffers leaks into a later."""
    com, frames, _, _ = corpus(4)
    _, a = tiled(frames, 2)
    _, c = tiled(frames, 3)
    assert a != c
    for fr in (a, a[100:105], c):
        assert same(run(com, fr, "device"), run(com, fr, "host"))


def test_frame_over_the_cap_goes_to_the_host():
    com, frames, _, _ = corpus(4)
    rec = unpack_first(4)
    pay = b"".join(struct.pack(">I", i) + bytes(28) + struct.pack("<I", 0) for i in range(1000))
    hb = rec["hb"][:40] + pay + rec["hb"][40 + 36 * rec["np"]:]
    big = {"hb": hb, "np": 1000, "id": O.digest32(hb), "sig": bytes(64), "votes": []}
    f = cert_frame(big, 0)
    assert len(f) > 36000 and ref_decode(f)[0] == 0 and ref_decode(f)[1]["hb"] == hb
    ost, _ = O.certificates_verify_many(com, pack([big]), headers_only=True)
    k, s, x, d, h = run(com, [frames[0], f, frames[1]], "device")
    assert (d, h) == (2, 1)
    assert k.tolist() == [2, 0, 2] and s[1] == ost[0]
    assert same((k, s, x), run(com, [frames[0], f, frames[1]], "host"))


def test_all_devices_refuses_the_device_flag():
    """Under nw_set_device(NW_ALL_DEVICES) the flag is NW_E_INVALID_ARG, as for the nw_dev_*
    calls; host decode (flags 0) still fans out."""
    from narwhal_amd import _lib
    com, frames, _, _ = corpus(4)
    ref = run(com, frames, "host")
    L = _lib.lib()
    assert L.nw_set_device(-1) == 0
    try:
        with pytest.raises(_lib.EngineError, match="NW_E_INVALID_ARG"):
            WI.verify_primary_messages(com, frames, decode="device")
        assert same(run(com, frames, "host"), ref)
    finally:
        assert L.nw_set_device(0) == 0
    assert same(run(com, frames, "device"), ref)


_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r]
from narwhal_amd import wire as WI
from test_wire import _corpus
com, frames = _corpus(N=4, copies=2)
k, s, x = WI.verify_primary_messages(com, frames)        # the plain call
d, h = WI.stats()
print("RESULT " + json.dumps({"k": k.tolist(), "s": s.tolist(), "x": x.tolist(), "d": d, "h": h}))
"""


def test_environment_switch():
    """NW_WIRE_DECODE=device makes the unchanged nw_primary_messages_verify_wire decode on the
    device (read once per process, hence a child)."""
    com, frames, _, _ = corpus(4)
    host = run(com, frames, None)
    assert (host[3], host[4]) == (0, len(frames))     # no switch here: host decode
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NW_WIRE_DECODE="device")
    p = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(tests), tests)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert r["k"] == host[0].tolist() and r["s"] == host[1].tolist() and r["x"] == host[2].tolist()
    assert (r["d"], r["h"]) == (len(frames) - 1, 1)
