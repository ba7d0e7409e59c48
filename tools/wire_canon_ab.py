#!/usr/bin/env python3
"""A/B of the wire ingest's three decode paths in ONE process: host decode (flags 0), device
decode (NW_WIRE_DECODE_DEVICE, which hands non-canonical frames back to the host) and device
decode with canonicalisation (| NW_WIRE_CANON_DEVICE), alternating round by round after a
warm-up of all three, as tools/wire_ab.py does for two. Parity is checked on every call.

Workloads:
  --reorder PCT   the bench's wire leg (N = 4 certificate frames, 1 % with one invalid vote)
                  with the parents of PCT % of the frames reversed on the wire; the decoded
                  certificates, and so the expected verdicts, are unchanged. PCT = 0: nothing
                  is reordered (what the canon launch and read-back cost where they do nothing).
  --worst         --frames header frames of 1,018 parents each in random order, the most a
                  frame under the default 32 KiB cap holds; validly signed, expected status 0.

Prints one JSON line per round and path and a summary line: median, min, max per path, the
spread between rounds of the same path, whether canon beats device (and device beats canon)
by more than that spread, and whether canon's median lies below, inside or above the range
of the device path's rounds.

    tools/wire_canon_ab.py [--frames 65536] [--rounds 5] [--calls 3] [--reorder 10 | --worst]
"""
import argparse
import base64
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from narwhal_amd import _lib, crypto as C, messages as M, wire as WI, workloads as W  # noqa: E402


def keys_of(N):
    return [(bytes(pk), bytes(sd) + bytes(pk)) for sd, pk in
            zip(W.fixture_seeds(N), C.keypair_from_seed_many(W.fixture_seeds(N)))]


def certificate_frames(n, N, pct):
    s = W.certificate_stream(n, keys_of(N), lambda sk, m: C.sign_many(sk, m),
                             lambda d, o: C.sha512_digest32_many(d, o[:-1], np.diff(o)), seed=100)
    s, exp_st, exp_ix = W.mutate_votes(s, np.arange(50, n, 100), seed=N + 7)
    data, offs = WI.frames_from_stream(s)
    nre = 0
    if pct:
        sel = np.random.default_rng(3).permutation(n)[:n * pct // 100]
        for i in sel:
            a = int(offs[i]) + 4
            a += 8 + int(data[a:a + 8].view(np.uint64)[0]) + 8          # author key, round
            a += 8 + 36 * int(data[a:a + 8].view(np.uint64)[0])         # payload
            nq = int(data[a:a + 8].view(np.uint64)[0])
            par = data[a + 8:a + 8 + 32 * nq].reshape(nq, 32)
            par[:] = par[::-1].copy()
            nre += nq >= 2
    return s["committee"], data, offs, exp_st, exp_ix, WI.MSG_CERTIFICATE, nre


def worst_frames(n, N, nparents=1018):
    keys = keys_of(N)
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (n, nparents, 32), dtype=np.uint8)
    hbs, frames = [], []
    for i in range(n):
        par = [raw[i, j].tobytes() for j in range(nparents)]
        hbs.append(keys[i % N][0] + struct.pack("<Q", 1 + i) + b"".join(sorted(set(par))))
    ho = np.zeros(n + 1, np.uint64)
    ho[1:] = np.cumsum([len(h) for h in hbs])
    ids = C.sha512_digest32_many(np.frombuffer(b"".join(hbs), np.uint8), ho[:-1], np.diff(ho))
    sks = np.array([np.frombuffer(keys[i % N][1], np.uint8) for i in range(n)])
    sigs = C.sign_many(sks, ids)
    for i in range(n):
        pk = base64.b64encode(keys[i % N][0])
        frames.append(struct.pack("<I", WI.MSG_HEADER) + struct.pack("<Q", len(pk)) + pk
                      + struct.pack("<Q", 1 + i) + struct.pack("<Q", 0)
                      + struct.pack("<Q", nparents) + raw[i].tobytes()
                      + ids[i].tobytes() + sigs[i].tobytes())
    data, offs = WI.frames_soa(frames)
    com = {"pks": np.array([np.frombuffer(pk, np.uint8) for pk, _ in sorted(keys)]),
           "stakes": np.ones(N, np.uint32), "worker_offsets": np.arange(N + 1, dtype=np.uint64),
           "worker_ids": np.zeros(N, np.uint32)}
    return com, data, offs, np.zeros(n, np.int32), np.zeros(n, np.uint64), WI.MSG_HEADER, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per round and path")
    ap.add_argument("--committee", type=int, default=4)
    ap.add_argument("--reorder", type=int, default=0, help="percent of frames with reversed parents")
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--paths", default="host,device,canon")
    a = ap.parse_args()
    L = _lib.lib()
    n, N = a.frames, a.committee
    if a.worst:
        com_d, data, offs, exp_st, exp_ix, exp_kind, nre = worst_frames(n, N)
    else:
        com_d, data, offs, exp_st, exp_ix, exp_kind, nre = certificate_frames(n, N, a.reorder)
    com = M.committee_struct(com_d)          # (points into com_d's arrays)
    kind, st, ix = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)

    def call(flags):
        st[:] = -1
        _lib.check(L.nw_primary_messages_verify_wire_ex(ctypes.byref(com), M._p(data), M._p(offs),
                                                        n, flags, M._p(kind), M._p(st), M._p(ix)),
                   "wire")
        return bool(np.array_equal(st, exp_st) and np.array_equal(ix, exp_ix)
                    and (kind == exp_kind).all())

    flags = {"host": 0, "device": WI.WIRE_DECODE_DEVICE,
             "canon": WI.WIRE_DECODE_DEVICE | WI.WIRE_CANON_DEVICE}
    paths = [(p, flags[p]) for p in a.paths.split(",")]
    for _ in range(2):                      # warm-up: buffers, key tables, clocks
        for _, fl in paths:
            assert call(fl), "parity"
    rates = {p: [] for p, _ in paths}
    for r in range(a.rounds):
        for name, fl in paths:
            d0, h0 = WI.stats()
            t0 = time.perf_counter()
            ok = all([call(fl) for _ in range(a.calls)])
            sec = (time.perf_counter() - t0) / a.calls
            d1, h1 = WI.stats()
            rates[name].append(n / sec / 1e6)
            print(json.dumps({"round": r, "path": name, "frames": n, "frame_bytes": int(offs[-1]),
                              "reordered": int(nre), "ms_per_call": round(sec * 1e3, 3),
                              "Mframes_s": round(n / sec / 1e6, 3), "parity": "ok" if ok else "FAIL",
                              "device_frames": d1 - d0, "host_frames": h1 - h0}), flush=True)
    summ = {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                "max": round(max(v), 3)} for k, v in rates.items()}
    spread = max(summ[k]["max"] - summ[k]["min"] for k in summ)
    out = {"summary": summ, "spread": round(spread, 3), "committee": N, "frames": n,
           "reordered": int(nre), "workload": "worst" if a.worst else f"reorder{a.reorder}"}
    if "canon" in summ and "device" in summ:
        out["canon_wins_beyond_spread"] = bool(summ["canon"]["min"] - summ["device"]["max"] > spread)
        out["device_wins_beyond_spread"] = bool(summ["device"]["min"] - summ["canon"]["max"] > spread)
        dv, cm = summ["device"], summ["canon"]["median"]
        # where canon's median lies against the rounds of the device path in this process
        out["canon_median_vs_device_rounds"] = ("below" if cm < dv["min"] else
                                                "above" if cm > dv["max"] else "inside")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
