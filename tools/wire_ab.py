#!/usr/bin/env python3
"""A/B of the wire ingest's two decoders in ONE process: host decode
(nw_primary_messages_verify_wire_ex, flags 0) against device decode (NW_WIRE_DECODE_DEVICE)
over the same frames, alternating round by round after a warm-up of both, so that clock
state, key tables and pooled buffers are shared. The workload is the bench's wire leg:
N = 4 certificate frames built by wire.frames_from_stream, 1 % with one invalid vote.
Prints one JSON line per round and a summary line (median, min, max per path, and whether
the device path wins by more than the spread between rounds of the same path).

    tools/wire_ab.py [--frames 65536] [--rounds 5] [--calls 3] [--committee 4]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from narwhal_amd import _lib, crypto as C, messages as M, wire as WI, workloads as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per round and path")
    ap.add_argument("--committee", type=int, default=4)
    a = ap.parse_args()
    L = _lib.lib()
    n, N = a.frames, a.committee
    keys = [(bytes(pk), bytes(sd) + bytes(pk)) for sd, pk in
            zip(W.fixture_seeds(N), C.keypair_from_seed_many(W.fixture_seeds(N)))]
    s = W.certificate_stream(n, keys, lambda sk, m: C.sign_many(sk, m),
                             lambda d, o: C.sha512_digest32_many(d, o[:-1], np.diff(o)), seed=100)
    s, exp_st, exp_ix = W.mutate_votes(s, np.arange(50, n, 100), seed=N + 7)
    data, offs = WI.frames_from_stream(s)
    com = M.committee_struct(s["committee"])
    kind, st, ix = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)

    def call(flags):
        st[:] = -1
        _lib.check(L.nw_primary_messages_verify_wire_ex(ctypes.byref(com), M._p(data), M._p(offs),
                                                        n, flags, M._p(kind), M._p(st), M._p(ix)),
                   "wire")
        return bool(np.array_equal(st, exp_st) and np.array_equal(ix, exp_ix)
                    and (kind == WI.MSG_CERTIFICATE).all())

    paths = (("host", 0), ("device", WI.WIRE_DECODE_DEVICE))
    for _ in range(2):                      # warm-up: buffers, key tables, clocks
        for _, fl in paths:
            assert call(fl), "parity"
    rates = {"host": [], "device": []}
    for r in range(a.rounds):
        for name, fl in paths:
            d0, h0 = WI.stats()
            t0 = time.perf_counter()
            ok = all([call(fl) for _ in range(a.calls)])
            sec = (time.perf_counter() - t0) / a.calls
            d1, h1 = WI.stats()
            rates[name].append(n / sec / 1e6)
            print(json.dumps({"round": r, "path": name, "frames": n, "frame_bytes": int(offs[-1]),
                              "ms_per_call": round(sec * 1e3, 3),
                              "Mcerts_s": round(n / sec / 1e6, 2), "parity": "ok" if ok else "FAIL",
                              "device_frames": d1 - d0, "host_frames": h1 - h0}), flush=True)
    summ = {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2),
                "max": round(max(v), 2)} for k, v in rates.items()}
    spread = max(summ[k]["max"] - summ[k]["min"] for k in summ)
    summ["device_wins_beyond_spread"] = bool(summ["device"]["min"] - summ["host"]["max"] > spread)
    print(json.dumps({"summary": summ, "committee": N, "frames": n}), flush=True)


if __name__ == "__main__":
    main()
