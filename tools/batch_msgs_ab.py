#!/usr/bin/env python3
"""A/B of verify_batch over per-vote messages (nw_verify_batch_msgs_many, DESIGN.md 5 "Round 17")
against the digest entry (nw_verify_batch_many) on the SAME votes in ONE process: every vote of a
batch signs the batch's 32-byte digest, so both entries are valid over the corpus (the new entry
takes each vote's message as the 32 bytes of its batch's digest). The two alternate round by round
after one untimed call each, `--launches` timed calls per entry and round. Prints one JSON line
per shape: the medians, every round's medians, the ratio new / digest round by round as median
(min-max), the digest entry's own rounds over their median (its spread), and the parity of the
verdicts.

Shapes: 9000x30 and 65536x4, each with the registry cleared and with the signers registered
(NAME#cleared, NAME#registered); 1x10000 (a lone large batch: the digest entry's fused launches
against the separate kernels); 9000x30m200 and 9000x30m1024: the first shape's batches with
messages of 200 and 1,024 bytes, new entry only (4,096 unique votes signed by the oracle, tiled).

    tools/batch_msgs_ab.py [--shapes NAME ...] [--rounds 5] [--launches 3] [--keys 64]
                           [--only digest|msgs]

--only runs one entry alone (e.g. for a kernel trace of the hash kernel's own time)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from narwhal_amd import _lib  # noqa: E402
from narwhal_amd import crypto as C  # noqa: E402

# batches, votes per batch, message bytes (32: the batch digest, both entries), registry
SHAPES = {"9000x30#cleared": (9000, 30, 32, False), "9000x30#registered": (9000, 30, 32, True),
          "65536x4#cleared": (65536, 4, 32, False), "65536x4#registered": (65536, 4, 32, True),
          "1x10000": (1, 10000, 32, False),
          "9000x30m200": (9000, 30, 200, False), "9000x30m1024": (9000, 30, 1024, False)}
UNIQUE = 4096


def digest_corpus(nb, q, nkeys, seed):
    """nb batches of q votes signed round-robin by nkeys keys over their batch's digest."""
    rng = np.random.Generator(np.random.PCG64(seed))
    seeds = rng.integers(0, 256, size=(nkeys, 32), dtype=np.uint8)
    pks = C.keypair_from_seed_many(seeds)
    sks = np.concatenate([seeds, pks], axis=1)
    key = np.arange(nb * q) % nkeys
    dig = rng.integers(0, 256, size=(nb, 32), dtype=np.uint8)
    sigs = C.sign_many(sks[key], np.repeat(dig, q, axis=0))
    moffs = (32 * np.repeat(np.arange(nb), q)).astype(np.uint64)
    return (dig, dig.reshape(-1), moffs, np.full(nb * q, 32, np.uint64),
            np.ascontiguousarray(pks[key]), sigs, pks)


def message_corpus(nb, q, length, nkeys, seed):
    """The same shape over messages of `length` bytes: UNIQUE votes signed by the oracle (test
    infrastructure, used here as the signer only), vote i of the call is unique vote i mod UNIQUE
    (message ranges may repeat)."""
    from oracle import oracle as O
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(nkeys)]
    data = rng.integers(0, 256, size=UNIQUE * length, dtype=np.uint8)
    upk = np.array([np.frombuffer(kps[i % nkeys][0], np.uint8) for i in range(UNIQUE)])
    usig = np.array([np.frombuffer(O.sign(kps[i % nkeys][1],
                                          data[i * length:(i + 1) * length].tobytes()), np.uint8)
                     for i in range(UNIQUE)])
    u = np.arange(nb * q) % UNIQUE
    return (None, data, (u * length).astype(np.uint64), np.full(nb * q, length, np.uint64),
            np.ascontiguousarray(upk[u]), np.ascontiguousarray(usig[u]),
            np.array([np.frombuffer(k[0], np.uint8) for k in kps]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--only", default=None, choices=["digest", "msgs"])
    a = ap.parse_args()
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    P = lambda x: ctypes.c_void_p(x.ctypes.data)
    for name in a.shapes:
        nb, q, length, registered = SHAPES[name]
        make = digest_corpus if length == 32 else message_corpus
        args = (nb, q, a.keys, 1700) if length == 32 else (nb, q, length, a.keys, 1700)
        dig, data, moffs, mlens, pk, sigs, keys = make(*args)
        off = (np.arange(nb + 1) * q).astype(np.uint64)
        st = {"digest": np.full(nb, -1, np.int32), "msgs": np.full(nb, -1, np.int32)}
        fi = np.zeros(nb, np.uint64)

        def call(entry):
            if entry == "digest":
                rc = L.nw_verify_batch_many(P(dig), P(pk), P(sigs), P(off), nb, None,
                                            P(st[entry]))
            else:
                rc = L.nw_verify_batch_msgs_many(P(data), P(moffs), P(mlens), P(pk), P(sigs),
                                                 P(off), nb, None, P(st[entry]), P(fi))
            assert rc == 0, L.nw_last_error()

        entries = [e for e in ("digest", "msgs") if (dig is not None or e == "msgs")
                   and a.only in (None, e)]
        reg = keys if registered else keys[:0]
        rc = L.nw_strict_signers_set(P(reg) if len(reg) else None, len(reg))
        assert rc == 0, L.nw_last_error()
        before = C.batch_signers_stats() + C.batch_signers_vote_stats()
        for e in entries:   # untimed: buffers, tables, clocks
            call(e)
        delta = [y - x for x, y in
                 zip(before, C.batch_signers_stats() + C.batch_signers_vote_stats())]
        times = {e: [] for e in entries}
        for _ in range(a.rounds):
            for e in entries:
                ts = []
                for _ in range(a.launches):
                    t0 = time.perf_counter()
                    call(e)
                    ts.append((time.perf_counter() - t0) * 1e3)
                times[e].append(float(np.median(ts)))
        L.nw_strict_signers_set(None, 0)
        line = {"shape": name, "batches": nb, "votes": nb * q, "message_bytes": length,
                "keys": a.keys, "registered": registered, "rounds": a.rounds,
                "launches": a.launches, "stats_delta": delta,
                "all_ok": bool(all((st[e] == 0).all() for e in entries))}
        for e in entries:
            line[e + "_ms"] = float(np.median(times[e]))
            line[e + "_round_medians_ms"] = times[e]
        if len(entries) == 2:
            r = np.array(times["msgs"]) / np.array(times["digest"])
            d = np.array(times["digest"]) / np.median(times["digest"])
            line["ratio_msgs_over_digest"] = {"median": float(np.median(r)), "min": float(r.min()),
                                              "max": float(r.max())}
            line["digest_rounds_over_median"] = {"min": float(d.min()), "max": float(d.max())}
            line["parity"] = bool(np.array_equal(st["digest"], st["msgs"]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
