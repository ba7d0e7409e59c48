#!/usr/bin/env python3
"""A/B of Signature::verify_batch under the registered signers (DESIGN.md 5 "Round 12"): the same
library in one process, rounds alternating between the registry set to the corpus' keys and
cleared, `--launches` timed nw_verify_batch_many calls per variant and round (one untimed call
first). Prints one JSON line per shape: medians, the medians of every round, whether every
registered round median is below the cleared variant's fastest round ("faster"), parity of the
verdicts between the variants, and the delta of nw_batch_signers_stats (and, where the library
has it, nw_batch_signers_vote_stats) of one registered call.

Shapes: 9000x30 (all valid), 9000x30b (1 % of the batches broken), 65536x4, 1x10000,
1x10000b (one vote broken), 1x34; 9000x30u and 65536x4u (every batch holds one valid vote under
a key left out of the registry), 1x10000c (100 votes broken).

--package-root DIR imports narwhal_amd from DIR, the build of another commit, so that the same
tool times both sides of a change (DESIGN.md 5 "Round 14": parent and tree alternating).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in sys.argv[1:-1]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, ROOT)

from narwhal_amd import _lib  # noqa: E402
from narwhal_amd import crypto as C  # noqa: E402

# batches, votes per batch, fraction of the batches broken, votes broken in each of those,
# whether every batch holds one valid vote under a key that is not registered
SHAPES = {"9000x30": (9000, 30, 0.0, 1, False), "9000x30b": (9000, 30, 0.01, 1, False),
          "65536x4": (65536, 4, 0.0, 1, False), "1x10000": (1, 10000, 0.0, 1, False),
          "1x10000b": (1, 10000, 1.0, 1, False), "1x34": (1, 34, 0.0, 1, False),
          "9000x30u": (9000, 30, 0.0, 1, True), "65536x4u": (65536, 4, 0.0, 1, True),
          "1x10000c": (1, 10000, 1.0, 100, False)}


def corpus(nb, q, broken, nbad, outsider, nkeys, seed):
    """nb batches of q votes signed round-robin by nkeys keys; a fraction `broken` of the batches
    (at least one when it is not 0) has the s of nbad votes changed, spread over the batch; with
    `outsider` the vote in the middle of every batch is signed by one more key, valid, which the
    returned registry leaves out."""
    rng = np.random.Generator(np.random.PCG64(seed))
    seeds = rng.integers(0, 256, size=(nkeys + 1, 32), dtype=np.uint8)
    pks = C.keypair_from_seed_many(seeds)
    sks = np.concatenate([seeds, pks], axis=1)
    key = np.arange(nb * q) % nkeys
    if outsider:
        key[np.arange(nb) * q + q // 2] = nkeys
    dig = rng.integers(0, 256, size=(nb, 32), dtype=np.uint8)
    sigs = C.sign_many(sks[key], np.repeat(dig, q, axis=0))
    bad = np.zeros(nb, bool)
    if broken:
        bad[rng.choice(nb, max(1, int(round(nb * broken))), replace=False)] = True
        for t in range(nbad):
            sigs[np.nonzero(bad)[0] * q + (q // 2 + t * (q // nbad)) % q, 40] ^= 1
    off = (np.arange(nb + 1) * q).astype(np.uint64)
    return dig, np.ascontiguousarray(pks[key]), sigs, off, pks[:nkeys], bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--package-root", default=None,
                    help="import narwhal_amd from this directory (a build of another commit)")
    ap.add_argument("--label", default="", help="copied into every line (e.g. parent, tree)")
    a = ap.parse_args()
    vote_stats = getattr(C, "batch_signers_vote_stats", None)   # absent before round 14
    stats = lambda: C.batch_signers_stats() + (vote_stats() if vote_stats else ())
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    P = lambda x: ctypes.c_void_p(x.ctypes.data)
    for name in a.shapes:
        nb, q, broken, nbad, outsider = SHAPES[name]
        dig, pk, sigs, off, keys, bad = corpus(nb, q, broken, nbad, outsider, a.keys, seed=1200)
        st = np.zeros(nb, np.int32)

        def call():
            rc = L.nw_verify_batch_many(P(dig), P(pk), P(sigs), P(off), nb, None, P(st))
            assert rc == 0, L.nw_last_error()

        times = {"registered": [], "cleared": []}
        verdicts, delta = {}, None
        for _ in range(a.rounds):
            for variant in ("registered", "cleared"):
                reg = keys if variant == "registered" else keys[:0]
                rc = L.nw_strict_signers_set(P(reg) if len(reg) else None, len(reg))
                assert rc == 0, L.nw_last_error()
                before = stats()
                call()
                if variant == "registered" and delta is None:
                    delta = [y - x for x, y in zip(before, stats())]
                verdicts.setdefault(variant, st.copy())
                ts = []
                for _ in range(a.launches):
                    t0 = time.perf_counter()
                    call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                times[variant].append(ts)
        L.nw_strict_signers_set(None, 0)
        med = {v: [float(np.median(r)) for r in times[v]] for v in times}
        print(json.dumps({
            "label": a.label, "shape": name, "batches": nb, "votes": nb * q, "keys": a.keys,
            "registered_ms": float(np.median(np.concatenate(times["registered"]))),
            "cleared_ms": float(np.median(np.concatenate(times["cleared"]))),
            "registered_round_medians_ms": med["registered"],
            "cleared_round_medians_ms": med["cleared"],
            "faster": bool(max(med["registered"]) < min(med["cleared"])),
            "slower": bool(min(med["registered"]) > max(med["cleared"])),
            "parity": bool(np.array_equal(verdicts["registered"], verdicts["cleared"]) and
                           np.array_equal(verdicts["cleared"] != 0, bad)),
            "stats_delta": delta}), flush=True)


if __name__ == "__main__":
    main()
