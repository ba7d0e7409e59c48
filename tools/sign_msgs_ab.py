#!/usr/bin/env python3
"""A/B timing of signing over messages of any length against the 32-byte signer, in ONE process
(GPU box).

    python tools/sign_msgs_ab.py [--items N] [--keys K] [--reps R] [--steps S] [--out FILE]

N items (default 1,048,576) under K keys (default 4,096; item i signs under key i mod K), every
input resident on the device: the keys come from nw_keypair_from_seed_many, the messages are
random bytes. Variants:

    y32    nw_dev_sign_many       over 32-byte digests: the yardstick
    m32    nw_dev_sign_msgs_many  over the same 32 bytes as messages
    m200   nw_dev_sign_msgs_many  over 200-byte messages
    m1024  nw_dev_sign_msgs_many  over 1,024-byte messages

After one warm-up launch of each, the variants alternate round-robin over R rounds of S launches
timed with device events, so clock drift hits all of them alike; one JSON line per variant with
the median of each round (rep_medians_ms), then one line of the ratios m / y32 with their range
over the rounds (a difference counts only beyond y_spread, the spread of the yardstick's own
rounds). m32's output must equal y32's array for array (equal_y32), and a few items of every
variant are compared with the oracle (oracle_ok). There is no pass / fail threshold on the times."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from narwhal_amd import _lib  # noqa: E402
from narwhal_amd import crypto as C  # noqa: E402
from oracle import oracle as O  # noqa: E402

LENGTHS = {"y32": 32, "m32": 32, "m200": 200, "m1024": 1024}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    stream = ctypes.c_void_p(ts.cuda_stream)
    L = _lib.lib()
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    n = a.items
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    rng = np.random.Generator(np.random.PCG64(1800))
    seeds = rng.integers(0, 256, size=(a.keys, 32), dtype=np.uint8)
    sks_host = np.concatenate([seeds, C.keypair_from_seed_many(seeds)], axis=1)
    idx = torch.arange(n, dtype=torch.int64, device=dev) % a.keys
    sks = torch.from_numpy(sks_host).to(dev).index_select(0, idx).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1801)
    corp = {}
    for length in sorted(set(LENGTHS.values())):
        corp[length] = {
            "m": torch.randint(0, 256, (n, length), dtype=torch.uint8, device=dev, generator=gen),
            "off": torch.arange(n, dtype=torch.int64, device=dev) * length,
            "len": torch.full((n,), length, dtype=torch.int64, device=dev)}
    out = {v: torch.zeros((n, 64), dtype=torch.uint8, device=dev) for v in LENGTHS}
    torch.cuda.synchronize()

    def launch(v):
        c = corp[LENGTHS[v]]
        if v == "y32":
            rc = L.nw_dev_sign_many(P(sks), 64, P(c["m"]), 32, n, P(out[v]), stream)
        else:
            rc = L.nw_dev_sign_msgs_many(P(sks), 64, P(c["m"]), P(c["off"]), P(c["len"]), n,
                                         P(out[v]), stream)
        assert rc == 0, L.nw_last_error()

    # warm-up launch of each shape, and the checks on its output
    checks = {}
    spots = [0, 1, a.keys - 1, n // 2 + 3, n - 1]
    for v in LENGTHS:
        launch(v)
        torch.cuda.synchronize()
        got = out[v][spots].cpu().numpy()
        msgs = corp[LENGTHS[v]]["m"][spots].cpu().numpy()
        checks[v] = all(got[j].tobytes() == O.sign(sks_host[i % a.keys].tobytes(), msgs[j].tobytes())
                        for j, i in enumerate(spots))
    equal_y32 = bool(torch.equal(out["y32"], out["m32"]))

    times = {v: [] for v in LENGTHS}
    for _ in range(a.reps):
        for v in LENGTHS:
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(a.steps)]
            for e0, e1 in evs:
                e0.record()
                launch(v)
                e1.record()
            torch.cuda.synchronize()
            times[v] += [e0.elapsed_time(e1) for e0, e1 in evs]
    meds = {}
    for v in LENGTHS:
        meds[v] = [float(np.median(times[v][r * a.steps:(r + 1) * a.steps]))
                   for r in range(a.reps)]
        ms = float(np.median(times[v]))
        line = {"variant": v, "items": n, "keys": a.keys, "message_bytes": LENGTHS[v],
                "median_ms": ms, "signatures_per_s": n / ms * 1e3,
                "min_ms": float(np.min(times[v])), "rep_medians_ms": meds[v],
                "oracle_ok": checks[v]}
        if v == "m32":
            line["equal_y32"] = equal_y32
        emit(line)
    base = meds["y32"]
    ratios = {"y_median_ms": float(np.median(base)),
              "y_spread": [min(base) / float(np.median(base)), max(base) / float(np.median(base))]}
    for v in ("m32", "m200", "m1024"):
        q = [x / y for x, y in zip(meds[v], base)]
        ratios[f"{v}/y32"] = {"median": float(np.median(q)), "min": min(q), "max": max(q)}
    emit(ratios)
    assert equal_y32 and all(checks.values()), (equal_y32, checks)


if __name__ == "__main__":
    main()
