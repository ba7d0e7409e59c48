#!/usr/bin/env python3
"""A/B timing of the strict launch over messages of any length against the 32-byte launch, in
ONE process (GPU box).

    python tools/strict_msgs_ab.py [--items N] [--unique U] [--keys K] [--reps R] [--steps S]
                                   [--only NAME]

The yardstick is the existing launch on the same items: U unique items under K signers, a tenth
of them invalid (half a flipped message bit, a quarter each a flipped bit of s and of R), signed
and judged by the oracle over the message's own bytes, tiled to N items on the device. Variants:

    a32    nw_dev_verify_strict_many       on 32-byte messages
    b32    nw_dev_verify_strict_msgs_many  on the same 32-byte messages (the price of the hash
           kernel and of the 32 B / item k plane)
    c200   nw_dev_verify_strict_msgs_many  on 200-byte messages
    d1024  nw_dev_verify_strict_msgs_many  on 1,024-byte messages

each with the registry cleared (NAME#cleared) and with the K signers registered
(NAME#registered, nw_strict_signers_set). The variants alternate round-robin over R rounds of S
launches, so clock drift hits all of them alike; one JSON line per variant with the median of
each round (rep_medians_ms), then one line of the ratios b / a, c / a and d / a per registry
state, each with the spread of its per-round ratios: a difference counts only beyond the spread
of a's own rounds (a_spread). Every variant's verdicts must equal the oracle's (parity).
--only NAME runs one variant alone (e.g. b32#registered, for a kernel trace)."""
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
from oracle import oracle as O  # noqa: E402

LENGTHS = {"a32": 32, "b32": 32, "c200": 200, "d1024": 1024}


def unique_items(u, nkeys, length, seed):
    """u items of `length` bytes under nkeys signers (item i: key i mod nkeys), a tenth invalid:
    (msgs u x length, pks, sigs, valid)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = [O.keypair_from_seed(rng.bytes(32)) for _ in range(nkeys)]
    msgs = rng.integers(0, 256, size=(u, length), dtype=np.uint8)
    pks = np.zeros((u, 32), np.uint8)
    sigs = np.zeros((u, 64), np.uint8)
    for i in range(u):
        pk, sk = kps[i % nkeys]
        pks[i] = np.frombuffer(pk, np.uint8)
        sigs[i] = np.frombuffer(O.sign(sk, msgs[i].tobytes()), np.uint8)
    bad = rng.choice(u, u // 10, replace=False)
    for j, i in enumerate(bad):
        bit = np.uint8(1 << rng.integers(0, 8))
        if j % 4 < 2:
            msgs[i, rng.integers(0, length)] ^= bit
        elif j % 4 == 2:
            sigs[i, 32 + rng.integers(0, 31)] ^= bit
        else:
            sigs[i, rng.integers(0, 32)] ^= bit
    valid = np.array([O.verify_strict(msgs[i].tobytes(), pks[i].tobytes(), sigs[i].tobytes()) == 0
                      for i in range(u)])
    return msgs, pks, sigs, valid, kps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--unique", type=int, default=1 << 14)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--only", default=None, help="one variant alone, e.g. d1024#registered")
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
    names = [f"{v}#{r}" for r in ("cleared", "registered") for v in LENGTHS]
    if a.only:
        assert a.only in names, names
        names = [a.only]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    idx = torch.arange(n, dtype=torch.int64, device=dev) % a.unique
    corp, signers = {}, None
    for length in sorted({LENGTHS[x.partition("#")[0]] for x in names}):
        m, p, s, valid, kps = unique_items(a.unique, a.keys, length, seed=1000)
        signers = np.ascontiguousarray(
            np.array([np.frombuffer(k[0], np.uint8) for k in kps]).reshape(-1, 32))
        md, pd, sd = (torch.from_numpy(x).to(dev).index_select(0, idx).contiguous()
                      for x in (m, p, s))
        corp[length] = {"m": md, "p": pd, "s": sd, "exp": np.resize(valid, n),
                        "off": torch.arange(n, dtype=torch.int64, device=dev) * length,
                        "len": torch.full((n,), length, dtype=torch.int64, device=dev)}
    st = torch.empty(n, dtype=torch.int32, device=dev)
    bm = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def launch(name):
        v = name.partition("#")[0]
        c = corp[LENGTHS[v]]
        if v == "a32":
            rc = L.nw_dev_verify_strict_many(P(c["m"]), 32, P(c["p"]), P(c["s"]), n, P(st), P(bm),
                                             stream)
        else:
            rc = L.nw_dev_verify_strict_msgs_many(P(c["m"]), P(c["off"]), P(c["len"]), P(c["p"]),
                                                  P(c["s"]), n, P(st), P(bm), stream)
        assert rc == 0, L.nw_last_error()

    times = {x: [] for x in names}
    parity = {}
    for rep in range(a.reps):
        for name in names:
            reg = signers if name.endswith("#registered") else signers[:0]
            rc = L.nw_strict_signers_set(reg.ctypes.data if len(reg) else None, len(reg))
            assert rc == 0, L.nw_last_error()
            st.fill_(-99)
            torch.cuda.synchronize()
            launch(name)
            torch.cuda.synchronize()
            if rep == 0:
                exp = corp[LENGTHS[name.partition("#")[0]]]["exp"]
                parity[name] = bool(np.array_equal(st.cpu().numpy() == 0, exp))
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(a.steps)]
            for e0, e1 in evs:
                e0.record()
                launch(name)
                e1.record()
            torch.cuda.synchronize()
            times[name] += [e0.elapsed_time(e1) for e0, e1 in evs]
    L.nw_strict_signers_set(None, 0)
    meds = {}
    for name in names:
        meds[name] = [float(np.median(times[name][r * a.steps:(r + 1) * a.steps]))
                      for r in range(a.reps)]
        ms = float(np.median(times[name]))
        print(json.dumps({"variant": name, "items": n, "median_ms": ms,
                          "verifies_per_s": n / ms * 1e3, "min_ms": float(np.min(times[name])),
                          "rep_medians_ms": meds[name], "parity": parity[name]}), flush=True)
    for r in ("cleared", "registered"):
        base = meds.get(f"a32#{r}")
        if not base:
            continue
        out = {"registry": r, "a_median_ms": float(np.median(base)),
               "a_spread": [min(base) / float(np.median(base)), max(base) / float(np.median(base))]}
        for v in ("b32", "c200", "d1024"):
            if f"{v}#{r}" in meds:
                q = [x / y for x, y in zip(meds[f"{v}#{r}"], base)]
                out[f"{v}/a32"] = {"median": float(np.median(q)), "min": min(q), "max": max(q)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
