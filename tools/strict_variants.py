#!/usr/bin/env python3
"""A/B timing of k_verify_strict builds in ONE process (GPU box).

    python tools/strict_variants.py [--items N] [--reps R] [--steps K] LIB [LIB ...]

Each LIB is a build of libnarwhal_amd.so (the in-tree one, or exp/<v>/libnarwhal_amd.so
built here with one kernel change). All are loaded side by side (ctypes, RTLD_LOCAL: every
copy has its own HIP module and constants), the config-4 corpus is built once (bench.py's
build_strict_corpus with the in-tree library), and the variants are timed interleaved
round-robin over R rounds of K launches, so clock drift hits all of them alike. Every
variant's statuses must equal the in-tree build's. One JSON line per variant, with the
median of each round (rep_medians_ms): a difference between two variants counts only
beyond the spread of one variant's own rounds.

Build knobs of the two-pass path (tools/build_variant.sh NAME "-D..."): NW_TRIAGE_WAVES,
NW_STRICT_WAVES, NW_PF_SWAP, NW_ADD_NEGC.

A variant may also be a run-time knob of one build: LIB@NAME=VALUE sets that environment
variable around the variant's launches (knobs read per launch only: NW_STRICT_KEYS, the
slots of the call's key set, 0 = off; NW_TRIAGE_SLICE; NW_STRICT_COMB_DECIDE, 0 = the comb
check's verdict is not carried to the triage, every listed item takes the ladder), e.g.
    LIB LIB@NW_STRICT_KEYS=0
--flood: every second item's message gets a flipped bit (a flood of wrong-message signatures
under the corpus's keys: those items fail the equation under whatever key they carry).
A library that has nw_dev_strict_decided_stats reports it for the variant's last launch
(decided_stats: items the triage settled as equation failures, items handed to the ladder),
one that has nw_dev_strict_keymajor_stats the key-major order's (keymajor_stats: items the sort
placed, key bins used, slices sorted; LIB@NW_STRICT_KEY_MAJOR=0 / =1 turns the order off / on).
--keys K: the corpus's signers (bench.py's config 4 has 4,096); K = 0: every item has a key
of its own (then all items are valid: keys and signatures made on the device, no edits).
--signers: every LIB becomes two variants of the same library and corpus, LIB#registered (the
corpus's K signers registered with nw_strict_signers_set before the round's launches) and
LIB#cleared (the registry emptied), alternating round by round (--registered-only: the first
alone, for a kernel trace).
--host-calls C: time C blocking host-buffer calls per round instead of device launches
(nw_signature_verify for --items 1, else nw_verify_strict_many), wall clock per call.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def split_variant(spec):
    """'LIB' or 'LIB@NAME=VALUE' -> (path, env dict)."""
    path, _, knob = spec.partition("@")
    env = {}
    if knob:
        k, _, v = knob.partition("=")
        env[k] = v
    return path, env


def distinct_key_corpus(dev, stream, n, seed):
    """n valid items, every one under its own key (device keygen and signing)."""
    from narwhal_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(seed)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(dev)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(dev)
    pks = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    bench.check(L.nw_dev_keypair_from_seed_many(bench.ptr(seeds), n, bench.ptr(pks), stream), "keygen")
    sks = torch.cat([seeds, pks], dim=1).contiguous()
    sigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    bench.check(L.nw_dev_sign_many(bench.ptr(sks), 64, bench.ptr(msgs), 32, n, bench.ptr(sigs), stream), "sign")
    torch.cuda.synchronize()
    return msgs, pks, sigs


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    P, S, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.nw_init.restype = I
    L.nw_set_device.argtypes = [I]
    L.nw_last_error.restype = ctypes.c_char_p
    L.nw_dev_verify_strict_many.argtypes = [P, S, P, P, S, P, P, P]
    L.nw_dev_verify_strict_many.restype = I
    L.nw_verify_strict_many.argtypes = [P, S, P, P, S, P, P]
    L.nw_verify_strict_many.restype = I
    L.nw_signature_verify.argtypes = [P, P, P]
    L.nw_signature_verify.restype = I
    if hasattr(L, "nw_strict_signers_set"):
        L.nw_strict_signers_set.argtypes = [P, S]
        L.nw_strict_signers_set.restype = I
    assert L.nw_init() > 0, L.nw_last_error()
    assert L.nw_set_device(0) == 0
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=12_500_000)
    ap.add_argument("--unique", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--all-valid", action="store_true",
                    help="tile only the corpus's valid items (no early-decided statuses)")
    ap.add_argument("--keys", type=int, default=4096,
                    help="signers of the corpus; 0 = a key per item (all valid)")
    ap.add_argument("--flood", action="store_true",
                    help="flip a message bit of every second item (wrong-message flood)")
    ap.add_argument("--signers", action="store_true",
                    help="each LIB as LIB#registered and LIB#cleared (nw_strict_signers_set)")
    ap.add_argument("--registered-only", action="store_true",
                    help="with --signers: the registered variant alone (for a kernel trace)")
    ap.add_argument("--host-calls", type=int, default=0,
                    help="time this many blocking host-buffer calls per round, not launches")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    if a.signers:
        tags = ("#registered",) if a.registered_only else ("#registered", "#cleared")
        a.libs = [x + tag for x in a.libs for tag in tags]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    stream = ctypes.c_void_p(ts.cuda_stream)
    from narwhal_amd import _lib
    assert _lib.lib().nw_init() > 0
    n = a.items
    if a.keys == 0:
        m, p, s = distinct_key_corpus(dev, stream, n, seed=1000)
        exp = np.ones(n, dtype=bool)
    else:
        m_u, p_u, s_u, valid = bench.build_strict_corpus(dev, stream, a.unique, a.keys, seed=1000)
        if a.all_valid:
            good = torch.from_numpy(np.nonzero(valid)[0]).to(dev)
            idx = good[torch.arange(n, dtype=torch.int64, device=dev) % good.numel()]
            valid = np.ones(good.numel(), dtype=bool)
        else:
            idx = torch.arange(n, dtype=torch.int64, device=dev) % a.unique
        m, p, s = (t.index_select(0, idx).contiguous() for t in (m_u, p_u, s_u))
        del idx
        exp = np.resize(valid, n)
    if a.flood:
        m[::2, :2] ^= 1   # two bits: the corpus's own wrong-message items flip one
        exp[::2] = False
    variants = [split_variant(x.partition("#")[0]) for x in a.libs]
    signers = None
    if a.signers:   # the K most used keys of the corpus
        keys, counts = np.unique(p.cpu().numpy(), axis=0, return_counts=True)
        signers = np.ascontiguousarray(keys[np.argsort(-counts, kind="stable")[:max(a.keys, 1)]])
    hm, hp, hs = ((t.cpu().numpy() for t in (m, p, s)) if a.host_calls else (None,) * 3)
    hst, hbm = np.zeros(n, np.int32), np.zeros((n + 7) // 8, np.uint8)
    loaded = {}
    for path, _ in variants:
        if path not in loaded:
            loaded[path] = load(path)
    libs = [loaded[path] for path, _ in variants]
    st = torch.empty(n, dtype=torch.int32, device=dev)
    bm = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    times = {x: [] for x in a.libs}
    ok = {}
    decided = {}
    keymajor = {}
    for rep in range(a.reps):
        for name, L, (_, env) in zip(a.libs, libs, variants):
            if a.signers:
                reg = signers if name.endswith("#registered") else signers[:0]
                rc = L.nw_strict_signers_set(reg.ctypes.data if len(reg) else None, len(reg))
                assert rc == 0, L.nw_last_error()

            def launch():
                old = {k: os.environ.get(k) for k in env}
                os.environ.update(env)
                try:
                    if not a.host_calls:
                        rc = L.nw_dev_verify_strict_many(P(m), 32, P(p), P(s), n, P(st), P(bm), stream)
                    elif n == 1:
                        rc = L.nw_signature_verify(hs.ctypes.data, hm.ctypes.data, hp.ctypes.data)
                        hst[0] = rc
                        rc = min(rc, 0)
                    else:
                        rc = L.nw_verify_strict_many(hm.ctypes.data, 32, hp.ctypes.data,
                                                     hs.ctypes.data, n, hst.ctypes.data,
                                                     hbm.ctypes.data)
                finally:
                    for k, v in old.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                assert rc == 0, L.nw_last_error()
            launch()
            torch.cuda.synchronize()
            if rep == 0:
                ok[name] = bool(np.array_equal((hst if a.host_calls else st.cpu().numpy()) == 0, exp))
            if a.host_calls:
                for _ in range(a.host_calls):
                    t0 = time.perf_counter()
                    launch()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                continue
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(a.steps)]
            for e0, e1 in evs:
                e0.record()
                launch()
                e1.record()
            torch.cuda.synchronize()
            times[name] += [e0.elapsed_time(e1) for e0, e1 in evs]
            if hasattr(L, "nw_dev_strict_decided_stats"):
                d = (ctypes.c_uint64 * 2)()
                L.nw_dev_strict_decided_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
                if L.nw_dev_strict_decided_stats(d, stream) == 0:
                    decided[name] = [int(d[0]), int(d[1])]
            if hasattr(L, "nw_dev_strict_keymajor_stats"):
                d = (ctypes.c_uint64 * 3)()
                L.nw_dev_strict_keymajor_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
                if L.nw_dev_strict_keymajor_stats(d, stream) == 0:
                    keymajor[name] = [int(d[0]), int(d[1]), int(d[2])]
    per = a.host_calls or a.steps
    if a.signers:
        for L in loaded.values():
            L.nw_strict_signers_set(None, 0)
    for name in a.libs:
        ms = float(np.median(times[name]))
        print(json.dumps({"lib": name, "median_ms": ms, "verifies_per_s": n / ms * 1e3,
                          "min_ms": float(np.min(times[name])),
                          "rep_medians_ms": [float(np.median(times[name][r * per:(r + 1) * per]))
                                             for r in range(a.reps)],
                          "parity": ok[name],
                          **({"decided_stats": decided[name]} if name in decided else {}),
                          **({"keymajor_stats": keymajor[name]} if name in keymajor else {})}),
              flush=True)


if __name__ == "__main__":
    main()
