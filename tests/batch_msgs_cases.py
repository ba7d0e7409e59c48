"""Inputs and the reference verdict of verify_batch over per-vote messages of any length
(nw_verify_batch_msgs_many and its submit, device and host forms). Test infrastructure, built
with the oracle alone.

ref_verify_batch_msgs is the checker: the oracle has no per-message verify_batch, so the checks
that come before the equation are applied here in the order of the oracle's verify_batch, and the
equation is the oracle's own multi-scalar multiplication over [B, R_0.., A_0..], which decodes as
dalek does and whose identity flag keeps the torsion: exact for every coefficient set.

The corpus: batches of 0, 1, 2, 3, 5, 12 and 64 votes under 8 keys, every vote of a batch with a
message of its own whose length runs through strict_msgs_cases.LENGTHS at the four start
alignments; each size all-valid and damaged at its first, a middle and its last vote in every
way that must (or must not) change the verdict, and the cases in which two failures compete."""
import functools

import numpy as np

from oracle import oracle as O

import strict_msgs_cases as SM

L_ORDER = SM.L_ORDER
SIZES = (0, 1, 2, 3, 5, 12, 64)
# damage kind -> the status it must give (None: whatever the checker says; the batch path does
# not reject small order)
KINDS = {"msg_last_flipped": 7, "short_length": 7, "byte_after": 0, "s_plus_l": 2,
         "s_high_bit": 1, "a_off_curve": 3, "r_off_curve": 4, "small_r": None}
_BASE = (1).to_bytes(32, "little")


def ref_verify_batch_msgs(msgs, pks, sigs, z16):
    """(status, index) of one batch: vote i is (msgs[i], pks[i], sigs[i]) with coefficient
    z16[i] (16 bytes). index: the failing vote, or the batch's size for the equation / Ok."""
    n = len(msgs)
    pks = [bytes(p) for p in pks]
    sigs = [bytes(s) for s in sigs]
    for i in range(n):
        if sigs[i][63] & 0xE0:
            return O.ERR_S_HIGH_BITS, i
        if O.decompress(pks[i]) is None:
            return O.ERR_A_DECODE, i
    for i in range(n):
        if int.from_bytes(sigs[i][32:], "little") >= L_ORDER:
            return O.ERR_S_NONCANONICAL, i
    for i in range(n):
        if O.decompress(sigs[i][:32]) is None:
            return O.ERR_R_DECODE, i
    if n == 0:
        return O.OK, 0
    zs = [bytes(z) for z in z16]
    assert len(zs) == n and all(len(z) == 16 for z in zs)
    bsum = 0
    cs = []
    for m, pk, sig, z in zip(msgs, pks, sigs, zs):
        k = O.hram(sig[:32], pk, bytes(m))
        cs.append(O.scalar_mul(z + bytes(16), k))
        bsum += int.from_bytes(z, "little") * int.from_bytes(sig[32:], "little")
    scalars = [((-bsum) % L_ORDER).to_bytes(32, "little")] + [z + bytes(16) for z in zs] + cs
    points = [O.scalarmult_base(_BASE)] + [s[:32] for s in sigs] + pks
    r = O.msm(scalars, points)
    assert r is not None
    return (O.OK if r[1] else O.ERR_EQUATION), n


class Call:
    """One call's arrays as the entries take them: data, per-vote moffs / mlens / pks / sigs / z,
    the batch offsets off, and per batch its name and the checker's (status, index)."""

    def __init__(self, data, moffs, mlens, pks, sigs, z, off, names, ref_st, ref_ix):
        self.data, self.moffs, self.mlens = data, moffs, mlens
        self.pks, self.sigs, self.z, self.off = pks, sigs, z, off
        self.names, self.ref_st, self.ref_ix = names, ref_st, ref_ix
        self.nb, self.n = len(off) - 1, len(moffs)

    def take(self, batches) -> "Call":
        """The batches named (any order) as a call of its own over the same data."""
        batches = [int(b) for b in batches]
        o = self.off.astype(np.int64)
        idx = np.concatenate([np.arange(o[b], o[b + 1]) for b in batches] +
                             [np.zeros(0, np.int64)]).astype(np.int64)
        off = np.zeros(len(batches) + 1, np.uint64)
        off[1:] = np.cumsum([o[b + 1] - o[b] for b in batches])
        return Call(self.data, self.moffs[idx].copy(), self.mlens[idx].copy(),
                    self.pks[idx].copy(), self.sigs[idx].copy(), self.z[idx].copy(), off,
                    [self.names[b] for b in batches], self.ref_st[batches].copy(),
                    self.ref_ix[batches].copy())

    def with_z(self, z) -> "Call":
        """The same votes under other coefficients, judged again by the checker."""
        c = Call(self.data, self.moffs, self.mlens, self.pks, self.sigs,
                 np.ascontiguousarray(z, np.uint8).reshape(self.n, 16), self.off, self.names,
                 None, None)
        c.judge()
        return c

    def messages(self, b=None) -> list:
        lo, hi = (0, self.n) if b is None else (int(self.off[b]), int(self.off[b + 1]))
        return [self.data[int(o):int(o) + int(l)].tobytes()
                for o, l in zip(self.moffs[lo:hi], self.mlens[lo:hi])]

    def judge(self):
        st, ix = [], []
        for b in range(self.nb):
            lo, hi = int(self.off[b]), int(self.off[b + 1])
            s, i = ref_verify_batch_msgs(self.messages(b), self.pks[lo:hi], self.sigs[lo:hi],
                                         self.z[lo:hi])
            st.append(s)
            ix.append(i)
        self.ref_st, self.ref_ix = np.array(st, np.int32), np.array(ix, np.uint64)


def _off_curve() -> bytes:
    return SM._off_curve_key()


def build(specs, seed) -> Call:
    """specs: (name, size, [(vote, kind), ...]) per batch. Vote i of a batch of `size` votes signs
    a random message of its own of LENGTHS[(7 i + 11 size) % 30] bytes (the next length where a
    damaged vote would have none to flip or shorten; one byte more where the batch has the message)
    placed at start alignment (i + size) % 4, under key (i + size) % 8; then the damages."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kps = O.keys(8)
    bad = _off_curve()
    data = bytearray()
    moffs, mlens, pks, sigs, off, names, aligns = [], [], [], [], [0], [], []
    for name, size, damages in specs:
        dmg, seen = {}, set()
        for v, kind in damages:
            dmg.setdefault(v, []).append(kind)
        for i in range(size):
            li = (7 * i + 11 * size) % len(SM.LENGTHS)
            kinds = dmg.get(i, [])
            if SM.LENGTHS[li] == 0 and {"msg_last_flipped", "short_length"} & set(kinds):
                li += 1
            ln = SM.LENGTHS[li]
            pk, sk = kps[(i + size) % 8]
            msg = bytearray(rng.bytes(ln))
            while bytes(msg) in seen:   # a batch's messages differ: one empty one at most
                ln += 1
                msg = bytearray(rng.bytes(ln))
            seen.add(bytes(msg))
            s = bytearray(O.sign(sk, bytes(msg)))
            after = 0x00
            for kind in kinds:
                if kind == "msg_last_flipped":
                    msg[-1] ^= 0x01
                elif kind == "short_length":
                    ln -= 1
                elif kind == "byte_after":
                    after = 0xFF
                elif kind == "s_plus_l":
                    s[32:] = (int.from_bytes(s[32:], "little") + L_ORDER).to_bytes(32, "little")
                elif kind == "s_high_bit":
                    s[63] |= 0x80
                elif kind == "a_off_curve":
                    pk = bad
                elif kind == "r_off_curve":
                    s[:32] = bad
                elif kind == "small_r":
                    s[:32] = SM.SMALL_R
                else:
                    raise AssertionError(kind)
            align = (i + size) % 4
            data.append(0xA5)   # at least one filler byte, then up to the wanted alignment
            while len(data) % 4 != align:
                data.append(0x5A)
            moffs.append(len(data))
            data.extend(msg)
            data.append(after)   # one byte behind the message
            mlens.append(ln)
            pks.append(np.frombuffer(bytes(pk), np.uint8))
            sigs.append(np.frombuffer(bytes(s), np.uint8))
            aligns.append(align)
        off.append(off[-1] + size)
        names.append(name)
    data.extend(b"\xA5" * 8)
    n = off[-1]
    c = Call(np.frombuffer(bytes(data), np.uint8).copy(), np.array(moffs, np.uint64),
             np.array(mlens, np.uint64), np.array(pks, np.uint8).reshape(n, 32),
             np.array(sigs, np.uint8).reshape(n, 64),
             rng.integers(0, 256, size=(n, 16), dtype=np.uint8), np.array(off, np.uint64), names,
             None, None)
    assert all(int(o) % 4 == a for o, a in zip(c.moffs, aligns))
    c.judge()
    return c


def _targets(size):
    return sorted({0, size // 2, size - 1})


@functools.lru_cache(maxsize=None)
def corpus() -> Call:
    specs, expect = [], {}
    for size in SIZES:
        specs.append((f"valid_{size}", size, []))
        expect[specs[-1][0]] = (0, size)
        if size == 0:
            continue
        for kind, st in KINDS.items():
            for v in _targets(size):
                name = f"{kind}_{size}_at_{v}"
                specs.append((name, size, [(v, kind)]))
                if st is not None:
                    expect[name] = (st, v if st not in (0, 7) else size)
    # which failure wins
    order = [
        # parse / A decode share a class: the first failing vote of either names the batch
        ("s_high_1_before_a_decode_3", 5, [(1, "s_high_bit"), (3, "a_off_curve")], (1, 1)),
        ("a_decode_1_before_s_high_3", 5, [(1, "a_off_curve"), (3, "s_high_bit")], (3, 1)),
        # s < l is checked over all votes before any R is decoded
        ("s_noncanonical_3_after_r_decode_1", 5, [(1, "r_off_curve"), (3, "s_plus_l")], (2, 3)),
        ("two_s_noncanonical", 5, [(1, "s_plus_l"), (3, "s_plus_l")], (2, 1)),
        ("two_flipped_messages", 12, [(2, "msg_last_flipped"), (9, "msg_last_flipped")], (7, 12)),
        ("a_decode_4_and_flipped_0", 5, [(0, "msg_last_flipped"), (4, "a_off_curve")], (3, 4)),
    ]
    for name, size, dmg, exp in order:
        specs.append((name, size, dmg))
        expect[name] = exp
    c = build(specs, 20271)
    for b, name in enumerate(c.names):
        if name in expect:
            assert (int(c.ref_st[b]), int(c.ref_ix[b])) == expect[name], \
                (name, int(c.ref_st[b]), int(c.ref_ix[b]), expect[name])
    assert set(c.ref_st.tolist()) == {0, 1, 2, 3, 4, 7}
    # every vote of a batch has a different message, and empty ones occur
    for b in range(c.nb):
        m = c.messages(b)
        assert len(set(m)) == len(m), c.names[b]
    assert (c.mlens == 0).any() and int(c.mlens.max()) == 1023
    return c


@functools.lru_cache(maxsize=None)
def all_empty() -> Call:
    """Batches whose votes all sign the empty message (nothing is read for them)."""
    rng = np.random.Generator(np.random.PCG64(20272))
    kps = O.keys(8)
    pks, sigs = [], []
    for i in range(9):
        pk, sk = kps[i % 8]
        s = bytearray(O.sign(sk, b""))
        if i == 7:
            s[40] ^= 1   # batch 2 fails its equation
        pks.append(np.frombuffer(pk, np.uint8))
        sigs.append(np.frombuffer(bytes(s), np.uint8))
    c = Call(np.zeros(0, np.uint8), np.zeros(9, np.uint64), np.zeros(9, np.uint64),
             np.array(pks), np.array(sigs), rng.integers(0, 256, size=(9, 16), dtype=np.uint8),
             np.array([0, 1, 4, 9], np.uint64), ["e1", "e3", "e5_bad"], None, None)
    c.judge()
    assert c.ref_st.tolist() == [0, 0, 7]
    return c


@functools.lru_cache(maxsize=None)
def sized(sizes, seed, broken=()) -> Call:
    """Valid batches of the given sizes with distinct messages; broken: (batch, vote, kind)."""
    specs = []
    for b, size in enumerate(sizes):
        specs.append((f"b{b}_{size}", size, [(v, k) for bb, v, k in broken if bb == b]))
    return build(specs, seed)


def digest_call(dig, pks, sigs, off, z) -> Call:
    """Batches of the digest entries as a call of these: every vote's message is its batch's
    32-byte digest (dig: nb x 32)."""
    dig = np.ascontiguousarray(dig, np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(off, np.uint64)
    sizes = np.diff(off.astype(np.int64))
    n = int(off[-1])
    moffs = (32 * np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint64)
    c = Call(dig.reshape(-1).copy(), moffs, np.full(n, 32, np.uint64),
             np.ascontiguousarray(pks, np.uint8).reshape(n, 32),
             np.ascontiguousarray(sigs, np.uint8).reshape(n, 64),
             np.ascontiguousarray(z, np.uint8).reshape(n, 16), off,
             [f"d{b}" for b in range(len(sizes))], None, None)
    c.judge()
    return c


def golden_call(golden):
    """The golden batches as one call (messages = the batch digest, the fixture's z), with the
    fixture's names, statuses and indices."""
    bs = golden["batches"]["batches"]
    hexs = lambda xs, w: np.array([np.frombuffer(bytes.fromhex(x), np.uint8) for x in xs],
                                  np.uint8).reshape(-1, w)
    dig = hexs([b["digest"] for b in bs], 32)
    pks = np.concatenate([hexs(b["pks"], 32) for b in bs])
    sigs = np.concatenate([hexs(b["sigs"], 64) for b in bs])
    z = np.concatenate([np.frombuffer(bytes.fromhex(b["z"]), np.uint8).reshape(-1, 16)
                        for b in bs])
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b["pks"]) for b in bs])
    c = digest_call(dig, pks, sigs, off, z)
    c.names = [b["name"] for b in bs]
    return c, dig, np.array([b["status"] for b in bs], np.int32), \
        np.array([b["index"] for b in bs], np.uint64)
