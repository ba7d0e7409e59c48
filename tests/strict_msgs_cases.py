"""The corpus of the strict verification over messages of any length (nw_verify_strict_msgs_many
and its submit, device and host forms): every length at which the hash of R || A || M changes
its path, at every start alignment, with the tampered variants that a wrong length, a wrong
padding or an over-wide byte mask would turn into a wrong verdict. Signed and judged by the
oracle (oracle.sign / oracle.verify_strict over the message's own bytes)."""
import functools

import numpy as np

from oracle import oracle as O

# len mod 128 = 47 / 48: the padding stops fitting the block of R || A || M; 64, 192: 64 + len
# is a whole number of blocks; 63 / 65, 127 / 129 either side; 110..113 and 175..177 the same
# places for a plain SHA-512 of len bytes; 255..257, 1023: several full blocks (double buffering)
LENGTHS = [0, 1, 2, 31, 32, 33, 46, 47, 48, 49, 63, 64, 65, 110, 111, 112, 113, 127, 128, 129,
           175, 176, 177, 191, 192, 193, 255, 256, 257, 1023]
L_ORDER = 2**252 + 27742317777372353535851937790883648493
SMALL_R = bytes([1] + [0] * 31)   # the identity's encoding: small order
VARIANTS = ("valid", "last_flipped", "first_flipped", "short_length", "byte_after", "s_plus_l",
            "s_high_bit", "small_r", "a_off_curve")


def _off_curve_key() -> bytes:
    for y in range(2, 64):
        enc = y.to_bytes(32, "little")
        if O.decompress(enc) is None:
            return enc
    raise AssertionError("no small y off the curve")


class Corpus:
    """data / offsets / lengths as the entries take them, pks (n x 32), sigs (n x 64), the
    oracle's statuses (ref, int32) and each item's variant name."""

    def __init__(self, data, offsets, lengths, pks, sigs, ref, variant):
        self.data, self.offsets, self.lengths = data, offsets, lengths
        self.pks, self.sigs, self.ref, self.variant = pks, sigs, ref, variant
        self.n = len(offsets)

    def take(self, idx) -> "Corpus":
        """The items idx (any order, repeats allowed) over the same data."""
        idx = np.asarray(idx, dtype=np.int64)
        return Corpus(self.data, self.offsets[idx].copy(), self.lengths[idx].copy(),
                      self.pks[idx].copy(), self.sigs[idx].copy(), self.ref[idx].copy(),
                      [self.variant[i] for i in idx])

    def messages(self) -> list:
        return [self.data[int(o):int(o) + int(l)].tobytes()
                for o, l in zip(self.offsets, self.lengths)]


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    rng = np.random.Generator(np.random.PCG64(20261))
    kps = O.keys(8)
    bad_key = _off_curve_key()
    data = bytearray()
    offsets, lengths, pks, sigs, variant, aligns = [], [], [], [], [], []

    def place(msg: bytes, align: int, after: int) -> int:
        # at least one filler byte, then up to the wanted alignment; one byte behind the message
        data.append(0xA5)
        while len(data) % 4 != align:
            data.append(0x5A)
        off = len(data)
        data.extend(msg)
        data.append(after)
        return off

    for li, ln in enumerate(LENGTHS):
        for align in range(4):
            pk, sk = kps[(li + align) % 8]
            msg = rng.bytes(ln)
            sig = O.sign(sk, msg)
            for v in VARIANTS:
                if ln == 0 and v in ("last_flipped", "first_flipped", "short_length"):
                    continue
                m, length, key, s = bytearray(msg), ln, pk, bytearray(sig)
                after = 0x00
                if v == "last_flipped":
                    m[-1] ^= 0x01
                elif v == "first_flipped":
                    m[0] ^= 0x80
                elif v == "short_length":
                    length = ln - 1
                elif v == "byte_after":
                    after = 0xFF
                elif v == "s_plus_l":
                    s[32:] = (int.from_bytes(sig[32:], "little") + L_ORDER).to_bytes(32, "little")
                elif v == "s_high_bit":
                    s[63] |= 0x80
                elif v == "small_r":
                    s[:32] = SMALL_R
                elif v == "a_off_curve":
                    key = bad_key
                offsets.append(place(bytes(m), align, after))
                lengths.append(length)
                pks.append(np.frombuffer(key, np.uint8))
                sigs.append(np.frombuffer(bytes(s), np.uint8))
                variant.append(v)
                aligns.append(align)
    data.extend(b"\xA5" * 8)
    c = Corpus(np.frombuffer(bytes(data), np.uint8).copy(), np.array(offsets, np.uint64),
               np.array(lengths, np.uint64), np.array(pks), np.array(sigs), None, variant)
    c.ref = np.array([O.verify_strict(m, p.tobytes(), s.tobytes())
                      for m, p, s in zip(c.messages(), c.pks, c.sigs)], np.int32)
    assert all(int(o) % 4 == a for o, a in zip(c.offsets, aligns))
    expect = {"valid": 0, "last_flipped": 7, "first_flipped": 7, "short_length": 7,
              "byte_after": 0, "s_plus_l": 2, "s_high_bit": 1, "small_r": 6, "a_off_curve": 3}
    for st, v in zip(c.ref, c.variant):
        assert st == expect[v], (v, st)
    assert set(c.ref.tolist()) >= {0, 1, 2, 3, 6, 7}
    return c


@functools.lru_cache(maxsize=None)
def tiled(n: int = 4096) -> Corpus:
    """n items: the corpus over and over, under its 8 keys (the slice and comb tests)."""
    c = corpus()
    return c.take(np.arange(n) % c.n)


def golden_edge(golden):
    """The golden edge corpus (32-byte messages) as (msgs n x 32, pks, sigs, statuses)."""
    items = golden["edge_corpus"]["items"]
    hexs = lambda k, w: np.array([np.frombuffer(bytes.fromhex(i[k]), np.uint8)
                                  for i in items]).reshape(-1, w)
    return (hexs("msg", 32), hexs("pk", 32), hexs("sig", 64),
            np.array([i["status"] for i in items], np.int32))
