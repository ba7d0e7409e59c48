"""The corpus of signing over messages of any length (nw_sign_msgs_many and its device form):
every length at which either hash of RFC 8032 signing, SHA-512(prefix || M) or
SHA-512(R || A || M), changes its path, at every start alignment, under 8 keys. The expected
signature is the oracle's (oracle.sign over the message's own bytes); rfc8032_sign below, a
pure-Python signer written from the RFC's text, pins the oracle where no literal vector exists."""
import functools
import hashlib

import numpy as np

from oracle import oracle as O
from strict_msgs_cases import LENGTHS as HRAM_LENGTHS

# 32 + len crosses the padding limit of a block (111 -> 112 mod 128: 79 / 80, 207 / 208), fills
# whole blocks (96, 224, 352) or, for either hash, becomes three blocks exactly (352; 320 for
# 64 + len), with the lengths either side
PREFIX_LENGTHS = [78, 79, 80, 81, 95, 96, 97, 207, 208, 209, 223, 224, 225, 320, 352]
LENGTHS = sorted(set(HRAM_LENGTHS) | set(PREFIX_LENGTHS))

# ---- RFC 8032 section 5.1 in plain integers: the affine Edwards law on -x^2 + y^2 = 1 + d x^2 y^2
P = 2**255 - 19
L_ORDER = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, -1, P) % P


def _recover_x(y: int, sign: int) -> int:
    x2 = (y * y - 1) * pow(D * y * y + 1, -1, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    assert (x * x - x2) % P == 0
    return P - x if (x & 1) != sign else x


def _add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 % P * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, -1, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, -1, P) % P)


@functools.lru_cache(maxsize=None)
def _base_doublings() -> tuple:
    by = 4 * pow(5, -1, P) % P
    out = [(_recover_x(by, 0), by)]
    for _ in range(252):
        out.append(_add(out[-1], out[-1]))
    return tuple(out)


def _mul_base(s: int):
    acc = (0, 1)
    for i, pt in enumerate(_base_doublings()):
        if (s >> i) & 1:
            acc = _add(acc, pt)
    return acc


def rfc8032_sign(sk: bytes, msg: bytes) -> bytes:
    """RFC 8032 5.1.6 with sk = seed || A: A is the second half as given, not recomputed."""
    h = hashlib.sha512(sk[:32]).digest()
    a = int.from_bytes(h[:32], "little") & ((1 << 254) - 8) | (1 << 254)
    r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L_ORDER
    x, y = _mul_base(r)
    R = (y | (x & 1) << 255).to_bytes(32, "little")
    k = int.from_bytes(hashlib.sha512(R + sk[32:] + msg).digest(), "little") % L_ORDER
    return R + ((r + k * a) % L_ORDER).to_bytes(32, "little")


class Corpus:
    """data / offsets / lengths as the entries take them, sks (n x 64), pks (n x 32: the key of
    each item's seed), sigs (n x 64: oracle.sign), each item's alignment, and `foreign`: the item
    whose secret key's second half is another key's public key."""

    def __init__(self, data, offsets, lengths, sks, pks, sigs, aligns, foreign, shared, falling):
        self.data, self.offsets, self.lengths = data, offsets, lengths
        self.sks, self.pks, self.sigs, self.aligns = sks, pks, sigs, aligns
        self.foreign, self.shared, self.falling = foreign, shared, falling
        self.n = len(offsets)

    def messages(self) -> list:
        return [self.data[int(o):int(o) + int(l)].tobytes()
                for o, l in zip(self.offsets, self.lengths)]


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    rng = np.random.Generator(np.random.PCG64(20262))
    kps = O.keys(8)
    data = bytearray()
    offsets, lengths, sks, pks, aligns = [], [], [], [], []

    def place(msg: bytes, align: int) -> int:
        # at least one filler byte, then up to the wanted alignment; 0xFF behind the message
        data.append(0xA5)
        while len(data) % 4 != align:
            data.append(0x5A)
        off = len(data)
        data.extend(msg)
        data.append(0xFF)
        return off

    def item(off: int, ln: int, sk: bytes, pk: bytes) -> int:
        offsets.append(off)
        lengths.append(ln)
        sks.append(np.frombuffer(sk, np.uint8))
        pks.append(np.frombuffer(pk, np.uint8))
        aligns.append(off % 4)
        return len(offsets) - 1

    for li, ln in enumerate(LENGTHS):
        for align in range(4):
            pk, sk = kps[(li + align) % 8]
            item(place(rng.bytes(ln), align), ln, sk, pk)
    grid = len(offsets)
    # two items over the same bytes (another key signs item 77's message)
    shared = (77, item(offsets[77], lengths[77], kps[0][1], kps[0][0]))
    assert not np.array_equal(sks[shared[0]], sks[shared[1]])
    # offsets that decrease: three earlier messages again, from the back of data to its front
    falling = [item(offsets[j], lengths[j], kps[(j + 3) % 8][1], kps[(j + 3) % 8][0])
               for j in (grid - 2, 90, 5)]
    # a secret key whose second half is another key's public key
    foreign = item(place(rng.bytes(100), 1), 100, kps[2][1][:32] + kps[5][0], kps[2][0])
    data.extend(b"\xA5" * 8)
    c = Corpus(np.frombuffer(bytes(data), np.uint8).copy(), np.array(offsets, np.uint64),
               np.array(lengths, np.uint64), np.array(sks), np.array(pks), None,
               np.array(aligns), foreign, shared, falling)
    c.sigs = np.array([np.frombuffer(O.sign(sk.tobytes(), m), np.uint8)
                       for sk, m in zip(c.sks, c.messages())])
    return c
