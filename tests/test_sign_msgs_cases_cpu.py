"""The corpus of signing over messages of any length (tests/sign_msgs_cases.py) and the oracle
that states its expected signatures, without a GPU: the corpus holds what it promises, and
oracle.sign equals a pure-Python RFC 8032 signer on every item and on the three literal RFC
vectors over their raw messages (no literal vector exists for the long ones)."""
import numpy as np

from oracle import oracle as O

import sign_msgs_cases as SG
import strict_msgs_cases as SM


def test_lengths():
    assert set(SM.LENGTHS) <= set(SG.LENGTHS)
    assert {78, 79, 80, 81, 95, 96, 97, 207, 208, 209, 223, 224, 225, 320, 352} <= set(SG.LENGTHS)
    assert len(SG.LENGTHS) == 45
    # the places the module's comment names, for the hash of 32 + len bytes
    assert all((32 + a) % 128 == 111 and (32 + a + 1) % 128 == 112 for a in (79, 207))
    assert all((32 + a) % 128 == 0 for a in (96, 224, 352))
    assert 32 + 352 == 3 * 128 and 64 + 320 == 3 * 128


def test_corpus_shape():
    c = SG.corpus()
    grid = 4 * len(SG.LENGTHS)
    assert c.n == grid + 1 + 3 + 1
    cells = {(int(l), int(a)) for l, a in zip(c.lengths[:grid], c.aligns[:grid])}
    assert cells == {(l, a) for l in SG.LENGTHS for a in range(4)}
    assert all(int(o) % 4 == a for o, a in zip(c.offsets, c.aligns))
    assert len({sk.tobytes() for sk in c.sks[:grid]}) == 8
    # a filler byte before every message and 0xFF behind it
    for o, l in zip(c.offsets, c.lengths):
        assert c.data[int(o) - 1] in (0xA5, 0x5A) and c.data[int(o) + int(l)] == 0xFF
    a, b = c.shared
    assert (c.offsets[a], c.lengths[a]) == (c.offsets[b], c.lengths[b])
    assert not np.array_equal(c.sigs[a], c.sigs[b])
    f = c.offsets[c.falling].astype(np.int64)
    assert len(f) == 3 and (np.diff(f) < 0).all()
    assert c.sigs.shape == (c.n, 64)


def test_foreign_key_half():
    c = SG.corpus()
    i = c.foreign
    sk, msg = c.sks[i].tobytes(), c.messages()[i]
    own = O.keypair_from_seed(sk[:32])[0]
    assert c.pks[i].tobytes() == own and sk[32:] != own
    assert sk[32:] in {p.tobytes() for p in c.pks}
    # signed with A as given: neither the seed's key nor the foreign one accepts it
    assert c.sigs[i].tobytes() != O.sign(sk[:32] + own, msg)
    assert O.verify_strict(msg, own, c.sigs[i].tobytes()) == 7
    assert O.verify_strict(msg, sk[32:], c.sigs[i].tobytes()) == 7


def test_valid_items_verify():
    c = SG.corpus()
    for i, (m, pk, sig) in enumerate(zip(c.messages(), c.pks, c.sigs)):
        if i != c.foreign:
            assert O.verify_strict(m, pk.tobytes(), sig.tobytes()) == 0, i


def test_python_signer_gives_the_rfc_vectors(golden):
    vec = golden["keys"]["rfc8032"]
    assert [len(bytes.fromhex(v["msg"])) for v in vec] == [0, 1, 2]
    for v in vec:
        sk = bytes.fromhex(v["seed"]) + bytes.fromhex(v["pk"])
        assert SG.rfc8032_sign(sk, bytes.fromhex(v["msg"])).hex() == v["sig"]


def test_oracle_equals_python_signer_on_every_item():
    c = SG.corpus()
    bad = [(i, int(c.lengths[i]), int(c.aligns[i]))
           for i, (sk, m, sig) in enumerate(zip(c.sks, c.messages(), c.sigs))
           if SG.rfc8032_sign(sk.tobytes(), m) != sig.tobytes()]
    assert not bad, bad[:8]
