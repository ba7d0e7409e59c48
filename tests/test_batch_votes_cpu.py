"""A vote the comb check passes may be left out of its batch's verify_batch, tied
to the device code's own pass criterion: the states come from tools/hostcheck.hip
hc_batch_signers_many, the CPU build of nw_strict.hpp batch_signers_vote, never from the oracle's
strict status. For every batch the check sends on, the oracle's verify_batch over the votes
whose state is not kVotePass, with their own coefficient rows and the failing index mapped back,
equals the oracle's verify_batch over the whole batch: status and index, for every coefficient
set, the sets included under which a mixed-order key's batch fails."""
import numpy as np
import pytest

from oracle import oracle as O

import batch_signers_cases as BS
import batch_votes_cases as BV
from test_hostcheck_batch_signers import PASS, _run, hc  # noqa: F401 (hc: fixture)


def _compare(hc, dig, pk, sigs, off, reg, zs):
    """Per coefficient set: (batches compared, of them with votes left out, statuses seen)."""
    settled, _, state, _ = _run(hc, dig, pk, sigs, off, reg)
    o = off.astype(np.int64)
    compared = holding = 0
    seen = set()
    for b in np.nonzero(settled == 0)[0]:
        a, e = o[b], o[b + 1]
        keep = state[a:e] != PASS
        assert keep.any(), b          # a batch wholly passed is settled
        for z in zs:
            whole = O.verify_batch(dig[b].tobytes(), pk[a:e], sigs[a:e], z[a:e])
            part = BV.reduced(dig[b].tobytes(), pk[a:e], sigs[a:e], z[a:e], keep)
            assert (int(whole[0]), int(whole[1])) == part, (b, whole, part)
            seen.add(int(whole[0]))
            compared += 1
            holding += int(not keep.all())
    return compared, holding, seen


@pytest.fixture(scope="module")
def corpus():
    dig, pk, sigs, off, keys = BS.corpus(120, 11, every=2)
    rng = np.random.Generator(np.random.PCG64(1401))
    zs = [rng.integers(0, 256, size=(len(pk), 16), dtype=np.uint8) for _ in range(3)]
    return dig, pk, sigs, off, keys, zs


@pytest.mark.parametrize("nreg", [16, 8])
def test_corpus(hc, corpus, nreg):
    """All and half of the keys registered: every failure class among the batches sent on; with
    half, also batches that are Ok although the check sent them on."""
    dig, pk, sigs, off, keys, zs = corpus
    compared, holding, seen = _compare(hc, dig, pk, sigs, off, keys[:nreg], zs)
    assert compared >= 150 and holding >= 0.8 * compared
    assert seen >= {1, 2, 3, 4, 7} and ((0 in seen) == (nreg == 8))


@pytest.mark.parametrize("registered", [True, False])
def test_mixed_order_key(hc, registered):
    """One strict-valid vote under a mixed-order key among five honest ones: the verdict depends
    on the coefficients (the oracle says Ok under some sets and NW_ERR_EQUATION under others),
    and leaving the five passed votes out changes it under none."""
    dig, pk, sigs, off, keys, zs = BS.mixed_batches(3)
    verdicts = {int(O.verify_batch(dig[b].tobytes(), pk[6 * b:6 * b + 6], sigs[6 * b:6 * b + 6],
                                   z[6 * b:6 * b + 6])[0]) for b in range(8) for z in zs}
    assert verdicts == {0, 7}
    reg = keys if registered else keys[:-1]
    compared, holding, seen = _compare(hc, dig, pk, sigs, off, reg, zs)
    assert compared == holding == 64 and seen == {0, 7}


def test_one_unregistered_valid_vote(hc):
    """A batch whose only vote that did not pass is valid under a key nobody registered: sent on,
    and Ok over that one vote as over all of them."""
    rng = np.random.Generator(np.random.PCG64(1402))
    dig, pk, sigs, off, keys = BV.honest([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 12], 1403)
    o = off.astype(np.int64)
    for b in range(12):
        if o[b + 1] > o[b]:
            BV.resign(pk, sigs, int(o[b] + rng.integers(0, o[b + 1] - o[b])), BV.stranger(rng),
                      dig[b].tobytes())
    zs = [rng.integers(0, 256, size=(len(pk), 16), dtype=np.uint8) for _ in range(3)]
    compared, holding, seen = _compare(hc, dig, pk, sigs, off, keys, zs)
    assert compared == 33 and seen == {0}
    settled, _, state, _ = _run(hc, dig, pk, sigs, off, keys)
    assert int((state != PASS).sum()) == int((settled == 0).sum())   # one vote per batch sent on
