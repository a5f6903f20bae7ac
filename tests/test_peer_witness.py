"""The inputs of tests/peer_witness.py discriminate: for every peer count of the
GPU sweep (tests/test_gpu_peer_counts.py) and every mistake of
``mutations(K)``, the oracle's fold of the mutated bucket list differs in
bits from the fold in order -- in the block of every region of every
partition, and in the count where the mistake touches a count slot.  Checked
against the oracle alone, never against the library: this is what keeps the
GPU comparisons from passing vacuously.
"""
import numpy as np
import pytest

import peer_witness as PW
from oracle import oracle as O

KS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # KFOLD and KROUND (K = 0 folds nothing)
P = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fold(rows, idx, prefix):
    """O.reduce of rows[idx]; the peers before the first changed index are
    taken from the in-order fold's own partial sums (prefix[j] = fold of peers
    0 .. j - 1), from which the oracle goes on."""
    j = 0
    while j < len(idx) and idx[j] == j:
        j += 1
    return O.reduce([rows[i] for i in idx[j:]], rows.shape[1], O.START_ACCUM, acc=prefix[j])


def _prefixes(rows):
    acc = np.zeros(rows.shape[1])
    out = [acc.copy()]
    for r in rows:
        acc = O.reduce([r], rows.shape[1], O.START_ACCUM, acc=acc)
        out.append(acc)
    return out


@pytest.mark.parametrize("fmt", PW.FMTS)
def test_every_mutation_changes_every_block(fmt):
    Kmax = max(KS)
    B = PW.block_width(Kmax, fmt)
    starts = (0, B + 5, 2 * B + 9)                 # three regions, the blocks at odd distances
    L = 3 * B + 20
    x = PW.layout(Kmax, P, L, starts, np.random.default_rng(1), fmt)
    assert np.array_equal(PW.quantize(x, fmt).view(np.uint64), x.view(np.uint64))   # exact in the format
    assert np.isfinite(x).all()
    blocks = [(q, s) for q in range(P) for s in starts]
    for K in KS:
        # the P partitions side by side: one fold covers them all
        rows = np.concatenate([x[q, :K] for q in range(P)], axis=1)
        prefix = _prefixes(rows)
        ref = prefix[K]
        assert np.array_equal(_bits(ref), _bits(O.reduce(list(rows), rows.shape[1], O.START_ZERO)))
        W = PW.n_witness(K, fmt)
        for q, s in blocks:
            assert not ref[q * L + s:q * L + s + W].any()        # every complete witness folds to 0.0 in order
        n = 0
        for name, idx in PW.mutations(K, order=fmt != "half"):
            got = _fold(rows, idx, prefix)
            for q, s in blocks:
                lo = q * L + s
                assert not np.array_equal(_bits(got[lo:lo + B]), _bits(ref[lo:lo + B])), \
                    f"{fmt} K={K}: '{name}' leaves the block at {s} of partition {q} unchanged"
            n += 1
        assert n >= (3 * K - 2 if K > 1 else 1)
        if fmt != "half" and K >= 3:
            # an exchange shows in its own witness column as 1.0 for 0.0
            for j in range(1, K - 1):
                idx = list(range(K))
                idx[j], idx[j + 1] = idx[j + 1], idx[j]
                got = _fold(rows, idx, prefix)
                assert all(got[q * L + s + j - 1] == 1.0 for q, s in blocks)


@pytest.mark.parametrize("fmt", PW.FMTS)
def test_count_slots(fmt):
    for K in KS:
        c, witnessed = PW.count_slots(K, P, fmt)
        assert np.array_equal(PW.quantize(c, fmt), c)
        ref = O.reduce(list(c.T), P, O.START_ZERO)
        assert ref[0] == K and np.isfinite(ref).all() and (ref != 0.0).all()
        if fmt == "half":
            assert not witnessed
        else:
            ends = sorted({j + 1 for _, j in witnessed})
            assert ends == [e for e in sorted({8, 64, 128, K - 1}) if 3 <= e <= K - 1]
        for q, j in witnessed:
            idx = list(range(K))
            idx[j], idx[j + 1] = idx[j + 1], idx[j]
            assert ref[q] == 4.0 and O.reduce(list(c.T[idx]), P, O.START_ZERO)[q] == 3.0
        for name, idx in PW.mutations(K, order=False):
            got = O.reduce(list(c.T[idx]), P, O.START_ZERO)
            if name.startswith("drop"):
                assert got[0] == K - 1                            # partition 0 counts the peers
            if fmt == "half" and K > 1:
                assert (got[1:] != ref[1:]).all(), f"half K={K}: '{name}' leaves a count unchanged"


def test_random_buckets_do_not_discriminate():
    """Why the witness columns exist: in a column of 129 random values most
    exchanges of adjacent peers change nothing."""
    rng = np.random.default_rng(5)
    K = 129
    rows = PW.random_values(rng, (K, 1), "f64")
    prefix = _prefixes(rows)
    same = 0
    for j in range(1, K - 1):
        idx = list(range(K))
        idx[j], idx[j + 1] = idx[j + 1], idx[j]
        same += np.array_equal(_bits(_fold(rows, idx, prefix)), _bits(prefix[K]))
    assert same > K // 4


def test_f16_sums_are_exact():
    """The order of a fold of halves cannot be observed: no witness columns for them."""
    rng = np.random.default_rng(2)
    rows = PW.random_values(rng, (129, 512), "half")
    ref = O.reduce(list(rows), 512, O.START_ZERO)
    for _ in range(5):
        assert np.array_equal(_bits(O.reduce(list(rows[rng.permutation(129)]), 512, O.START_ZERO)), _bits(ref))
