"""Inputs for the peer-count sweep (test_peer_witness.py, test_gpu_peer_counts.py):
buckets for which a wrong peer order, a dropped peer or a peer read twice
changes the bits of the fold, at every peer index up to K - 1.

Random buckets do not do that.  With 129 buckets of normals most exchanges of
two adjacent peers leave a given element bit-identical (the two roundings
absorb the difference), so a kernel that folds a group of 8 loads in another
order can pass a test on random values.

Witness columns.  ``make(K, n_random, rng, fmt)`` returns K rows of doubles.
Column c < K - 2 is the witness of the exchange of peers j = c + 1 and j + 1:
peer 0 holds 2^53, peer j holds 1.0, peer j + 1 holds -2^53, every other peer
+0.0.  In order the fold is (2^53 + 1) - 2^53 = 0.0, because 2^53 + 1 rounds
to 2^53; with j and j + 1 exchanged it is (2^53 - 2^53) + 1 = 1.0.  The first
k < K rows of the block are the witnesses of every exchange among k peers (the
columns past k - 3 then hold a finite sum that proves nothing), so one pool of
K rows serves every smaller peer count.  The exchange (0, 1) from a +0.0 start
is commutative and has no witness.  The n_random columns that follow are
normals scaled by 10^-3 .. 10^3 per element, rounded through the format so
that they widen exactly; they show a dropped or a duplicated peer.  2^53, 1.0
and -2^53 are exact in f64, f32 and bf16.

float16 has no witness columns: every finite f16 value is a multiple of 2^-24
below 2^16, so an f64 sum of up to 129 of them is exact and the order of the
fold cannot be observed at all.  For "half" the block is the random columns
only; they still show dropped and duplicated peers.

Count slots (``count_slots``).  Partition 0 keeps 1.0 in every bucket, so its
count is K.  Every other partition carries the witness of one exchange in its
count slot, those that end at peers 8, 64, 128 and K - 1: 2^53 in peer 0, 2.0
in peer 1, 1.0 in peer j, -2^53 in peer j + 1.  In order the count is
((2^53 + 2) + 1) - 2^53 = 4.0 (the tie rounds to even), exchanged it is 3.0:
finite and nonzero both ways, so the averages go through the division and
show the difference in every format.  The extra 2.0 needs a peer between 0
and j, so the witnessed exchanges have j >= 2.  Halves get 1.0, 2.0, 3.0
repeating instead (drops and neighbour duplicates change the count).

``mutations(K)`` lists the mistakes a fold kernel can make with its peer
indices; test_peer_witness.py shows with the oracle alone that each of them
changes the bits of every block and, where it applies, of the count.
"""
import numpy as np

import h16_ref as R

BIG = 2.0 ** 53
N_RANDOM = 17            # random columns of a block (at least 16); 129 - 2 + 17 = 144 columns at K = 129
FMTS = ("f64", "f32", "half", "bf16")
COUNT_ENDS = (8, 64, 128)   # exchanges that end here get a count-slot witness, and the one that ends at K - 1


def quantize(x, fmt):
    """Doubles rounded through the format: the values a bucket of it can hold, as doubles."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if fmt == "f64":
        return x.copy()
    f = x.astype(np.float32)
    if fmt == "f32":
        return f.astype(np.float64)
    return R.widen(R.narrow(f, fmt), fmt).reshape(x.shape)


def to_bits(x, fmt):
    """Doubles that the format holds exactly -> its bit patterns (f64: the doubles themselves)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if fmt == "f64":
        return x
    f = x.astype(np.float32)
    out = f.view(np.uint32).copy() if fmt == "f32" else R.narrow(f, fmt).reshape(x.shape).copy()
    return out


def n_witness(K, fmt="f64"):
    return 0 if fmt == "half" else max(K - 2, 0)


def block_width(K, fmt="f64", n_random=N_RANDOM):
    return n_witness(K, fmt) + n_random


def random_values(rng, shape, fmt):
    return quantize(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape), fmt)


def plant_witness(rows, at, fmt="f64"):
    """Overwrite columns at .. at + K - 3 of the K rows with the witness columns (none for halves)."""
    K = rows.shape[0]
    for c in range(n_witness(K, fmt)):
        j = c + 1
        rows[:, at + c] = 0.0
        rows[0, at + c], rows[j, at + c], rows[j + 1, at + c] = BIG, 1.0, -BIG


def make(K, n_random, rng, fmt="f64"):
    """K rows of one block: n_witness(K, fmt) witness columns, then n_random random ones."""
    assert n_random >= 16
    b = random_values(rng, (K, block_width(K, fmt, n_random)), fmt)
    plant_witness(b, 0, fmt)
    return b


def layout(K, P, L, starts, rng, fmt="f64", n_random=N_RANDOM):
    """x[q][j] = bucket j of partition q, L doubles that the format holds exactly.
    One pool of K random rows; partition q is the pool rotated by q blocks'
    worth of columns (peer 0 stays peer 0), with one block's witness columns
    planted at each of `starts`.  The count slot L - 1 is left to set_counts."""
    B = block_width(K, fmt, n_random)
    for s in starts:
        assert 0 <= s and s + B <= L - 1, (s, B, L)
    pool = random_values(rng, (K, L), fmt)
    x = np.empty((P, K, L))
    for q in range(P):
        x[q] = np.roll(pool, q * B, axis=1)
        for s in starts:
            plant_witness(x[q], s, fmt)
    x[:, :, L - 1] = 1.0
    return x


def count_swaps(K):
    """The j of the exchanges (j, j + 1) that get a count-slot witness among K peers."""
    return [e - 1 for e in sorted(set(COUNT_ENDS + (K - 1,))) if 3 <= e <= K - 1]


def count_column(K, j):
    c = np.zeros(K)
    c[0], c[1], c[j], c[j + 1] = BIG, 2.0, 1.0, -BIG
    return c


def count_slots(K, P, fmt="f64"):
    """(c, witnessed): c[q][j] = count slot of bucket j of partition q among K
    peers; witnessed = [(q, j)]: partition q's count is 4.0 in order and 3.0
    with peers j and j + 1 exchanged."""
    c = np.ones((P, K))
    witnessed = []
    if fmt == "half":
        c[1:] = np.arange(K) % 3 + 1.0
        return c, witnessed
    for q, j in zip(range(1, P), count_swaps(K)):
        c[q] = count_column(K, j)
        witnessed.append((q, j))
    return c, witnessed


def mutations(K, order=True):
    """(name, peer indices) of every mistake: each exchange (j, j + 1) with
    j >= 1, each single drop, each peer replaced by a neighbour, and the
    reversal and the rotation by one of every aligned group of 8 and of 64.
    order=False (halves): drops and duplicates only."""
    ident = list(range(K))
    seen = {tuple(ident)}
    if K >= 2:
        seen.add(tuple([1, 0] + ident[2:]))   # commutative from a +0.0 start: no witness
    for j in range(K):
        yield f"drop {j}", ident[:j] + ident[j + 1:]
        for d in (-1, 1):
            if 0 <= j + d < K:
                p = list(ident)
                p[j] = j + d
                yield f"dup {j + d} for {j}", p
    if not order:
        return
    for j in range(1, K - 1):
        p = list(ident)
        p[j], p[j + 1] = p[j + 1], p[j]
        seen.add(tuple(p))
        yield f"swap {j},{j + 1}", p
    for G in (8, 64):
        for g0 in range(0, K, G):
            g = ident[g0:g0 + G]
            for name, h in (("reverse", g[::-1]), ("rotate", g[-1:] + g[:-1])):
                p = ident[:g0] + h + ident[g0 + G:]
                if tuple(p) not in seen:
                    seen.add(tuple(p))
                    yield f"{name} {g0}..{g0 + len(g) - 1}", p
