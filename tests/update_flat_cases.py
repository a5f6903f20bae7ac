"""Inputs and oracle-side expectations shared by the whole-gradient streamed
update tests (test_gpu_update_flat.py on the GPU, test_update_flat_boundary.py
on the oracle alone): the five source kinds as raw bytes plus their exact
widening, the residue sweep's geometry and planted vectors, the expected state
(oracle.organize_gradients on the widened vector, then oracle.fold), and the
concurrency witnesses.
"""
import itertools

import numpy as np

import narrow_fmt as F

KINDS = ("f64", "be", "f32", "half", "bf16")
P_SWEEP = 9

# doubles: -0.0, +-inf, NaN, smallest / largest (negative) subnormal, +- largest finite
EDGE_F64 = np.array([0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000,
                     0x0000000000000001, 0x800fffffffffffff, 0x7fefffffffffffff, 0xffefffffffffffff],
                    dtype=np.uint64)


def esize(kind):
    return 8 if kind in ("f64", "be") else F.esize(kind)


def call_args(kind):
    """The big_endian= / dtype= of UpdateGradientChunked for the kind."""
    if kind in ("f64", "be"):
        return dict(big_endian=kind == "be")
    return dict(dtype=F.np_dtype(kind))


def edge_bits(kind):
    return EDGE_F64 if kind in ("f64", "be") else F.EDGE_BITS[kind]


def vector(rng, n, kind, plant=()):
    """A flat gradient of n values of the kind: (raw bytes as the source hands
    them out, the exact doubles they widen to).  The format's edge values sit at
    the positions `plant`."""
    if kind in ("f64", "be"):
        bits = rng.standard_normal(n).view(np.uint64).copy()
        e = EDGE_F64
    else:
        bits = F.from_f32(rng.standard_normal(n).astype(np.float32), kind)
        e = F.EDGE_BITS[kind]
    for i, pos in enumerate(sorted({p for p in plant if 0 <= p < n})):
        bits[pos] = e[i % e.size]
    return raw_of(bits, kind), widen(bits, kind)


def raw_of(bits, kind):
    bits = np.ascontiguousarray(bits)
    if kind == "be":
        return bits.astype(">u8").view(np.uint8).copy()
    return bits.view(np.uint8).copy()


def widen(bits, kind):
    if kind in ("f64", "be"):
        return np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64).copy()
    return F.widen(bits, kind)


def from_doubles(x, kind):
    """Raw bytes of doubles that the kind holds exactly."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if kind in ("f64", "be"):
        return raw_of(x.view(np.uint64), kind)
    bits = F.from_f32(x.astype(np.float32), kind)
    assert np.array_equal(F.widen(bits, kind), x), "not exact in the format"
    return raw_of(bits, kind)


def sweep_model_size(chunk):
    """M for P_SWEEP partitions of stride `chunk` (== 1 mod 8: partitions 0..8
    start at residues 0..8 mod 8); the last partition copies chunk - 9 values."""
    assert chunk % 8 == 1
    M = P_SWEEP * (chunk - 1)
    assert M // P_SWEEP + 1 == chunk
    return M


def sweep_chunks(T):
    """No vector step; one full tile; full tiles, a vector step and a remainder."""
    return (9, T + 9, 2 * T + 8 * 3 + 1)


def sweep_plant(M, P, T):
    """Each partition's first and last value and both sides of every tile seam."""
    c = M // P + 1
    pos = set()
    for p in range(P):
        lo, hi = p * c, min((p + 1) * c, M)
        if hi <= lo:
            continue
        pos.update((lo, lo + 1, hi - 1, hi - 2))
        for seam in range(lo + T, hi, T):
            pos.update((seam - 1, seam, seam + 1))
    return sorted(x for x in pos if 0 <= x < M)


def expected(O, acc, wide, n, M, P, owned):
    """The accumulators after UpdateGradient of wide[:n] over `owned` (in list
    order, repeats fold again): organize_gradients, then fold -- the oracle alone."""
    parts = O.organize_gradients(wide[:n], M, P)
    out = [np.array(a, dtype=np.float64, copy=True) for a in acc]
    for p in owned:
        O.fold(out[p], parts[p])
    return out


def zeros(O, M, P):
    return [np.zeros(O.partition_len(M, P, p)) for p in range(P)]


# ---- concurrency witnesses ----
def order_witness():
    """(base, A, B): per element (base + B) + A and (base + A) + B differ in bits."""
    base, a, b = 1.0, 2.0 ** 53, 1.0
    assert (base + b) + a != (base + a) + b
    return base, a, b


def serial_witness(O, M, P, n_threads=4):
    """A base and n_threads whole gradients (doubles) whose n_threads! serial
    orders give pairwise distinct bit patterns in EVERY partition."""
    for seed in range(64):
        rng = np.random.default_rng(1000 + seed)
        base = rng.standard_normal(M) * 10.0 ** rng.integers(-3, 4, M)
        grads = [rng.standard_normal(M) * 10.0 ** rng.integers(-3, 4, M) for _ in range(n_threads)]
        table = serial_orders(O, base, grads, M, P)
        if all(len({table[o][p].tobytes() for o in table}) == len(table) for p in range(P)):
            return base, grads, table
    raise AssertionError("no seed separates the serial orders")


def serial_orders(O, base, grads, M, P):
    start = expected(O, zeros(O, M, P), base, M, M, P, range(P))
    return {o: expected_seq(O, start, [grads[i] for i in o], M, P) for o in itertools.permutations(range(len(grads)))}


def expected_seq(O, acc, grads, M, P):
    for g in grads:
        acc = expected(O, acc, g, M, M, P, range(P))
    return acc
