"""Inputs and a plain numpy model of the unfused round: k_finalize, k_divide, the big-endian outputs.

Shared by tests/test_unfused_cases.py (CPU: the inputs discriminate) and
tests/test_gpu_unfused_round.py (GPU: the kernels, bit for bit against the
oracle).  numpy only: importable without a GPU, the library or the oracle.

Geometry of the kernels under test (ipls_kernels.hpp; test_unfused_cases.py
parses the header and compares):
  TILE_FIN  k_finalize's tile, kFinTile = kBlock * 2 * kFinV   (:37, :598, :599)
  TILE_DIV  k_divide's tile,   kDivTile = kBlock * 2 * kDivV   (:37, :598, :599)
  LINE      doubles per 128-B line: k_divide's `to_line` / `head` (:708-709)
  WAVE      doubles one wave stores per V step of `wave_base`, 64 lanes x 16 B (:716)

k_divide lays its tiles over the OUTPUT: block 0 writes `head` elements up to
the next 128-B line of this partition's output, tile t then covers [head + t *
TILE_DIV, + TILE_DIV), and inside a whole tile wave w owns [w * 128 * kDivV, +
128 * kDivV) in steps of 128.  The head depends on the output pointer alone,
so one W serves every output offset when it carries the seams of every head:
seam_positions(L) with head=None lists them for heads 0 .. 15 at once.  The
multiples of 128 are listed through the whole partition, not only inside the
first whole tile (a superset: the later tiles have the same wave seams).

weights() plants special_values() on those seams, rotated by partition, over a
body without two equal elements; accumulators() plants PAIRS the same way in
AGG and REP.  planted() is the plan both are built from, so a test can count
what stands where.  The model_* functions restate the operations and the wrong
variants a kernel could compute instead; they are there to show that the
inputs tell the variants apart, never to check the library (the GPU tests
compare with the oracle).
"""
import numpy as np

TILE_FIN = 4096   # kFinTile = kBlock (256, ipls_kernels.hpp:37) * 2 * kFinV (8, :598), :599
TILE_DIV = 2048   # kDivTile = kBlock (256, ipls_kernels.hpp:37) * 2 * kDivV (4, :598), :599
LINE = 16         # doubles per 128-B line, ipls_kernels.hpp:708
WAVE = 128        # doubles per wave and V step, ipls_kernels.hpp:716

GUARD = 64                       # sentinel elements on each side of a caller-owned output
SENTINEL = 0x7FF45EA1A15EF47F    # the signalling NaN of tests/test_gpu_wide_small.py: no result can take it
NAN_BITS = 0x7FF80000DEADBEEF    # the one quiet NaN of the inputs
CANON_NAN = 0x7FF8000000000000   # what writeDouble makes of every NaN

MAX_SUB = 2.225073858507201e-308   # largest subnormal
MIN_NORMAL = 2.2250738585072014e-308
MAX_F64 = 1.7976931348623157e308

# count slots (IPLS.java:1159-1174): ordinary ones, the two zeros (both pass through: Java's ==), NaN, +inf,
# a negative one, 5e-324 (quotients overflow) and 1e300 (secure: 1e12 * cnt = inf, quotients +-0.0)
COUNTS = (1.0, 3.0, 7.0, 32.0, 0.0, -0.0, float("nan"), float("inf"), -3.0, 5e-324, 1e300)


def _f(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def _b(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# --------------------------------------------------------------------------
# geometry (IPLS.java:1019-1028, restated so that this file stands alone)
# --------------------------------------------------------------------------
def lengths_of(model=None, P=0, L=0):
    """Partition lengths, count slot included: Aggregator(M, P) (`model`) or the synthetic (P, bucket_len)."""
    if model is None:
        return [L] * P
    M, P = model
    c = M // P + 1
    return [M - i * c + 1 if (i + 1) * c > M else c + 1 for i in range(P)]


def offsets_of(model=None, P=0, L=0):
    """Flat offset of every partition's averages."""
    if model is None:
        return [p * (L - 1) for p in range(P)]
    M, P = model
    return [p * (M // P + 1) for p in range(P)]


def flat_size(lengths, offsets):
    return max(o + L - 1 for o, L in zip(offsets, lengths))


# --------------------------------------------------------------------------
# seams
# --------------------------------------------------------------------------
def seam_classes(L, head=None, tile=TILE_DIV):
    """{position: class} over the body [0, L - 1) of a partition of L
    elements (the count slot L - 1 is no seam): "first", "last" (n - 1),
    "tile" (head + tile * t - 1, + 0, + 1), "head" (head - 1, head, head + 1)
    and "wave" (head + 128 * m - 1, + 0, + 1), for one head or, with
    head=None, for every head 0 .. LINE - 1."""
    n = L - 1
    heads = range(LINE) if head is None else (head,)
    cls = {}

    def add(e, name):
        if 0 <= e < n:
            cls.setdefault(e, name)

    add(0, "first")
    add(n - 1, "last")
    for name in ("tile", "head", "wave"):
        for h in heads:
            if name == "head":
                steps = (0,)
            else:
                steps = [m for m in range(WAVE, n + WAVE, WAVE) if (m % tile == 0) == (name == "tile")]
            for m in steps:
                for d in (-1, 0, 1):
                    add(h + m + d, name)
    return cls


def seam_positions(L, head=None, tile=TILE_DIV):
    return sorted(seam_classes(L, head, tile))


def special_values(cnt, secure):
    """[(name, bits)] planted in W of a partition whose count slot is `cnt`.
    The values with a subnormal quotient for an ordinary divisor stand four
    apart, so a few consecutive seams always hold one.  "x_den" is the normal
    1e-308 * |den| whose quotient by this partition's divisor is subnormal
    (1e-308 itself where no such normal exists: |den| < 2.3, or not finite)."""
    den = 1e12 * cnt if secure else cnt
    with np.errstate(all="ignore"):
        x = np.float64(1e-308) * np.abs(np.float64(den))
    x_den = float(x) if np.isfinite(x) and x >= MIN_NORMAL else 1e-308
    vals = [("x_den", _b(x_den)), ("-0", _b(-0.0)), ("+inf", _b(np.inf)), ("5e-324", _b(5e-324)),
            ("n3", _b(3e-308)),            # normal; / 3 and / 7 subnormal
            ("+max", _b(MAX_F64)), ("nan", NAN_BITS), ("-5e-324", _b(-5e-324)),
            ("maxsub", _b(MAX_SUB)), ("-inf", _b(-np.inf)), ("+0", _b(0.0)), ("-max", _b(-MAX_F64)),
            ("minnormal", _b(MIN_NORMAL)),
            ("n7", _b(1.4e-307)),          # normal; / 7 subnormal, / 3 normal
            ("-n3", _b(-3e-308))]
    if secure:
        vals += [("1e13", _b(1e13)), ("1e-300", _b(1e-300)), ("3e12", _b(3e12)), ("-1e-300", _b(-1e-300)),
                 ("-1e13", _b(-1e13))]
    return vals


def planted(L, cnt, secure, rot=0, head=None, tile=TILE_DIV):
    """[(position, class, name, bits)]: seam j of the partition, at element e,
    holds special (j + rot + e // tile) mod their number -- consecutive seams
    hold consecutive specials, and the tile index keeps the elements one tile
    apart different whatever the number of seams in a tile."""
    cls = seam_classes(L, head, tile)
    S = special_values(cnt, secure)
    return [(e, cls[e]) + S[(j + rot + e // tile) % len(S)] for j, e in enumerate(sorted(cls))]


# every special of PAIRS as (name, AGG value, REP value); never two different NaNs in one element
PAIRS = (("-0,-0", -0.0, -0.0), ("-0,+0", -0.0, 0.0), ("cancel", 1e16, -1e16 + 1), ("inf,-inf", np.inf, -np.inf),
         ("nan,1", _f(NAN_BITS), 1.0), ("1,nan", 1.0, _f(NAN_BITS)), ("big", 1e308, 1e308),
         ("sub", 5e-324, 1e-310))


def planted_pairs(L, rot=0):
    """[(position, class, name, AGG bits, REP bits)] on seam_positions(L, 0, TILE_FIN), indexed as in planted()."""
    cls = seam_classes(L, 0, TILE_FIN)
    out = []
    for j, e in enumerate(sorted(cls)):
        name, a, r = PAIRS[(j + rot + e // TILE_FIN) % len(PAIRS)]
        out.append((e, cls[e], name, _b(a), _b(r)))
    return out


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def _body(total, seed):
    """`total` doubles, no two equal, magnitudes over [1e-3, 1e3), random mantissas and signs."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 10.0, total) * 10.0 ** (np.arange(total) % 6 - 3.0)
    x = np.where(rng.integers(0, 2, total) == 1, -x, x)
    assert np.unique(bits(x)).size == total
    return x


def weights(lengths, counts, seed, secure=False, rot=0):
    """One W array per partition: a position-distinct body (over the whole
    handle), planted() on every seam of every head with the specials rotated
    by partition, the count in the last element."""
    body = _body(sum(lengths), seed)
    out, o = [], 0
    for p, (L, c) in enumerate(zip(lengths, counts)):
        w = body[o:o + L].copy()
        o += L
        for e, _, _, b in planted(L, c, secure, rot + p):
            w.view(np.uint64)[e] = b
        w[L - 1] = c
        out.append(w)
    return out


def accumulators(lengths, seed, counts=None):
    """(AGG, REP) contents per partition: position-distinct bodies with PAIRS
    on seam_positions(L, 0, TILE_FIN), rotated by twice the partition; `counts` are the
    (AGG, REP) count slots, default (2.0, 1.0)."""
    total = sum(lengths)
    body = _body(2 * total, seed)
    aggs, reps, o = [], [], 0
    for p, L in enumerate(lengths):
        a, r = body[o:o + L].copy(), body[total + o:total + o + L].copy()
        o += L
        for e, _, _, ab, rb in planted_pairs(L, 2 * p):
            a.view(np.uint64)[e], r.view(np.uint64)[e] = ab, rb
        a[L - 1], r[L - 1] = (2.0, 1.0) if counts is None else counts[p]
        aggs.append(a)
        reps.append(r)
    return aggs, reps


# --------------------------------------------------------------------------
# the case lists of tests/test_gpu_unfused_round.py
# --------------------------------------------------------------------------
def _counts(P, first=0):
    return [COUNTS[(first + p) % len(COUNTS)] for p in range(P)]


def divide_cases():
    """name -> dict(model | (P, L), counts): the handles of sections a to c,
    each opened with secure False and True.
      p17-*   P = 17, L - 1 = 1 mod 16: the flat offsets p * (L - 1) take every residue mod 16
      p3-*    P = 3 at the lengths around a line and a tile
      model   Aggregator(30011, 3): a short last partition
      count   Aggregator(7, 8): the last partition holds the count slot only (n = 0)"""
    cases = {}
    for n in (17, 2049, 2 * TILE_DIV + 17):
        cases[f"p17-{n}"] = dict(P=17, L=n + 1, counts=_counts(17))
    nan, inf = float("nan"), float("inf")
    for n, counts in ((1, [3.0, 0.0, nan]), (2, [7.0, -0.0, inf]), (15, [32.0, -3.0, 5e-324]),
                      (16, [1e300, 1.0, 3.0]), (2047, [7.0, -0.0, -3.0]), (2048, [3.0, 0.0, 1e300])):
        cases[f"p3-{n}"] = dict(P=3, L=n + 1, counts=counts)
    cases["model"] = dict(model=(30011, 3), counts=[3.0, -0.0, 7.0])
    cases["count"] = dict(model=(7, 8), counts=_counts(8, 1))
    return cases


def case_geometry(case):
    """(lengths, offsets, flat size) of a case."""
    kw = {k: case[k] for k in ("model", "P", "L") if k in case}
    lens, offs = lengths_of(**kw), offsets_of(**kw)
    return lens, offs, flat_size(lens, offs)


def case_weights(name, case, secure):
    seed = sum(ord(ch) for ch in name) * 2 + int(secure)
    return weights(case_geometry(case)[0], case["counts"], seed, secure)


# k_finalize: the chunk rule shortens only the last partition, and by at most
# P elements, so 4095, 4096, 4097, 2 * 4096 + 1 and 1 cannot stand in one
# handle.  Four model handles of P = 5 hold them: every other partition is
# one element longer than a tile (or two tiles), the last one is the short one.
FINALIZE_MODELS = {
    "last4095": (20478, 5),   # 4097 x 4 (one whole tile + 1), 4095 (no whole tile)
    "last4096": (20479, 5),   # 4097 x 4, 4096 (exactly one tile: its second block leaves at base >= len)
    "two-tiles": (40959, 5),  # 8193 x 4 (two whole tiles + 1), 8192 (the third block leaves early)
    "count-only": (4, 5),     # 2 x 4, 1 (the count slot alone)
}
FINALIZE_LENGTHS = {"last4095": [4097] * 4 + [4095], "last4096": [4097] * 4 + [4096],
                    "two-tiles": [8193] * 4 + [8192], "count-only": [2] * 4 + [1]}
# (AGG, REP) count slots: W's count is 3, -0.0 (pass-through), 7, 1, 32 with REP and 2, +0.0, 6, 1, 31 without
FINALIZE_COUNTS = [(2.0, 1.0), (-0.0, -0.0), (6.0, 1.0), (1.0, 0.0), (31.0, 1.0)]
REP_MODES = {"none": (), "one": (1,), "all": (0, 1, 2, 3, 4)}   # partitions whose REP holds values


def finalize_inputs(name):
    lens = lengths_of(FINALIZE_MODELS[name])
    return accumulators(lens, 1000 + sum(ord(ch) for ch in name), FINALIZE_COUNTS)


# the unfused fallback of aggregate_round: P = 5, two divide tiles + a head + a tail, more than one finalize tile
FALLBACK = dict(P=5, L=2 * TILE_DIV + 18, K=3, p_first=1, n_parts=3, agg_in=2, rep_in=3)


def fallback_inputs():
    """(buckets[q][k], AGG prefill, REP prefill) of the sub-range: K buckets
    per partition built like W (count slot 1.0, specials on the divide's
    seams, rotated so that one element never meets two NaNs), and PAIRS-free
    position-distinct accumulators with count slots 2.0 and 1.0."""
    F = FALLBACK
    L, K, n = F["L"], F["K"], F["n_parts"]
    rows = []
    for q in range(n):
        bk = weights([L] * K, [1.0] * K, 77 + q, rot=4 * q)
        rows.append(bk)
    pre = weights([L, L], [2.0, 1.0], 99, rot=7)
    return rows, pre[0], pre[1]


# --------------------------------------------------------------------------
# the model and its wrong variants
# --------------------------------------------------------------------------
DIVIDE_VARIANTS = ("recip", "no-passthrough", "negzero-nonzero", "ftz")
SECURE_VARIANTS = ("two-step-1e12-first", "two-step-cnt-first", "secure-ignored")


def model_divide(w, secure, variant=None):
    """GetPartitions of one partition (IPLS.java:1159-1174): x / cnt, secure
    x / (1e12 * cnt), the values themselves when cnt == 0.0 -- or what a wrong
    kernel would give (DIVIDE_VARIANTS, SECURE_VARIANTS)."""
    w = np.asarray(w, dtype=np.float64)
    x, cnt = w[:-1], w[-1]
    with np.errstate(all="ignore"):
        if variant == "negzero-nonzero":
            passes = _b(cnt) == 0
        elif variant == "no-passthrough":
            passes = False
        else:
            passes = cnt == 0.0
        if passes:
            return x.copy()
        den = cnt if (not secure or variant == "secure-ignored") else np.float64(1e12) * cnt
        if variant == "recip":
            return x * (np.float64(1.0) / den)
        if variant == "two-step-1e12-first" and secure:
            return (x / 1e12) / cnt
        if variant == "two-step-cnt-first" and secure:
            return (x / cnt) / 1e12
        q = x / den
        if variant == "ftz":
            sub = (q != 0.0) & (np.abs(q) < MIN_NORMAL)
            q = np.where(sub, np.copysign(0.0, q), q)
        return q


def model_wire(q, canonical=True):
    """DataOutputStream.writeDouble of the averages (Middleware.java:164-170):
    big-endian, every NaN 0x7ff8000000000000 -- or, wrongly, its raw bits."""
    b = bits(q).copy()
    if canonical:
        b[np.isnan(np.asarray(q, dtype=np.float64))] = CANON_NAN
    return b.byteswap().tobytes()


def model_finalize(agg, rep, rep_present, variant=None):
    """AggregatePartition (IPLS.java:1255-1270): W = AGG + REP, where a
    logically zero REP is +0.0 -- or "rep-ignored" (AGG + 0.0 whatever REP
    holds) and "negzero-kept" (W = AGG where REP is logically zero, so that
    -0.0 survives; -0.0 + 0.0 is +0.0)."""
    agg = np.asarray(agg, dtype=np.float64)
    with np.errstate(all="ignore"):
        if variant == "rep-ignored" or (not rep_present and variant is None):
            return agg + 0.0
        if not rep_present:            # negzero-kept
            return agg + (-0.0)
        return agg + np.asarray(rep, dtype=np.float64)


SHIFTS = (1, -1, WAVE, -WAVE)


def model_shift(out, i, d):
    """`out` with the element at seam i taken from index i + d."""
    o = np.array(out, dtype=np.float64, copy=True)
    o.view(np.uint64)[i] = bits(out)[i + d]
    return o


def same(got, want, raw=True):
    """Bitwise equality element by element.  A NaN that the inputs do not hold
    (inf - inf, 0 / 0, inf / inf: any bits but NAN_BITS in `want`) is
    generated, and neither Java nor IEEE 754 fixes its sign or payload: there
    NaN must meet NaN.  raw=False is assert_bits_equal's rule for quotients:
    NaN / cnt may carry any payload."""
    g, w = bits(got), bits(want)
    wn = np.isnan(np.asarray(want, dtype=np.float64))
    loose = wn & ((w != NAN_BITS) | (not raw))
    return np.where(loose, np.isnan(np.asarray(got, dtype=np.float64)), g == w)


def ordinary(cnt, secure):
    """A count whose quotients can be subnormal: finite, |den| >= 1 and den
    finite.  (cnt == 0 passes values through, NaN gives NaN, inf and an
    overflowing 1e12 * cnt give +-0.0, and |den| < 1 only enlarges.)"""
    with np.errstate(all="ignore"):
        den = np.float64(1e12) * cnt if secure else np.float64(cnt)
    return bool(np.isfinite(den) and abs(den) >= 1.0)
