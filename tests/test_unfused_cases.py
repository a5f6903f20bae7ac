"""The inputs of tests/test_gpu_unfused_round.py discriminate (CPU, numpy only).

For every case list of the GPU file: each wrong variant of
tests/unfused_cases.py differs from the correct model at a compared value,
the specials stand where planted() says, the quotients reach the subnormal
range in every tile, and the tile constants are the header's.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import unfused_cases as C

HPP = Path(__file__).resolve().parent.parent / "ipls-java-api_amd" / "csrc" / "ipls_kernels.hpp"

DIV = [(name, secure) for name in C.divide_cases() for secure in (False, True)]


def _differs(a, b):
    return bool((C.bits(a) != C.bits(b)).any())


def test_constants_match_the_header():
    src = HPP.read_text()
    block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    m = re.search(r"constexpr int kFinV = (\d+), kDivV = (\d+);", src)
    fin_v, div_v = int(m.group(1)), int(m.group(2))
    assert re.search(r"kFinTile = \(int64_t\)kBlock \* 2 \* kFinV, kDivTile = \(int64_t\)kBlock \* 2 \* kDivV;", src)
    assert C.TILE_FIN == block * 2 * fin_v == 4096
    assert C.TILE_DIV == block * 2 * div_v == 2048
    assert re.search(r"to_line = \(16 - \(int64_t\)\(\(\(uintptr_t\)o >> 3\) & 15\)\) & 15;", src) and C.LINE == 16
    assert re.search(r"\(threadIdx\.x >> 6\) \* 128 \* kV \+ 2 \* \(threadIdx\.x & 63\)", src) and C.WAVE == 128


def test_special_literals():
    """Every special is what its name says (1e-310 and 2.5e-308 would already be subnormal)."""
    tiny = np.finfo(np.float64).tiny
    assert C.MIN_NORMAL == tiny and C.MAX_SUB == np.nextafter(tiny, 0.0) and C.MAX_F64 == np.finfo(np.float64).max
    S = dict(C.special_values(3.0, True))
    f = {k: C._f(v) for k, v in S.items()}
    for k in ("n3", "n7", "x_den", "minnormal"):
        assert abs(f[k]) >= tiny, k
    with np.errstate(all="ignore"):
        assert 0 < f["n3"] / 3 < tiny and 0 < f["n3"] / 7 < tiny
        assert f["n7"] / 3 >= tiny and 0 < f["n7"] / 7 < tiny
        assert 0 < f["x_den"] / 3e12 < tiny and 0 < f["1e-300"] / 3e12 < tiny
    assert len(S) == 20 and len(C.special_values(3.0, False)) == 15
    assert S["nan"] == C.NAN_BITS and np.isnan(f["nan"]) and f["5e-324"] == 5e-324 > 0
    assert np.signbit(f["-0"]) and f["-0"] == 0 and S["+0"] == 0
    for need in ("-0", "+0", "5e-324", "-5e-324", "maxsub", "minnormal", "n3", "n7", "+max", "-max", "+inf", "-inf",
                 "nan", "1e13", "-1e13", "1e-300", "-1e-300", "3e12"):
        assert need in S
    assert set(C.COUNTS[:6]) == {1.0, 3.0, 7.0, 32.0, 0.0} and np.signbit(C.COUNTS[5])


def test_seam_positions():
    """The seams the issue lists, for one head and for every head at once."""
    n, head = 2 * C.TILE_DIV + 17, 5
    pos = set(C.seam_positions(n + 1, head))
    want = {0, n - 1, head - 1, head, head + 1}
    want |= {head + m + d for m in range(128, C.TILE_DIV + 1, 128) for d in (-1, 0, 1)}   # inside the first whole tile
    want |= {head + C.TILE_DIV * t + d for t in (1, 2) for d in (-1, 0, 1)}
    assert {e for e in want if 0 <= e < n} <= pos and max(pos) == n - 1
    every = set(C.seam_positions(n + 1))
    for h in range(C.LINE):
        assert set(C.seam_positions(n + 1, h)) <= every
    assert n not in every                      # the count slot is no seam
    assert C.seam_positions(1) == [] and C.seam_positions(2) == [0]
    fin = C.seam_classes(2 * C.TILE_FIN + 2, 0, C.TILE_FIN)
    assert [fin[e] for e in (C.TILE_FIN - 1, C.TILE_FIN, C.TILE_FIN + 1, 2 * C.TILE_FIN - 1)] == ["tile"] * 4
    assert fin[511] == fin[512] == fin[513] == "wave"


@pytest.mark.parametrize("name,secure", DIV)
def test_weights_are_built_as_planned(name, secure):
    """The body is position-distinct, the count is the last element, every
    seam holds the special planted() names, and over the handle every seam
    class has seen every special on the P = 17 handles (where a class has
    fewer positions than there are specials, as many different ones as it has
    positions; the handles of three partitions are too small to ask that)."""
    case = C.divide_cases()[name]
    lens, offs, M = C.case_geometry(case)
    W = C.case_weights(name, case, secure)
    assert [len(w) for w in W] == lens and M == sum(L - 1 for L in lens)
    seen, free = {}, []
    for p, (w, L, c) in enumerate(zip(W, lens, case["counts"])):
        assert C._b(w[-1]) == C._b(c)
        plan = C.planted(L, c, secure, p)
        assert [e for e, *_ in plan] == C.seam_positions(L)
        mask = np.ones(L, dtype=bool)
        mask[-1] = False
        for e, cls, nm, b in plan:
            assert C.bits(w)[e] == b, (p, e, nm)
            seen.setdefault(cls, []).append(nm)
            mask[e] = False
        free.append(C.bits(w)[mask])
        mag = np.abs(w[mask])
        assert ((mag >= 1e-3) & (mag < 1e3)).all()
    free = np.concatenate(free)
    assert np.unique(free).size == free.size
    n_spec = len(C.special_values(1.0, secure))
    for cls, names in seen.items():
        if name.startswith("p17"):
            assert len(set(names)) == min(len(names), n_spec), (cls, len(names), sorted(set(names)))


@pytest.mark.parametrize("name,secure", DIV)
def test_divide_variants_differ(name, secure):
    """Every wrong divide differs from the right one at a compared value of
    the handle; the variants that need a certain count differ in every
    partition that has it."""
    case = C.divide_cases()[name]
    W = C.case_weights(name, case, secure)
    lens = C.case_geometry(case)[0]
    hit = {v: 0 for v in C.DIVIDE_VARIANTS + C.SECURE_VARIANTS + ("wire-raw-nan", "shift")}
    for p, (w, c) in enumerate(zip(W, case["counts"])):
        n = len(w) - 1
        if n == 0:
            continue
        right = C.model_divide(w, secure)
        for v in C.DIVIDE_VARIANTS + (C.SECURE_VARIANTS if secure else ()):
            hit[v] += _differs(C.model_divide(w, secure, v), right)
        hit["wire-raw-nan"] += C.model_wire(right) != C.model_wire(right, canonical=False)
        if c == 0.0:                      # +0.0 and -0.0: the pass-through shows wherever a value is not its own quotient
            assert _differs(C.model_divide(w, secure, "no-passthrough"), right), p
            if np.signbit(c):
                assert _differs(C.model_divide(w, secure, "negzero-nonzero"), right), p
            if n >= 7:                    # a pass-through partition carries the NaN payload to the wire
                assert C.model_wire(right) != C.model_wire(right, canonical=False), p
        if C.ordinary(c, secure):
            if secure and n >= 15:
                assert _differs(C.model_divide(w, secure, "secure-ignored"), right), p
            if abs(c) in (3.0, 7.0) and n >= 64:          # by 1.0 and by 32.0 the wrong forms are exact too; n >= 64: a body
                assert _differs(C.model_divide(w, secure, "recip"), right), p
                for v in C.SECURE_VARIANTS[:2] if secure else ():
                    assert _differs(C.model_divide(w, secure, v), right), (p, v)
                if n >= C.TILE_DIV:                       # and in a tenth of the quotients, specials included
                    for v in ("recip",) + (C.SECURE_VARIANTS[:2] if secure else ()):
                        assert (C.bits(C.model_divide(w, secure, v)) != C.bits(right)).mean() >= 0.1, (p, v)
            if n >= 32:
                assert _differs(C.model_divide(w, secure, "ftz"), right), p
            if n < 16:
                continue
            # one element taken from i +- 1, +- 128, +- TILE at a seam
            for d in C.SHIFTS + (C.TILE_DIV, -C.TILE_DIV):
                seams = [i for i in C.seam_positions(len(w)) if 0 <= i + d < n]
                shows = [i for i in seams if _differs(C.model_shift(right, i, d), right)]
                assert len(seams) < 3 or shows, (p, d)      # one or two seams may hold quotients that happen to be equal
                hit["shift"] += bool(shows)
    if name.startswith("p17") or name == "model":
        for v, k in hit.items():
            if v in C.SECURE_VARIANTS and not secure:
                continue
            assert k, f"{name}: variant {v} never shows"


def test_reassociation_shares():
    """Conditions on the inputs: with count 3.0 and with 7.0 at least a tenth
    of a partition's quotients differ between x / cnt and x * (1 / cnt), and a
    tenth of a secure partition's under each two-step division."""
    lens = [C.TILE_DIV + 1] * 2
    for secure in (False, True):
        for w in C.weights(lens, [3.0, 7.0], 5, secure):
            right = C.model_divide(w, secure)
            for v in ("recip",) + (C.SECURE_VARIANTS[:2] if secure else ()):
                share = (C.bits(C.model_divide(w, secure, v)) != C.bits(right)).mean()
                assert share >= 0.1, (secure, w[-1], v, share)


@pytest.mark.parametrize("name,secure", DIV)
def test_subnormal_quotient_in_every_tile(name, secure):
    """For every head, every window one block of k_divide works on -- the head
    elements together with the first tile, then tile by tile -- holds a
    subnormal quotient, in every partition whose divisor allows one
    (ordinary()).  Windows shorter than 32 elements are the last few of a
    partition and may hold fewer seams than there are specials: they are
    covered by the window before them, which the same partition always has."""
    case = C.divide_cases()[name]
    for p, (w, c) in enumerate(zip(C.case_weights(name, case, secure), case["counts"])):
        n = len(w) - 1
        if not C.ordinary(c, secure) or n < 32:
            continue
        q = C.model_divide(w, secure)
        sub = (q != 0.0) & (np.abs(q) < C.MIN_NORMAL)
        for head in range(C.LINE):
            lo = 0
            for hi in list(range(head + C.TILE_DIV, n, C.TILE_DIV)) + [n]:
                if hi - lo >= 32:
                    assert sub[lo:hi].any(), (p, head, lo, hi)
                lo = hi


@pytest.mark.parametrize("name", list(C.FINALIZE_MODELS))
def test_accumulators_are_built_as_planned(name):
    lens = C.lengths_of(C.FINALIZE_MODELS[name])
    assert lens == C.FINALIZE_LENGTHS[name]
    aggs, reps = C.finalize_inputs(name)
    free, seen = [], {}
    for p, (a, r, L) in enumerate(zip(aggs, reps, lens)):
        assert (a[-1], r[-1]) == C.FINALIZE_COUNTS[p] and np.signbit(a[-1]) == np.signbit(C.FINALIZE_COUNTS[p][0])
        plan = C.planted_pairs(L, 2 * p)
        assert [e for e, *_ in plan] == C.seam_positions(L, 0, C.TILE_FIN)
        mask = np.ones(L, dtype=bool)
        mask[-1] = False
        for e, cls, nm, ab, rb in plan:
            assert (C.bits(a)[e], C.bits(r)[e]) == (ab, rb)
            assert not (np.isnan(a[e]) and np.isnan(r[e]))          # never two NaNs in one element
            seen.setdefault(cls, []).append(nm)
            mask[e] = False
        free += [C.bits(a)[mask], C.bits(r)[mask]]
    free = np.concatenate(free)
    assert np.unique(free).size == free.size
    for cls, names in seen.items():       # every pair on every class of seam that the handle has a dozen times
        if len(names) >= 12:
            assert len(set(names)) == len(C.PAIRS), (cls, names)


@pytest.mark.parametrize("name", list(C.FINALIZE_MODELS))
def test_finalize_variants_differ(name):
    """REP ignored shows in every partition with a REP, -0.0 kept in every
    partition without one that holds a -0.0, an index shift at a seam."""
    aggs, reps = C.finalize_inputs(name)
    for mode, present in C.REP_MODES.items():
        for p, (a, r) in enumerate(zip(aggs, reps)):
            has = p in present
            right = C.model_finalize(a, r, has)
            if has:
                assert _differs(C.model_finalize(a, r, has, "rep-ignored"), right), (mode, p)
            elif np.signbit(a[a == 0.0]).any():
                assert _differs(C.model_finalize(a, r, has, "negzero-kept"), right), (mode, p)
            if len(a) < 32:
                continue
            for d in C.SHIFTS + (C.TILE_FIN, -C.TILE_FIN):
                seams = [i for i in C.seam_positions(len(a), 0, C.TILE_FIN) if 0 <= i + d < len(a)]
                assert not seams or any(_differs(C.model_shift(right, i, d), right) for i in seams), (mode, p, d)
    # every handle with a body has a -0.0 pair in a partition whose REP is logically zero
    if max(len(a) for a in aggs) >= 32:
        assert any(np.signbit(a[:-1][a[:-1] == 0.0]).any() for a in aggs)


def test_fallback_inputs():
    """The fallback's buckets never bring two different NaNs together, and the case reaches both kernels' seams."""
    F = C.FALLBACK
    rows, a0, r0 = C.fallback_inputs()
    assert len(rows) == F["n_parts"] and all(len(r) == F["K"] for r in rows)
    assert F["L"] - 1 > 2 * C.TILE_DIV + C.LINE and F["L"] > C.TILE_FIN
    for q, bk in enumerate(rows):
        ops = list(bk) + ([a0] if F["p_first"] + q == F["agg_in"] else []) + ([r0] if F["p_first"] + q == F["rep_in"] else [])
        nan_bits = np.stack([np.where(np.isnan(o), C.bits(o), 0) for o in ops])
        assert set(np.unique(nan_bits)) <= {0, C.NAN_BITS}
        assert np.isnan(np.stack(ops)).any()
