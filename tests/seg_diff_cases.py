"""Inputs and expectations shared by the difference-list tests
(test_gpu_seg_diff.py on the GPU, test_seg_diff_cases.py on the CPU).  The
layouts are seg_cases.py's; every case gets a SECOND list of the same lengths
and formats, each subtrahend view at its own residue in its own backing array
with junk around it.  The expected difference is numpy's alone -- native for
f64 and f32, native float16 subtraction for halves, float32 subtraction
narrowed by seg_cases.narrow for bf16 -- widened and handed to seg_cases'
oracle-side expectations.  Planted operand pairs, the coverage conditions
(asserted) and numpy models of the mistakes a difference kernel can make.
"""
import numpy as np

import seg_cases as S

FMTS = S.FMTS
P = S.P
LAYOUTS = S.LAYOUTS
MANT = {"f64": 53, "f32": 24, "half": 11, "bf16": 8}            # significand bits, the hidden one included
EMIN = {"f64": -1022, "f32": -126, "half": -14, "bf16": -126}   # exponent of the smallest normal
MAXF = {"f64": float(np.finfo(np.float64).max), "f32": float(np.finfo(np.float32).max), "half": 65504.0,
        "bf16": float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])}
PAIR_KINDS = ("tie", "inexact", "subnormal", "overflow", "equal", "negzero", "infinf", "nan")


def enc(values, fmt):
    """Bit patterns of doubles the format holds exactly."""
    bits = S.narrow(np.asarray(values, dtype=np.float64), fmt)
    w = S.widen(bits, fmt)
    assert all(x == y or (x != x and y != y) for x, y in zip(w, np.asarray(values, dtype=np.float64))), (values, fmt)
    return bits


def pairs(fmt):
    """{kind: (minuend bits, subtrahend bits)}: operand pairs whose difference
    is a round-to-even tie (1 - 2^-(m+1) -> 1.0), inexact and no tie, subnormal
    in the format, an overflow to +inf, +0.0 from equal operands, -0.0 from
    (-0.0, +0.0), inf - inf, and one NaN operand."""
    m, e = MANT[fmt], EMIN[fmt]
    v = {
        "tie": (1.0, 2.0 ** -(m + 1)),
        "inexact": (1.0, 3.0 * 2.0 ** -(m + 2)),
        "subnormal": (1.5 * 2.0 ** e, 2.0 ** e),
        "overflow": (MAXF[fmt], -MAXF[fmt]),
        "equal": (1.5, 1.5),
        "negzero": (-0.0, 0.0),
        "infinf": (np.inf, np.inf),
        "nan": (np.nan, 1.0),
    }
    return {k: (enc([a], fmt)[0], enc([b], fmt)[0]) for k, (a, b) in v.items()}


def sub_bits(a_bits, b_bits, fmt):
    """The difference in the format, as bit patterns: numpy alone."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if fmt == "f64":
            return (a_bits.view(np.float64) - b_bits.view(np.float64)).view(np.uint64)
        if fmt == "f32":
            return (a_bits.view(np.float32) - b_bits.view(np.float32)).view(np.uint32)
        if fmt == "half":
            return (a_bits.view(np.float16) - b_bits.view(np.float16)).view(np.uint16)
        f = S.widen(a_bits, fmt).astype(np.float32) - S.widen(b_bits, fmt).astype(np.float32)
        return S.narrow(f.astype(np.float64), "bf16")


def shape_b(name, spec):
    """The subtrahend's residue per segment: the layout's own residue moved by
    an amount that differs from segment to segment, so that both sources meet
    aligned and unaligned tiles independently of each other."""
    kind = name.partition("-")[0]
    out = []
    for i, (fmt, n, r) in enumerate(spec):
        k = S.residues(fmt)
        d = {"whole": 1, "residues": 0}.get(kind, i + 2)
        out.append((fmt, n, (r + d) % k))
    return out


def build(rng, name, c, T):
    """(minuend Segs, subtrahend Segs): normals, the planted pairs at every
    segment end, tile seam and partition boundary, junk around every view."""
    spec = S.shape(name, c, T)
    M = S.model_size(c)
    plant = S.plant_positions(spec, c, T, M)
    A, B, at, k = [], [], 0, 0
    for (fmt, n, ra), (_, _, rb) in zip(spec, shape_b(name, spec)):
        def backing(r):
            x = rng.standard_normal(r + n + S.PAD)
            return x.view(np.uint64).copy() if fmt == "f64" else S.F.from_f32(x.astype(np.float32), fmt)
        a, b = backing(ra), backing(rb)
        pr = pairs(fmt)
        for i in range(n):
            if at + i in plant:
                a[ra + i], b[rb + i] = pr[PAIR_KINDS[k % len(PAIR_KINDS)]]
                k += 1
        A.append(S.Seg(fmt, n, ra, a))
        B.append(S.Seg(fmt, n, rb, b))
        at += n
    return A, B


def difference(A, B):
    """The difference list as Segs (residue 0) of the result's bit patterns."""
    return [S.Seg(a.fmt, a.n, 0, sub_bits(a.bits, b.bits, a.fmt)) for a, b in zip(A, B)]


def expected_update(O, acc, A, B, c, owned):
    return S.expected_update(O, acc, difference(A, B), c, owned)


def expected_texts(O, A, B, c, parts, iteration, origin, pid=3):
    return S.expected_texts(O, difference(A, B), c, parts, iteration, origin, pid)


# ---- coverage ----
def coverage(name, c, T):
    """({(fmt, minuend residue 0?, subtrahend residue 0?)} of the whole tiles,
    {number of segments a partial tile's pieces span})."""
    spec = S.shape(name, c, T)
    rb = [s[2] for s in shape_b(name, spec)]
    segs = [S.Seg(f, k, r) for f, k, r in spec]
    n = sum(s[1] for s in spec)
    whole, spans = set(), set()
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, n) - p * c)
        for lo in range(0, ncopy, T):
            hi = min(lo + T, ncopy)
            pcs = S.pieces_of(segs, p * c + lo, p * c + hi)
            if len(pcs) == 1 and hi - lo == T:
                i, e, _ = pcs[0]
                fmt, _, ra = spec[i]
                k = S.residues(fmt)
                whole.add((fmt, (ra + e) % k == 0, (rb[i] + e) % k == 0))
            else:
                spans.add(len(pcs))
    return whole, spans


def check_coverage(T):
    """Over the chunks and layouts: whole tiles of every format in all four
    alignment combinations, and partial tiles over two and over three segments."""
    whole, spans = set(), set()
    for c in S.chunks(T):
        for name in LAYOUTS:
            w, s = coverage(name, c, T)
            whole |= w
            spans |= s
    for fmt in FMTS:
        for a0 in (True, False):
            for b0 in (True, False):
                assert (fmt, a0, b0) in whole, f"no whole {fmt} tile with minuend aligned={a0}, subtrahend aligned={b0}"
    assert 2 in spans and 3 in spans, spans
    return whole, spans


# ---- the mistakes, each as the flat vector a kernel making it would produce ----
def _trunc_sub(a_bits, b_bits, fmt):
    """The difference rounded toward zero instead of to nearest-even, widened."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if fmt == "f64":
            a, nb = a_bits.view(np.float64), -b_bits.view(np.float64)
            s = a + nb
            bp = s - a
            err = (a - (s - bp)) + (nb - bp)               # TwoSum: a - b = s + err exactly
            away = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((err < 0) == (s > 0))
            return np.where(away, np.nextafter(s, 0.0), s)
        d = S.widen(a_bits, fmt) - S.widen(b_bits, fmt)
        if fmt == "bf16":
            f = d.astype(np.float32)
            f = np.where(np.isfinite(f) & (np.abs(f.astype(np.float64)) > np.abs(d)), np.nextafter(f, np.float32(0)), f)
            return S.widen((f.view(np.uint32) >> 16).astype(np.uint16), "bf16")
        t = np.float32 if fmt == "f32" else np.float16
        r = d.astype(t)
        r = np.where(np.isfinite(r) & (np.abs(r.astype(np.float64)) > np.abs(d)), np.nextafter(r, t(0)), r)
        return r.astype(np.float64)


def _flush(bits, fmt):
    """Subnormal results to a zero of their sign."""
    w = S.widen(bits, fmt)
    tiny = (w != 0) & (np.abs(w) < 2.0 ** EMIN[fmt])
    return np.where(tiny, np.copysign(0.0, w), w)


def _cat(parts):
    return np.concatenate(list(parts) + [np.zeros(0)])


def mistake_vectors(A, B, c):
    """{mistake: flat vector}; only the mistakes whose premise the layout has."""
    live = [(a, b) for a, b in zip(A, B) if a.n]
    out = {}
    if not live:
        return out
    wide = lambda bits, fmt: S.widen(bits, fmt)   # noqa: E731
    out["operands exchanged"] = _cat(wide(sub_bits(b.bits, a.bits, a.fmt), a.fmt) for a, b in live)
    with np.errstate(over="ignore", invalid="ignore"):
        out["subtraction after widening"] = _cat(a.wide - b.wide for a, b in live)
        out["float result not rounded to the format"] = _cat(
            (a.wide.astype(np.float32) - b.wide.astype(np.float32)).astype(np.float64) if a.fmt in ("half", "bf16")
            else wide(sub_bits(a.bits, b.bits, a.fmt), a.fmt) for a, b in live)
    out["truncation instead of nearest-even"] = _cat(_trunc_sub(a.bits, b.bits, a.fmt) for a, b in live)
    out["subnormal results flushed"] = _cat(_flush(sub_bits(a.bits, b.bits, a.fmt), a.fmt) for a, b in live)
    out["-0.0 lost"] = _cat(wide(sub_bits(a.bits, b.bits, a.fmt), a.fmt) + 0.0 for a, b in live)
    if any(a.r != b.r for a, b in live):
        out["subtrahend read at the minuend's residue"] = _cat(
            wide(sub_bits(a.bits, b.backing[a.r:a.r + a.n], a.fmt), a.fmt) for a, b in live)
    # the subtrahend's piece start taken from the segment start: a piece that begins at element e0 > 0 of its
    # segment reads the subtrahend from element 0
    n = S.total(A)
    vec, hit = [], False
    for p in range(P):
        for i, e0, k in S.pieces_of(A, p * c, min((p + 1) * c, n)):
            a, b = A[i], B[i]
            vec.append(wide(sub_bits(a.bits[e0:e0 + k], b.bits[:k], a.fmt), a.fmt))
            hit = hit or e0 > 0
    if hit:
        out["subtrahend piece start from the segment start"] = _cat(vec)
    if len(live) > 1:
        vec, prev = [], None
        for a, b in live:
            bb = b.bits.copy()
            if prev is not None:
                bb[0] = S.narrow(prev.wide[-1:], a.fmt)[0]
            vec.append(wide(sub_bits(a.bits, bb, a.fmt), a.fmt))
            prev = b
        out["previous segment's subtrahend for a first element"] = _cat(vec)
    return out


MISTAKES = 9
