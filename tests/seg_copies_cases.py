"""Inputs and expectations shared by the output-copy-list tests
(test_gpu_seg_copies.py on the GPU, test_seg_copies_cases.py on the CPU):
n_lists lists over one layout of seg_cases.py, every one written by ONE
GetPartitions call.  Every list's views sit at their own residues
(seg_peers_cases.peer_spec) in their own backing arrays, which are filled with
SENTINEL before the call, PAD junk elements around each view; three extra
segments lie past the model and are never written.

W is seg_cases.weights (a different count per partition, one of them 0.0)
plus planted values at every output-segment end, every tile seam (of the
partitions and of the output tiles) and every partition seam: in plain mode
W = q * cnt with the product exact in double, so the quotient is q itself, for
the q of PLANTED.  The expectation is the oracle's alone: get_partitions, then
seg_cases.narrow per segment -- the same bits for every list.

image() is a numpy model of the memory the call leaves: per list and segment
the backing array's bytes.  With a `mistake` it is the memory a kernel making
that mistake would leave; MISTAKES names them.
"""
import numpy as np

import seg_cases as S
import seg_peers_cases as C

FMTS = S.FMTS
P = S.P
NS = (1, 2, 3, 9)                                           # n_lists
EXTRA = [("f32", 5, 3), ("half", 0, 0), ("f64", 7, 1)]      # past the model: never written
ZERO_COUNT = 4                                              # seg_cases.weights: the partition whose count is 0.0

# q: what each is planted for (test_seg_copies_cases.py asserts it)
PLANTED = {
    "negative zero": -0.0,
    "f32 tie": 1.0 + 2.0 ** -24,                            # halfway between 1 and 1 + 2^-23: to even, 1.0
    "bf16 double rounding": 1.0 + 2.0 ** -8 + 2.0 ** -40,   # above the bf16 tie; its float IS the tie
    "half double rounding": 1.0 + 2.0 ** -11 + 2.0 ** -40,  # above the half tie; its float IS the tie
    "half overflow": 70000.0,
    "f32 subnormal": 2.0 ** -140,
    "nan": float("nan"),
}
MISTAKES = ("1 list k stored at list 0's residue", "2 pointer table read segment-major", "3 last list skipped",
            "4 head item written to list 0 only", "5 vector body at a misaligned list, rounded down to 16 B",
            "6 the element at the model size written", "7 the neighbour's count across a partition seam",
            "8 the zero count divided", "9 one rounding for the 16-bit formats", "10 the secure divisor dropped")


def layouts(c):
    """The layouts that hold the whole model (an output list may not be shorter)."""
    M = S.model_size(c)
    return tuple(name for name in S.LAYOUTS if sum(s[1] for s in S.shape(name, c, S.TILE_DEFAULT)) >= M)


def out_spec(name, c, T):
    """List 0's layout: seg_cases' plus the three segments past the model."""
    return S.shape(name, c, T) + EXTRA


def list_spec(spec, k):
    """List k's residues (list 0 keeps the layout's)."""
    return C.peer_spec(spec, k)


def items(spec, M, T):
    """The plan's items over list 0: (segment, lo, hi, flat of lo, is_head, whole) -- per output segment the head up
    to the first 128-B line (backing arrays start on a line), then tiles of T; nothing at or past M."""
    out, at = [], 0
    for i, (fmt, n, r) in enumerate(spec):
        k = max(0, min(at + n, M) - at)
        if k:
            a = (r * S.esize(fmt)) % 128
            head = min(((128 - a) % 128) // S.esize(fmt), k)
            lo = 0
            while lo < k:
                is_head = lo == 0 and head > 0
                hi = lo + head if is_head else min(lo + T, k)
                out.append((i, lo, hi, at + lo, is_head, hi - lo))
                lo = hi
        at += n
    return out


def plant_positions(spec, c, T, M):
    """Flat positions below M: seg_cases' (segment ends, partition tile seams, partition boundaries) and both sides
    of every output-tile seam."""
    pos = {f for f in S.plant_positions(spec, c, T, M) if 0 <= f < M}
    for _, lo, hi, flat, _, _ in items(spec, M, T):
        pos.update(f for f in (flat - 1, flat, flat + (hi - lo) - 1) if 0 <= f < M)
    return sorted(pos)


def weights(rng, O, name, c, T):
    """(W per partition, {flat position: name of the planted q})."""
    w = S.weights(rng, O, c)
    M = S.model_size(c)
    names = list(PLANTED)
    where = {}
    for t, f in enumerate(plant_positions(out_spec(name, c, T), c, T, M)):
        p, j = f // c, f % c
        q = PLANTED[names[t % len(names)]]
        cnt = w[p][-1]
        w[p][j] = q if cnt == 0.0 else q * cnt
        where[f] = names[t % len(names)]
    return w, where


def expected(O, w, spec, M, secure):
    """Per segment the bit patterns of the elements below M: the same for every list."""
    return S.expected_outputs(O.get_partitions(w, secure), spec, M)


# ---- the memory a call leaves ----
def blank(specs):
    """[[backing bytes per segment] per list], every byte SENTINEL."""
    return [[np.full((r + n + S.PAD) * S.esize(fmt), S.SENTINEL, dtype=np.uint8) for fmt, n, r in sp] for sp in specs]


def direct16(x, fmt):
    """Doubles rounded ONCE to the 16-bit format (the mistake; where that is not plain to do, the two-step bits)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    two = S.narrow(x, fmt)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if fmt == "half":
            return np.where(np.isnan(x), two, x.astype(np.float16).view(np.uint16))
        m, e = np.frexp(x)
        ok = np.isfinite(x) & (np.abs(x) >= 2.0 ** -126) & (np.abs(x) < 2.0 ** 127)
        y = np.ldexp(np.rint(np.where(ok, m, 0.0) * 256.0) / 256.0, e)     # 8 significand bits, ties to even
        once = (y.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        return np.where(ok, once, two)


def flat_model(O, w, spec, c, T, secure, mistake=None):
    """The flat model of doubles a kernel would narrow: the oracle's, or a mistake's."""
    M = S.model_size(c)
    if mistake == MISTAKES[6]:
        return S.mistake_models(w, spec, c, T, secure).get("the neighbour's count across a partition seam")
    if mistake == MISTAKES[7]:
        with np.errstate(divide="ignore", invalid="ignore"):
            parts = [x[:-1] / (1e12 * x[-1] if secure else x[-1]) for x in w]
        return np.concatenate(parts)[:M]
    if mistake == MISTAKES[9]:
        return O.get_partitions(w, False) if secure else None
    return O.get_partitions(w, secure)


def image(O, w, name, c, T, n_lists, secure, mistake=None):
    """The backing arrays after the call, or None when the mistake's premise is not in the case."""
    M = S.model_size(c)
    spec = out_spec(name, c, T)
    specs = [list_spec(spec, k) for k in range(n_lists)]
    model = flat_model(O, w, spec, c, T, secure, mistake)
    if model is None:
        return None
    n_segs = len(spec)
    mem = blank(specs)
    hit = mistake is None or mistake in MISTAKES[6:]

    def put(k, i, e, bits, shift=0):
        """bits -> elements [e, ..) of the view of list k's segment i, `shift` bytes lower; clipped to the backing."""
        fmt, _, r = specs[k][i]
        raw = np.ascontiguousarray(bits).view(np.uint8)
        a = (r + e) * S.esize(fmt) - shift
        b = mem[k][i]
        n = max(0, min(raw.size, b.size - a))
        b[a:a + n] = raw[:n]

    for i, lo, hi, flat, is_head, n in items(spec, M, T):
        fmt = spec[i][0]
        x = model[flat:flat + n]
        bits = direct16(x, fmt) if mistake == MISTAKES[8] and fmt in ("half", "bf16") else S.narrow(x, fmt)
        whole = not is_head and n == T and flat // c == (flat + T - 1) // c
        for k in range(n_lists):
            if mistake == MISTAKES[2] and k == n_lists - 1:
                hit = True
                continue
            if mistake == MISTAKES[3] and is_head and k:
                hit = True
                continue
            if mistake == MISTAKES[0] and specs[k][i][2] != spec[i][2]:
                hit = True
                put(k, i, lo - specs[k][i][2] + spec[i][2], bits)
                continue
            if mistake == MISTAKES[1]:
                kk, ii = divmod(i * n_lists + k, n_segs)
                hit = hit or (kk, ii) != (k, i)
                # the segment's values land where that array's view starts, in that array's element size
                raw = bits.view(np.uint8)
                tf, _, tr = specs[kk][ii]
                a = tr * S.esize(tf) + lo * S.esize(fmt)
                b = mem[kk][ii]
                m = max(0, min(raw.size, b.size - a))
                b[a:a + m] = raw[:m]
                continue
            shift = 0
            if mistake == MISTAKES[4] and whole:
                shift = ((specs[k][i][2] + lo) * S.esize(fmt)) % 16
                hit = hit or shift != 0
            put(k, i, lo, bits, shift)
    if mistake == MISTAKES[5]:
        at = 0
        for i, (fmt, n, r) in enumerate(spec):
            if at <= M < at + n:
                hit = True
                for k in range(n_lists):
                    put(k, i, M - at, S.narrow(np.array([1.0]), fmt))
            at += n
    return mem if hit else None


def same(a, b):
    return all(np.array_equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))


# ---- coverage ----
def coverage(name, c, T, n_lists):
    """({(fmt, lists aligned at the tile and lists not?)} of the whole tiles, {segments a partial tile spans},
    a partial tile holds a partition seam?)"""
    M = S.model_size(c)
    spec = out_spec(name, c, T)
    specs = [list_spec(spec, k) for k in range(n_lists)]
    whole, seam = set(), False
    for i, lo, hi, flat, is_head, n in items(spec, M, T):
        fmt = spec[i][0]
        if not is_head and n == T and flat // c == (flat + T - 1) // c:
            al = {((specs[k][i][2] + lo) * S.esize(fmt)) % 16 == 0 for k in range(n_lists)}
            whole.add((fmt, len(al) == 2))
        elif flat // c != (flat + n - 1) // c:
            seam = True
    # the partitions' own tiles (the twin's notion of a partial tile): how many segments one spans
    segs = [S.Seg(f, n, r) for f, n, r in spec]
    spans = set()
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, M) - p * c)
        for lo in range(0, ncopy, T):
            pcs = S.pieces_of(segs, p * c + lo, p * c + min(lo + T, ncopy))
            if not (len(pcs) == 1 and min(lo + T, ncopy) - lo == T):
                spans.add(len(pcs))
    return whole, spans, seam


def check_coverage(T):
    whole, spans, seam = set(), set(), False
    for c in S.chunks(T):
        for name in layouts(c):
            w, s, m = coverage(name, c, T, max(NS))
            whole |= w
            spans |= s
            seam = seam or m
    for fmt in FMTS:
        assert (fmt, True) in whole, f"no whole {fmt} tile with 16-B aligned and unaligned lists"
    assert 2 in spans and 3 in spans, spans
    assert seam, "no partial tile holds a partition seam"
    return whole, spans, seam
