"""The fused aggregation round over trainer-format buckets (k_round_narrow):
``aggregate_round`` with 16-B aligned DEV_F32 / DEV_F16 / DEV_BF16 buckets and
averages of a trainer format (or none) is one pass -- fold, W = AGG + REP, the
GetPartitions divide narrowed to the averages' format.

Every comparison is bit for bit against the oracle: ``O.reduce`` on the widened
values, ``O.aggregate_partition``, ``O.get_partitions``, then
``.astype(np.float32)`` and, for a 16-bit format, ``h16_ref.narrow``.  NaN
positions must match, payloads are free.

A 16-bit array is carried as uint16 patterns, an f32 array as uint32 patterns.
T (= block x 4 x vectors) and block are read from the launch record of one
fused call per element size; every length is under 100k elements.
"""
import numpy as np
import pytest

from conftest import assert_bits_equal

import h16_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMTS = ("f32", "half", "bf16")
KS = (1, 3, 9)
LNAMES = ("9", "T", "T+1", "2T+8b+14")


@pytest.fixture(scope="module")
def ipls():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu run without a visible GPU")
    import ipls as m
    return m


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


# --------------------------------------------------------------------------
# formats
# --------------------------------------------------------------------------
_TDT = {"f32": torch.float32, "half": torch.float16, "bf16": torch.bfloat16}
_CARRIER = {"f32": torch.int32, "half": torch.int16, "bf16": torch.int16}
_NPBITS = {"f32": np.uint32, "half": np.uint16, "bf16": np.uint16}
_NPDT = {"f32": np.float32, "half": np.float16, "bf16": "bf16"}


def _esz(fmt):
    return 4 if fmt == "f32" else 2


def _to_fmt(x, fmt):
    """Doubles / floats rounded to the format (float first): its bit patterns."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.ascontiguousarray(x).astype(np.float32)
    return f.view(np.uint32).copy() if fmt == "f32" else R.narrow(f, fmt).reshape(f.shape).copy()


def _widen(bits, fmt):
    """The exact doubles of the format's bit patterns."""
    with np.errstate(invalid="ignore"):
        if fmt == "f32":
            return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)
        return R.widen(bits, fmt).reshape(np.shape(bits))


def _narrow_out(q64, fmt):
    """The averages' rule: the f64 quotient rounded to float, then to the format."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        f = np.ascontiguousarray(q64, dtype=np.float64).astype(np.float32)
    return f.view(np.uint32).copy() if fmt == "f32" else R.narrow(f, fmt)


def _is_nan(bits, fmt):
    if fmt == "f32":
        return (np.asarray(bits, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000
    return R.is_nan(bits, fmt)


def _exact_out(got, want, fmt, what):
    got = np.ascontiguousarray(got).view(_NPBITS[fmt])
    want = np.ascontiguousarray(want).view(_NPBITS[fmt])
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = _is_nan(got, fmt), _is_nan(want, fmt)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"


def _dev_rows(bits, fmt, offs=0):
    """The rows of a 2-D pattern array as device tensors of the format's torch
    dtype; row j's base is 16-B aligned plus offs (or offs[j]) elements."""
    bits = np.ascontiguousarray(bits, dtype=_NPBITS[fmt])
    n, L = bits.shape
    offs = [offs] * n if isinstance(offs, int) else list(offs)
    per16 = 16 // _esz(fmt)
    stride = (L + max(offs) + per16 - 1) // per16 * per16
    t = torch.zeros((n, stride), dtype=_CARRIER[fmt], device="cuda")
    src = torch.from_numpy(bits.view(np.int32 if fmt == "f32" else np.int16)).cuda()
    for j in range(n):
        t[j, offs[j]:offs[j] + L] = src[j]
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, [t[j, offs[j]:offs[j] + L].view(_TDT[fmt]) for j in range(n)]


def _db(ipls, rows):
    return [ipls.DeviceBuffer.from_tensor(r) for r in rows]


def _table(ipls, x, fmt, offs=0):
    """x[q][j] = bucket j of partition q (patterns) -> (keep-alive, bucket table)."""
    P, k, L = x.shape
    keep, rows = _dev_rows(x.reshape(P * k, L), fmt, offs)
    bufs = _db(ipls, rows)
    return keep, [[bufs[q * k + j] for j in range(k)] for q in range(P)]


_SENT = {"f32": 0x55555555, "half": 0x5555, "bf16": 0x5555}


class _DevOut:
    """n averages of a format in device memory, `off` elements past a 16-B
    boundary, sentinels around them."""

    def __init__(self, ipls, n, fmt, off):
        self.n, self.fmt, self.off = n, fmt, off
        self.t = torch.full((n + off + 40,), _SENT[fmt], dtype=_CARRIER[fmt], device="cuda")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.buf = ipls.DeviceBuffer.from_tensor(self.t[off:off + n].view(_TDT[fmt]))

    def bits(self):
        h = self.t.cpu().numpy().view(_NPBITS[self.fmt])
        s = _SENT[self.fmt]
        assert np.all(h[:self.off] == s) and np.all(h[self.off + self.n:] == s), "wrote outside the output"
        return h[self.off:self.off + self.n].copy()


def _round_kernel(ipls, fmt):
    return ipls.KERNEL_ROUND_F32 if fmt == "f32" else ipls.KERNEL_ROUND_H16


def _fold_kernel(ipls, fmt):
    return ipls.KERNEL_REDUCE_F32 if fmt == "f32" else ipls.KERNEL_REDUCE_H16


_TILE = {}


def _tile(ipls, fmt):
    """(T, block) of the fused round over buckets of fmt's element size, from the launch record."""
    key = _esz(fmt)
    if key not in _TILE:
        x = np.full((1, 1, 9), _to_fmt(np.ones(1), fmt)[0], dtype=_NPBITS[fmt])
        keep, tab = _table(ipls, x, fmt)
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as agg:
            agg.aggregate_round(0, tab, with_average=False)
            li = agg.last_launch()
        assert li["kernel"] == _round_kernel(ipls, fmt), li
        _TILE[key] = (li["block"] * 4 * li["vectors"], li["block"])
        assert _TILE[key][0] <= 32768
    return _TILE[key]


def _length(ipls, fmt, name):
    T, b = _tile(ipls, fmt)
    L = {"9": 9, "T": T, "T+1": T + 1, "2T+8b+14": 2 * T + 8 * b + 14}[name]   # + 14, not + 13: (L - 1) mod 4 == 1
    assert L < 100000
    return L


def _buckets(rng, P, k, lengths, fmt, count=1.0):
    """Normals rounded to the format, `count` in every count slot, zeros past it."""
    Lm = max(lengths)
    x = _to_fmt(rng.standard_normal((P, k, Lm)), fmt)
    c = _to_fmt(np.array([count]), fmt)[0]
    for q, L in enumerate(lengths):
        x[q, :, L - 1] = c
        x[q, :, L:] = 0
    return x


def _oracle_ws(O, x, fmt, lengths, k, rep=None, pre=None):
    """W of every partition: the fold of the first k buckets in order (from
    pre[q] when AGG was loaded, else from +0.0), then AGG + REP."""
    ws = []
    for q, L in enumerate(lengths):
        b = [_widen(x[q, j, :L], fmt) for j in range(k)]
        with np.errstate(all="ignore"):
            if pre is not None and pre[q] is not None:
                a = O.reduce(b, L, O.START_ACCUM, acc=pre[q][:L])
            else:
                a = O.reduce(b, L, O.START_ZERO)
            w, wa = np.zeros(L), np.zeros(L)
            r = np.zeros(L) if rep is None or rep[q] is None else np.array(rep[q][:L], dtype=np.float64)
            O.aggregate_partition(a, r, w, wa)
        ws.append(w)
    return ws


def _want(O, ws, secure, fmt):
    with np.errstate(all="ignore"):
        return _narrow_out(O.get_partitions(ws, secure), fmt)


def _check_w(agg, ipls, ws, what):
    for q, w in enumerate(ws):
        assert_bits_equal(agg.read(q, ipls.TGT_WEIGHTS), w, f"{what}: W p={q}")


def _check_consumed(agg, ipls, P, what):
    """AGG and REP ended logically zero: a round without buckets gives W = +0.0."""
    agg.aggregate_round(0, [[] for _ in range(P)], with_average=False)
    for q in range(P):
        w = agg.read(q, ipls.TGT_WEIGHTS)
        assert not w.view(np.uint64).any(), f"{what}: W p={q} of an empty following round is not +0.0"


# --------------------------------------------------------------------------
# 1. the launch record
# --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_launch_record(ipls, O, fmt):
    T, block = _tile(ipls, fmt)
    P, k, L = 2, 3, T + 6
    rng = np.random.default_rng(11)
    x = _buckets(rng, P, k, [L] * P, fmt)
    ws = _oracle_ws(O, x, fmt, [L] * P, k)
    want = _want(O, ws, False, fmt)
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        keep, tab = _table(ipls, x, fmt)
        got = agg.aggregate_round(0, tab, dtype=_NPDT[fmt])
        li = agg.last_launch()
        assert li["kernel"] == _round_kernel(ipls, fmt), li
        assert li["block"] == block and li["block"] * 4 * li["vectors"] == T
        assert li["seqf"] == 1 and li["map"] == 3 and li["start"] == ipls.START_ZERO
        assert li["grid"] == 2 * P                       # one full and one partial tile per partition
        _exact_out(got, want, fmt, "fused")
        _check_w(agg, ipls, ws, "fused")
        # no averages: still the fused kernel
        agg.aggregate_round(0, tab, with_average=False)
        assert agg.last_launch()["kernel"] == _round_kernel(ipls, fmt)
        # one bucket one element past a 16-B boundary: the three steps, same bits
        offs = [0] * (P * k)
        offs[k + 1] = 1
        keep2, tab2 = _table(ipls, x, fmt, offs)
        got2 = agg.aggregate_round(0, tab2, dtype=_NPDT[fmt])
        li2 = agg.last_launch()
        assert li2["kernel"] == _fold_kernel(ipls, fmt) and li2["seqf"] == 0, li2
        _exact_out(got2, want, fmt, "three steps")
        _check_w(agg, ipls, ws, "three steps")
        # f64 averages from narrow buckets keep the three steps too
        got3 = agg.aggregate_round(0, tab)
        assert agg.last_launch()["kernel"] == _fold_kernel(ipls, fmt)
        with np.errstate(all="ignore"):
            assert_bits_equal(got3, O.get_partitions(ws), "f64 averages")
    # a length that is a whole number of tiles: partition-major (map 0)
    x1 = _buckets(rng, 1, 1, [T], fmt)
    with ipls.Aggregator(n_partitions=1, bucket_len=T) as agg:
        keep, tab = _table(ipls, x1, fmt)
        agg.aggregate_round(0, tab, with_average=False)
        li = agg.last_launch()
        assert li["kernel"] == _round_kernel(ipls, fmt) and li["map"] == 0 and li["grid"] == 1, li


# --------------------------------------------------------------------------
# 2. parity over S x A, secure on and off, lengths, k, output placements
# --------------------------------------------------------------------------
@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("src", FMTS)
def test_parity(ipls, O, src, lname):
    L, P, kmax = _length(ipls, src, lname), 4, max(KS)
    lengths = [L] * P
    rng = np.random.default_rng(21)
    x = _buckets(rng, P, kmax, lengths, src)
    keep, full = _table(ipls, x, src)
    n_avg = P * (L - 1)
    aggs = {s: ipls.Aggregator(n_partitions=P, bucket_len=L, secure=s) for s in (False, True)}
    try:
        if lname == "2T+8b+14":
            assert sorted(o % 4 for o in aggs[False].offsets) == [0, 1, 2, 3]   # the partitions land at m = 0..3
        for k in KS:
            tab = [row[:k] for row in full]
            ws = _oracle_ws(O, x, src, lengths, k)
            for secure, agg in aggs.items():
                first = True
                for avg in FMTS:
                    what = f"{src}->{avg} L={lname} k={k} secure={secure}"
                    want = _want(O, ws, secure, avg)
                    for off in (0, 3):
                        out = _DevOut(ipls, n_avg, avg, off)
                        assert agg.aggregate_round(0, tab, out=out.buf) is out.buf
                        agg.sync()
                        assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
                        _exact_out(out.bits(), want, avg, f"{what} device+{off}")
                    got = agg.aggregate_round(0, tab, dtype=_NPDT[avg])
                    assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
                    _exact_out(got, want, avg, f"{what} host")
                    if first:
                        _check_w(agg, ipls, ws, what)
                        _check_consumed(agg, ipls, P, what)
                        first = False
    finally:
        for a in aggs.values():
            a.close()


# --------------------------------------------------------------------------
# 3. the reference geometry
# --------------------------------------------------------------------------
@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("src", FMTS)
def test_reference_geometry(ipls, O, src, secure):
    M, P, k = 3 * 4133 - 1, 3, 3
    rng = np.random.default_rng(31)
    with ipls.Aggregator(M, P, secure=secure) as agg:
        lengths = agg.lengths
        assert len(set(lengths)) == 2                    # the last partition differs, as the chunk rule gives
        Lm = max(lengths) + 5                            # the buckets are longer than L_p
        x = _to_fmt(rng.standard_normal((P, k, Lm)), src)
        for q, L in enumerate(lengths):
            x[q, :, L - 1] = _to_fmt(np.ones(1), src)[0]
        keep, tab = _table(ipls, x, src)
        ws = _oracle_ws(O, x, src, lengths, k)
        for avg in FMTS:
            want = _want(O, ws, secure, avg)
            out = _DevOut(ipls, agg.flat_size, avg, 1)
            agg.aggregate_round(0, tab, out=out.buf)
            agg.sync()
            assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
            _exact_out(out.bits(), want, avg, f"reference geometry {src}->{avg} secure={secure}")
            _exact_out(agg.aggregate_round(0, tab, dtype=_NPDT[avg]), want, avg, f"reference geometry {src}->{avg} host")
        _check_w(agg, ipls, ws, "reference geometry")
        _check_consumed(agg, ipls, P, "reference geometry")


# --------------------------------------------------------------------------
# 4. start and REP
# --------------------------------------------------------------------------
def _classes_len(ipls, fmt):
    """A length with full-tile, vector-step and scalar-remainder elements, (L - 1) mod 4 == 1."""
    T, b = _tile(ipls, fmt)
    return T + 4 * b + 6


def _set_exact(ipls, agg, p, target, v):
    """target[p] = v exactly (a FIRST-started fold of one f64 device bucket keeps -0.0)."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    agg.reduce_batch(p, [[ipls.DeviceBuffer.from_tensor(t)]], start_mode=ipls.START_FIRST, target=target)
    agg.sync()


@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("src", FMTS)
def test_start_and_rep(ipls, O, src, secure):
    L, P, k = _classes_len(ipls, src), 4, 3
    lengths = [L] * P
    rng = np.random.default_rng(41)
    x = _buckets(rng, P, k, lengths, src)
    x[2, :, L - 1] = 0                                   # partition 2: every count slot +0.0
    x[3, :, L - 1] = _to_fmt(np.array([-0.0]), src)[0]   # partition 3: the count is -0.0
    rep = [rng.standard_normal(L), None, None, rng.standard_normal(L)]
    pre = [None, rng.standard_normal(L), None, rng.standard_normal(L)]
    rep[0][L - 1] = 0.0
    pre[1][L - 1] = 2.0                                  # two earlier arrivals
    rep[3][L - 1] = pre[3][L - 1] = -0.0
    ws = _oracle_ws(O, x, src, lengths, k, rep=rep, pre=pre)
    assert [w[-1] for w in ws[:3]] == [k, k + 2.0, 0.0] and ws[3][-1] == 0.0 and np.signbit(ws[3][-1])
    with np.errstate(all="ignore"):
        q64 = O.get_partitions(ws, secure)
    # partitions 2 and 3 pass through undivided
    assert_bits_equal(q64[2 * (L - 1):3 * (L - 1)], ws[2][:-1], "oracle: count +0.0")
    assert_bits_equal(q64[3 * (L - 1):], ws[3][:-1], "oracle: count -0.0")
    keep, tab = _table(ipls, x, src)
    for avg in FMTS:
        with ipls.Aggregator(n_partitions=P, bucket_len=L, secure=secure) as agg:
            agg.Update(rep[0], 0, from_clients=False)    # REP non-zero on 0 and 3, logically zero on 1 and 2
            agg.Update(pre[1], 1)                        # AGG loaded on one partition only: a partly-zero range
            _set_exact(ipls, agg, 3, ipls.TGT_AGG, pre[3])
            _set_exact(ipls, agg, 3, ipls.TGT_REP, rep[3])
            out = _DevOut(ipls, P * (L - 1), avg, 2)
            agg.aggregate_round(0, tab, out=out.buf)
            agg.sync()
            li = agg.last_launch()
            assert li["kernel"] == _round_kernel(ipls, src) and li["start"] == ipls.START_ACCUM, li
            _exact_out(out.bits(), _narrow_out(q64, avg), avg, f"start/REP {src}->{avg} secure={secure}")
            _check_w(agg, ipls, ws, f"start/REP {src}->{avg}")
            _check_consumed(agg, ipls, P, f"start/REP {src}->{avg}")


# --------------------------------------------------------------------------
# 5. edge values
# --------------------------------------------------------------------------
_QNAN = np.float64(np.float32(np.nan))
# (quotient, the bits it must give without secure mode, or None: the reference narrowing decides)
_QUOT = {
    "f32": [(3.4028235677973366e38, 0x7F800000), (3.4028235677973362e38, 0x7F7FFFFF), (-1e39, 0xFF800000),   # overflow
            (2.0**-149, 0x00000001), (2.0**-150, 0x00000000), (1.5 * 2.0**-149, 0x00000002), (2.0**-127, 0x00400000),
            (1 + 2.0**-24, 0x3F800000), (1 + 3 * 2.0**-24, 0x3F800002),                     # ties to even
            (-0.0, 0x80000000), (np.inf, 0x7F800000), (-np.inf, 0xFF800000), (_QNAN, None)],
    "half": [(1 + 2.0**-11 + 2.0**-30, 0x3C00),         # two roundings; a single one would give 0x3c01
             (1 + 2.0**-11, 0x3C00), (1 + 3 * 2.0**-11, 0x3C02), (1 + 2.0**-11 + 2.0**-20, 0x3C01),
             (65520.0, 0x7C00), (65519.99, 0x7BFF), (-1e39, 0xFC00), (1e6, 0x7C00),          # overflow
             (2.0**-24, 0x0001), (2.0**-25, 0x0000), (1.5 * 2.0**-24, 0x0002), (2.0**-15, 0x0200),   # subnormal results
             (-0.0, 0x8000), (np.inf, 0x7C00), (-np.inf, 0xFC00), (_QNAN, None)],
    "bf16": [(1 + 2.0**-8 + 2.0**-30, 0x3F80),          # two roundings; a single one would give 0x3f81
             (1 + 2.0**-8, 0x3F80), (1 + 3 * 2.0**-8, 0x3F82), (1 + 2.0**-8 + 2.0**-20, 0x3F81),
             (3.3961775e38, None), (1e39, 0x7F80), (-1e39, 0xFF80), (3.3895314e38, 0x7F7F),  # overflow
             (2.0**-133, 0x0001), (2.0**-134, 0x0000), (1.5 * 2.0**-133, 0x0002), (2.0**-127, 0x0040),
             (-0.0, 0x8000), (np.inf, 0x7F80), (-np.inf, 0xFF80), (_QNAN, None)],
}
# source patterns: +-0, smallest / largest subnormal, smallest normal, largest finite, +-inf, a quiet NaN, 1.0,
# a cancelling pair, negative subnormal / largest finite
_SRC_EDGE = {
    "f32": np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0x3F800000, 0x3EAAAAAB, 0xBEAAAAAB, 0x80000001, 0xFF7FFFFF], dtype=np.uint32),
    "half": R.edge_bits("half"),
    "bf16": R.edge_bits("bf16"),
}


@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("avg", FMTS)
@pytest.mark.parametrize("src", FMTS)
def test_edge_values(ipls, O, src, avg, secure):
    """Count k = 2 (a power of two), the buckets +0.0 where REP = 2 q: W = 2 q and
    the quotient is q exactly without secure mode, in every position class and
    at m = 0..3.  Source edge values sit in the buckets right after them."""
    L, P, k = _classes_len(ipls, src), 4, 2
    T, b = _tile(ipls, src)
    lengths = [L] * P
    rng = np.random.default_rng(61)
    x = _buckets(rng, P, k, lengths, src)
    qs = _QUOT[avg]
    nq, edge = len(qs), _SRC_EDGE[src]
    starts = [0, T - nq - len(edge) - 1, T, T + 4 * b]   # full tile (both ends), vector steps, scalar remainder
    rep = [rng.standard_normal(L) for _ in range(P)]
    rep[1] = None                                        # REP logically zero on one partition
    for q in range(P):
        for s in starts[:3] if q != 1 else ():
            x[q, :, s:s + nq] = 0
            # W = +0.0 + REP is never -0.0: the -0.0 quotient comes from -2^-1074 / 2, a tie that rounds to -0.0
            rep[q][s:s + nq] = [-5e-324 if (v == 0.0 and np.signbit(v)) else 2.0 * v for v, _ in qs]
        for j, s in enumerate(starts):
            s2 = s + nq if s != T + 4 * b else s         # the remainder is 5 elements: source edges only
            n = min(len(edge), L - 1 - s2)
            x[q, j % k, s2:s2 + n] = edge[:n]
            x[q, (j + 1) % k, s2:s2 + n] = np.roll(edge, q + 1)[:n]   # edge meets edge: inf - inf, sub + sub
        if rep[q] is not None:
            rep[q][L - 1] = 0.0
    ws = _oracle_ws(O, x, src, lengths, k, rep=rep)
    assert all(w[-1] == 2.0 for w in ws)
    want = _want(O, ws, secure, avg)
    if not secure:
        for q in (0, 2, 3):
            for s in starts[:3]:
                for i, (v, bits) in enumerate(qs):
                    if bits is not None:
                        assert want[q * (L - 1) + s + i] == bits, (v, hex(want[q * (L - 1) + s + i]), hex(bits))
    keep, tab = _table(ipls, x, src)
    with ipls.Aggregator(n_partitions=P, bucket_len=L, secure=secure) as agg:
        for q in range(P):
            if rep[q] is not None:
                agg.Update(rep[q], q, from_clients=False)
        out = _DevOut(ipls, P * (L - 1), avg, 0)
        agg.aggregate_round(0, tab, out=out.buf)
        agg.sync()
        assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
        _exact_out(out.bits(), want, avg, f"edge values {src}->{avg} secure={secure}")
        _check_w(agg, ipls, ws, f"edge values {src}->{avg}")


# --------------------------------------------------------------------------
# 6. order
# --------------------------------------------------------------------------
@pytest.mark.parametrize("src", FMTS)
def test_order(ipls, O, src):
    """1e16, 1.0, -1e16 per element (the nearest values of the format): in f64 the
    given order gives (1e16 + 1) - 1e16 = 0, the order 1e16, -1e16, 1 gives 1.
    (Halves have no such finite witness: 1e16 narrows to inf and the sum is a
    NaN in every order; sums of three finite halves are exact in f64.)"""
    L, P, k = _classes_len(ipls, src), 2, 3
    lengths = [L] * P
    x = np.empty((P, k, L), dtype=_NPBITS[src])
    for j, v in enumerate((1e16, 1.0, -1e16)):
        x[:, j, :] = _to_fmt(np.array([v]), src)[0]
    x[:, :, L - 1] = _to_fmt(np.ones(1), src)[0]
    ws = _oracle_ws(O, x, src, lengths, k)
    if src != "half":
        other = _oracle_ws(O, x[:, [0, 2, 1], :], src, lengths, k)
        assert ws[0][0] == 0.0 and other[0][0] == 1.0
    keep, tab = _table(ipls, x, src)
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        got = agg.aggregate_round(0, tab, dtype=_NPDT[src])
        assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
        _exact_out(got, _want(O, ws, False, src), src, f"order {src}")
        _check_w(agg, ipls, ws, f"order {src}")
        # a queued arrival folds before the round's buckets: 1e16 queued, then 1.0, -1e16
        for q in range(P):
            agg.UpdateAsync(tab[q][0], q)
        got = agg.aggregate_round(0, [row[1:] for row in tab], dtype=_NPDT[src])
        assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
        _exact_out(got, _want(O, ws, False, src), src, f"queued first {src}")
        _check_w(agg, ipls, ws, f"queued first {src}")


# --------------------------------------------------------------------------
# 7. two shards
# --------------------------------------------------------------------------
@pytest.mark.parametrize("src", FMTS)
def test_two_shards(ipls, O, src):
    L, P, k = _classes_len(ipls, src), 4, 3
    lengths = [L] * P
    rng = np.random.default_rng(71)
    x = _buckets(rng, P, k, lengths, src)
    rep = [None, rng.standard_normal(L), rng.standard_normal(L), None]
    for r in rep:
        if r is not None:
            r[L - 1] = 0.0
    ws = _oracle_ws(O, x, src, lengths, k, rep=rep)
    keep, tab = _table(ipls, x, src)
    with ipls.Aggregator(n_partitions=P, bucket_len=L, devices=[0, 0]) as agg:
        assert len({agg.partition_device(p)[1] for p in range(P)}) == 2   # the range below spans both shards
        for q in range(P):
            if rep[q] is not None:
                agg.Update(rep[q], q, from_clients=False)
        for avg in FMTS:
            # partitions 1..3: the averages at their flat offsets from partition 1's
            out = _DevOut(ipls, 3 * (L - 1), avg, 1)
            agg.aggregate_round(1, tab[1:], out=out.buf)
            agg.sync()
            assert agg.last_launch()["kernel"] == _round_kernel(ipls, src)
            w = ws[1:] if avg == FMTS[0] else _oracle_ws(O, x, src, lengths, k)[1:]   # REP is consumed by the first
            _exact_out(out.bits(), _want(O, w, False, avg), avg, f"two shards {src}->{avg}")
            for q in range(1, P):
                assert_bits_equal(agg.read(q, ipls.TGT_WEIGHTS), w[q - 1], f"two shards W p={q}")
