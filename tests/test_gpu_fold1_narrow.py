"""k_fold1_narrow through agg.Update: one f32 / f16 / bf16 arrival folded into
one partition with the pointers as kernel arguments (launch-record codes 9 and
10).  Every comparison is bit for bit against the oracle fed the widened
values (conftest.assert_bits_equal: NaN meets NaN, everything else the bits).

Shapes come from the launch record: b = block, v = vectors, G = 4 b v is one
block's trip.  Lengths: 1..9 (remainder only, one group, a group and a
remainder), 4b-1, 4b, 4b+1 (one vector step of every lane), G-1, G, G+1 (the
first whole trip: the whole-line stores), G+4b+1, 2G+3 (two blocks), and one
length past grid x G so that a block makes a second trip.
"""
import numpy as np
import pytest

from conftest import assert_bits_equal
import narrow_fmt as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMTS = F.FMTS
LNAMES = ("1", "2", "3", "4", "5", "7", "8", "9", "4b-1", "4b", "4b+1", "G-1", "G", "G+1", "G+4b+1", "2G+3")


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


_SHAPE = {}


def _shape(ipls, fmt):
    """(b, G) of k_fold1_narrow for the format, read from one launch's record."""
    if fmt not in _SHAPE:
        bits = np.full(9, F.ONE[fmt], dtype=F.bits_dtype(fmt))
        keep, d = F.dev(ipls, torch, bits, fmt)
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as agg:
            agg.Update(d, 0)
            li = agg.last_launch()
        assert li["kernel"] == F.fold_kernel(ipls, fmt), li
        assert li["block"] > 0 and li["vectors"] > 0 and li["grid"] >= 1, li
        _SHAPE[fmt] = (li["block"], 4 * li["block"] * li["vectors"])
        assert _SHAPE[fmt][1] <= 1 << 16, "a trip this long makes the length sweep slow"
    return _SHAPE[fmt]


def _length(ipls, fmt, name):
    b, G = _shape(ipls, fmt)
    expr = name.replace("4b", "4*b").replace("2G", "2*G")
    return int(eval(expr, {"b": b, "G": G}))   # noqa: S307 -- the names of LNAMES only


def _plant(b, G, L):
    return (0, 3, 4, 4 * b - 1, 4 * b, G - 1, G, L - 2)


def _targets(ipls):
    return (("AGG", ipls.TGT_AGG, dict(from_clients=True)), ("REP", ipls.TGT_REP, dict(from_clients=False)),
            ("FUTURE", ipls.TGT_FUTURE, dict(from_future=True)))


def _check_length(ipls, O, fmt, L, rng, *, expect_trips=False):
    b, G = _shape(ipls, fmt)
    x1, x2 = F.bucket(rng, L, fmt, _plant(b, G, L)), F.bucket(rng, L, fmt, _plant(b, G, L)[::-1])
    w1, w2 = F.widen(x1, fmt), F.widen(x2, fmt)
    nz = np.full(L, F.NEG_ZERO[fmt], dtype=F.bits_dtype(fmt))
    nz[L - 1] = F.ONE[fmt]
    base = rng.standard_normal(L)
    k1, d1 = F.dev(ipls, torch, x1, fmt)
    k2, d2 = F.dev(ipls, torch, x2, fmt)
    kz, dz = F.dev(ipls, torch, nz, fmt)
    code = F.fold_kernel(ipls, fmt)
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        def rec(start):
            li = agg.last_launch()
            assert li["kernel"] == code and li["seqf"] == 1 and li["start"] == start, (L, li)
            return li
        # ZERO: -0.0 everywhere gives +0.0 (+0.0 + -0.0), the count slot 1.0
        agg.Update(dz, 0)
        li = rec(ipls.START_ZERO)
        if expect_trips:
            assert li["grid"] * G < L, f"grid {li['grid']} x trip {G} covers L = {L}: no second trip"
        want = np.zeros(L)
        want[L - 1] = 1.0
        assert_bits_equal(agg.read(0), want, f"{fmt} L={L} -0.0 into a fresh accumulator")
        # every target: ZERO into the fresh one, then ACCUM on top
        for name, tgt, kw in _targets(ipls):
            agg.reset()
            agg.Update(d1, 0, **kw)
            rec(ipls.START_ZERO)
            assert_bits_equal(agg.read(0, tgt), O.reduce([w1], L, O.START_ZERO), f"{fmt} L={L} {name} ZERO")
            agg.Update(d2, 0, **kw)
            rec(ipls.START_ACCUM)
            assert_bits_equal(agg.read(0, tgt), O.reduce([w1, w2], L, O.START_ZERO), f"{fmt} L={L} {name} ACCUM")
        # ACCUM onto a non-zero accumulator of doubles
        agg.reset()
        agg.Update(base, 0)
        agg.Update(d1, 0)
        rec(ipls.START_ACCUM)
        assert_bits_equal(agg.read(0), O.reduce([w1], L, O.START_ACCUM, 0.0 + base), f"{fmt} L={L} ACCUM on doubles")
    del k1, k2, kz


@pytest.mark.parametrize("fmt", FMTS)
def test_record(ipls, fmt):
    """Update(DeviceBuffer) and Update(host array) both take k_fold1_narrow."""
    b, G = _shape(ipls, fmt)
    L = G + 5
    rng = np.random.default_rng(3)
    x = F.bucket(rng, L, fmt)
    keep, d = F.dev(ipls, torch, x, fmt)
    with ipls.Aggregator(n_partitions=2, bucket_len=L) as agg:
        for p, op in ((0, d), (1, F.host(torch, x, fmt))):
            agg.Update(op, p)
            li = agg.last_launch()
            assert li["kernel"] == F.fold_kernel(ipls, fmt) and li["seqf"] == 1, (p, li)
            assert li["block"] == b and 4 * li["block"] * li["vectors"] == G and li["grid"] == 2, (p, li)
            assert li["be_in"] == 0 and li["be_out"] == 0 and li["start"] == ipls.START_ZERO
    assert ipls.KERNEL_FOLD1_F32 == 9 and ipls.KERNEL_FOLD1_H16 == 10


@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_lengths(ipls, O, fmt, lname):
    L = _length(ipls, fmt, lname)
    _check_length(ipls, O, fmt, L, np.random.default_rng(100 + L))


@pytest.mark.parametrize("fmt", FMTS)
def test_second_trip(ipls, O, fmt):
    """A length past grid x G (read from the launch's own record): blocks make
    a second trip of the grid-stride loop."""
    b, G = _shape(ipls, fmt)
    for L in ((1 << 23) + 5, (1 << 24) + 5, 1 << 25):
        # the grid of a launch depends on L alone: ask with a short-lived handle and a zeroed bucket
        t = torch.zeros(L * F.esize(fmt) + 64, dtype=torch.uint8, device="cuda")
        with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
            agg.Update(ipls.DeviceBuffer(t.data_ptr(), L, dtype=fmt), 0)
            li = agg.last_launch()
        del t
        if li["grid"] * G < L:
            break
    else:
        pytest.fail(f"no second trip up to 2^25 elements: grid {li['grid']} x {G}")
    _check_length(ipls, O, fmt, L, np.random.default_rng(7), expect_trips=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_source_offsets(ipls, O, fmt):
    """Sources at every element offset within 16 B: the load-aligned ones (16 B
    of floats, 8 B of 16-bit elements) take k_fold1_narrow, the others keep
    k_reduce_narrow's element-by-element form; the oracle's bits either way."""
    b, G = _shape(ipls, fmt)
    s = F.esize(fmt)
    for L in (9, G + 4 * b + 1):
        rng = np.random.default_rng(50 + L)
        x1, x2 = F.bucket(rng, L, fmt, _plant(b, G, L)), F.bucket(rng, L, fmt, _plant(b, G, L))
        w = [F.widen(x1, fmt), F.widen(x2, fmt)]
        want = O.reduce(w, L, O.START_ZERO)
        with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
            for off in range(16 // s):
                k1, d1 = F.dev(ipls, torch, x1, fmt, off)
                k2, d2 = F.dev(ipls, torch, x2, fmt, off)
                assert d1.ptr % 16 == off * s
                agg.reset()
                for d in (d1, d2):     # ZERO, then ACCUM
                    agg.Update(d, 0)
                    li = agg.last_launch()
                    if (off * s) % (4 * s) == 0:
                        assert li["kernel"] == F.fold_kernel(ipls, fmt) and li["seqf"] == 1, (off, li)
                    else:
                        assert li["kernel"] == F.reduce_kernel(ipls, fmt) and li["seqf"] == 0, (off, li)
                assert_bits_equal(agg.read(0), want, f"{fmt} L={L} offset {off}")


@pytest.mark.parametrize("fmt", FMTS)
def test_neighbours_untouched(ipls, O, fmt):
    """The fold into the middle partition's AGG leaves the neighbouring
    partitions' AGG and its own REP and Weights bit-identical: a whole-line
    exchange that wrote past L would show here."""
    b, G = _shape(ipls, fmt)
    for L in (5, 4 * b + 1, G - 1, G + 1, G + 4 * b + 1):
        rng = np.random.default_rng(9 + L)
        x1, x2 = F.bucket(rng, L, fmt), F.bucket(rng, L, fmt)
        k1, d1 = F.dev(ipls, torch, x1, fmt)
        k2, d2 = F.dev(ipls, torch, x2, fmt)
        with ipls.Aggregator(n_partitions=3, bucket_len=L) as agg:
            for p in (0, 2):
                agg.Update(rng.standard_normal(L), p)
            agg.Update(rng.standard_normal(L), 1, from_clients=False)
            agg.cache_partition(1, rng.standard_normal(L))
            watch = [(0, ipls.TGT_AGG), (2, ipls.TGT_AGG), (1, ipls.TGT_REP), (1, ipls.TGT_WEIGHTS)]
            before = [agg.read(p, t).view(np.uint64).copy() for p, t in watch]
            agg.Update(d1, 1)
            agg.Update(d2, 1)
            assert agg.last_launch()["kernel"] == F.fold_kernel(ipls, fmt)
            assert_bits_equal(agg.read(1), O.reduce([F.widen(x1, fmt), F.widen(x2, fmt)], L, O.START_ZERO),
                              f"{fmt} L={L} middle partition")
            for (p, t), was in zip(watch, before):
                assert np.array_equal(agg.read(p, t).view(np.uint64), was), f"{fmt} L={L}: partition {p} target {t} changed"


def test_order_f32_f64_f32(ipls, O):
    """1e16f, 1.0, -1e16f through f32 / f64 / f32 Updates into one partition:
    the call order decides the bits, so a per-arrival fold that overtook or
    waited for a fold of another format would show."""
    b, G = _shape(ipls, "f32")
    for L in (7, G + 1):
        b1 = np.full(L, 1e16, dtype=np.float32)
        b2 = np.full(L, 1.0)
        b3 = np.full(L, -1e16, dtype=np.float32)
        w = [b1.astype(np.float64), b2, b3.astype(np.float64)]
        want = O.reduce(w, L, O.START_ZERO)
        u = lambda a: np.ascontiguousarray(a).view(np.uint64)   # noqa: E731
        # 1.0 is absorbed by 1e16f and survives only when it arrives after the
        # two large values have cancelled: those orders give other bits
        assert not np.array_equal(u(want), u(O.reduce([w[0], w[2], w[1]], L, O.START_ZERO)))
        assert not np.array_equal(u(want), u(O.reduce([w[2], w[0], w[1]], L, O.START_ZERO)))
        k1, d1 = F.dev(ipls, torch, b1.view(np.uint32), "f32")
        k3, d3 = F.dev(ipls, torch, b3.view(np.uint32), "f32")
        t2 = torch.from_numpy(b2).cuda()
        d2 = ipls.DeviceBuffer.from_tensor(t2)
        with ipls.Aggregator(n_partitions=2, bucket_len=L) as agg:
            kernels = []
            for d in (d1, d2, d3):
                agg.Update(d, 0)
                kernels.append(agg.last_launch()["kernel"])
            assert kernels == [ipls.KERNEL_FOLD1_F32, ipls.KERNEL_FOLD1, ipls.KERNEL_FOLD1_F32]
            assert_bits_equal(agg.read(0), want, f"L={L} device operands")
            for h in (b1, b2, b3):
                agg.Update(h, 1)
            assert_bits_equal(agg.read(1), want, f"L={L} host operands")
