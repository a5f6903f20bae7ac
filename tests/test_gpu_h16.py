"""The half-precision trainer boundary on the GPU: IPLS_DEV_F16 / IPLS_HOST_F16 /
IPLS_DEV_BF16 / IPLS_HOST_BF16 sources and outputs, each test for both formats.

Sources are bit-exact against the oracle fed the widened values (h16_ref.widen:
f16 -> f32 -> f64, or bits << 16 as an f32 -> f64; both exact).  Outputs are
bit-exact against the oracle's f64 quotient narrowed in two steps
(``.astype(np.float32)``, then h16_ref.narrow, which test_h16_boundary.py checks
against torch's CPU casts), and against the F32 output of the same handle
narrowed on the CPU.  Only sums a NaN reaches get conftest.assert_bits_equal's
NaN allowance; the only NaN fed in is a quiet one.

Shapes: T = block x 4 x vectors (the sweep chose the layout with 4 elements per
lane per vector) and block are read from ipls_agg_last_launch after one launch.
Fold lengths {1, 9, 8 block + 3, T - 1, T, T + 1, 2T + 8 block + 13} (< 100k
elements for any tile up to 32,768), k in {1, 2, 3, 9} (9 = one full group of 8
peers in flight plus one).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal

import h16_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 9)
LNAMES = ("1", "9", "8b+3", "T-1", "T", "T+1", "2T+8b+13")
INVAL = -1
FMTS = R.FORMATS


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


def _tdt(fmt):
    return torch.float16 if fmt == "half" else torch.bfloat16


def _dev_kind(ipls, fmt):
    return ipls.DEV_F16 if fmt == "half" else ipls.DEV_BF16


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _exact(a, b, what):
    assert np.array_equal(_u64(a), _u64(b)), what


def _exact16(got, want, fmt, what):
    """16-bit patterns: NaN must meet NaN, everything else the same bits."""
    got = np.ascontiguousarray(got).view(np.uint16)
    want = np.ascontiguousarray(want).view(np.uint16)
    assert got.shape == want.shape, what
    gn, wn = R.is_nan(got, fmt), R.is_nan(want, fmt)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"


def _dev_rows(bits, fmt, offs=0):
    """The rows of a 2-D uint16 array as device tensors of the format's torch
    dtype; row j's base is 16-B aligned plus offs (or offs[j]) elements."""
    n, L = bits.shape
    offs = [offs] * n if isinstance(offs, int) else list(offs)
    stride = (L + max(offs) + 7) // 8 * 8
    t = torch.zeros((n, stride), dtype=torch.int16, device="cuda")
    src = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()
    for j in range(n):
        t[j, offs[j]:offs[j] + L] = src[j]
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, [t[j, offs[j]:offs[j] + L].view(_tdt(fmt)) for j in range(n)]


def _db(ipls, rows):
    return [ipls.DeviceBuffer.from_tensor(r) for r in rows]


def _host_op(bits, fmt):
    """A host operand the HOST_F16 / HOST_BF16 way: numpy float16, or a CPU
    torch.bfloat16 tensor (numpy has no bfloat16)."""
    if fmt == "half":
        return np.ascontiguousarray(bits).view(np.float16)
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


_TILE = {}


def _tile(ipls):
    """(T, block) of k_reduce_narrow over 16-bit buckets, read from the launch record."""
    if not _TILE:
        bits = np.full((1, 9), R.one("half"), dtype=np.uint16)
        keep, rows = _dev_rows(bits, "half")
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as agg:
            agg.reduce_batch(0, [_db(ipls, rows)])
            li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_H16
        _TILE["T"], _TILE["block"] = li["block"] * 4 * li["vectors"], li["block"]
        assert _TILE["T"] <= 32768
    return _TILE["T"], _TILE["block"]


def _length(ipls, name):
    T, b = _tile(ipls)
    return {"1": 1, "9": 9, "8b+3": 8 * b + 3, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+8b+13": 2 * T + 8 * b + 13}[name]


def _classes(ipls, L):
    """Position classes of a fold of L elements (count slot excluded): the
    full tiles, the partial tile's vector steps, the scalar remainder."""
    T, b = _tile(ipls)
    full = L // T * T
    vec = full + (L - full) // (4 * b) * (4 * b)      # a vector step is 4 elements per lane
    return [(lo, hi) for lo, hi in ((0, full), (full, vec), (vec, L - 1)) if hi > lo]


def _buckets(ipls, rng, n, L, fmt):
    """n buckets of L patterns: narrowed normals, the edge values planted in
    every position class, a cancelling pair at each class's first position in
    buckets 0 and 1, 1.0 in the count slot."""
    x = R.narrow(rng.standard_normal((n, L)).astype(np.float32), fmt).reshape(n, L).copy()
    edge = R.edge_bits(fmt)
    for lo, hi in _classes(ipls, L):
        for j in range(n):
            pos = rng.integers(lo, hi, size=edge.size)
            x[j, pos] = edge
        x[0, lo] = edge[10]
        if n > 1:
            x[1, lo] = edge[11]
    x[:, L - 1] = R.one(fmt)
    return x


def _widen(x, fmt):
    with np.errstate(invalid="ignore"):
        return [R.widen(r, fmt) for r in x]


# --------------------------------------------------------------------------
# from_tensor; the tile constant and the two paths
# --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_from_tensor_16bit(ipls, fmt):
    b = ipls.DeviceBuffer.from_tensor(torch.ones(24, dtype=_tdt(fmt), device="cuda"))
    assert b.n == 24 and b.dtype == fmt and b.kind == _dev_kind(ipls, fmt)
    with pytest.raises(ValueError):
        ipls.DeviceBuffer.from_tensor(torch.ones(24, dtype=_tdt(fmt), device="cuda"), big_endian=True)
    c = ipls.DeviceBuffer.from_tensor(torch.zeros(8, dtype=torch.float64, device="cuda"))
    assert c.n == 8 and c.kind == ipls.DEV_F64


@pytest.mark.parametrize("fmt", FMTS)
def test_tile_and_paths(ipls, O, fmt):
    T, block = _tile(ipls)
    rng = np.random.default_rng(1)
    L = T + 1
    x = _buckets(ipls, rng, 3, L, fmt)
    want = O.reduce(_widen(x, fmt), L)
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        keep, rows = _dev_rows(x, fmt)
        agg.reduce_batch(0, [_db(ipls, rows)])
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["block"] == block
        assert li["seqf"] == 1 and li["grid"] == 2       # all aligned: vector path, one full and one partial tile
        assert_bits_equal(agg.read(0), want, "aligned")
        # one bucket 1 element (2 B) off, one 4 elements (8 B) off, one aligned, in the same table
        keep2, rows2 = _dev_rows(x, fmt, offs=[1, 4, 0])
        bufs = _db(ipls, rows2)
        assert [b.ptr % 16 for b in bufs] == [2, 8, 0]
        agg.reduce_batch(0, [bufs])
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["seqf"] == 0   # element by element
        assert_bits_equal(agg.read(0), want, "mixed alignment")


# --------------------------------------------------------------------------
# the batched fold: every length, k, start mode and destination byte order
# --------------------------------------------------------------------------
@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_batch_h16(ipls, O, fmt, lname):
    L = _length(ipls, lname)
    rng = np.random.default_rng(1000 + 7 * L + len(fmt))
    kmax = max(KS)
    x = _buckets(ipls, rng, kmax, L, fmt)
    wide = _widen(x, fmt)
    keep, rows = _dev_rows(x, fmt)
    bufs = _db(ipls, rows)
    acc0 = rng.standard_normal(L)
    Lp = (L + 1) // 2 * 2
    d = torch.zeros(Lp, dtype=torch.int64, device="cuda")
    modes = ((ipls.START_ZERO, O.START_ZERO), (ipls.START_FIRST, O.START_FIRST), (ipls.START_ACCUM, O.START_ACCUM))
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        for k in KS:
            tab = [bufs[:k]]
            for be in (False, True):
                for mode, omode in modes:
                    what = f"{fmt} L={L} k={k} be={be} mode={mode}"
                    init = acc0.astype(">f8") if be else acc0
                    d[:L] = torch.from_numpy(init.view(np.int64).copy()).cuda()
                    torch.cuda.synchronize()
                    agg.reduce_batch_out(0, tab, [ipls.DeviceBuffer(d.data_ptr(), L, be)], start_mode=mode,
                                         big_endian_out=be)
                    li = agg.last_launch()
                    assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["seqf"] == 1, what
                    agg.sync()
                    h = d.cpu().numpy()[:L]
                    got = h.view(">f8").astype(np.float64) if be else h.view(np.float64)
                    assert_bits_equal(got, O.reduce(wide[:k], L, omode, acc0), what)
            # into the handle's own accumulator: ACCUM onto a non-zero AGG
            agg.reset()
            agg.Update(acc0, 0)
            agg.reduce_batch(0, tab, start_mode=ipls.START_ACCUM)
            assert_bits_equal(agg.read(0), O.reduce(wide[:k], L, O.START_ACCUM, 0.0 + acc0), f"{fmt} L={L} k={k} AGG")


@pytest.mark.parametrize("k", (1, 9))
@pytest.mark.parametrize("lname", ("7", "T+1", "2T+3", "T+4b+1"))
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_batch_out_accum_big_endian(ipls, O, fmt, lname, k):
    """ACCUM onto big-endian caller destinations that hold random doubles: three
    partitions in one launch, bit-exact against the oracle's ACCUM fold.  T + 4b + 1
    (b lanes) gives the partial tile one vector step of 4 elements per lane."""
    T, b = _tile(ipls)
    L, P = {"7": 7, "T+1": T + 1, "2T+3": 2 * T + 3, "T+4b+1": T + 4 * b + 1}[lname], 3
    rng = np.random.default_rng(900 + 10 * L + k + len(fmt))
    xs = [_buckets(ipls, rng, k, L, fmt) for _ in range(P)]
    keeps, tab = [], []
    for x in xs:
        keep, rows = _dev_rows(x, fmt)
        keeps.append(keep)
        tab.append(_db(ipls, rows))
    prior = rng.standard_normal((P, L))
    Lp = (L + 1) // 2 * 2
    d = torch.zeros((P, Lp), dtype=torch.int64, device="cuda")
    d[:, :L] = torch.from_numpy(prior.astype(">f8").view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        agg.reduce_batch_out(0, tab, [ipls.DeviceBuffer(d[q].data_ptr(), L, True) for q in range(P)],
                             start_mode=ipls.START_ACCUM, big_endian_out=True)
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["seqf"] == 1
        agg.sync()
    got = d.cpu().numpy().view(">f8").astype(np.float64)
    for q in range(P):
        assert_bits_equal(got[q, :L], O.reduce(_widen(xs[q], fmt), L, O.START_ACCUM, prior[q]),
                          f"{fmt} L={L} k={k} p={q}")


@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_batch_three_partitions(ipls, O, fmt):
    """One launch over partitions of lengths T + 1, T + 1, T - 1: partial tiles
    are scheduled first, and the last partition has no full tile at all."""
    T, _ = _tile(ipls)
    M, P, k = 3 * T - 2, 3, 3
    rng = np.random.default_rng(31)
    with ipls.Aggregator(M, P) as agg:
        assert list(agg.lengths) == [T + 1, T + 1, T - 1]
        xs = [_buckets(ipls, rng, k, L, fmt) for L in agg.lengths]
        keeps, tab = [], []
        for x in xs:
            keep, rows = _dev_rows(x, fmt)
            keeps.append(keep)
            tab.append(_db(ipls, rows))
        for mode in (ipls.START_ZERO, ipls.START_FIRST):
            agg.reduce_batch(0, tab, start_mode=mode)
            li = agg.last_launch()
            assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["seqf"] == 1 and li["grid"] == 6
            for q, L in enumerate(agg.lengths):
                assert_bits_equal(agg.read(q), O.reduce(_widen(xs[q], fmt), L, mode), f"{fmt} mode={mode} p={q}")


# --------------------------------------------------------------------------
# Update / UpdateAsync per arrival; call order across formats
# --------------------------------------------------------------------------
@pytest.mark.parametrize("lname", ("9", "T+1"))
@pytest.mark.parametrize("fmt", FMTS)
def test_update_per_arrival(ipls, O, fmt, lname):
    L = _length(ipls, lname)
    rng = np.random.default_rng(5 + L)
    x = _buckets(ipls, rng, 3, L, fmt)
    want = O.reduce(_widen(x, fmt), L, O.START_ZERO)
    keep, rows = _dev_rows(x, fmt)
    keep1, rows1 = _dev_rows(x, fmt, offs=1)
    with ipls.Aggregator(n_partitions=4, bucket_len=L) as agg:
        for d in _db(ipls, rows):
            agg.Update(d, 0)
        assert_bits_equal(agg.read(0), want, "Update device")
        for d in _db(ipls, rows1):
            agg.Update(d, 1)
        assert_bits_equal(agg.read(1), want, "Update device, 2 B off")
        for j in range(3):
            agg.Update(_host_op(x[j], fmt), 2)
        assert_bits_equal(agg.read(2), want, "Update host")
        agg.set_coalesce(32)
        t = 0
        for d in _db(ipls, rows):
            t = agg.UpdateAsync(d, 3)
        agg.Wait(t)
        assert_bits_equal(agg.read(3), want, "UpdateAsync")
        with pytest.raises(ipls.IplsError) as e:     # a short bucket is refused, in elements
            agg.Update(ipls.DeviceBuffer(rows[0].data_ptr(), L - 1, dtype=fmt), 0)
        assert e.value.code == -2
        assert_bits_equal(agg.read(0), want, "after the refusal")


@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_format_queue_order(ipls, fmt):
    """1e16 (F64), 1.0 (16-bit), -1e16 (F64) into one partition give 0.0; with
    the 16-bit bucket last they give 1.0: a change of format must not reorder."""
    L = 9
    big = torch.full((L + 1,), 1e16, dtype=torch.float64, device="cuda")
    neg = torch.full((L + 1,), -1e16, dtype=torch.float64, device="cuda")
    keep, (one,) = _dev_rows(np.full((1, L), R.one(fmt), dtype=np.uint16), fmt)
    torch.cuda.synchronize()
    D = ipls.DeviceBuffer
    b, n, o = D(big.data_ptr(), L), D(neg.data_ptr(), L), D.from_tensor(one)
    with ipls.Aggregator(n_partitions=4, bucket_len=L) as agg:
        agg.set_coalesce(32)
        for p, order, want in ((0, (b, o, n), 0.0), (1, (b, n, o), 1.0)):
            t = 0
            for d in order:
                t = agg.UpdateAsync(d, p)
            agg.Wait(t)
            _exact(agg.read(p), np.full(L, want), f"UpdateAsync order {p}")
            for d in order:
                agg.Update(d, p + 2)
            _exact(agg.read(p + 2), np.full(L, want), f"Update order {p}")


# --------------------------------------------------------------------------
# UpdateGradient / OrganizeGradients / InitializeWeights: ETHModel's geometry
# --------------------------------------------------------------------------
def _flat_operands(ipls, bits, fmt):
    M = bits.size
    out = []
    for off in (0, 1):
        t = torch.zeros(M + 8, dtype=torch.int16, device="cuda")
        t[off:off + M] = torch.from_numpy(bits.view(np.int16)).cuda()
        torch.cuda.synchronize()
        out.append((f"device+{off}", ipls.DeviceBuffer.from_tensor(t[off:off + M].view(_tdt(fmt))), t))
    out.append(("host", _host_op(bits, fmt), None))
    if fmt == "half":   # a CPU torch.float16 tensor goes up as HOST_F16 too
        out.append(("host torch", torch.from_numpy(bits.view(np.float16).copy()), None))
    return out


def _check_flat_paths(ipls, O, open_agg, bits, P, fmt):
    M = bits.size
    with np.errstate(invalid="ignore"):
        og = O.organize_gradients(R.widen(bits, fmt), M, P)
    for name, op, keep in _flat_operands(ipls, bits, fmt):
        with open_agg() as agg:
            assert agg.flat_size == M
            got = agg.OrganizeGradients(op)
            for p in range(P):
                assert_bits_equal(got[p], og[p], f"OrganizeGradients {fmt} {name} p={p}")
            if name == "device+1":
                gbe = agg.OrganizeGradients(op, big_endian_out=True)
                for p in range(P):
                    assert_bits_equal(np.frombuffer(gbe[p], dtype=">f8").astype(np.float64), og[p], f"BE {name} p={p}")
            for auth in ([1], list(range(P))):
                agg.reset()
                agg.UpdateGradient(op, auth)               # into a logically zero AGG: +0.0 + v
                agg.UpdateGradient(op, auth)               # then AGG + v
                for p in range(P):
                    want = (0.0 + og[p]) + og[p] if p in auth else np.zeros_like(og[p])
                    assert_bits_equal(agg.read(p), want, f"UpdateGradient {fmt} {name} auth={auth} p={p}")
            agg.InitializeWeights(op)
            for p in range(P):
                w = og[p].copy()
                w[-1] = 0.0
                assert_bits_equal(agg.read(p, ipls.TGT_WEIGHTS), w, f"InitializeWeights {fmt} {name} p={p}")


@pytest.mark.parametrize("fmt", FMTS)
def test_flat_vectors_ethmodel(ipls, O, ethmodel, fmt):
    """-pa 3 on the 443,610 values of ETHModel, narrowed to the format."""
    assert ethmodel.size == 443610
    with np.errstate(over="ignore"):
        bits = R.narrow(ethmodel.astype(np.float32), fmt)
    _check_flat_paths(ipls, O, lambda: ipls.Aggregator(ethmodel.size, 3), bits, 3, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_flat_vectors_every_residue(ipls, O, fmt):
    # chunk = 7 elements: the partitions' slices start at 0, 14, 12, 10, 8 mod 16 B
    rng = np.random.default_rng(12)
    bits = R.narrow(rng.standard_normal(32).astype(np.float32), fmt)
    bits[:14] = R.edge_bits(fmt)
    _check_flat_paths(ipls, O, lambda: ipls.Aggregator(32, 5), bits, 5, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_two_shards(ipls, O, fmt):
    """devices=[0, 0]: the element-size arithmetic of the shard fronts."""
    M, P = 30011, 3
    rng = np.random.default_rng(13)
    bits = R.narrow(rng.standard_normal(M).astype(np.float32), fmt)
    og = O.organize_gradients(R.widen(bits, fmt), M, P)
    keep, (row,) = _dev_rows(bits[None], fmt)
    with ipls.Aggregator(M, P, devices=[0, 0]) as agg:
        for op in (ipls.DeviceBuffer.from_tensor(row), _host_op(bits, fmt)):
            agg.reset()
            agg.UpdateGradient(op, [0, 1, 2])
            for p in range(P):
                assert_bits_equal(agg.read(p), 0.0 + og[p], f"two shards UpdateGradient p={p}")
            agg.InitializeWeights(op)
        # W = the model, counts 0: GetPartitions gives the values back narrowed, i.e. as they were
        for name, got in _get_16_all_ways(ipls, agg, fmt, offs=(0, 3)):
            _exact16(got, bits, fmt, f"two shards GetPartitions {name}")


# --------------------------------------------------------------------------
# the narrowing: GetPartitions and aggregate_round with 16-bit outputs
# --------------------------------------------------------------------------
def _quotients(fmt):
    """Doubles planted as quotients (count 1.0), with the bits they must give
    where those are worked out by hand (None: h16_ref.narrow decides)."""
    qnan = np.float64(np.float32(np.nan))
    if fmt == "half":
        return [(1 + 2.0**-11 + 2.0**-30, 0x3C00),        # two roundings; a single one would give 0x3c01
                (1 + 2.0**-11, 0x3C00), (1 + 3 * 2.0**-11, 0x3C02),       # exact ties: to even below, above
                (1 + 2.0**-11 + 2.0**-20, 0x3C01),
                (65520.0, 0x7C00), (65519.99, 0x7BFF), (-1e39, 0xFC00), (1e6, 0x7C00),   # overflow
                (2.0**-24, 0x0001), (2.0**-25, 0x0000), (1.5 * 2.0**-24, 0x0002), (2.0**-15, 0x0200),   # subnormal results
                (-0.0, 0x8000), (np.inf, 0x7C00), (qnan, None)]
    return [(1 + 2.0**-8 + 2.0**-30, 0x3F80),             # two roundings; a single one would give 0x3f81
            (1 + 2.0**-8, 0x3F80), (1 + 3 * 2.0**-8, 0x3F82),
            (1 + 2.0**-8 + 2.0**-20, 0x3F81),
            (3.3961775e38, None), (1e39, 0x7F80), (-1e39, 0xFF80), (3.3895314e38, 0x7F7F),
            (2.0**-133, 0x0001), (2.0**-134, 0x0000), (1.5 * 2.0**-133, 0x0002), (2.0**-127, 0x0040),
            (-0.0, 0x8000), (np.inf, 0x7F80), (qnan, None)]


def _get_16_all_ways(ipls, agg, fmt, offs=(0, 1, 3, 5)):
    """GetPartitions as 16-bit patterns: the host array and device outputs at
    some elements past a 128-B line."""
    n = agg.flat_size
    host = agg.GetPartitions(dtype=np.float16 if fmt == "half" else "bf16")
    assert host.dtype == (np.float16 if fmt == "half" else np.uint16)
    outs = [("host", host.view(np.uint16))]
    for off in offs:
        t = torch.full((n + 72,), 0x5555, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        r = agg.GetPartitions(out=ipls.DeviceBuffer.from_tensor(t[off:off + n].view(_tdt(fmt))))
        assert r.dtype == fmt
        agg.sync()
        h = t.cpu().numpy().view(np.uint16)
        assert np.all(h[:off] == 0x5555) and np.all(h[off + n:] == 0x5555), "wrote outside the output"
        outs.append((f"device+{off}", h[off:off + n].copy()))
    return outs


@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("fmt", FMTS)
def test_get_partitions_h16(ipls, O, fmt, secure):
    # chunk 4133: the partitions' outputs start at 0, 5, 2 mod 8 elements;
    # each has a head, two full tiles of the divide and a tail
    M, P = 3 * 4133 - 1, 3
    rng = np.random.default_rng(41)
    cnts = [1.0, 3.0, 0.0]                               # partition 2: count 0, W passes through
    qs = _quotients(fmt)
    with ipls.Aggregator(M, P, secure=secure) as agg:
        assert [o % 8 for o in agg.offsets] == [0, 5, 2]
        ws = []
        for p, L in enumerate(agg.lengths):
            w = rng.standard_normal(L)
            pos = rng.permutation(L - 1)[:len(qs)]
            w[pos] = [v * (1.0 if cnts[p] <= 1.0 else cnts[p]) for v, _ in qs]
            if p == 0:
                w[:len(qs)] = [v for v, _ in qs]         # also in the head / first lines
            w[-1] = cnts[p]
            ws.append(w)
            agg.cache_partition(p, w)
        with np.errstate(all="ignore"):
            want64 = O.get_partitions(ws, secure)
            want32 = want64.astype(np.float32)
            want = R.narrow(want32, fmt)
        if not secure:
            for i, (v, b) in enumerate(qs):              # the bits worked out by hand
                if b is not None:
                    assert want[i] == b, (v, hex(want[i]), hex(b))
        got32 = agg.GetPartitions(dtype=np.float32)
        assert np.array_equal(got32.view(np.uint32)[~np.isnan(want32)], want32.view(np.uint32)[~np.isnan(want32)])
        for name, got in _get_16_all_ways(ipls, agg, fmt):
            _exact16(got, want, fmt, f"{fmt} secure={secure} {name}")
            # the F32 output of the same handle, narrowed by the trainer
            _exact16(got, R.narrow(got32, fmt), fmt, f"{fmt} secure={secure} {name} vs narrowed f32 output")
        _exact(agg.GetPartitions()[~np.isnan(want64)], want64[~np.isnan(want64)], "the f64 output is unchanged")


@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("fmt", FMTS)
def test_aggregate_round_h16(ipls, O, fmt, secure):
    M, P, k = 3 * 4133 - 1, 3, 3
    rng = np.random.default_rng(51)
    qs = _quotients(fmt)
    with ipls.Aggregator(M, P, secure=secure) as r1, ipls.Aggregator(M, P, secure=secure) as r2:
        lengths, Lm = r1.lengths, max(r1.lengths)
        x = R.narrow(rng.standard_normal((P * k, Lm)).astype(np.float32), fmt).reshape(P, k, Lm).copy()
        for q, L in enumerate(lengths):
            x[q, :, L - 1] = R.one(fmt) if q < 2 else 0      # partition 2: count slots +0.0, a count-0 partition
        keep, rows = _dev_rows(x.reshape(P * k, Lm), fmt)
        bufs = _db(ipls, rows)
        tab = [[bufs[q * k + j] for j in range(k)] for q in range(P)]
        # REP carries the planted quotients times the count k, so that sum / k hits them
        rep = rng.standard_normal((P, Lm))
        for q, L in enumerate(lengths):
            rep[q, L - 1:] = 0.0
        ws = []
        for q, L in enumerate(lengths):
            agg = O.reduce(_widen(x[q], fmt), L, O.START_ZERO)
            if q == 1:
                rep[q, :len(qs)] = [v * k for v, _ in qs] - agg[:len(qs)]
            w, wa = np.zeros(L), np.zeros(L)
            with np.errstate(all="ignore"):
                O.aggregate_partition(agg, rep[q][:L].copy(), w, wa)
            ws.append(w)
        assert [w[-1] for w in ws] == [k, k, 0.0]        # the sums of partition 2 pass through undivided
        with np.errstate(all="ignore"):
            want32 = O.get_partitions(ws, secure).astype(np.float32)
            want = R.narrow(want32, fmt)
        for r in (r1, r2):
            for q in range(P):
                r.Update(rep[q, :lengths[q]], q, from_clients=False)
        got = r1.aggregate_round(0, tab, dtype=np.float16 if fmt == "half" else "bf16")
        _exact16(got, want, fmt, f"aggregate_round host {fmt} secure={secure}")
        # a second handle: 16-bit buckets, float averages, narrowed on the CPU
        got32 = r2.aggregate_round(0, tab, dtype=np.float32)
        _exact16(got, R.narrow(got32, fmt), fmt, "vs the F32 averages narrowed")
        # again into a device buffer 3 elements past a line (REP is zero now)
        t = torch.zeros(r1.flat_size + 16, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        out = ipls.DeviceBuffer.from_tensor(t[3:3 + r1.flat_size].view(_tdt(fmt)))
        assert r1.aggregate_round(0, tab, out=out) is out
        r1.sync()
        ws0 = [O.reduce(_widen(x[q], fmt), L, O.START_ZERO) for q, L in enumerate(lengths)]
        want0 = R.narrow(O.get_partitions(ws0, secure).astype(np.float32), fmt)
        _exact16(t.cpu().numpy().view(np.uint16)[3:3 + r1.flat_size], want0, fmt, "aggregate_round device")


# --------------------------------------------------------------------------
# refusals leave the accumulators as they were
# --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_refusals(ipls, fmt):
    from ipls import _native as N
    L, P = 9, 3
    rng = np.random.default_rng(71)
    dk = _dev_kind(ipls, fmt)
    hk = N.HOST_F16 if fmt == "half" else N.HOST_BF16
    x = R.narrow(rng.standard_normal((2, L)).astype(np.float32), fmt).reshape(2, L)
    keep, rows = _dev_rows(x, fmt)
    d = _db(ipls, rows)
    hbuf = np.ascontiguousarray(x[0])
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for p in range(P):
            agg.cache_partition(p, rng.standard_normal(L))
            agg.Update(rng.standard_normal(L), p)
            agg.Update(rng.standard_normal(L), p, from_clients=False)
        tgts = (ipls.TGT_AGG, ipls.TGT_REP, ipls.TGT_WEIGHTS)
        before = [[agg.read(p, t).view(np.uint64).copy() for t in tgts] for p in range(P)]
        lib, h = agg._lib, agg.handle

        def refused(fn):
            with pytest.raises(ipls.IplsError) as e:
                fn()
            assert e.value.code == INVAL
            after = [[agg.read(p, t).view(np.uint64) for t in tgts] for p in range(P)]
            assert all(np.array_equal(a, b) for ra, rb in zip(after, before) for a, b in zip(ra, rb))

        def rc(code):
            return lambda: N.check(code(), h)

        refused(lambda: agg.cache_partition(0, d[0]))                       # set_weights
        refused(lambda: agg.OtherReplicaGradients(0, 1, d[0]))              # other_replica
        src = N.CHUNK_SOURCE(lambda ctx, dst, off, cnt: 0)
        for kind, ptr in ((dk, d[0].ptr), (hk, hbuf.ctypes.data)):
            refused(rc(lambda: lib.ipls_agg_accumulate_chunked(h, 0, N.TGT_AGG, L, kind, 2, src, None)))
            refused(rc(lambda: lib.ipls_agg_set_weights(h, 0, ptr, L, kind)))
            refused(rc(lambda: lib.ipls_agg_other_replica(h, 0, 1, ptr, L, kind)))
        out = torch.zeros(16, dtype=torch.int16, device="cuda").view(_tdt(fmt))
        refused(lambda: agg.reduce_batch_out(0, [[d[0]]], [ipls.DeviceBuffer.from_tensor(out)]))
        arr = (ctypes.c_void_p * 1)(d[0].ptr)
        darr = (ctypes.c_void_p * 1)(out.data_ptr())
        refused(rc(lambda: lib.ipls_agg_reduce_batch_out(h, 0, 1, arr, 1, dk, N.START_ZERO, darr, dk)))
        refused(rc(lambda: lib.ipls_agg_reduce_batch(h, 0, 1, arr, 1, hk, N.START_ZERO, N.TGT_AGG)))   # HOST kind
        refused(lambda: agg.reduce_partial(0, 0, [[d[0]]]))
        # the other F64-only calls that take a kind, through the C-ABI, DEV and HOST kinds
        tk = ctypes.c_uint64()
        sink = N.CHUNK_SINK(lambda *a: 0)
        hout = np.zeros(2 * L)
        for kind, ptr in ((dk, d[0].ptr), (hk, hbuf.ctypes.data)):
            refused(rc(lambda: lib.ipls_agg_blend(h, 0, N.TGT_WEIGHTS, ptr, L, kind, 0.6, 0.4)))
            refused(rc(lambda: lib.ipls_agg_accumulate_range(h, 0, N.TGT_AGG, ptr, 0, 2, kind, ctypes.byref(tk))))
            refused(rc(lambda: lib.ipls_agg_read_range(h, 0, N.TGT_AGG, hout.ctypes.data, 0, 2, kind, ctypes.byref(tk))))
            refused(rc(lambda: lib.ipls_agg_read(h, 0, N.TGT_AGG, hout.ctypes.data, L, kind)))
            refused(rc(lambda: lib.ipls_agg_finalize(h, 0, hout.ctypes.data, kind, None)))
            refused(rc(lambda: lib.ipls_agg_finalize_chunked(h, 0, kind, 2, sink, None)))
        # reduce_partial's C entry, on a handle where slot 1 does not own partition 0:
        # the same call with DEV_F64 is accepted, so the refusal is the kind's
        f64 = torch.ones(L + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with ipls.Aggregator(n_partitions=P, bucket_len=L, devices=[0, 0]) as two:
            a16 = (ctypes.c_void_p * 1)(d[0].ptr)
            a64 = (ctypes.c_void_p * 1)(f64.data_ptr())
            assert two._lib.ipls_agg_reduce_partial(two.handle, 1, 0, 1, a16, 1, dk, N.START_ZERO) == INVAL
            assert two._lib.ipls_agg_reduce_partial(two.handle, 1, 0, 1, a16, 1, hk, N.START_ZERO) == INVAL
            assert two._lib.ipls_agg_reduce_partial(two.handle, 1, 0, 1, a64, 1, N.DEV_F64, N.START_ZERO) == 0
            two.sync()
        odd = ipls.DeviceBuffer(d[0].ptr + 1, L, dtype=fmt)                 # an odd address
        refused(lambda: agg.reduce_batch(0, [[odd]]))
        refused(lambda: agg.Update(odd, 0))
        refused(lambda: agg.UpdateGradient(ipls.DeviceBuffer(d[0].ptr + 1, agg.flat_size, dtype=fmt), [0]))
        refused(lambda: agg.GetPartitions(out=ipls.DeviceBuffer(out.data_ptr() + 1, agg.flat_size, dtype=fmt)))
