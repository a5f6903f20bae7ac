"""The float32 trainer boundary on the GPU: IPLS_DEV_F32 / IPLS_HOST_F32 sources
and outputs against the oracle fed ``x.astype(np.float64)`` (Java's widening
``(double)f`` is exact) and narrowed with ``expected.astype(np.float32)``
(Java's ``(float)d``: one round to nearest even).  Everything is bit-exact;
only sums that a NaN reaches get conftest.assert_bits_equal's NaN allowance,
and the only NaN fed in is the canonical quiet one.

References: Model.java:423 (toDoubleVector -> UpdateGradient, IPLS.java:1737-
1743; OrganizeGradients 1018-1040), Model.java:388-390 (GetPartitions 1140-1174
narrowed), Updater.java:115-117 (the arrival fold), IPLS.java:1248-1274.

Shapes: T is the tile of k_reduce_narrow over floats (1024 lanes x 4 floats x
2 vectors; one shape class); L in {1, 2, 3, 4, 5, 7, 9, T-1, T, T+1, 2T+3}, P in {3, 5}, k in
{1, 2, 3, 8, 9, 33}; the reference geometry M = 30,011 with 3 partitions, also
on a two-shard handle; ETHModel (443,610 values) once.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T = 8192             # elements per tile of k_reduce_narrow over floats: block 1024 x 4 x vectors 2
KS = (1, 2, 3, 8, 9, 33)
LS = (1, 2, 3, 4, 5, 7, 9, T - 1, T, T + 1, 2 * T + 3)
INVAL = -1
QNAN = 0x7fc00000
EDGE_BITS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7f7fffff, QNAN],
                     dtype=np.uint32)


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


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _exact(a, b, what):
    assert np.array_equal(_u64(a), _u64(b)), what


def _exact32(a, b, what):
    a, b = _u32(a), _u32(b)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {a[bad[0]]:#x} != {b[bad[0]]:#x}"


def _f32_buckets(rng, n, L):
    """n float buckets of L elements: normals with the edge values planted,
    1.0f in the count slot (the last element)."""
    x = rng.standard_normal((n, L)).astype(np.float32)
    if L > 1:
        for j in range(n):
            pos = rng.integers(0, L - 1, size=EDGE_BITS.size)
            x[j].view(np.uint32)[pos] = EDGE_BITS
    x[:, L - 1] = 1.0
    return x


def _dev_rows(x, off=0):
    """The rows of a 2-D float32 / float64 array as device tensors whose bases
    are 16-B aligned plus `off` elements; returns (keepalive, [row views])."""
    n, L = x.shape
    stride = (L + off + 7) // 8 * 8
    t = torch.zeros((n, stride), dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    t[:, off:off + L] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t, [t[j, off:off + L] for j in range(n)]


def _db(ipls, rows):
    return [ipls.DeviceBuffer.from_tensor(r) for r in rows]


def _widen(x):
    return [r.astype(np.float64) for r in x]


# --------------------------------------------------------------------------
# 8. the old hazard; the tile constant
# --------------------------------------------------------------------------
def test_from_tensor_float32(ipls):
    b = ipls.DeviceBuffer.from_tensor(torch.ones(8, dtype=torch.float32, device="cuda"))
    assert b.n == 8 and b.dtype == "f32" and b.kind == ipls.DEV_F32
    # byte carriers keep today's arithmetic
    for dt, n in ((torch.float64, 8), (torch.int64, 8), (torch.uint8, 1)):
        c = ipls.DeviceBuffer.from_tensor(torch.zeros(8, dtype=dt, device="cuda"))
        assert c.n == n and c.dtype == "f64" and c.kind == ipls.DEV_F64


def test_tile_constant_and_paths(ipls, O):
    rng = np.random.default_rng(1)
    L = T + 1
    x = _f32_buckets(rng, 2, L)
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        keep, rows = _dev_rows(x)
        agg.reduce_batch(0, [_db(ipls, rows)])
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_F32
        assert li["block"] * 4 * li["vectors"] == T
        assert li["seqf"] == 1 and li["grid"] == 2       # vector path, one full and one partial tile
        assert_bits_equal(agg.read(0), O.reduce(_widen(x), L), "aligned")
        keep2, rows2 = _dev_rows(x, off=1)
        agg.reduce_batch(0, [_db(ipls, rows2)])
        assert agg.last_launch()["seqf"] == 0             # 4 mod 16 bases: element by element
        assert_bits_equal(agg.read(0), O.reduce(_widen(x), L), "misaligned")


# --------------------------------------------------------------------------
# 1. the batched fold
# --------------------------------------------------------------------------
@pytest.mark.parametrize("P", (3, 5))
@pytest.mark.parametrize("L", LS)
def test_reduce_batch_f32(ipls, O, L, P):
    rng = np.random.default_rng(1000 * P + L)
    kmax = max(KS)
    x = _f32_buckets(rng, P * kmax, L).reshape(P, kmax, L)
    keep, rows = _dev_rows(x.reshape(P * kmax, L))
    bufs = _db(ipls, rows)
    acc0 = rng.standard_normal((P, L))
    Lp = (L + 1) // 2 * 2
    dn = torch.zeros((P, Lp), dtype=torch.float64, device="cuda")
    db = torch.zeros((P, Lp), dtype=torch.int64, device="cuda")
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for k in KS:
            tab = [[bufs[q * kmax + j] for j in range(k)] for q in range(P)]
            wide = [_widen(x[q, :k]) for q in range(P)]
            what = f"L={L} P={P} k={k}"
            # START_ZERO
            agg.reduce_batch(0, tab, start_mode=ipls.START_ZERO)
            assert agg.last_launch()["kernel"] == ipls.KERNEL_REDUCE_F32
            for q in range(P):
                assert_bits_equal(agg.read(q), O.reduce(wide[q], L, O.START_ZERO), what + " ZERO")
            # ACCUM onto a non-zero AGG
            agg.reset()
            for q in range(P):
                agg.Update(acc0[q], q)
            agg.reduce_batch(0, tab, start_mode=ipls.START_ACCUM)
            for q in range(P):
                assert_bits_equal(agg.read(q), O.reduce(wide[q], L, O.START_ACCUM, 0.0 + acc0[q]), what + " ACCUM")
            # FIRST (keeps bucket 0's -0.0)
            agg.reduce_batch(0, tab, start_mode=ipls.START_FIRST)
            for q in range(P):
                assert_bits_equal(agg.read(q), O.reduce(wide[q], L, O.START_FIRST), what + " FIRST")
            # reduce_batch_out: native doubles (ZERO), big-endian bytes (FIRST)
            agg.reduce_batch_out(0, tab, [ipls.DeviceBuffer(dn[q].data_ptr(), L) for q in range(P)],
                                 start_mode=ipls.START_ZERO)
            agg.reduce_batch_out(0, tab, [ipls.DeviceBuffer(db[q].data_ptr(), L, True) for q in range(P)],
                                 start_mode=ipls.START_FIRST, big_endian_out=True)
            agg.sync()
            hn = dn.cpu().numpy()
            hb = db.cpu().numpy().view(">f8").astype(np.float64)
            for q in range(P):
                assert_bits_equal(hn[q, :L], O.reduce(wide[q], L, O.START_ZERO), what + " out native")
                assert_bits_equal(hb[q, :L], O.reduce(wide[q], L, O.START_FIRST), what + " out BE")
    del keep


@pytest.mark.parametrize("off", (1, 2, 3))
def test_reduce_batch_f32_misaligned(ipls, O, off):
    """Buckets at 4, 8, 12 mod 16: the scalar path, same bits."""
    L, P, k = T + 1, 3, 9
    rng = np.random.default_rng(77 + off)
    x = _f32_buckets(rng, P * k, L)
    keep, rows = _dev_rows(x, off=off)
    bufs = _db(ipls, rows)
    assert all(b.ptr % 16 == 4 * off for b in bufs)
    tab = [[bufs[q * k + j] for j in range(k)] for q in range(P)]
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for mode in (ipls.START_ZERO, ipls.START_FIRST):
            agg.reduce_batch(0, tab, start_mode=mode)
            li = agg.last_launch()
            assert li["kernel"] == ipls.KERNEL_REDUCE_F32 and li["seqf"] == 0
            for q in range(P):
                assert_bits_equal(agg.read(q), O.reduce(_widen(x[q * k:(q + 1) * k]), L, mode), f"off={off} mode={mode}")


_TILE = {}


def _tile(ipls):
    """(T, block) of the fold over floats, read from the launch record."""
    if not _TILE:
        keep, rows = _dev_rows(np.ones((1, 9), dtype=np.float32))
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as agg:
            agg.reduce_batch(0, [_db(ipls, rows)])
            li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_F32
        _TILE["T"], _TILE["block"] = li["block"] * 4 * li["vectors"], li["block"]
        assert _TILE["T"] <= 32768
    return _TILE["T"], _TILE["block"]


@pytest.mark.parametrize("k", (1, 9))
@pytest.mark.parametrize("lname", ("7", "T+1", "2T+3", "T+4b+1"))
def test_reduce_batch_out_accum_big_endian_f32(ipls, O, lname, k):
    """ACCUM onto big-endian caller destinations that hold random doubles: three
    partitions in one launch, bit-exact against the oracle's ACCUM fold.  T + 4b + 1
    (b lanes) gives the partial tile one vector step of 4 elements per lane."""
    Tl, b = _tile(ipls)
    L, P = {"7": 7, "T+1": Tl + 1, "2T+3": 2 * Tl + 3, "T+4b+1": Tl + 4 * b + 1}[lname], 3
    rng = np.random.default_rng(900 + 10 * L + k)
    x = _f32_buckets(rng, P * k, L).reshape(P, k, L)
    keep, rows = _dev_rows(x.reshape(P * k, L))
    bufs = _db(ipls, rows)
    tab = [[bufs[q * k + j] for j in range(k)] for q in range(P)]
    prior = rng.standard_normal((P, L))
    Lp = (L + 1) // 2 * 2
    d = torch.zeros((P, Lp), dtype=torch.int64, device="cuda")
    d[:, :L] = torch.from_numpy(prior.astype(">f8").view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        agg.reduce_batch_out(0, tab, [ipls.DeviceBuffer(d[q].data_ptr(), L, True) for q in range(P)],
                             start_mode=ipls.START_ACCUM, big_endian_out=True)
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_F32 and li["seqf"] == 1
        agg.sync()
    got = d.cpu().numpy().view(">f8").astype(np.float64)
    for q in range(P):
        assert_bits_equal(got[q, :L], O.reduce(_widen(x[q]), L, O.START_ACCUM, prior[q]), f"L={L} k={k} p={q}")


# --------------------------------------------------------------------------
# 2. accumulate / UpdateAsync: f32, f64, f32 into one partition, in call order
# --------------------------------------------------------------------------
def _order_case(rng, L):
    big = np.float32(1e16)
    pat = rng.integers(0, 3, size=L)
    b1 = np.where(pat == 0, big, np.where(pat == 1, np.float32(1.0), -big)).astype(np.float32)
    b2 = np.where(pat == 0, 1.0, np.where(pat == 1, float(big), 3.0)).astype(np.float64)
    b3 = np.where(pat == 0, -big, np.where(pat == 1, -big, big)).astype(np.float32)
    b1[-1] = b3[-1] = 1.0
    b2[-1] = 1.0
    return b1, b2, b3


@pytest.mark.parametrize("L", (7, T + 1))
def test_accumulate_mixed_order(ipls, O, L):
    rng = np.random.default_rng(5 + L)
    b1, b2, b3 = _order_case(rng, L)
    w = [b1.astype(np.float64), b2, b3.astype(np.float64)]
    want = O.reduce(w, L, O.START_ZERO)
    # the order matters for these values: other orders give other bits
    assert not np.array_equal(_u64(want), _u64(O.reduce([w[0], w[2], w[1]], L, O.START_ZERO)))
    assert not np.array_equal(_u64(want), _u64(O.reduce([w[1], w[2], w[0]], L, O.START_ZERO)))
    k1, (r1,) = _dev_rows(b1[None])
    k2, (r2,) = _dev_rows(b2[None])
    k3, (r3,) = _dev_rows(b3[None])
    d1, d2, d3 = _db(ipls, [r1, r2, r3])
    assert (d1.kind, d2.kind, d3.kind) == (ipls.DEV_F32, ipls.DEV_F64, ipls.DEV_F32)
    with ipls.Aggregator(n_partitions=3, bucket_len=L) as agg:
        for d in (d1, d2, d3):                   # synchronous, device operands
            agg.Update(d, 0)
        _exact(agg.read(0), want, "Update device")
        for h in (b1, b2, b3):                   # synchronous, host operands (HOST_F32 / HOST_F64)
            agg.Update(h, 1)
        _exact(agg.read(1), want, "Update host")
        agg.set_coalesce(32)
        t = 0
        for d in (d1, d2, d3):                   # queued: a change of kind must not reorder
            t = agg.UpdateAsync(d, 2)
        agg.Wait(t)
        _exact(agg.read(2), want, "UpdateAsync")
        # a short f32 bucket is refused as a short f64 one is
        with pytest.raises(ipls.IplsError) as e:
            agg.Update(ipls.DeviceBuffer(d1.ptr, L - 1, dtype="f32"), 0)
        assert e.value.code == -2
        _exact(agg.read(0), want, "after the refusal")


# --------------------------------------------------------------------------
# 3. UpdateGradient / OrganizeGradients / InitializeWeights from floats
# --------------------------------------------------------------------------
def _flat_f32(rng, M):
    f = rng.standard_normal(M).astype(np.float32)
    pos = rng.integers(0, M, size=4 * EDGE_BITS.size)
    f.view(np.uint32)[pos] = np.tile(EDGE_BITS, 4)
    return f


def _operands(ipls, flat):
    """(name, operand, keepalive) for every operand form of a float vector."""
    M = flat.size
    out = []
    for off in (0, 1):
        t = torch.zeros(M + 8, dtype=torch.float32, device="cuda")
        t[off:off + M] = torch.from_numpy(flat).cuda()
        torch.cuda.synchronize()
        out.append((f"device+{off}", ipls.DeviceBuffer.from_tensor(t[off:off + M]), t))
    out.append(("pageable", flat.copy(), None))
    pin = ipls.PinnedBuffer(4 * M)
    v = pin.view(np.float32)
    v[:] = flat
    out.append(("pinned", v, pin))
    return out


def _check_flat_paths(ipls, O, open_agg, M, P, seed):
    rng = np.random.default_rng(seed)
    f1, f2 = _flat_f32(rng, M), _flat_f32(rng, M)
    og1 = O.organize_gradients(f1.astype(np.float64), M, P)
    og2 = O.organize_gradients(f2.astype(np.float64), M, P)
    ops2 = _operands(ipls, f2)
    for i, (name, op, keep) in enumerate(_operands(ipls, f1)):
        with open_agg() as agg:
            assert agg.flat_size == M
            got = agg.OrganizeGradients(op)
            gbe = agg.OrganizeGradients(op, big_endian_out=True)
            for p in range(P):
                _exact(got[p], og1[p], f"OrganizeGradients {name} p={p}")
                _exact(np.frombuffer(gbe[p], dtype=">f8").astype(np.float64), og1[p], f"OrganizeGradients BE {name} p={p}")
            for auth in ([1], list(range(P)), [0, P - 1]):
                agg.reset()
                agg.UpdateGradient(op, auth)               # into a logically zero AGG: +0.0 + v
                agg.UpdateGradient(ops2[i][1], auth)       # then AGG + v
                for p in range(P):
                    want = (0.0 + og1[p]) + og2[p] if p in auth else np.zeros_like(og1[p])
                    assert_bits_equal(agg.read(p), want, f"UpdateGradient {name} auth={auth} p={p}")
            agg.InitializeWeights(op)
            for p in range(P):
                w = og1[p].copy()
                w[-1] = 0.0
                _exact(agg.read(p, ipls.TGT_WEIGHTS), w, f"InitializeWeights {name} p={p}")


def test_flat_vectors_reference_geometry(ipls, O):
    _check_flat_paths(ipls, O, lambda: ipls.Aggregator(30011, 3), 30011, 3, 11)


def test_flat_vectors_every_residue(ipls, O):
    # chunk = 7 floats: the partitions' slices start at 0, 12, 8, 4, 0 mod 16 B
    _check_flat_paths(ipls, O, lambda: ipls.Aggregator(32, 5), 32, 5, 12)


def test_flat_vectors_two_shards(ipls, O):
    _check_flat_paths(ipls, O, lambda: ipls.Aggregator(30011, 3, devices=[0, 0]), 30011, 3, 13)


def test_ethmodel_as_floats(ipls, ethmodel):
    """The reference's own data: every ETHModel value is a widened float, so
    the f32 path must give the very bits the f64 path gives."""
    f32 = ethmodel.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64).view(np.uint64), ethmodel.view(np.uint64))
    M, P = ethmodel.size, 3
    t = torch.from_numpy(f32).cuda()
    torch.cuda.synchronize()
    with ipls.Aggregator(M, P, max_peers=3) as a64, ipls.Aggregator(M, P, max_peers=3) as a32:
        a64.InitializeWeights(ethmodel)
        a64.UpdateGradient(ethmodel, [0, 1, 2])
        for op in (f32, ipls.DeviceBuffer.from_tensor(t)):
            a32.reset()
            a32.InitializeWeights(op)
            a32.UpdateGradient(op, [0, 1, 2])
            for p in range(P):
                for tgt in (ipls.TGT_WEIGHTS, ipls.TGT_AGG):
                    assert a32.checksum(p, tgt) == a64.checksum(p, tgt)
                _exact(a32.read(p), a64.read(p), f"AGG p={p}")
        g64 = a64.GetPartitions()
        _exact32(a32.GetPartitions(dtype=np.float32), g64.astype(np.float32), "GetPartitions")
        _exact32(a32.GetPartitions(dtype=np.float32), f32, "the model comes back as the floats it was")


# --------------------------------------------------------------------------
# 4. GetPartitions narrowed to float
# --------------------------------------------------------------------------
NARROW = [(1e39, 0x7f800000), (-1e39, 0xff800000), (2.0 ** -150, 0), (1.5 * 2.0 ** -149, 2), (1.4e-45, 1),
          (1 + 2.0 ** -24, 0x3f800000), (1 + 2.0 ** -24 + 2.0 ** -50, 0x3f800001), (1 + 3 * 2.0 ** -24, 0x3f800002),
          (3.4028235677973366e38, 0x7f800000), (3.4028235677973362e38, 0x7f7fffff), (-0.0, 0x80000000),
          (np.inf, 0x7f800000), (-np.inf, 0xff800000), (np.float64(np.float32(np.nan)), QNAN)]


def _weights(rng, lengths, cnts):
    ws = []
    for p, L in enumerate(lengths):
        w = rng.standard_normal(L)
        if cnts[p] == 1.0 and L > 1:
            pos = rng.permutation(L - 1)[:len(NARROW)]
            w[pos] = [v for v, _ in NARROW][:pos.size]
        w[-1] = cnts[p]
        ws.append(w)
    return ws


def _get_f32_all_ways(ipls, agg):
    """GetPartitions as floats: the host array and device outputs at 0..3 floats past a 128-B line."""
    n = agg.flat_size
    outs = [("host", agg.GetPartitions(dtype=np.float32))]
    for off in (0, 1, 2, 3):
        t = torch.full((n + 40,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r = agg.GetPartitions(out=ipls.DeviceBuffer.from_tensor(t[off:off + n]))
        assert r.dtype == "f32"
        agg.sync()
        h = t.cpu().numpy()
        assert np.all(h[:off] == 7.0) and np.all(h[off + n:] == 7.0), "wrote outside the output"
        outs.append((f"device+{off}", h[off:off + n].copy()))
    return outs


@pytest.mark.parametrize("shape", [(3, 5000), (5, 7), (3, 2), (3, 2 * 2048 + 36)])
@pytest.mark.parametrize("secure", (False, True))
def test_get_partitions_f32(ipls, O, shape, secure):
    P, L = shape
    rng = np.random.default_rng(41)
    cnts = [[1.0, 3.0, 7.0, 0.0, 1.0][p] for p in range(P)]
    with ipls.Aggregator(n_partitions=P, bucket_len=L, secure=secure) as agg:
        ws = _weights(rng, agg.lengths, cnts)
        for p, w in enumerate(ws):
            agg.cache_partition(p, w)
        with np.errstate(all="ignore"):
            want64 = O.get_partitions(ws, secure)
            want = want64.astype(np.float32)
            if not secure and L == 5000:
                # the planted doubles narrow to the bits worked out by hand ...
                for v, b in NARROW:
                    hit = np.flatnonzero(_u64(ws[0][:-1]) == np.float64(v).view(np.uint64))
                    assert hit.size and all(_u32(want[hit])[i] == b for i in range(hit.size)), v
                # ... and an f32 division would not pass: it differs from the narrowed f64 quotient
                for p in (1, 2):
                    o = agg.offsets[p]
                    f32div = ws[p][:-1].astype(np.float32) / np.float32(cnts[p])
                    assert np.any(_u32(f32div) != _u32(want[o:o + L - 1]))
        for name, got in _get_f32_all_ways(ipls, agg):
            _exact32(got, want, f"P={P} L={L} secure={secure} {name}")
        _exact(agg.GetPartitions(), want64, "the f64 output is unchanged")


def test_get_partitions_f32_two_shards(ipls, O):
    rng = np.random.default_rng(43)
    with ipls.Aggregator(30011, 3, devices=[0, 0]) as agg:
        ws = _weights(rng, agg.lengths, [1.0, 3.0, 7.0])
        for p, w in enumerate(ws):
            agg.cache_partition(p, w)
        with np.errstate(all="ignore"):
            want = O.get_partitions(ws).astype(np.float32)
        for name, got in _get_f32_all_ways(ipls, agg):
            _exact32(got, want, f"two shards {name}")


# --------------------------------------------------------------------------
# 5. a whole round; 6. the batched fold on two shards
# --------------------------------------------------------------------------
def _round_oracle(O, x, rep, lengths, k):
    ws = []
    for q, L in enumerate(lengths):
        agg = O.reduce(_widen(x[q, :k]), L, O.START_ZERO)
        w, wa = np.zeros(L), np.zeros(L)
        O.aggregate_partition(agg, rep[q][:L].copy(), w, wa)
        ws.append(w)
    return ws


def _round_buckets(rng, lengths, k):
    """(P, k, max L) floats, 1.0f in each partition's count slot (the last
    partition of the reference geometry is one shorter; longer buckets are fine)."""
    P, Lm = len(lengths), max(lengths)
    x = rng.standard_normal((P, k, Lm)).astype(np.float32)
    for q, L in enumerate(lengths):
        x[q, :, L - 1] = 1.0
    return x


@pytest.mark.parametrize("devices", (None, [0, 0]))
@pytest.mark.parametrize("geom", [("synthetic", T + 1, 3), ("reference", 30011, 3)])
def test_aggregate_round_f32(ipls, O, geom, devices):
    kind, a, P = geom
    opn = (lambda: ipls.Aggregator(n_partitions=P, bucket_len=a, devices=devices)) if kind == "synthetic" else \
          (lambda: ipls.Aggregator(a, P, devices=devices))
    rng = np.random.default_rng(51)
    k = 9
    with opn() as r1, opn() as r2:
        lengths = r1.lengths
        L = max(lengths)
        x = _round_buckets(rng, lengths, k)
        keep, rows = _dev_rows(x.reshape(P * k, L))
        bufs = _db(ipls, rows)
        tab = [[bufs[q * k + j] for j in range(k)] for q in range(P)]
        rep = rng.standard_normal((P, L))
        for q, Lq in enumerate(lengths):
            rep[q, Lq - 1:] = 0.0
        rep[0] = 0.0                                      # partition 0: REP logically zero
        ws = _round_oracle(O, x, rep, lengths, k)
        want = O.get_partitions(ws).astype(np.float32)
        for r in (r1, r2):
            for q in range(1, P):
                r.Update(rep[q, :lengths[q]], q, from_clients=False)
        # one call, host floats out
        got = r1.aggregate_round(0, tab, dtype=np.float32)
        _exact32(got, want, "aggregate_round host f32")
        # the three steps on a second handle
        r2.reduce_batch(0, tab, start_mode=ipls.START_ACCUM)
        for q in range(P):
            r2.AggregatePartition(q)
        _exact32(r2.GetPartitions(dtype=np.float32), want, "three steps")
        for q in range(P):
            _exact(r1.read(q, ipls.TGT_WEIGHTS), ws[q], f"W p={q}")
            assert r1.checksum(q, ipls.TGT_WEIGHTS) == r2.checksum(q, ipls.TGT_WEIGHTS)
        # again into a device float buffer (REP is zero now), and f64 averages from f32 buckets
        t = torch.zeros(r1.flat_size + 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r1.aggregate_round(0, tab, out=ipls.DeviceBuffer.from_tensor(t))
        r1.sync()
        ws0 = _round_oracle(O, x, np.zeros((P, L)), lengths, k)
        _exact32(t.cpu().numpy()[:r1.flat_size], O.get_partitions(ws0).astype(np.float32), "aggregate_round device f32")
        _exact(r1.aggregate_round(0, tab), O.get_partitions(ws0), "aggregate_round f64 averages")


def test_reduce_batch_f32_two_shards(ipls, O):
    rng = np.random.default_rng(61)
    P, k = 3, 9
    with ipls.Aggregator(30011, 3, devices=[0, 0]) as agg:
        L = max(agg.lengths)
        x = _f32_buckets(rng, P * k, L).reshape(P, k, L)
        keep, rows = _dev_rows(x.reshape(P * k, L))
        bufs = _db(ipls, rows)
        tab = [[bufs[q * k + j] for j in range(k)] for q in range(P)]
        for mode in (ipls.START_ZERO, ipls.START_ACCUM, ipls.START_FIRST):
            agg.reset()
            agg.reduce_batch(0, tab, start_mode=mode)
            for q, Lq in enumerate(agg.lengths):
                assert_bits_equal(agg.read(q), O.reduce(_widen(x[q]), Lq, mode, np.zeros(Lq)),
                                  f"two shards mode={mode} p={q}")


# --------------------------------------------------------------------------
# 7. refusals leave the accumulators as they were
# --------------------------------------------------------------------------
def test_refusals(ipls):
    from ipls import _native as N
    L, P = 9, 3
    rng = np.random.default_rng(71)
    x = _f32_buckets(rng, 2, L)
    keep, rows = _dev_rows(x)
    d = _db(ipls, rows)
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for p in range(P):
            agg.cache_partition(p, rng.standard_normal(L))
            agg.Update(rng.standard_normal(L), p)
        tgts = (ipls.TGT_AGG, ipls.TGT_REP, ipls.TGT_WEIGHTS)
        before = [[agg.read(p, t).view(np.uint64).copy() for t in tgts] for p in range(P)]

        def refused(fn):
            with pytest.raises(ipls.IplsError) as e:
                fn()
            assert e.value.code == INVAL
            after = [[agg.read(p, t).view(np.uint64) for t in tgts] for p in range(P)]
            assert all(np.array_equal(a, b) for ra, rb in zip(after, before) for a, b in zip(ra, rb))

        refused(lambda: agg.cache_partition(0, d[0]))                       # set_weights
        src = N.CHUNK_SOURCE(lambda ctx, dst, off, cnt: 0)
        for kind in (N.DEV_F32, N.HOST_F32):                                 # UpdateChunked's call
            refused(lambda: N.check(agg._lib.ipls_agg_accumulate_chunked(agg.handle, 0, N.TGT_AGG, L, kind, 2, src, None),
                                    agg.handle))
        out = torch.zeros(16, dtype=torch.float32, device="cuda")
        refused(lambda: agg.reduce_batch_out(0, [[d[0]]], [ipls.DeviceBuffer.from_tensor(out)]))
        arr = (ctypes.c_void_p * 1)(d[0].ptr)
        darr = (ctypes.c_void_p * 1)(out.data_ptr())
        refused(lambda: N.check(agg._lib.ipls_agg_reduce_batch_out(agg.handle, 0, 1, arr, 1, N.DEV_F32, N.START_ZERO,
                                                                   darr, N.DEV_F32), agg.handle))
        odd = ipls.DeviceBuffer(d[0].ptr + 1, L, dtype="f32")               # an odd address
        refused(lambda: agg.reduce_batch(0, [[odd]]))
        refused(lambda: agg.Update(odd, 0))
        refused(lambda: agg.UpdateGradient(ipls.DeviceBuffer(d[0].ptr + 1, agg.flat_size, dtype="f32"), [0]))
        refused(lambda: agg.GetPartitions(out=ipls.DeviceBuffer(out.data_ptr() + 1, agg.flat_size, dtype="f32")))
        refused(lambda: agg.OtherReplicaGradients(0, 1, d[0]))
