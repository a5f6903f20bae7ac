"""The streamed trainer-format calls on the GPU: UpdateChunked(dtype=...)
(ipls_agg_accumulate_chunked_narrow: 4 or 2 B per value through the source,
the pinned ring and PCIe, k_fold1_narrow from the call's stage) and
GetPartitionsChunked(dtype=...) (ipls_agg_get_partitions_chunked_narrow: the
narrowing divide into the stage, bytes out).  Bit for bit against the oracle
fed the widened values, and against Update / GetPartitions of the same kind.

Where a callback has to stay blocked while another thread works, it waits for
that thread's event (bounded by a timeout that only a deadlock reaches) rather
than sleeping: if the call held the shard lock, the other thread could never
set the event and the wait would report it.
"""
import ctypes
import itertools
import threading

import numpy as np
import pytest

from conftest import assert_bits_equal
import h16_ref as R
import narrow_fmt as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMTS = F.FMTS
INVAL, RANGE = -1, -2
WAIT = 20.0   # seconds; reached only when a call deadlocks


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
    """(b, G) of k_fold1_narrow for the format, from one launch's record."""
    if fmt not in _SHAPE:
        keep, d = F.dev(ipls, torch, np.full(9, F.ONE[fmt], dtype=F.bits_dtype(fmt)), fmt)
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as agg:
            agg.Update(d, 0)
            li = agg.last_launch()
        assert li["kernel"] == F.fold_kernel(ipls, fmt), li
        _SHAPE[fmt] = (li["block"], 4 * li["block"] * li["vectors"])
    return _SHAPE[fmt]


def _source(bits, fmt, calls=None, stop_at=None):
    """A chunk source over the bucket's bit patterns; records (offset, count)."""
    s = F.esize(fmt)
    raw = np.ascontiguousarray(bits)

    def src(dst, off, cnt):
        if calls is not None:
            calls.append((off, cnt))
        if stop_at is not None and len(calls) - 1 == stop_at:
            return False
        ctypes.memmove(dst, raw.ctypes.data + off * s, cnt * s)
        return True
    return src


def _state(agg, P):
    return [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in (0, 1, 2)]


@pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
@pytest.mark.parametrize("fmt", FMTS)
def test_update_chunked(ipls, O, fmt, devices):
    b, G = _shape(ipls, fmt)
    for L in (9, 4 * b + 1, G + 4 * b + 1):
        rng = np.random.default_rng(11 + L)
        x1, x2 = F.bucket(rng, L, fmt, (0, 3, 4, L - 2)), F.bucket(rng, L, fmt, (0, 3, 4, L - 2))
        w = [F.widen(x1, fmt), F.widen(x2, fmt)]
        want = O.reduce(w, L, O.START_ZERO)
        with ipls.Aggregator(n_partitions=2, bucket_len=L, devices=devices) as agg:
            if devices:
                assert agg.partition_device(1) is not None
            # Update of the whole bucket is the reference the chunked call must equal
            agg.Update(F.host(torch, x1, fmt), 1)
            agg.Update(F.host(torch, x2, fmt), 1)
            whole = agg.read(1).copy()
            assert_bits_equal(whole, want, f"{fmt} L={L} Update")
            for chunk in sorted({2, 6, L - 1 - (L - 1) % 2 if L > 3 else 2, L + (L & 1), 2 * L + 2}):
                agg.reset()
                calls = []
                agg.UpdateChunked(1, L, _source(x1, fmt, calls), chunk=chunk, dtype=F.np_dtype(fmt))
                li = agg.last_launch()
                assert li["kernel"] == F.fold_kernel(ipls, fmt) and li["start"] == ipls.START_ZERO, li
                c = min(chunk, L)
                assert calls == [(o, min(c, L - o)) for o in range(0, L, c)], (chunk, calls[:4])
                agg.UpdateChunked(1, L + 3, _source(np.concatenate([x2, x2[:3]]), fmt), chunk=chunk,
                                  dtype=F.np_dtype(fmt))     # values past L_p are never asked for
                assert agg.last_launch()["start"] == ipls.START_ACCUM
                got = agg.read(1)
                assert_bits_equal(got, want, f"{fmt} L={L} chunk={chunk}")
                assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))
                assert not agg.read(0).any(), "partition 0 (the other shard) is untouched"


@pytest.mark.parametrize("fmt", FMTS)
def test_stopped_source_and_short_bucket(ipls, O, fmt):
    b, G = _shape(ipls, fmt)
    L, P = G + 4 * b + 1, 2
    rng = np.random.default_rng(5)
    x = F.bucket(rng, L, fmt)
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for p in range(P):
            agg.Update(rng.standard_normal(L), p)
            agg.Update(rng.standard_normal(L), p, from_clients=False)
            agg.cache_partition(p, rng.standard_normal(L))
        before = _state(agg, P)
        calls = []
        with pytest.raises(ipls.IplsError) as e:
            agg.UpdateChunked(0, L, _source(x, fmt, calls, stop_at=1), chunk=2 * b, dtype=F.np_dtype(fmt))
        assert e.value.code == INVAL and len(calls) == 2
        for a, was in zip(_state(agg, P), before):
            assert np.array_equal(a, was), "a stopped source changed an accumulator"
        calls = []
        with pytest.raises(ipls.IplsError) as e:
            agg.UpdateChunked(0, L - 1, _source(x, fmt, calls), chunk=2 * b, dtype=F.np_dtype(fmt))
        assert e.value.code == RANGE and calls == []
        for a, was in zip(_state(agg, P), before):
            assert np.array_equal(a, was)
        # and the handle still works
        agg.reset()
        agg.UpdateChunked(0, L, _source(x, fmt), chunk=2 * b, dtype=F.np_dtype(fmt))
        assert_bits_equal(agg.read(0), O.reduce([F.widen(x, fmt)], L, O.START_ZERO), f"{fmt} after the refusals")


def test_refusals(ipls):
    from ipls import _native as N
    L = 9
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        lib, h = agg._lib, agg._h
        n_calls = []

        @N.CHUNK_SOURCE
        def src(ctx, dst, off, n):
            n_calls.append(off)
            return 1
        for kind in (N.HOST_F64, N.HOST_BE, N.DEV_F64, N.DEV_BE, N.HOST_FRAME, N.DEV_F32, N.DEV_F16, N.DEV_BF16, 99):
            assert lib.ipls_agg_accumulate_chunked_narrow(h, 0, N.TGT_AGG, L, kind, 2, src, None) == INVAL, kind
        for kind in (N.HOST_F32, N.HOST_F16, N.HOST_BF16):
            assert lib.ipls_agg_accumulate_chunked(h, 0, N.TGT_AGG, L, kind, 2, src, None) == INVAL, kind
            for chunk in (0, 1, 3, -2):
                assert lib.ipls_agg_accumulate_chunked_narrow(h, 0, N.TGT_AGG, L, kind, chunk, src, None) == INVAL
            assert lib.ipls_agg_accumulate_chunked_narrow(h, 1, N.TGT_AGG, L, kind, 2, src, None) == RANGE
            assert lib.ipls_agg_accumulate_chunked_narrow(h, 0, 7, L, kind, 2, src, None) == INVAL

        @N.BYTE_SINK
        def sink(ctx, b, off, n):
            n_calls.append(off)
            return 1
        for kind in (N.HOST_F64, N.HOST_BE, N.HOST_BE_CANON, N.DEV_F64, N.DEV_F32, N.DEV_F16, N.DEV_BF16, 99):
            assert lib.ipls_agg_get_partitions_chunked_narrow(h, kind, 2, sink, None) == INVAL, kind
        for chunk in (0, 1, 3):
            assert lib.ipls_agg_get_partitions_chunked_narrow(h, N.HOST_F32, chunk, sink, None) == INVAL
        assert n_calls == []
        assert not agg.read(0).any()


def test_lock_scope_of_the_source(ipls, O):
    """While a chunked f32 source is blocked after its first chunk, an f64
    Update into the same partition and a GetPartitions return; afterwards the
    partition holds (base + B) + A: the chunked arrival A took effect when its
    last chunk landed, after B.  base = 1e16f, B = 1.0, A = -1e16f: (base + B)
    + A is 0.0 and (base + A) + B is 1.0."""
    L = 4099
    base = np.full(L, np.float32(1e16), dtype=np.float64)
    B = np.full(L, 1.0)
    A = np.full(L, -1e16, dtype=np.float32)
    want = O.reduce([base, B, A.astype(np.float64)], L, O.START_ZERO)
    other = O.reduce([base, A.astype(np.float64), B], L, O.START_ZERO)
    assert not np.array_equal(want.view(np.uint64), other.view(np.uint64)) and base.all()
    done, errs = threading.Event(), []
    with ipls.Aggregator(n_partitions=1, bucket_len=L) as agg:
        agg.Update(base, 0)

        def second():
            try:
                agg.Update(B, 0)
                agg.GetPartitions()
            except BaseException as e:   # noqa: BLE001 -- reported by the main thread
                errs.append(repr(e))
            done.set()
        t = threading.Thread(target=second)
        raw, calls = A.view(np.uint32), []

        def src(dst, off, cnt):
            ctypes.memmove(dst, raw.ctypes.data + 4 * off, 4 * cnt)
            calls.append(off)
            if len(calls) == 1:
                t.start()
                assert done.wait(WAIT), "Update / GetPartitions waited for the blocked source"
            return True
        agg.UpdateChunked(0, L, src, chunk=1024, dtype=np.float32)
        t.join(WAIT)
        assert not errs, errs
        assert len(calls) == 5
        assert_bits_equal(agg.read(0), want, "(base + B) + A")


def _w_case(rng, lengths, fmt):
    """Weights per partition: normals with the first count slot 0 (W passes
    through), the others 3.0; the two-roundings value at [1][0]."""
    ws = []
    for q, L in enumerate(lengths):
        w = rng.standard_normal(L) * 4.0
        w[L - 1] = 0.0 if q == 0 else 3.0
        ws.append(w)
    return ws


def _narrow_model(O, ws, fmt, secure):
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = O.get_partitions(ws, secure).astype(np.float32)
    return f32.view(np.uint32) if fmt == "f32" else R.narrow(f32, fmt)


def _gather(agg, fmt, chunk, nbytes, pieces=None):
    out = bytearray(nbytes)

    def sink(ptr, off, cnt):
        if pieces is not None:
            pieces.append((off, cnt))
        out[off:off + cnt] = ctypes.string_at(ptr, cnt)
        return True
    agg.GetPartitionsChunked(sink, chunk=chunk, dtype=F.np_dtype(fmt))
    return np.frombuffer(bytes(out), dtype=F.bits_dtype(fmt))


def _same_bits(got, want, fmt, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if fmt == "f32":
        nan = (want & 0x7fffffff) > 0x7f800000
        gn = (got & 0x7fffffff) > 0x7f800000
    else:
        nan, gn = R.is_nan(want, fmt), R.is_nan(got, fmt)
    assert np.array_equal(nan, gn), what
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"


@pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
@pytest.mark.parametrize("secure", (False, True), ids=("plain", "secure"))
@pytest.mark.parametrize("fmt", FMTS)
def test_get_partitions_chunked(ipls, O, fmt, secure, devices):
    M, P = 10007, 3      # odd; partitions of 3336, 3336, 3335 values
    s = F.esize(fmt)
    rng = np.random.default_rng(21)
    with ipls.Aggregator(M, P, secure=secure, devices=devices) as agg:
        lengths = list(agg.lengths)
        assert len(set(lengths)) > 1 and agg.flat_size == M
        ws = _w_case(rng, lengths, fmt)
        # 1 + 2^-11 + 2^-30 as the quotient of partition 1's first value
        q = 1.0 + 2.0 ** -11 + 2.0 ** -30
        ws[1][0] = q * 3.0 * (1e12 if secure else 1.0)
        for p in range(P):
            agg.cache_partition(p, ws[p])
        want = _narrow_model(O, ws, fmt, secure)
        assert want.size == M
        if fmt == "half" and not secure:
            assert O.get_partitions(ws, secure)[lengths[0] - 1] == q
            assert want[lengths[0] - 1] == 0x3c00, "the two roundings (a single one gives 0x3c01)"
        whole = agg.GetPartitions(dtype=F.np_dtype(fmt))
        _same_bits(np.ascontiguousarray(whole).view(F.bits_dtype(fmt)), want, fmt, f"{fmt} GetPartitions")
        for chunk in (2, 1000, M + 1, 4 * M):      # M is odd: M + 1 is the first even chunk >= M
            pieces = []
            got = _gather(agg, fmt, chunk, M * s, pieces)
            _same_bits(got, want, fmt, f"{fmt} secure={secure} chunk={chunk}")
            assert np.array_equal(got, np.ascontiguousarray(whole).view(F.bits_dtype(fmt)))
            # whole elements, in model order, byte offsets running on across the shard boundary
            assert all(o % s == 0 and c % s == 0 and c > 0 for o, c in pieces)
            assert [o for o, _ in pieces] == list(np.cumsum([0] + [c for _, c in pieces[:-1]]))
            assert pieces[-1][0] + pieces[-1][1] == M * s
        # a sink that stops ends the call; the next call works
        seen = []

        def stop(ptr, off, cnt):
            seen.append(off)
            return False
        with pytest.raises(ipls.IplsError) as e:
            agg.GetPartitionsChunked(stop, chunk=1000, dtype=F.np_dtype(fmt))
        assert e.value.code == INVAL and seen == [0]
        _same_bits(_gather(agg, fmt, 1000, M * s), want, fmt, "after a stopped sink")
        with pytest.raises(ValueError):
            agg.GetPartitionsChunked(stop, wire=True, dtype=F.np_dtype(fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_snapshot_under_a_blocked_sink(ipls, O, fmt):
    """The sink is held at its first piece while another thread's
    cache_partition rewrites every partition: the call still delivers the
    model as of the call."""
    M, P = 10007, 3
    s = F.esize(fmt)
    rng = np.random.default_rng(33)
    with ipls.Aggregator(M, P, devices=[0, 0]) as agg:
        ws = _w_case(rng, list(agg.lengths), fmt)
        new = _w_case(rng, list(agg.lengths), fmt)
        for p in range(P):
            agg.cache_partition(p, ws[p])
        want, want_new = _narrow_model(O, ws, fmt, False), _narrow_model(O, new, fmt, False)
        assert not np.array_equal(want, want_new)
        done, errs = threading.Event(), []

        def rewrite():
            try:
                for p in range(P):
                    agg.cache_partition(p, new[p])
                agg.sync()
            except BaseException as e:   # noqa: BLE001
                errs.append(repr(e))
            done.set()
        t = threading.Thread(target=rewrite)
        out, n = bytearray(M * s), []

        def sink(ptr, off, cnt):
            if not n:
                t.start()
                assert done.wait(WAIT), "cache_partition waited for the blocked sink"
            n.append(off)
            out[off:off + cnt] = ctypes.string_at(ptr, cnt)
            return True
        agg.GetPartitionsChunked(sink, chunk=500, dtype=F.np_dtype(fmt))
        t.join(WAIT)
        assert not errs, errs
        _same_bits(np.frombuffer(bytes(out), dtype=F.bits_dtype(fmt)), want, fmt, "the model as of the call")
        _same_bits(_gather(agg, fmt, 500, M * s), want_new, fmt, "the next call sees the rewrite")


def test_concurrent_chunked_arrivals(ipls, O):
    """Four threads, two per partition, each sending three chunked arrivals
    (f32, bf16 and f64 mixed, random chunk sizes).  An arrival is one unit, so
    each partition ends as one interleaving of its two threads' sequences: the
    result must equal the oracle's fold in one of those serial orders."""
    b, G = _shape(ipls, "f32")
    L, P, T, n_arr = G + 4 * b + 1, 2, 4, 3
    chunks = (2, 510, 2 * b, L + 1, 1 << 16)
    plan = {}
    for tid in range(T):
        rng = np.random.default_rng(900 + tid)
        seq = []
        for i in range(n_arr):
            fmt = ("f32", "bf16", "f64")[int(rng.integers(0, 3))]
            if fmt == "f64":
                g = rng.standard_normal(L)
                seq.append((fmt, g, g, int(rng.choice(chunks))))
            else:
                x = F.bucket(rng, L, fmt)
                seq.append((fmt, x, F.widen(x, fmt), int(rng.choice(chunks))))
        plan[tid] = seq
    errs = []
    with ipls.Aggregator(n_partitions=P, bucket_len=L, devices=[0, 0]) as agg:
        def worker(tid):
            try:
                p = tid % P
                for fmt, data, _, chunk in plan[tid]:
                    s = 8 if fmt == "f64" else F.esize(fmt)
                    raw = np.ascontiguousarray(data)

                    def src(dst, off, cnt, raw=raw, s=s):
                        ctypes.memmove(dst, raw.ctypes.data + off * s, cnt * s)
                        return True
                    if fmt == "f64":
                        agg.UpdateChunked(p, L, src, big_endian=False, chunk=chunk)
                    else:
                        agg.UpdateChunked(p, L, src, chunk=chunk, dtype=F.np_dtype(fmt))
            except BaseException as e:   # noqa: BLE001 -- reported by the main thread
                errs.append((tid, repr(e)))
        ths = [threading.Thread(target=worker, args=(tid,)) for tid in range(T)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(60)
        assert not errs, errs
        for p in range(P):
            a, c = [w for _, _, w, _ in plan[p]], [w for _, _, w, _ in plan[p + P]]
            got = agg.read(p).view(np.uint64)
            orders = set()
            for pos in itertools.combinations(range(2 * n_arr), n_arr):
                ia, ic, seq = iter(a), iter(c), []
                for i in range(2 * n_arr):
                    seq.append(next(ia) if i in pos else next(ic))
                orders.add(O.reduce(seq, L, O.START_ZERO).view(np.uint64).tobytes())
            assert len(orders) > 1, "the serial orders must be told apart"
            assert got.tobytes() in orders, f"partition {p} matches no serial order of its arrivals"
