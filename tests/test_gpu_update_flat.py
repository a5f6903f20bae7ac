"""UpdateGradientChunked on the GPU (ipls_agg_update_gradient_chunked, one
launch of k_update_flat per shard): one whole flat gradient, streamed, applied
to every owned partition at one instant or not at all.  Expected values come
from the oracle alone (organize_gradients on the widened vector, then fold);
UpdateGradient of the same vector on a second handle must agree too.

Where a source has to stay blocked while another thread works, it waits for
that thread's event (bounded by a timeout that only a deadlock reaches) rather
than sleeping, the idiom of test_gpu_narrow_chunked.py.
"""
import ctypes
import threading

import numpy as np
import pytest

from conftest import assert_bits_equal
import narrow_fmt as F
import update_flat_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -2
WAIT = 20.0   # seconds; reached only when a call deadlocks
P = C.P_SWEEP
DEVICES = pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))


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


_TILE = {}


def _tile(ipls, kind):
    """The kernel's tile T for the kind, from one launch's record."""
    if kind not in _TILE:
        raw = C.from_doubles(np.ones(8), kind)
        with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
            agg.UpdateGradientChunked(8, _source(raw, kind), [0], **C.call_args(kind))
            li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_UPDATE_FLAT, li
        _TILE[kind] = li["block"] * (2 if C.esize(kind) == 8 else 4) * li["vectors"]
    return _TILE[kind]


def _source(raw, kind, calls=None, stop_at=None, gate=None):
    """A chunk source over the vector's bytes; records (offset, count); stops at
    call `stop_at`; after its first chunk waits for `gate` = (reached, go)."""
    s = C.esize(kind)
    raw = np.ascontiguousarray(raw)
    seen = [0]

    def src(dst, off, cnt):
        k = seen[0]
        seen[0] += 1
        if calls is not None:
            calls.append((off, cnt))
        if stop_at is not None and k == stop_at:
            return False
        ctypes.memmove(dst, raw.ctypes.data + off * s, cnt * s)
        if gate is not None and k == 0:
            gate[0].set()
            assert gate[1].wait(WAIT), "the other thread never got through: a lock is held while the source runs"
        return True
    return src


def _tiles(n, chunk, bounds=()):
    """The source calls that tile [0, n): at most chunk, cut at every bound."""
    out, pos = [], 0
    while pos < n:
        ln = min(chunk, n - pos)
        for b in bounds:
            if pos < b < pos + ln:
                ln = b - pos
        out.append((pos, ln))
        pos += ln
    return out


TARGETS = (0, 1, 2, 4)   # AGG, REP, W, FUT


def _state(agg):
    return [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in TARGETS]


def _preload(agg, rng, agg_too=False):
    """Something in REP, W and FUT (and AGG) of every partition, so that a stray write shows."""
    for p in range(P):
        L = agg.lengths[p]
        agg.Update(rng.standard_normal(L), p, from_clients=False)
        agg.cache_partition(p, rng.standard_normal(L))
        agg.Update(rng.standard_normal(L), p, from_future=True)
        if agg_too:
            agg.Update(rng.standard_normal(L), p)


def _check(agg, want_agg, others, what):
    for p in range(P):
        assert_bits_equal(agg.read(p), want_agg[p], f"{what} AGG[{p}]")
        for t in TARGETS[1:]:
            assert np.array_equal(agg.read(p, t).view(np.uint64), others[(p, t)]), f"{what}: target {t} of {p} changed"


def _others(agg):
    return {(p, t): agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in TARGETS[1:]}


def _host_operand(raw, kind):
    """The same vector as UpdateGradient takes it."""
    if kind in ("f64", "be"):
        return C.widen(raw.view(">u8" if kind == "be" else np.uint64).astype(np.uint64), kind)
    return F.host(torch, raw.view(F.bits_dtype(kind)), kind)


# ---- the residue sweep ----
@DEVICES
@pytest.mark.parametrize("kind", C.KINDS)
def test_residue_sweep(ipls, O, kind, devices):
    T = _tile(ipls, kind)
    for c in C.sweep_chunks(T):
        M = C.sweep_model_size(c)
        rng = np.random.default_rng(c)
        plant = C.sweep_plant(M, P, T)
        raw1, w1 = C.vector(rng, M, kind, plant)
        raw2, w2 = C.vector(rng, M, kind, plant[1:])
        want1 = C.expected(O, C.zeros(O, M, P), w1, M, M, P, range(P))
        want2 = C.expected(O, want1, w2, M, M, P, range(P))
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg, \
                ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as ref:
            assert [agg.partition_offset(p) % 8 for p in range(P)] == [p % 8 for p in range(P)]
            _preload(agg, rng)
            others = _others(agg)
            for raw, want, start in ((raw1, want1, ipls.START_ZERO), (raw2, want2, ipls.START_ACCUM)):
                calls = []
                agg.UpdateGradientChunked(M, _source(raw, kind, calls), range(P), chunk=1024, **C.call_args(kind))
                li = agg.last_launch()
                assert li["kernel"] == ipls.KERNEL_UPDATE_FLAT and li["start"] == start, li
                assert li["be_in"] == (kind == "be"), li
                n_jobs = P if not devices else P - _second_shard(devices)
                blocks = -(-(c + 1) // T)
                assert li["grid"] == blocks * n_jobs, ("one launch per shard", li, blocks, n_jobs)
                # the last partition copies c - 9 values: a full tile exactly when c - 9 >= T
                assert li["seqf"] == (1 if c - 9 >= T else 0), li
                assert calls == _tiles(M, 1024, _bounds(devices, c)), calls[:6]
                _check(agg, want, others, f"{kind} c={c} start={start}")
                ref.UpdateGradient(_host_operand(raw, kind), range(P))
                for p in range(P):
                    assert np.array_equal(ref.read(p).view(np.uint64), agg.read(p).view(np.uint64)), \
                        f"{kind} c={c}: UpdateGradient differs in partition {p}"


def _second_shard(devices):
    """First partition of the second shard of a two-shard handle of P partitions."""
    if not devices:
        return P
    from ipls.aggregator import shard_plan
    return shard_plan(P, len(devices)).index(1)


def _bounds(devices, c):
    return () if not devices else (_second_shard(devices) * c,)


# ---- short and long vectors ----
@pytest.mark.parametrize("kind", ("be", "f32", "bf16"))
def test_short_and_long_vectors(ipls, O, kind):
    T = _tile(ipls, kind)
    c = T + 9
    M = C.sweep_model_size(c)
    rng = np.random.default_rng(3)
    raw, w = C.vector(rng, M, kind, C.sweep_plant(M, P, T))
    neg = torch.full((c + 1,), -0.0, dtype=torch.float64, device="cuda")
    for n in (6 * c + 5, 6 * c + T + 3, 7 * c, 0):   # inside partition 6 (before / after its seam), at 7's start, nothing
        with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
            # AGG = -0.0 everywhere (FIRST of a -0.0 bucket): the zeros above the count slot make it +0.0
            agg.reduce_batch(0, [[ipls.DeviceBuffer.from_tensor(neg[:agg.lengths[p]])] for p in range(P)],
                             start_mode=ipls.START_FIRST)
            start = [agg.read(p).copy() for p in range(P)]
            assert all(np.signbit(a).all() for a in start)
            calls = []
            agg.UpdateGradientChunked(n, _source(raw, kind, calls), range(P), chunk=4096, **C.call_args(kind))
            assert calls == _tiles(n, 4096)
            want = C.expected(O, start, w, n, M, P, range(P))
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{kind} n={n} AGG[{p}]")
            tail = agg.read(8)
            assert not np.signbit(tail).any() and tail[0] == 1.0, "the tail above the count slot was skipped"
            if n == 7 * c:
                assert agg.read(7)[0] == 1.0 and not agg.read(7)[1:].any()
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        before = _state(agg)
        calls = []
        big = np.zeros((M + 2) * C.esize(kind), dtype=np.uint8)
        with pytest.raises(ipls.IplsError) as e:
            agg.UpdateGradientChunked(M + 1, _source(big, kind, calls), range(P), **C.call_args(kind))
        assert e.value.code == RANGE and calls == []
        assert all(np.array_equal(a, b) for a, b in zip(_state(agg), before))


# ---- owned subsets ----
@DEVICES
def test_owned_subsets(ipls, O, devices):
    kind = "f32"
    T = _tile(ipls, kind)
    c = T + 9
    M = C.sweep_model_size(c)
    rng = np.random.default_rng(4)
    raw, w = C.vector(rng, M, kind, C.sweep_plant(M, P, T))
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, rng, agg_too=True)
        for owned in ([1, 3], [8], [], [4, 4]):
            before = [agg.read(p).copy() for p in range(P)]
            others = _others(agg)
            calls = []
            agg.UpdateGradientChunked(M, _source(raw, kind, calls), owned, chunk=2048, **C.call_args(kind))
            assert calls == (_tiles(M, 2048, _bounds(devices, c)) if owned else []), (owned, calls[:4])
            want = C.expected(O, before, w, M, M, P, owned)
            _check(agg, want, others, f"owned={owned}")
            for p in set(range(P)) - set(owned):
                assert np.array_equal(agg.read(p).view(np.uint64), before[p].view(np.uint64)), (owned, p)
        # [4, 4] is two folds
        twice = C.expected(O, C.expected(O, before, w, M, M, P, [4]), w, M, M, P, [4])
        assert_bits_equal(agg.read(4), twice[4], "[4, 4]")


# ---- chunk edges ----
@DEVICES
@pytest.mark.parametrize("kind", ("f64", "half"))
def test_chunk_edges(ipls, O, kind, devices):
    c = 41   # 1 mod 8; small, so chunk = 2 stays quick
    M = C.sweep_model_size(c)
    rng = np.random.default_rng(6)
    raw, w = C.vector(rng, M, kind, (0, 1, c - 1, c, M - 1))
    bound = _bounds(devices, c)
    for n in (M, M - 1):   # M is even here: M - 1 is odd, the last chunk of 2 holds one element
        want = C.expected(O, C.zeros(O, M, P), w, n, M, P, range(P))
        # 2; one that straddles partition (and, at [0, 0], shard) boundaries; >= n
        for chunk in (2, 2 * (c // 2) + 2, M + 2):
            with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
                calls = []
                agg.UpdateGradientChunked(n, _source(raw, kind, calls), range(P), chunk=chunk, **C.call_args(kind))
                assert calls == _tiles(n, chunk, bound), (chunk, calls[:5])
                if bound and chunk > 2:
                    assert any(o + k == bound[0] for o, k in calls), "no chunk ends at the shard boundary"
                    assert _tiles(n, chunk) != calls, "the case never reached the split"
                for p in range(P):
                    assert_bits_equal(agg.read(p), want[p], f"{kind} n={n} chunk={chunk} AGG[{p}]")
    assert M % 2 == 0 and _tiles(M - 1, 2)[-1][1] == 1


# ---- all or nothing ----
@DEVICES
def test_all_or_nothing(ipls, O, devices):
    kind = "be"
    T = _tile(ipls, kind)
    c = T + 9
    M = C.sweep_model_size(c)
    rng = np.random.default_rng(7)
    raw, w = C.vector(rng, M, kind)
    chunk = 1024
    n_calls = len(_tiles(M, chunk, _bounds(devices, c)))
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, rng)               # AGG stays logically zero
        before = _state(agg)
        for stop in (0, n_calls // 2, n_calls - 1):
            calls = []
            with pytest.raises(ipls.IplsError) as e:
                agg.UpdateGradientChunked(M, _source(raw, kind, calls, stop_at=stop), range(P), chunk=chunk,
                                          **C.call_args(kind))
            assert e.value.code == INVAL and len(calls) == stop + 1
            assert all(np.array_equal(a, b) for a, b in zip(_state(agg), before)), f"stop at {stop} changed state"
        # the flags survived: a fold of a -0.0 bucket into the still logically-zero AGG gives +0.0
        for p in (0, P - 1):
            agg.Update(np.full(agg.lengths[p], -0.0), p)
            got = agg.read(p)
            assert not got.any() and not np.signbit(got).any(), f"partition {p}: the zero flag was lost"
        agg.reset()
        agg.UpdateGradientChunked(M, _source(raw, kind), range(P), chunk=chunk, **C.call_args(kind))
        want = C.expected(O, C.zeros(O, M, P), w, M, M, P, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"after the stops AGG[{p}]")


def test_refusals(ipls):
    from ipls import _native as N
    M = C.sweep_model_size(9)
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        lib, h = agg._lib, agg._h
        n_calls = []

        @N.CHUNK_SOURCE
        def cb(ctx, dst, off, cnt):
            n_calls.append((off, cnt))
            return 0
        own = (ctypes.c_int32 * 2)(0, 1)
        bad = (ctypes.c_int32 * 2)(0, P)
        before = _state(agg)
        f = lib.ipls_agg_update_gradient_chunked
        assert f(h, M, N.DEV_F64, own, 2, 4, cb, None) == INVAL          # bad kind
        assert f(h, M, N.HOST_FRAME, own, 2, 4, cb, None) == INVAL
        assert f(h, M, 99, own, 2, 4, cb, None) == INVAL
        assert f(h, M, N.HOST_BE, own, 2, 3, cb, None) == INVAL          # odd chunk
        assert f(h, M, N.HOST_BE, own, 2, 0, cb, None) == INVAL          # chunk < 2
        assert f(h, M, N.HOST_BE, own, 2, 4, None, None) == INVAL        # null source
        assert f(h, M, N.HOST_BE, bad, 2, 4, cb, None) == RANGE          # owned index out of range
        assert f(h, M + 1, N.HOST_BE, own, 2, 4, cb, None) == RANGE      # overrun
        assert f(h, M, N.HOST_BE, own, 0, 4, cb, None) == 0              # nothing owned: a no-op
        assert n_calls == []
        assert all(np.array_equal(a, b) for a, b in zip(_state(agg), before))
        with pytest.raises(ValueError):
            agg.UpdateGradientChunked(M, lambda *a: True, [0], dtype=np.int32)


# ---- no lock while the source runs, and the unit ----
@DEVICES
def test_no_lock_while_the_source_runs(ipls, O, devices):
    kind = "be"
    c = 41
    M = C.sweep_model_size(c)
    base, a, b = C.order_witness()
    wa = np.full(M, a)
    raw = C.from_doubles(wa, kind)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        Ls = agg.lengths
        for p in range(P):
            agg.Update(np.full(Ls[p], base), p)
        reached, go = threading.Event(), threading.Event()
        err = []

        def thread_a():
            try:
                agg.UpdateGradientChunked(M, _source(raw, kind, gate=(reached, go)), range(P), chunk=8,
                                          **C.call_args(kind))
            except BaseException as e:   # noqa: BLE001 -- reported by the main thread
                err.append(e)
        t = threading.Thread(target=thread_a)
        t.start()
        assert reached.wait(WAIT), "the source was never called"
        # A's source is blocked: folds into both shards and a read of the model all return
        for p in range(P):
            agg.Update(np.full(Ls[p], b), p)
        mid = agg.GetPartitions()
        assert mid.size == M
        go.set()
        t.join(WAIT)
        assert not t.is_alive() and not err, err
        start = [np.full(Ls[p], base) for p in range(P)]
        want = C.expected(O, [O.fold(s, np.full(len(s), b)) for s in start], wa, M, M, P, range(P))
        other = [O.fold(s, np.full(len(s), b)) for s in C.expected(O, [np.full(Ls[p], base) for p in range(P)],
                                                                     wa, M, M, P, range(P))]
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"(base + B) + A in partition {p}")
            if Ls[p] > 1:
                assert want[p][0] != other[p][0], "the other order would not show"


# ---- whole gradients serialise across partitions ----
def test_whole_gradients_serialise(ipls, O):
    c = 65
    M = C.sweep_model_size(c)
    base, grads, table = C.serial_witness(O, M, P)
    raws = [C.from_doubles(g, "f64") for g in grads]
    for rep in range(3):
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=[0, 0]) as agg:
            agg.UpdateGradient(base, range(P))
            go = threading.Barrier(len(grads))
            err = []

            def run(i):
                try:
                    go.wait(WAIT)
                    agg.UpdateGradientChunked(M, _source(raws[i], "f64"), range(P), chunk=16 + 2 * i,
                                              big_endian=False)
                except BaseException as e:   # noqa: BLE001
                    err.append(e)
            ts = [threading.Thread(target=run, args=(i,)) for i in range(len(grads))]
            for t in ts:
                t.start()
            for t in ts:
                t.join(WAIT)
            assert not err and not any(t.is_alive() for t in ts), err
            got = [agg.read(p).view(np.uint64) for p in range(P)]
        match = [o for o, want in table.items()
                 if all(np.array_equal(got[p], want[p].view(np.uint64)) for p in range(P))]
        assert len(match) == 1, f"repeat {rep}: {len(match)} of {len(table)} serial orders match all partitions"
