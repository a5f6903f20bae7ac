"""The unfused round at the seams: k_finalize, k_divide and the big-endian outputs, bit for bit.

What the Java-facing API and both Middleware servers run every iteration:
AggregatePartition -> finalize_range -> k_finalize (W = AGG + REP),
GetPartitions -> divide_range -> k_divide (the averaged flat model, native or
as writeDouble bytes), the big-endian sums through launch_bswap, and the
unfused fallback of aggregate_round, which calls the first two on a
sub-range.  Inputs and seams: tests/unfused_cases.py (special values on every
seam of every head, rotated by partition; tests/test_unfused_cases.py shows on
the CPU that they tell a wrong kernel from a right one).  The oracle is the
reference here: O.divide, O.get_partitions, O.be_encode,
O.be_encode_canonical, O.reduce and plain agg + rep.  (Division of labour:
production sizes in test_gpu_shapes.py, the fold kernels' seams in
test_gpu_wide_small.py, the unfused round's seams here.)

How bits are compared (unfused_cases.same):
  * little-endian quotients by assert_bits_equal's rule: NaN meets NaN (the
    payload of NaN / cnt is not specified);
  * pass-through partitions (count +0.0 or -0.0), W, the sums and their
    big-endian bytes raw, the payload of the inputs' one NaN included: a
    single NaN operand goes through v_add_f64 unchanged;
  * wire bytes exactly as O.be_encode_canonical gives them;
  * one exception to raw: a NaN that no input holds (inf + -inf of the
    accumulator pairs, or a bucket's +inf meeting another's -inf) is generated
    by the adder, and neither Java nor IEEE 754 fixes the sign or payload of a
    generated NaN (x86, where the oracle runs, sets its sign bit): there NaN
    meets NaN.

Caller-owned device outputs lie between guard bands of 64 sentinels (a
signalling NaN that no result can take) at every offset a past a 128-B line,
are fetched whole with one copy and compared in full; both bands stay intact.

What the geometry forbids:
  * the chunk rule (IPLS.java:1019-1028) shortens only the last partition, by
    at most P elements, so the lengths 4095, 4096, 4097, 2 * 4096 + 1 and 1
    cannot stand in one handle of five partitions.  Four model handles
    (unfused_cases.FINALIZE_MODELS) hold them: 4097 x 4 + 4095, 4097 x 4 +
    4096, 8193 x 4 + 8192 and 2 x 4 + 1.  In each, tiles_per_part comes from
    the long partitions and the short last one leaves early (base >= len).
  * AggregatePartition consumes AGG and REP, so one partition gets one kind of
    single-partition call per pass: three passes, re-planted, give every
    partition the big-endian sum, the native sum and the average.
"""
import ctypes

import numpy as np
import pytest

import unfused_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD, SENTINEL = C.GUARD, C.SENTINEL


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


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def dev_bits(a):
    """Host doubles -> int64 device tensor of their bits."""
    return torch.from_numpy(C.bits(a).view(np.int64).copy()).to("cuda")


def check(got, want, what, raw=True):
    """`raw`: a bool, or a mask per element (True: raw bits, False: NaN meets NaN)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if isinstance(raw, (bool, np.bool_)):
        ok = C.same(got, want, bool(raw))
    else:
        ok = np.where(raw, C.same(got, want, True), C.same(got, want, False))
    bad = np.flatnonzero(~ok)
    assert not bad.size, (f"{what}: {bad.size} of {got.size} elements differ; first at {bad[0]}: "
                          f"{C.bits(got)[bad[0]]:#018x} != {C.bits(want)[bad[0]]:#018x}")


def from_be(data):
    """Big-endian bytes -> the doubles, bits untouched."""
    return np.frombuffer(bytes(data), dtype=np.uint64).byteswap().view(np.float64)


class Guarded:
    """A device buffer of `M` doubles at `a` elements past a 128-B line, 64 sentinels before and after."""

    def __init__(self, M):
        self.M = M
        self.t = torch.empty(GUARD + C.LINE + M + GUARD, dtype=torch.int64, device="cuda")
        assert int(self.t.data_ptr()) % 128 == 0

    def at(self, ipls, a):
        self.a = a
        self.t.fill_(SENTINEL)
        torch.cuda.synchronize()   # the fill ran on torch's stream; the handle's does not order after it
        return ipls.DeviceBuffer(int(self.t.data_ptr()) + 8 * (GUARD + a), self.M)

    def fetch(self, what):
        """The M values (one copy of the whole buffer); asserts both bands."""
        torch.cuda.synchronize()
        h = self.t.cpu().numpy().view(np.uint64)
        lo = GUARD + self.a
        assert (h[:lo] == SENTINEL).all(), f"{what}: the band before the output was written"
        assert (h[lo + self.M:] == SENTINEL).all(), f"{what}: the band after the output was written"
        return h[lo:lo + self.M].view(np.float64)


class Sink:
    """Chunk sink of the *Chunked calls: keeps the 8-byte words and the (offset, count) of every call."""

    def __init__(self, n):
        self.words, self.calls, self.n = np.zeros(n, dtype=np.uint64), [], n

    def __call__(self, ptr, off, cnt):
        assert 0 <= off and off + cnt <= self.n and cnt > 0
        self.words[off:off + cnt] = np.frombuffer(ctypes.string_at(ptr, 8 * cnt), dtype=np.uint64)
        self.calls.append((off, cnt))
        return True

    def tiled(self, chunk, what):
        """The calls tile [0, n) in order, none longer than the chunk."""
        pos = 0
        for off, cnt in self.calls:
            assert off == pos and cnt <= chunk, f"{what}: chunk ({off}, {cnt}) after {pos}, chunk size {chunk}"
            pos += cnt
        assert pos == self.n, f"{what}: chunks end at {pos} of {self.n}"


def open_handle(ipls, case, secure, devices=None):
    if "model" in case:
        return ipls.Aggregator(case["model"][0], case["model"][1], secure=secure, devices=devices)
    return ipls.Aggregator(n_partitions=case["P"], bucket_len=case["L"], secure=secure, devices=devices)


class Div:
    """A handle whose W is planted with cache_partition, and the oracle's flat model of it."""

    def __init__(self, ipls, O, name, secure, devices=None):
        self.ipls, self.O, self.name, self.secure = ipls, O, name, secure
        case = C.divide_cases()[name]
        self.lens, self.offs, self.M = C.case_geometry(case)
        self.W = C.case_weights(name, case, secure)
        self.agg = open_handle(ipls, case, secure, devices)
        assert (self.agg.lengths, self.agg.offsets, self.agg.flat_size) == (self.lens, self.offs, self.M)
        for p, w in enumerate(self.W):
            self.agg.cache_partition(p, w)
        with np.errstate(all="ignore"):
            self.want = O.get_partitions(self.W, secure)
            self.want32 = self.want.astype(np.float32)
        assert self.want.size == self.M
        # pass-through partitions compare raw, NaN payload included
        self.raw = np.concatenate([np.full(L - 1, bool(c == 0.0)) for L, c in zip(self.lens, case["counts"])])
        self.wire = O.be_encode_canonical(self.want)
        self.out = Guarded(self.M)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.agg.close()
        self.out = None

    def what(self, s):
        return f"{self.name} secure={self.secure} devices={self.agg.devices}: {s}"

    def device(self, a):
        self.agg.GetPartitions(out=self.out.at(self.ipls, a))
        self.agg.sync()
        check(self.out.fetch(self.what(f"a={a}")), self.want, self.what(f"device output at a={a}"), self.raw)

    def host(self):
        check(self.agg.GetPartitions(), self.want, self.what("GetPartitions()"), self.raw)

    def host_wire(self):
        assert self.agg.GetPartitions(wire=True) == self.wire, self.what("GetPartitions(wire=True)")

    def pinned(self):
        pb = self.ipls.PinnedBuffer(8 * max(self.M, 1))
        try:
            pb.view()[:] = 0x5A
            got = self.agg.GetPartitions(out=pb)
            check(np.array(got), self.want, self.what("GetPartitions(out=PinnedBuffer)"), self.raw)
            pb.view()[:] = 0x5A
            got = self.agg.GetPartitions(out=pb, wire=True)
            assert bytes(got) == self.wire, self.what("GetPartitions(out=PinnedBuffer, wire=True)")
        finally:
            pb.close()

    def chunked(self, chunk, wire):
        s = Sink(self.M)
        self.agg.GetPartitionsChunked(s, wire=wire, chunk=chunk)
        what = self.what(f"GetPartitionsChunked(chunk={chunk}, wire={wire})")
        s.tiled(chunk, what)
        if wire:
            assert s.words.tobytes() == self.wire, what
        else:
            check(s.words.view(np.float64), self.want, what, self.raw)

    def f32(self):
        """The narrow twin on the same W: the f64 result rounded once to float."""
        got = self.agg.GetPartitions(dtype=np.float32)
        g, w = got.view(np.uint32), self.want32.view(np.uint32)
        bad = np.flatnonzero((g != w) & ~(np.isnan(got) & np.isnan(self.want32)))
        assert not bad.size, self.what(f"dtype=float32: {bad.size} differ; first at {bad[0]}: "
                                       f"{g[bad[0]]:#010x} != {w[bad[0]]:#010x}")


# ---------------------------------------------------------------------------
# a. k_divide, device output, every head
# ---------------------------------------------------------------------------
def _offsets(name):
    if name.startswith("p17"):
        return range(C.LINE)
    return (0, 1, 15) if name.startswith("p3") else (0, 5)


@pytest.mark.parametrize("secure", [False, True], ids=["plain", "secure"])
@pytest.mark.parametrize("name", list(C.divide_cases()))
def test_divide_device(ipls, O, name, secure):
    """GetPartitions into a DeviceBuffer at every offset a past a 128-B line.
    p17-*: the flat offsets p * (L - 1) take every residue mod 16, so with a =
    0 .. 15 every partition's output meets every head; L - 1 = 17 stays below
    a tile, 2049 is one whole tile with a head or a tail, 2 * 2048 + 17 two
    tiles.  p3-*: lengths around a line and a tile at a = 0, 1, 15.  model:
    Aggregator(30011, 3), a short last partition.  count: Aggregator(7, 8),
    the last partition holds the count slot only (n = 0).  Every partition
    has another count slot (unfused_cases.COUNTS)."""
    with Div(ipls, O, name, secure) as d:
        if name.startswith("p17"):
            assert sorted(o % C.LINE for o in d.offs[:C.LINE]) == list(range(C.LINE))
        if name == "count":
            assert d.lens[-1] == 1
        for a in _offsets(name):
            d.device(a)


# ---------------------------------------------------------------------------
# b. k_divide, host and wire
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("secure", [False, True], ids=["plain", "secure"])
@pytest.mark.parametrize("name", [n for n in C.divide_cases() if n.startswith("p17")])
def test_divide_host_and_wire(ipls, O, name, secure):
    """The three host calls and the two chunked ones on the P = 17 handles:
    the library's scratch is line aligned, so the heads are the residues of
    the partitions' own offsets -- every one, for OUT_BE x SECURE.  Chunks of
    2, of 2050 and of more than M tile [0, M) and carry the same bits.
    GetPartitions(dtype=float32) equals the f64 result narrowed once."""
    with Div(ipls, O, name, secure) as d:
        d.host()
        d.host_wire()
        d.pinned()
        for chunk in (2, 2050, (d.M + 3) // 2 * 2):
            d.chunked(chunk, wire=False)
            d.chunked(chunk, wire=True)
        d.f32()


# ---------------------------------------------------------------------------
# c. several shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("secure", [False, True], ids=["plain", "secure"])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2shards", "3shards"])
def test_divide_shards(ipls, O, devices, secure):
    """P = 17, L - 1 = 2049 over two and three shards on one GPU: every shard
    writes its own segment of the output (out + 8 * off[first partition of the
    shard]), so its heads differ from the one-shard run's; the result does not."""
    name = "p17-2049"
    with Div(ipls, O, name, secure) as one, Div(ipls, O, name, secure, devices) as d:
        assert len(set(ipls.shard_plan(17, len(devices)))) == len(devices)
        ref = one.agg.GetPartitions()
        for a in (0, 3):
            d.device(a)
            got = d.out.fetch("shards")
            assert np.array_equal(C.bits(got), C.bits(ref)), d.what(f"device output a={a} != the one-shard result")
        d.host()
        assert np.array_equal(C.bits(d.agg.GetPartitions()), C.bits(ref)), d.what("host != the one-shard result")
        d.host_wire()
        assert d.agg.GetPartitions(wire=True) == one.agg.GetPartitions(wire=True)
        d.chunked(2050, wire=True)
        d.chunked(2050, wire=False)


# ---------------------------------------------------------------------------
# d. k_finalize
# ---------------------------------------------------------------------------
class Fin:
    """A model handle of five ragged partitions with AGG and REP planted raw
    (a START_FIRST fold of one device bucket is an exact copy) and W filled
    with a value that no result equals."""

    def __init__(self, ipls, O, name, secure=False, devices=None):
        self.ipls, self.O, self.name, self.secure = ipls, O, name, secure
        M, P = C.FINALIZE_MODELS[name]
        self.agg = ipls.Aggregator(M, P, secure=secure, devices=devices)
        self.lens = self.agg.lengths
        assert self.lens == C.FINALIZE_LENGTHS[name]
        self.P = P
        self.a, self.r = C.finalize_inputs(name)
        self.da, self.dr = [dev_bits(x) for x in self.a], [dev_bits(x) for x in self.r]
        assert all(int(t.data_ptr()) % 16 == 0 for t in self.da + self.dr)
        torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.agg.close()

    def plant(self, mode):
        """-> the expected W per partition."""
        ipls, agg = self.ipls, self.agg
        agg.reset()
        present = C.REP_MODES[mode]
        want = []
        for p, L in enumerate(self.lens):
            agg.cache_partition(p, np.full(L, 7.25))
            agg.reduce_batch(p, [[ipls.DeviceBuffer(int(self.da[p].data_ptr()), L)]], start_mode=ipls.START_FIRST)
            if p in present:
                agg.reduce_batch(p, [[ipls.DeviceBuffer(int(self.dr[p].data_ptr()), L)]],
                                 start_mode=ipls.START_FIRST, target=ipls.TGT_REP)
            with np.errstate(all="ignore"):
                want.append(self.a[p] + (self.r[p] if p in present else 0.0))
        for p in range(self.P):   # planted raw: -0.0 and the NaN payload are in place
            check(agg.read(p), self.a[p], f"{self.name}/{mode}: planted AGG[{p}]")
            if p in present:
                check(agg.read(p, ipls.TGT_REP), self.r[p], f"{self.name}/{mode}: planted REP[{p}]")
        return want

    def after(self, want, what, parts=None):
        """W and Weight_Address equal agg + rep raw; AGG and REP read as +0.0."""
        ipls, agg = self.ipls, self.agg
        for p in range(self.P) if parts is None else parts:
            check(agg.read(p, ipls.TGT_WEIGHTS), want[p], f"{what}: W[{p}]")
            check(agg.read(p, ipls.TGT_WADDR), want[p], f"{what}: Weight_Address[{p}]")
            assert from_be(agg.read(p, ipls.TGT_WEIGHTS, big_endian=True)).tobytes() == \
                agg.read(p, ipls.TGT_WEIGHTS).tobytes(), f"{what}: big-endian read of W[{p}]"
            for tgt in (ipls.TGT_AGG, ipls.TGT_REP):
                assert not C.bits(agg.read(p, tgt)).any(), f"{what}: target {tgt} of {p} is not +0.0 afterwards"

    def model_and_refill(self, want, what):
        """GetPartitions equals the oracle's; then one Update into each
        accumulator gives 0.0 + x: the arena still holds the old AGG and REP,
        which must not show."""
        ipls, O, agg = self.ipls, self.O, self.agg
        with np.errstate(all="ignore"):
            model = O.get_partitions(want, self.secure)
        raw = np.concatenate([np.full(len(w) - 1, bool(w[-1] == 0.0)) for w in want])
        check(agg.GetPartitions(), model, f"{what}: GetPartitions", raw)
        assert agg.GetPartitions(wire=True) == O.be_encode_canonical(model), f"{what}: wire"
        for p in range(self.P):
            agg.Update(self.r[p], p)
            agg.Update(self.a[p], p, from_clients=False)
        for p in range(self.P):
            check(agg.read(p), 0.0 + self.r[p], f"{what}: AGG[{p}] after one Update")
            check(agg.read(p, ipls.TGT_REP), 0.0 + self.a[p], f"{what}: REP[{p}] after one Update")

    def all_at_once(self, mode):
        want = self.plant(mode)
        self.agg.AggregatePartition(self.ipls.ALL_PARTITIONS)
        what = f"{self.name}/{mode} secure={self.secure} devices={self.agg.devices} ALL_PARTITIONS"
        self.after(want, what)
        self.model_and_refill(want, what)

    def one_by_one(self, mode, passes=(0, 1, 2)):
        O, agg = self.O, self.agg
        for k in passes:
            want = self.plant(mode)
            what = f"{self.name}/{mode} secure={self.secure} devices={agg.devices} single calls, pass {k}"
            for p in range(self.P):
                kind = (p + k) % 3
                if kind == 0:      # the update_file bytes (k_bswap64)
                    s, _ = agg.AggregatePartition(p, with_sum=True, sum_big_endian=True)
                    check(from_be(s), from_be(O.be_encode(want[p])), f"{what}: big-endian sum of {p}")
                elif kind == 1:
                    s, _ = agg.AggregatePartition(p, with_sum=True, sum_big_endian=False)
                    check(s, want[p], f"{what}: sum of {p}")
                else:              # divide_range(p, 1) into scratch
                    _, a = agg.AggregatePartition(p, with_average=True)
                    with np.errstate(all="ignore"):
                        check(a, O.divide(want[p], self.secure), f"{what}: average of {p}", bool(want[p][-1] == 0.0))
                self.after(want, what, [p])
            self.model_and_refill(want, what)


@pytest.mark.parametrize("mode", list(C.REP_MODES))
@pytest.mark.parametrize("name", list(C.FINALIZE_MODELS))
def test_finalize(ipls, O, name, mode):
    """W = AGG + REP over ragged lengths around the tile of 4096, with REP
    logically zero everywhere (k_finalize<true, ..>), present in one partition
    only (every REP is materialised, k_finalize<false, ..> over the batch; the
    single call on a partition without REP still runs the REP_ZERO form) and
    present everywhere; by AggregatePartition(ALL_PARTITIONS) and by single
    calls with the big-endian sum, the native sum and the average."""
    with Fin(ipls, O, name) as f:
        f.all_at_once(mode)
        f.one_by_one(mode)


@pytest.mark.parametrize("mode", ["none", "all"])
def test_finalize_secure(ipls, O, mode):
    """The same with the secure divisor behind it (with_average, GetPartitions)."""
    with Fin(ipls, O, "last4095", secure=True) as f:
        f.all_at_once(mode)
        f.one_by_one(mode)


def test_finalize_chunked(ipls, O):
    """AggregatePartitionChunked in both byte orders, with chunks of 2 and one chunk larger than L."""
    with Fin(ipls, O, "last4095") as f:
        want = f.plant("all")
        for p, (be, chunk) in enumerate([(True, 2), (False, 2), (True, 8192), (False, 8192), (True, 2)]):
            s = Sink(f.lens[p])
            f.agg.AggregatePartitionChunked(p, s, big_endian=be, chunk=chunk)
            what = f"AggregatePartitionChunked({p}, big_endian={be}, chunk={chunk})"
            s.tiled(chunk, what)
            assert len(s.calls) == (1 if chunk > f.lens[p] else -(-f.lens[p] // 2))
            if be:
                check(from_be(s.words.tobytes()), from_be(O.be_encode(want[p])), what)
            else:
                check(s.words.view(np.float64), want[p], what)
            f.after(want, what, [p])
        f.model_and_refill(want, "after the chunked calls")


def test_finalize_shards(ipls, O):
    """REP in one partition, the handle over two shards of one GPU."""
    with Fin(ipls, O, "last4095", devices=[0, 0]) as f:
        f.all_at_once("one")
        f.one_by_one("one", passes=(0, 2))


# ---------------------------------------------------------------------------
# e. the unfused fallback of aggregate_round
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("secure", [False, True], ids=["plain", "secure"])
def test_round_fallback(ipls, O, secure):
    """Device buckets at 8 mod 16 (frames at odd offsets) on the sub-range 1
    .. 3 of five partitions, AGG pre-filled in one partition and REP in
    another: the fold runs k_reduce_scalar (the launch record shows that the
    fused kernel did not run), then finalize_range and divide_range on the
    sub-range.  Averages into a device buffer at a = 0 and 7 with bands, and
    to the host.  W and the averages equal the oracle's, and the fused call's
    on 16-B aligned copies of the same buckets."""
    F = C.FALLBACK
    P, L, K, p0, n = F["P"], F["L"], F["K"], F["p_first"], F["n_parts"]
    rows, a0, r0 = C.fallback_inputs()
    odd = [[torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), dev_bits(b)]) for b in bk] for bk in rows]
    even = [[dev_bits(b) for b in bk] for bk in rows]
    da, dr = dev_bits(a0), dev_bits(r0)
    torch.cuda.synchronize()
    tab_odd = [[ipls.DeviceBuffer(int(t.data_ptr()) + 8, L) for t in bk] for bk in odd]
    tab_even = [[ipls.DeviceBuffer(int(t.data_ptr()), L) for t in bk] for bk in even]
    assert all(d.ptr % 16 == 8 for r in tab_odd for d in r) and all(d.ptr % 16 == 0 for r in tab_even for d in r)
    W, avg = [], []
    with np.errstate(all="ignore"):
        for q in range(n):
            p = p0 + q
            s = O.reduce(rows[q], L, O.START_ACCUM, acc=a0 if p == F["agg_in"] else np.zeros(L))
            w = s + (r0 if p == F["rep_in"] else 0.0)
            W.append(w)
            avg.append(O.divide(w, secure))
    avg = np.concatenate(avg)
    n_avg = n * (L - 1)
    out = Guarded(n_avg)
    seen = {}
    with ipls.Aggregator(n_partitions=P, bucket_len=L, secure=secure) as agg:
        for fused, tab in ((False, tab_odd), (True, tab_even)):
            for a in (0, 7, None):
                what = f"aggregate_round fused={fused} secure={secure} averages at {'the host' if a is None else a}"
                agg.reset()
                for p in range(P):
                    agg.cache_partition(p, np.full(L, 7.25))
                agg.reduce_batch(F["agg_in"], [[ipls.DeviceBuffer(int(da.data_ptr()), L)]], start_mode=ipls.START_FIRST)
                agg.reduce_batch(F["rep_in"], [[ipls.DeviceBuffer(int(dr.data_ptr()), L)]], start_mode=ipls.START_FIRST,
                                 target=ipls.TGT_REP)
                if a is None:
                    got = agg.aggregate_round(p0, tab)
                else:
                    agg.aggregate_round(p0, tab, out=out.at(ipls, a))
                li = agg.last_launch()
                if fused:
                    assert li["kernel"] == ipls.KERNEL_ROUND, li
                else:
                    rec = {f: li[f] for f in ("kernel", "block", "vectors", "map", "grid", "be_in", "be_out", "start")}
                    assert rec == dict(kernel=ipls.KERNEL_REDUCE_SCALAR, block=256, vectors=1, map=0,
                                       grid=-(-L // 2048) * n, be_in=0, be_out=0, start=ipls.START_ACCUM), rec
                if a is not None:
                    agg.sync()
                    got = out.fetch(what)
                check(got, avg, f"{what}: averages", raw=False)
                ws = [agg.read(p0 + q, ipls.TGT_WEIGHTS) for q in range(n)]
                for q in range(n):
                    check(ws[q], W[q], f"{what}: W[{p0 + q}]")
                    for tgt in (ipls.TGT_AGG, ipls.TGT_REP):
                        assert not C.bits(agg.read(p0 + q, tgt)).any(), f"{what}: target {tgt} of {p0 + q} not +0.0"
                for p in (0, P - 1):   # outside the sub-range nothing moved
                    assert (agg.read(p, ipls.TGT_WEIGHTS) == 7.25).all(), f"{what}: W[{p}] outside the sub-range"
                seen[(fused, a)] = (C.bits(got).copy(), [C.bits(w).copy() for w in ws])
    for a in (0, 7, None):   # the fused call's bits on aligned copies of the same buckets
        assert np.array_equal(seen[(False, a)][0], seen[(True, a)][0]), f"averages at {a}: unfused != fused"
        for q in range(n):
            assert np.array_equal(seen[(False, a)][1][q], seen[(True, a)][1][q]), f"W[{p0 + q}] at {a}: unfused != fused"
