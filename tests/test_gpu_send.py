"""Aggregator.SendGradients (k_b64url_encode_flat) against the oracle, byte for byte.

Every case of tests/send_cases.py for each of the ten source kinds (host and
device memory x doubles, big-endian doubles, floats, halves, bfloat16s), to
host texts and to device texts.  The expectation is the oracle's restatement
alone (send_cases.oracle_text: organize_gradients, frame_encode,
java_b64url_encode over the source converted to float64 by numpy);
tests/test_send_cases.py shows on the CPU what the cases reach and that they
tell a wrong kernel from the right one.  Device sources lie between PAD junk
elements that no text may show; device texts between bands of 0xAB, and the
whole buffer is fetched and compared, bands and the gaps of a batch included.
"""
import functools

import numpy as np
import pytest

import codec_cases as C
import send_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL, GUARD, PAD = S.FILL, S.GUARD, S.PAD
KINDS = [(fmt, where) for fmt in S.FMTS for where in ("host", "dev")]
DTYPE = {"f64": "f64", "be": "f64", "f32": "f32", "f16": "half", "bf16": "bf16"}
CASES = S.all_cases()
MAX_TEXTS = max(C.batch_layout([C.text_len(c.frame_len(p)) for p in c.parts])[1] for c in CASES)


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


@pytest.fixture(scope="module")
def handles(ipls):
    """One handle per model geometry, shared by every test that only sends (the call changes no state)."""
    made = {}

    def get(M, P):
        if (M, P) not in made:
            made[(M, P)] = ipls.Aggregator(M, P)
            assert made[(M, P)].lengths == S.lengths(M, P)
        return made[(M, P)]

    yield get
    for a in made.values():
        a.close()


@functools.lru_cache(maxsize=None)
def _expected(case_name, fmt):
    from oracle import oracle as o
    case = next(c for c in CASES if c.name == case_name)
    return tuple(S.oracle_text(o, case, fmt, p) for p in case.parts)


def expected(case, fmt):
    """The oracle's texts of the case's listed partitions: computed once, shared, never changed."""
    return list(_expected(case.name, fmt))


def operand(ipls, case, fmt, where):
    """(keepalive, what SendGradients takes) for the case's source of the kind."""
    bits = S.source_bits(case, fmt)
    own = bits[PAD:PAD + case.n]
    if where == "host":
        if fmt == "be":
            return None, np.frombuffer(own.astype(">u8").tobytes(), dtype=np.uint8)
        if fmt == "bf16":
            return None, torch.from_numpy(own.view(np.int16).copy()).view(torch.bfloat16)
        return None, own.view({"f64": np.float64, "f32": np.float32, "f16": np.float16}[fmt]).copy()
    raw = np.frombuffer(S.source_bytes(bits, fmt), dtype=np.uint8).copy()
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, ipls.DeviceBuffer(t.data_ptr() + PAD * S.ESIZE[fmt], case.n, big_endian=fmt == "be", dtype=DTYPE[fmt])


def same_text(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        n = min(len(got), len(want))
        i = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: lengths {len(got)} / {len(want)}, first difference at char {i} "
                             f"(lane {i // S.GROUP_CHARS}): {got[max(0, i - 4):i + 8]!r} != {want[max(0, i - 4):i + 8]!r}")


class DeviceText:
    """A device byte buffer for texts of up to `cap` bytes between two bands of GUARD bytes, all FILL before a call."""

    def __init__(self, cap):
        self.t = torch.empty(GUARD + cap + 16 + GUARD, dtype=torch.uint8, device="cuda")
        assert int(self.t.data_ptr()) % 16 == 0 and GUARD % 16 == 0

    def at(self, shift=0):
        self.shift = shift
        self.t.fill_(FILL)
        torch.cuda.synchronize()   # the fill ran on torch's stream; the handle's does not order after it
        return int(self.t.data_ptr()) + GUARD + shift

    def check(self, agg, placed, what):
        """The whole buffer is FILL but for the texts [(offset, text)]."""
        agg.sync()
        got = self.t.cpu().numpy()
        want = np.full(got.size, FILL, dtype=np.uint8)
        lo = GUARD + self.shift
        for off, text in placed:
            want[lo + off:lo + off + len(text)] = np.frombuffer(text, dtype=np.uint8)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0]) - lo
            where = "before the first text" if i < 0 else f"at offset {i}"
            raise AssertionError(f"{what}: {bad.size} bytes differ, first {where}: {got[bad[0]]:#04x} != {want[bad[0]]:#04x}")


@pytest.fixture(scope="module")
def dev_text():
    return DeviceText(MAX_TEXTS)


def send_both(agg, dev_text, case, src, want, what, shifts=(0,)):
    """The call to host texts and to guarded device texts."""
    kw = dict(origin=case.origin, pid=case.pid)
    got = agg.SendGradients(src, case.parts, case.iteration, **kw)
    assert len(got) == len(want), what
    for p, g, t in zip(case.parts, got, want):
        same_text(g, t, f"{what}: host text of partition {p}")
    lens = [len(t) for t in want]
    offs, end = C.batch_layout(lens)
    for shift in shifts:
        addr = dev_text.at(shift)
        assert agg.SendGradients(src, case.parts, case.iteration, out=addr, out_cap=end, **kw) == (lens, offs), what
        dev_text.check(agg, list(zip(offs, want)), f"{what}: device texts at 16-B + {shift}")


# ---------------------------------------------------------------------------
# every case x every kind x both outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,where", KINDS, ids=[f"{w}-{f}" for f, w in KINDS])
def test_send_cases(ipls, handles, dev_text, fmt, where):
    for case in CASES:
        agg = handles(case.M, case.P)
        keep, src = operand(ipls, case, fmt, where)
        send_both(agg, dev_text, case, src, expected(case, fmt), f"{case} {where} {fmt}")
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_ENCODE_FLAT and li["be_in"] == (fmt == "be"), (case, li)
        assert li["grid"] % len(case.parts) == 0 and li["grid"] >= len(case.parts)
        assert li["seqf"] == int(any(case.fast(p) for p in case.parts)), (case, li)
        del keep


def test_unaligned_device_text(ipls, handles, dev_text):
    """A device text buffer one byte past a 16-B boundary goes through the scratch buffer and a copy."""
    for case in S.residue_cases() + S.short_cases() + S.tiny_cases()[:2]:
        keep, src = operand(ipls, case, "f32", "dev")
        send_both(handles(case.M, case.P), dev_text, case, src, expected(case, "f32"), f"{case} shifted", shifts=(1,))


def test_torch_tensors_and_pinned_output(ipls, handles):
    """A GPU tensor is read where it lies, a CPU tensor as a host vector; a PinnedBuffer takes host texts."""
    (case,) = S.residue_cases()
    agg = handles(case.M, case.P)
    for fmt, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16), ("f64", torch.float64)):
        own = S.source_bits(case, fmt)[PAD:PAD + case.n]
        signed = {2: np.int16, 4: np.int32, 8: np.int64}[S.ESIZE[fmt]]
        cpu = torch.from_numpy(own.view(signed).copy()).view(dt)
        want = expected(case, fmt)
        kw = dict(origin=case.origin, pid=case.pid)
        for t in (cpu, cpu.cuda()):
            torch.cuda.synchronize()
            got = agg.SendGradients(t, case.parts, case.iteration, **kw)
            for p, g, w in zip(case.parts, got, want):
                same_text(g, w, f"torch {fmt} {t.device.type}: partition {p}")
        lens = [len(t) for t in want]
        offs, end = C.batch_layout(lens)
        pin = ipls.PinnedBuffer(end + 64)
        v = pin.view()
        v[:] = FILL
        assert agg.SendGradients(cpu, case.parts, case.iteration, out=pin, **kw) == (lens, offs)
        ref = np.full(v.size, FILL, dtype=np.uint8)
        for o, t in zip(offs, want):
            ref[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
        assert (v == ref).all(), f"pinned texts of {fmt}"
        pin.close()


# ---------------------------------------------------------------------------
# the launch report, the null gradient, the size query
# ---------------------------------------------------------------------------
def test_last_launch(ipls, handles):
    (case,) = S.residue_cases()
    agg = handles(case.M, case.P)
    for fmt in S.FMTS:
        keep, src = operand(ipls, case, fmt, "dev")
        agg.SendGradients(src, case.parts, case.iteration)
        li = agg.last_launch()
        assert (li["kernel"], li["seqf"], li["block"], li["be_in"]) == (12, 1, 256, int(fmt == "be")), li
        assert li["grid"] % len(case.parts) == 0 and li["grid"] > 0
    tiny = S.all_tiny_case()
    agg = handles(tiny.M, tiny.P)
    keep, src = operand(ipls, tiny, "f64", "host")
    agg.SendGradients(src, tiny.parts, tiny.iteration)
    li = agg.last_launch()
    assert (li["kernel"], li["seqf"]) == (12, 0) and li["grid"] == len(tiny.parts), li


def send_raw(ipls, agg, ptr, n, kind, parts, iteration, pid, origin, out, cap, out_kind, lens=None, offs=None):
    parts = np.ascontiguousarray(parts, dtype=np.int32)
    o = np.frombuffer(bytes(origin), dtype=np.uint8)
    return ipls.lib().ipls_agg_send_gradients(agg.handle, ptr, n, kind, parts.ctypes.data, parts.size, iteration, pid,
                                              o.ctypes.data if o.size else None, o.size, out, cap, out_kind, lens, offs)


def test_null_gradient_and_size_query(ipls, O, handles, dev_text):
    for case in S.short_cases() + S.tiny_cases()[:1] + S.residue_cases():
        agg = handles(case.M, case.P)
        want = [S.null_text(case, p) for p in case.parts]
        for p, t in zip(case.parts, want):     # the model's null text is the oracle's Marshall_Packet(null, ...)
            assert t == O.java_b64url_encode(O.frame_encode(None, p, case.iteration, case.pid, case.origin))
        send_both(agg, dev_text, case, None, want, f"{case} null gradient", shifts=(0, 1))
        # out == NULL: the sizes alone, equal to what the real call returns, lays out and writes
        for fmt, texts in (("f32", expected(case, "f32")), (None, want)):
            src = None if fmt is None else operand(ipls, case, fmt, "host")[1]
            ptr, n, kind = (None, 0, ipls.HOST_F64) if src is None else (src.ctypes.data, src.size, ipls.HOST_F32)
            k = len(case.parts)
            lens, offs = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
            args = (ipls, agg, ptr, n, kind, case.parts, case.iteration, case.pid, case.origin)
            total = send_raw(*args, None, 0, ipls.HOST_TEXT, lens.ctypes.data, offs.ctypes.data)
            assert lens.tolist() == [len(t) for t in texts] and (offs.tolist(), total) == C.batch_layout(lens.tolist())
            buf = np.full(total + 1, FILL, dtype=np.uint8)
            l2, o2 = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
            assert send_raw(*args, buf.ctypes.data, total, ipls.HOST_TEXT, l2.ctypes.data, o2.ctypes.data) == total
            assert (l2 == lens).all() and (o2 == offs).all() and buf[total] == FILL
            for o, t in zip(offs.tolist(), texts):
                same_text(buf[o:o + len(t)].tobytes(), t, f"{case} raw call")


# ---------------------------------------------------------------------------
# the receiving side, the sender's state, two shards
# ---------------------------------------------------------------------------
def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("fmt", ["f64", "f32", "bf16"])
def test_round_trip_through_ingest(ipls, fmt):
    """The texts, ingested as one layer by a second handle, leave exactly the
    AGG bits that UpdateGradient of the same vector leaves on a third handle
    started from the same non-zero AGG."""
    M, P = S.SHORT_MODEL
    case = S.Case("round-trip", M, P, 333, range(P), 9)
    start = np.random.default_rng(7).standard_normal(M)
    _, src = operand(ipls, case, fmt, "host")
    with ipls.Aggregator(M, P) as sender, ipls.Aggregator(M, P) as rx, ipls.Aggregator(M, P) as own:
        rx.UpdateGradient(start, range(P))
        own.UpdateGradient(start, range(P))
        texts = sender.SendGradients(src, case.parts, case.iteration, origin=case.origin)
        k, st = rx.ingest_pubsub(texts, layers=1)
        assert (k, st) == (P, [0] * P)
        own.UpdateGradient(src, range(P))
        for p in range(P):
            a, b = u64(rx.read(p)), u64(own.read(p))
            assert (a == b).all(), f"{fmt}: partition {p} differs at {np.flatnonzero(a != b)[:4]}"
            assert np.isnan(rx.read(p)).any() or case.ncopy(p) == 0    # the planted NaN went through


def test_sender_state_is_untouched(ipls):
    """AGG, REP, W and FUT of every partition keep their checksums, and an
    arrival queued by UpdateAsync is still queued after the call: the fold
    that Wait then launches reads the bucket as it is at that time."""
    M, P = S.SHORT_MODEL
    case = S.Case("state", M, P, M, range(P), 3)
    rng = np.random.default_rng(11)
    targets = (ipls.TGT_AGG, ipls.TGT_REP, ipls.TGT_WEIGHTS, ipls.TGT_FUTURE)
    with ipls.Aggregator(M, P) as agg:
        agg.UpdateGradient(rng.standard_normal(M), range(P))
        for p in range(P):
            L = agg.lengths[p]
            agg.Update(rng.standard_normal(L), p, from_clients=False)
            agg.Update(rng.standard_normal(L), p, from_future=True)
            agg.cache_partition(p, rng.standard_normal(L))
        before = {(p, t): agg.checksum(p, t) for p in range(P) for t in targets}
        agg0 = agg.read(1).copy()
        L = agg.lengths[1]
        first, second = rng.standard_normal(L), rng.standard_normal(L)
        bucket = torch.from_numpy(first.copy()).cuda()
        torch.cuda.synchronize()
        ticket = agg.UpdateAsync(ipls.DeviceBuffer.from_tensor(bucket), 1)
        keep, src = operand(ipls, case, "f32", "dev")
        texts = agg.SendGradients(src, case.parts, case.iteration, origin=case.origin, pid=case.pid)
        assert texts == expected_for(case, "f32")
        assert agg.last_launch()["kernel"] == ipls.KERNEL_ENCODE_FLAT
        bucket.copy_(torch.from_numpy(second))
        torch.cuda.synchronize()
        agg.Wait(ticket)
        assert agg.last_launch()["kernel"] != ipls.KERNEL_ENCODE_FLAT      # the fold was launched by Wait
        assert (u64(agg.read(1)) == u64(agg0 + second)).all(), "the queued arrival was folded before Wait"
        after = {(p, t): agg.checksum(p, t) for p in range(P) for t in targets}
        changed = [k for k in before if before[k] != after[k]]
        assert changed == [(1, ipls.TGT_AGG)], changed                     # the arrival's fold alone


def expected_for(case, fmt):
    from oracle import oracle as o
    return [S.oracle_text(o, case, fmt, p) for p in case.parts]


def test_two_shards_give_the_same_texts(ipls, handles, dev_text):
    (case,) = S.residue_cases()
    one = handles(case.M, case.P)
    with ipls.Aggregator(case.M, case.P, devices=[0, 0]) as two:
        order = (5, 0, 7, 3, 4, 1)                                      # both shards, neither in order
        mixed = S.Case(case.name, case.M, case.P, case.n, order, case.o)
        for fmt, where in (("f32", "host"), ("f64", "dev"), ("bf16", "dev"), ("be", "host")):
            keep, src = operand(ipls, case, fmt, where)                 # the case's own vector, planted for all 8
            want = [expected(case, fmt)[p] for p in order]
            kw = dict(origin=mixed.origin, pid=mixed.pid)
            assert one.SendGradients(src, order, mixed.iteration, **kw) == want
            send_both(two, dev_text, mixed, src, want, f"two shards {where} {fmt}", shifts=(0, 1))
        send_both(two, dev_text, mixed, None, [S.null_text(mixed, p) for p in order], "two shards null")


# ---------------------------------------------------------------------------
# refusals: the code, the message, and an output that still holds FILL
# ---------------------------------------------------------------------------
def test_refusals(ipls, handles, dev_text):
    M, P = S.SHORT_MODEL
    agg = handles(M, P)
    case = S.Case("refusals", M, P, M, (0, 3), 2)
    _, src = operand(ipls, case, "f64", "host")
    long = np.concatenate([src, np.ones(1)])                  # M + 1 values: the last partition holds 99 + the count slot
    total = C.batch_layout([C.text_len(case.frame_len(p)) for p in case.parts])[1]
    N = ipls
    split_dst = np.empty(agg.lengths[0])
    rc = ipls.lib().ipls_agg_split(agg.handle, src.ctypes.data, src.size, N.HOST_FRAME, 0, split_dst.ctypes.data, N.HOST_F64)
    from ipls import _native
    split_msg = _native.last_error(agg.handle)
    assert rc == _native.IPLS_E_INVAL and "src_kind" in split_msg
    calls = [
        ("overrun", (long.ctypes.data, long.size, N.HOST_F64, case.parts), total, _native.IPLS_E_RANGE, "overruns partition 3"),
        ("index P", (src.ctypes.data, src.size, N.HOST_F64, (0, P)), total, _native.IPLS_E_RANGE, f"partition {P} out of range"),
        ("HOST_FRAME", (src.ctypes.data, src.size, N.HOST_FRAME, case.parts), total, _native.IPLS_E_INVAL, split_msg),
        ("out_cap", (src.ctypes.data, src.size, N.HOST_F64, case.parts), total - 1, _native.IPLS_E_RANGE, "need"),
    ]
    for name, (ptr, n, kind, parts), cap, code, msg in calls:
        host = np.full(total + 64, FILL, dtype=np.uint8)
        rc = send_raw(ipls, agg, ptr, n, kind, parts, 1, 3, b"ab", host.ctypes.data, cap, N.HOST_TEXT)
        err = _native.last_error(agg.handle)
        assert rc == code and msg in err, (name, rc, err)
        assert (host == FILL).all(), f"{name}: the host output was written"
        addr = dev_text.at(0)
        rc = send_raw(ipls, agg, ptr, n, kind, parts, 1, 3, b"ab", addr, cap, N.DEV_TEXT)
        assert rc == code and msg in _native.last_error(agg.handle), (name, rc)
        dev_text.check(agg, [], f"{name}: the device output")
    # and the same vector, one value shorter, is taken
    assert send_raw(ipls, agg, src.ctypes.data, src.size, N.HOST_F64, case.parts, 1, 3, b"ab", None, 0, N.HOST_TEXT) == total
