"""The trainer boundary over a list of tensors on the GPU: UpdateGradient,
SendGradients and GetPartitions(out=) over ipls.Segments
(ipls_agg_update_gradient_segs / _send_gradients_segs / _get_partitions_segs;
k_update_segs, k_b64url_encode_segs, k_divide_segs), on one shard and on two
shards of one GPU.  Expected values come from the oracle alone
(organize_gradients on the widened concatenation, then fold; get_partitions,
then the format's narrowing; frame_encode under java_b64url_encode); agreement
with the flat call on the concatenation is a second check, never the first.
Layouts, planted values and the expectations are seg_cases.py's.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal
import seg_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -2
P = S.P
TARGETS = (0, 1, 2, 4)   # AGG, REP, W, FUT
DEVICES = pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
CHUNK = pytest.mark.parametrize("ci", range(3), ids=("c9", "cT+9", "c2T+25"))
TORCH_DTYPE = {"f64": torch.float64, "f32": torch.float32, "half": torch.float16, "bf16": torch.bfloat16}


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
def T(ipls):
    """The segment kernels' tile, block x vectors, from one launch's record."""
    g = torch.ones(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
        agg.UpdateGradient([g], [0])
        li = agg.last_launch()
    assert li["kernel"] == ipls.KERNEL_UPDATE_SEGS, li
    return li["block"] * li["vectors"]


def _upload(segs, fill=None):
    """The backing arrays on the device and the views as tensors: [(backing tensor, view tensor)].  The view starts
    r elements into its backing array, which starts on a 128-B line."""
    out = []
    for s in segs:
        raw = np.ascontiguousarray(s.backing).view(np.uint8)
        if fill is not None:
            raw = np.full_like(raw, fill)
        b = torch.from_numpy(raw.copy()).cuda()
        assert b.data_ptr() % 128 == 0
        v = b.view(TORCH_DTYPE[s.fmt])[s.r:s.r + s.n]
        assert v.is_contiguous() and (not s.n or v.data_ptr() == b.data_ptr() + s.r * S.esize(s.fmt))
        out.append((b, v))
    torch.cuda.synchronize()
    return out


def _segments(ipls, up):
    return ipls.Segments.from_tensors([v for _, v in up])


def _preload(agg, rng, agg_too=False):
    for p in range(P):
        L = agg.lengths[p]
        agg.Update(rng.standard_normal(L), p, from_clients=False)
        agg.cache_partition(p, rng.standard_normal(L))
        agg.Update(rng.standard_normal(L), p, from_future=True)
        if agg_too:
            agg.Update(rng.standard_normal(L), p)


def _state(agg):
    return [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in TARGETS]


def _others(agg):
    return {(p, t): agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in TARGETS[1:]}


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _last_shard_parts(ipls, devices, parts):
    """The partitions of `parts` on the last shard that holds any: what last_launch reports."""
    if devices is None:
        return list(parts)
    owner = ipls.shard_plan(P, len(devices))
    last = max(owner[p] for p in parts)
    return [p for p in parts if owner[p] == last]


def _has_whole(segs, c, T, parts):
    n = S.total(segs)
    for p in parts:
        ncopy = max(0, min((p + 1) * c, n) - p * c)
        for lo in range(0, ncopy - T + 1, T):
            if len(S.pieces_of(segs, p * c + lo, p * c + lo + T)) == 1:
                return True
    return False


# ---- UpdateGradient ----
@DEVICES
@CHUNK
def test_update_every_layout(ipls, O, T, devices, ci):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for li_, name in enumerate(S.LAYOUTS):
        rng = np.random.default_rng(1000 * ci + li_)
        segs = S.build(rng, S.shape(name, c, T), c, T)
        up = _upload(segs)
        seg = _segments(ipls, up)
        assert seg.n == S.total(segs) and seg.n_segs == len(segs)
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            _preload(agg, rng)
            others = _others(agg)     # not AGG: reading it would end its logically-zero state
            acc = S.U.zeros(O, M, P)
            for rnd, start in ((0, ipls.START_ZERO), (1, ipls.START_ACCUM)):   # into logical zeros, then into the result
                agg.UpdateGradient(seg, range(P))
                acc = S.expected_update(O, acc, segs, c, range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), acc[p], f"{name} c={c} round {rnd} AGG[{p}]")
                info = agg.last_launch()
                mine = _last_shard_parts(ipls, devices, range(P))
                assert info["kernel"] == ipls.KERNEL_UPDATE_SEGS and info["start"] == start, (name, info)
                assert info["block"] * info["vectors"] == T
                assert info["grid"] == S.n_update_items(O, c, T, mine), (name, info)
                assert info["seqf"] == int(_has_whole(segs, c, T, mine)), (name, info)
            for key, b in _others(agg).items():
                assert np.array_equal(others[key], b), f"{name}: target {key[1]} of partition {key[0]} changed"
            # second check: the flat call on the concatenation, into a fresh handle twice
            flat = torch.from_numpy(S.concat(segs)).cuda()
            torch.cuda.synchronize()
            with ipls.Aggregator(model_size=M, n_partitions=P) as ref:
                for _ in range(2):
                    ref.UpdateGradient(ipls.DeviceBuffer.from_tensor(flat), range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), ref.read(p), f"{name} c={c} against the flat call, AGG[{p}]")


@DEVICES
@CHUNK
@pytest.mark.parametrize("owned", ([1, 3], [8], [], [4, 4]), ids=("1-3", "8", "none", "4-4"))
def test_update_owned_subsets(ipls, O, T, devices, ci, owned):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for name in ("tiny", "residues-f32"):
        rng = np.random.default_rng(50 + ci)
        segs = S.build(rng, S.shape(name, c, T), c, T)
        seg = _segments(ipls, up := _upload(segs))
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            _preload(agg, rng, agg_too=True)
            before = _state(agg)
            acc = [agg.read(p).copy() for p in range(P)]
            agg.UpdateGradient(seg, owned)
            want = S.expected_update(O, acc, segs, c, owned)   # [4, 4]: two folds
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{name} owned={owned} AGG[{p}]")
            now = _state(agg)
            for k, (a, b) in enumerate(zip(now, before)):
                if k % 4 or k // 4 not in owned:
                    assert np.array_equal(a, b), f"{name} owned={owned}: target {TARGETS[k % 4]} of {k // 4} changed"
        del up


@DEVICES
@CHUNK
def test_update_negative_zero_accumulator(ipls, O, T, devices, ci):
    """AGG all -0.0: the add is made above the count slot too, so the tail becomes +0.0."""
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    neg = torch.full((c + 1,), -0.0, dtype=torch.float64, device="cuda")
    for name in ("short-a", "short-b", "short-c", "tiny"):
        segs = S.build(np.random.default_rng(5), S.shape(name, c, T), c, T)
        seg = _segments(ipls, up := _upload(segs))
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            agg.reduce_batch(0, [[ipls.DeviceBuffer.from_tensor(neg[:agg.lengths[p]])] for p in range(P)],
                             start_mode=ipls.START_FIRST)
            start = [agg.read(p).copy() for p in range(P)]
            assert all(np.signbit(x).all() and not x.any() for x in start)
            agg.UpdateGradient(seg, range(P))
            want = S.expected_update(O, start, segs, c, range(P))
            for p in range(P):
                got = agg.read(p)
                assert_bits_equal(got, want[p], f"{name} c={c} AGG[{p}]")
                ncopy = max(0, min((p + 1) * c, seg.n) - p * c)
                assert not np.signbit(got[ncopy:]).any(), f"{name}: a -0.0 survived above the values of {p}"
        del up


@DEVICES
def test_update_no_values_and_overrun(ipls, O, T, devices):
    """n_segs == 0 is a vector of no values (the count slots still count); sum n = M + 1 overruns."""
    c = S.chunks(T)[1]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, np.random.default_rng(1), agg_too=True)
        acc = [agg.read(p).copy() for p in range(P)]
        agg.UpdateGradient(ipls.Segments.from_tensors([]), range(P))
        want = S.U.expected(O, acc, np.zeros(0), 0, M, P, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"no values, AGG[{p}]")
        before = _state(agg)
        segs = S.build(np.random.default_rng(2), [("f32", M - 3, 1), ("bf16", 4, 3)], c, T)
        seg = _segments(ipls, up := _upload(segs))
        with pytest.raises(ipls.IplsError) as e:
            agg.UpdateGradient(seg, range(P))
        assert e.value.code == RANGE
        assert _same(_state(agg), before), "an overrunning list changed the state"
        del up


@DEVICES
def test_update_refusals_leave_the_state(ipls, T, devices):
    c = S.chunks(T)[0]
    M = S.model_size(c)
    g = torch.ones(M + 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    owned = (ctypes.c_int32 * P)(*range(P))

    def call(agg, ptrs, ns, kinds, k):
        a = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
        b = (ctypes.c_int64 * max(len(ns), 1))(*ns) if ns is not None else None
        d = (ctypes.c_int32 * max(len(kinds), 1))(*kinds) if kinds is not None else None
        return agg._lib.ipls_agg_update_gradient_segs(agg._h, a, b, d, k, owned, P)

    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, np.random.default_rng(3), agg_too=True)
        before = _state(agg)
        ptr = g.data_ptr()
        assert call(agg, [ptr, ptr], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F32], 2) == 0     # the table itself is fine
        after_ok = _state(agg)
        assert not _same(after_ok, before)
        bad = {
            "a misaligned pointer": ([ptr, ptr + 2], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F32], 2),
            "a misaligned half pointer": ([ptr, ptr + 1], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F16], 2),
            "a host kind": ([ptr, ptr], [M - 8, 8], [ipls.DEV_F32, ipls.HOST_F32], 2),
            "a big-endian kind": ([ptr, ptr], [M - 8, 8], [ipls.DEV_BE, ipls.DEV_F32], 2),
            "kind 99": ([ptr, ptr], [M - 8, 8], [99, ipls.DEV_F32], 2),
            "a null table": (None, [M], [ipls.DEV_F32], 1),
            "a null length table": ([ptr], None, [ipls.DEV_F32], 1),
            "a negative length": ([ptr, ptr], [M, -1], [ipls.DEV_F32, ipls.DEV_F32], 2),
            "a null pointer": ([ptr, None], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F32], 2),
            "a negative count": ([ptr], [M], [ipls.DEV_F32], -1),
        }
        for what, args in bad.items():
            assert call(agg, *args) == INVAL, what
            assert _same(_state(agg), after_ok), f"{what} changed the state"
        assert call(agg, [ptr, ptr + 4], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F32], 2) == 0
        assert call(agg, [ptr, ptr + 2], [M - 8, 8], [ipls.DEV_F32, ipls.DEV_F32], 2) == INVAL
        msg = agg._lib.ipls_agg_last_error(None).decode()
        assert "segment 1" in msg, msg


# ---- GetPartitions ----
@DEVICES
@CHUNK
@pytest.mark.parametrize("secure", (False, True), ids=("plain", "secure"))
def test_get_partitions_every_layout(ipls, O, T, devices, ci, secure):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    rng = np.random.default_rng(70 + ci)
    w = S.weights(rng, O, c)
    model = O.get_partitions(w, secure)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        for p in range(P):
            agg.cache_partition(p, w[p])
        flat = {}
        for name in S.LAYOUTS:
            spec = S.shape(name, c, T)
            if sum(s[1] for s in spec) < M:
                continue
            spec = spec + [("f32", 5, 3), ("half", 0, 0), ("f64", 7, 1)]     # past the model: never written
            segs = S.build(rng, spec, c, T)
            up = _upload(segs, fill=S.SENTINEL)
            agg.GetPartitions(out=_segments(ipls, up))
            agg.sync()
            info = agg.last_launch()
            assert info["kernel"] == ipls.KERNEL_DIVIDE_SEGS and info["block"] * info["vectors"] == T, info
            if devices is None:
                assert info["grid"] == S.n_divide_items(spec, M, T), (name, info)
            want = S.expected_outputs(model, spec, M)
            for i, (s, (b, _)) in enumerate(zip(segs, up)):
                got = b.cpu().numpy().view(S.bits_dtype(s.fmt))
                k = want[i].size
                mine = got[s.r:s.r + k]
                nan = S.is_nan(mine, s.fmt) & S.is_nan(want[i], s.fmt)
                assert np.array_equal(mine[~nan], want[i][~nan]), f"{name} c={c} output segment {i} ({s.fmt})"
                junk = np.concatenate([got[:s.r], got[s.r + k:]]).view(np.uint8)
                assert (junk == S.SENTINEL).all(), f"{name} c={c}: bytes around segment {i} were written"
            # second check: the flat call per format
            for fmt in {s.fmt for s in segs[:-3]}:
                if fmt not in flat:
                    buf = torch.zeros(M, dtype=TORCH_DTYPE[fmt], device="cuda")
                    torch.cuda.synchronize()
                    agg.GetPartitions(out=ipls.DeviceBuffer.from_tensor(buf))
                    agg.sync()
                    flat[fmt] = buf.cpu().view(getattr(torch, "int" + str(8 * S.esize(fmt)))).numpy()
            at = 0
            for i, s in enumerate(segs):
                k = want[i].size
                ref = flat[s.fmt][at:at + k].view(S.bits_dtype(s.fmt)) if k else want[i]
                nan = S.is_nan(ref, s.fmt) & S.is_nan(want[i], s.fmt)
                assert np.array_equal(ref[~nan], want[i][~nan]), f"{name}: the flat call disagrees in segment {i}"
                at += s.n


@DEVICES
def test_get_partitions_short_list_is_refused(ipls, T, devices):
    c = S.chunks(T)[0]
    M = S.model_size(c)
    out = torch.full((M,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        with pytest.raises(ipls.IplsError) as e:
            agg.GetPartitions(out=ipls.Segments.from_tensors([out[:M - 1]]))
        assert e.value.code == RANGE
        with pytest.raises(ipls.IplsError) as e:
            agg.GetPartitions(out=ipls.Segments.from_tensors([]))
        assert e.value.code == RANGE
        agg.sync()
    assert (out == 7.0).all()


# ---- SendGradients ----
@DEVICES
@pytest.mark.parametrize("ci", range(2), ids=("c9", "cT+9"))
@pytest.mark.parametrize("origin", (b"", b"Qm5by"), ids=("origin0", "origin5"))
def test_send_gradients(ipls, O, T, devices, ci, origin):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    lists = (list(range(P)), [7, 2, 5], [3, 3, 0])
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        for li_, name in enumerate(("whole-f64", "whole-bf16", "tiny", "aligned", "short-b")):
            segs = S.build(np.random.default_rng(30 + li_), S.shape(name, c, T), c, T)
            seg = _segments(ipls, up := _upload(segs))
            for parts in lists:
                want = S.expected_texts(O, segs, c, parts, 11, origin)
                got = agg.SendGradients(seg, parts, 11, origin=origin)
                assert got == want, f"{name} c={c} parts={parts}: host texts"
                info = agg.last_launch()
                assert info["kernel"] == ipls.KERNEL_ENCODE_SEGS, info
                # a device text buffer
                total = sum((len(t) + 63) // 64 * 64 for t in want) + 64
                dev = torch.full((total,), S.SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                lens, offs = agg.SendGradients(seg, parts, 11, origin=origin, out=dev.data_ptr(), out_cap=total)
                agg.sync()
                host = dev.cpu().numpy()
                assert [host[o:o + n].tobytes() for o, n in zip(offs, lens)] == want, f"{name} parts={parts}: device texts"
            # second check: the flat call on the concatenation
            flat = torch.from_numpy(S.concat(segs)).cuda()
            torch.cuda.synchronize()
            assert agg.SendGradients(flat, lists[1], 11, origin=origin) == S.expected_texts(O, segs, c, lists[1], 11, origin)
            del up
        # no tensors: a vector of no values, not the null gradient
        none = agg.SendGradients(ipls.Segments.from_tensors([]), [0, 8], 4, origin=origin)
        g = O.organize_gradients(np.zeros(0), M, P)
        assert none == [O.java_b64url_encode(O.frame_encode(g[p], p, 4, 3, origin)) for p in (0, 8)]
        assert none != agg.SendGradients(None, [0, 8], 4, origin=origin)


# ---- the Python surface ----
def test_list_of_tensors_is_the_segments_built_from_it(ipls, O, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    segs = S.build(np.random.default_rng(9), S.shape("tiny", c, T), c, T)
    up = _upload(segs)
    tensors = [v for _, v in up]
    got = []
    for arg in (ipls.Segments.from_tensors(tensors), tensors, tuple(tensors)):
        with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
            agg.UpdateGradient(arg, range(P))
            got.append(([agg.read(p).view(np.uint64).copy() for p in range(P)], agg.SendGradients(arg, [1, 6], 2)))
    assert _same(got[0][0], got[1][0]) and _same(got[0][0], got[2][0])
    assert got[0][1] == got[1][1] == got[2][1]
    want = S.expected_update(O, S.U.zeros(O, M, P), segs, c, range(P))
    for p in range(P):
        assert_bits_equal(got[0][0][p].view(np.float64), want[p], f"AGG[{p}]")


def test_initialize_weights_from_segments(ipls, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    segs = S.build(np.random.default_rng(10), S.shape("tiny", c, T), c, T)
    up = _upload(segs)
    with ipls.Aggregator(model_size=M, n_partitions=P) as a, ipls.Aggregator(model_size=M, n_partitions=P) as b:
        a.InitializeWeights(_segments(ipls, up))
        b.InitializeWeights(S.concat(segs))
        for p in range(P):
            for t in TARGETS:
                assert np.array_equal(a.read(p, t).view(np.uint64), b.read(p, t).view(np.uint64)), (p, t)
