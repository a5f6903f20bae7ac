"""The trainer's update as the difference of two tensor lists on the GPU:
UpdateGradient and SendGradients over ipls.Difference
(ipls_agg_update_gradient_segs_diff / _send_gradients_segs_diff;
k_update_segs_diff, k_b64url_encode_segs_diff), on one shard and on two shards
of one GPU.  Expected values come from numpy and the oracle alone
(seg_diff_cases.py: the difference in each segment's own format, widened, then
organize_gradients / fold / frame_encode); agreement with torch.sub per tensor
fed to the existing Segments calls is a second check, never the first.  A NaN
is compared as a NaN only, in the accumulators and in the texts.
"""
import base64
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal
import seg_cases as S
import seg_diff_cases as D

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
    """The segment kernels' tile, block x vectors, from one launch's record; the twins' tile."""
    a = torch.ones(8, dtype=torch.float32, device="cuda")
    b = torch.ones(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
        agg.UpdateGradient([a], [0])
        twin = agg.last_launch()
        agg.UpdateGradient(ipls.Difference([a], [b]), [0])
        li = agg.last_launch()
    assert twin["kernel"] == ipls.KERNEL_UPDATE_SEGS and li["kernel"] == ipls.KERNEL_UPDATE_SEGS_DIFF, (twin, li)
    assert (li["block"], li["vectors"]) == (twin["block"], twin["vectors"])
    return li["block"] * li["vectors"]


def _upload(segs, flush=False):
    """[(backing tensor, view tensor)]: the view starts r elements into its backing array, which starts on a 128-B
    line; flush: the backing array ends with the view's last element."""
    out = []
    for s in segs:
        backing = s.backing[:s.r + s.n] if flush else s.backing
        raw = np.ascontiguousarray(backing).view(np.uint8)
        b = torch.from_numpy(raw.copy()).cuda()
        assert b.data_ptr() % 128 == 0
        v = b.view(TORCH_DTYPE[s.fmt])[s.r:s.r + s.n]
        assert v.is_contiguous() and (not s.n or v.data_ptr() == b.data_ptr() + s.r * S.esize(s.fmt))
        assert not flush or v.numel() == 0 or v.data_ptr() + v.numel() * v.element_size() == b.data_ptr() + b.numel()
        out.append((b, v))
    torch.cuda.synchronize()
    return out


def _difference(ipls, A, B, flush=False):
    ua, ub = _upload(A, flush), _upload(B, flush)
    return ipls.Difference([v for _, v in ua], [v for _, v in ub]), (ua, ub)


def _torch_sub(ipls, keep):
    """The parent route: torch.sub per tensor, as a Segments."""
    ua, ub = keep
    out = [torch.sub(a, b) for (_, a), (_, b) in zip(ua, ub)]
    torch.cuda.synchronize()
    return ipls.Segments.from_tensors(out)


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


def _assert_texts(got, want, L_of, origin, what):
    """Byte-exact, except that a payload double that is a NaN on both sides may differ in sign and payload."""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        assert len(g) == len(w), f"{what}: text {i} length"
        fg, fw = (np.frombuffer(base64.urlsafe_b64decode(t), dtype=np.uint8) for t in (g, w))
        L = L_of[i]
        assert fg.size == fw.size == 14 + 8 * L + len(origin), f"{what}: text {i} frame length"
        assert np.array_equal(fg[:14], fw[:14]) and np.array_equal(fg[14 + 8 * L:], fw[14 + 8 * L:]), f"{what}: text {i}"
        vg = fg[14:14 + 8 * L].view(">u8").astype(np.uint64).view(np.float64)
        vw = fw[14:14 + 8 * L].view(">u8").astype(np.uint64).view(np.float64)
        assert_bits_equal(vg, vw, f"{what}: text {i} payload")


# ---- UpdateGradient ----
@DEVICES
@CHUNK
def test_update_every_layout(ipls, O, T, devices, ci):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for li_, name in enumerate(D.LAYOUTS):
        rng = np.random.default_rng(2000 * ci + li_)
        A, B = D.build(rng, name, c, T)
        diff, keep = _difference(ipls, A, B)
        assert diff.n == S.total(A) and diff.n_segs == len(A)
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            _preload(agg, rng)
            others = _others(agg)     # not AGG: reading it would end its logically-zero state
            acc = S.U.zeros(O, M, P)
            for rnd, start in ((0, ipls.START_ZERO), (1, ipls.START_ACCUM)):   # into logical zeros, then into the result
                agg.UpdateGradient(diff, range(P))
                acc = D.expected_update(O, acc, A, B, c, range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), acc[p], f"{name} c={c} round {rnd} AGG[{p}]")
                info = agg.last_launch()
                mine = _last_shard_parts(ipls, devices, range(P))
                assert info["kernel"] == ipls.KERNEL_UPDATE_SEGS_DIFF and info["start"] == start, (name, info)
                assert info["block"] * info["vectors"] == T
                assert info["grid"] == S.n_update_items(O, c, T, mine), (name, info)
                assert info["seqf"] == int(_has_whole(A, c, T, mine)), (name, info)
            for key, b in _others(agg).items():
                assert np.array_equal(others[key], b), f"{name}: target {key[1]} of partition {key[0]} changed"
            # second check: torch.sub per tensor through the existing Segments call, into a fresh handle twice
            sub = _torch_sub(ipls, keep)
            with ipls.Aggregator(model_size=M, n_partitions=P) as ref:
                for _ in range(2):
                    ref.UpdateGradient(sub, range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), ref.read(p), f"{name} c={c} against torch.sub, AGG[{p}]")


@DEVICES
@CHUNK
@pytest.mark.parametrize("owned", ([1, 3], [8], [], [4, 4]), ids=("1-3", "8", "none", "4-4"))
def test_update_owned_subsets(ipls, O, T, devices, ci, owned):
    """Into preloaded non-zero accumulators; a repeated partition folds again; nothing else changes."""
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for name in ("tiny", "residues-f32", "whole-bf16"):
        rng = np.random.default_rng(60 + ci)
        A, B = D.build(rng, name, c, T)
        diff, keep = _difference(ipls, A, B)
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            _preload(agg, rng, agg_too=True)
            before = _state(agg)
            acc = [agg.read(p).copy() for p in range(P)]
            agg.UpdateGradient(diff, owned)
            want = D.expected_update(O, acc, A, B, c, owned)   # [4, 4]: two folds
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{name} owned={owned} AGG[{p}]")
            now = _state(agg)
            for k, (a, b) in enumerate(zip(now, before)):
                if k % 4 or k // 4 not in owned:
                    assert np.array_equal(a, b), f"{name} owned={owned}: target {TARGETS[k % 4]} of {k // 4} changed"
        del keep


@DEVICES
def test_update_no_values(ipls, O, T, devices):
    """n_segs == 0 is the vector of no values: the count slots still count."""
    c = S.chunks(T)[1]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, np.random.default_rng(1), agg_too=True)
        acc = [agg.read(p).copy() for p in range(P)]
        agg.UpdateGradient(ipls.Difference([], []), range(P))
        want = S.U.expected(O, acc, np.zeros(0), 0, M, P, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"no values, AGG[{p}]")
        assert agg.last_launch()["kernel"] == ipls.KERNEL_UPDATE_SEGS_DIFF


# ---- SendGradients ----
@DEVICES
@CHUNK
@pytest.mark.parametrize("origin", (b"", b"Qm5by"), ids=("origin0", "origin5"))
def test_send_gradients(ipls, O, T, devices, ci, origin):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    lists = (list(range(P)), [7, 2, 5], [3, 3, 0])
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        for li_, name in enumerate(D.LAYOUTS):
            A, B = D.build(np.random.default_rng(40 + li_), name, c, T)
            diff, keep = _difference(ipls, A, B)
            for parts in lists[:1] if li_ % 3 else lists:
                L_of = [agg.lengths[p] for p in parts]
                want = D.expected_texts(O, A, B, c, parts, 11, origin)
                got = agg.SendGradients(diff, parts, 11, origin=origin)
                _assert_texts(got, want, L_of, origin, f"{name} c={c} parts={parts}: host texts")
                info = agg.last_launch()
                assert info["kernel"] == ipls.KERNEL_ENCODE_SEGS_DIFF and info["vectors"] == 3, info
                # a device text buffer with guard bytes before, between and after the texts
                total = sum((len(t) + 63) // 64 * 64 for t in want) + 64
                dev = torch.full((total + 128,), S.SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                lens, offs = agg.SendGradients(diff, parts, 11, origin=origin, out=dev.data_ptr() + 64, out_cap=total)
                agg.sync()
                assert lens == [len(t) for t in want], f"{name}: the sizes of out=None"
                host = dev.cpu().numpy()
                texts = [host[64 + o:64 + o + n].tobytes() for o, n in zip(offs, lens)]
                _assert_texts(texts, want, L_of, origin, f"{name} parts={parts}: device texts")
                guard = np.ones(host.size, dtype=bool)
                for o, n in zip(offs, lens):
                    guard[64 + o:64 + o + n] = False
                assert (host[guard] == S.SENTINEL).all(), f"{name} parts={parts}: bytes around the texts were written"
            # second check: torch.sub per tensor through the existing Segments call
            sub = _torch_sub(ipls, keep)
            _assert_texts(agg.SendGradients(diff, lists[1], 11, origin=origin),
                          agg.SendGradients(sub, lists[1], 11, origin=origin), [agg.lengths[p] for p in lists[1]],
                          origin, f"{name} c={c}: against torch.sub")
            del keep
        # no tensors: a vector of no values, not the null gradient
        none = agg.SendGradients(ipls.Difference([], []), [0, 8], 4, origin=origin)
        g = O.organize_gradients(np.zeros(0), M, P)
        assert none == [O.java_b64url_encode(O.frame_encode(g[p], p, 4, 3, origin)) for p in (0, 8)]


# ---- aliasing ----
@DEVICES
def test_a_list_minus_itself(ipls, T, devices):
    """Difference(x, x): +0.0 everywhere except where x is NaN or infinite (NaN there), count slot 1.0."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    for name in ("tiny", "whole-f32", "residues-half"):
        segs = S.build(np.random.default_rng(8), S.shape(name, c, T), c, T)    # with the formats' edge values
        up = _upload(segs)
        x = [v for _, v in up]
        wide = S.concat(segs)
        assert np.isnan(wide).any() and np.isinf(wide).any() and (wide == 0).any()
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            agg.UpdateGradient(ipls.Difference(x, x), range(P))
            for p in range(P):
                got = agg.read(p)
                w = wide[p * c:min((p + 1) * c, M)]
                bad = ~np.isfinite(w)
                assert np.isnan(got[:w.size][bad]).all(), f"{name} AGG[{p}]: inf - inf and NaN - NaN are NaN"
                rest = got[:w.size][~bad]
                assert not rest.any() and not np.signbit(rest).any(), f"{name} AGG[{p}]: x - x is +0.0"
                assert got[w.size] == 1.0 and not got[w.size + 1:].any(), f"{name} AGG[{p}]: count slot and tail"


# ---- refusals ----
def _tables(ptrs, ns, kinds):
    a = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    b = (ctypes.c_int64 * max(len(ns), 1))(*ns) if ns is not None else None
    d = (ctypes.c_int32 * max(len(kinds), 1))(*kinds) if kinds is not None else None
    return a, b, d


@DEVICES
def test_refusals_leave_every_target(ipls, O, T, devices):
    c = S.chunks(T)[0]
    M = S.model_size(c)
    ga = torch.ones(M + 8, dtype=torch.float32, device="cuda")
    gb = torch.full((M + 8,), 0.25, dtype=torch.float32, device="cuda")
    out = torch.full((1 << 16,), S.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    owned = (ctypes.c_int32 * P)(*range(P))
    F32, F16 = ipls.DEV_F32, ipls.DEV_F16

    def update(agg, a_ptrs, b_ptrs, ns, kinds, k, own=owned, n_own=P):
        a, n_, d = _tables(a_ptrs, ns, kinds)
        b = _tables(b_ptrs, None, None)[0]
        return agg._lib.ipls_agg_update_gradient_segs_diff(agg._h, a, b, n_, d, k, own, n_own)

    def send(agg, a_ptrs, b_ptrs, ns, kinds, k, parts=owned, n_parts=P):
        a, n_, d = _tables(a_ptrs, ns, kinds)
        b = _tables(b_ptrs, None, None)[0]
        return agg._lib.ipls_agg_send_gradients_segs_diff(agg._h, a, b, n_, d, k, parts, n_parts, 1, 3, None, 0,
                                                          out.data_ptr(), out.numel(), ipls.DEV_TEXT, None, None)

    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, np.random.default_rng(3), agg_too=True)
        before = _state(agg)
        pa, pb = ga.data_ptr(), gb.data_ptr()
        ok = ([pa, pa + 4 * (M - 8)], [pb, pb + 4 * (M - 8)], [M - 8, 8], [F32, F32], 2)
        assert update(agg, *ok) == 0                                  # the tables themselves are fine
        after_ok = _state(agg)
        assert not _same(after_ok, before)
        want = S.U.expected(O, [b.view(np.float64) for b in before[::4]], np.full(M, 0.75), M, M, P, range(P))
        for p in range(P):
            assert_bits_equal(after_ok[4 * p].view(np.float64), want[p], f"AGG[{p}]")
        bad = {
            "a null subtrahend table": (ok[0], None, *ok[2:]),
            "a null subtrahend pointer": (ok[0], [pb, None], *ok[2:]),
            "a misaligned subtrahend pointer": (ok[0], [pb, pb + 2], *ok[2:]),
            "a misaligned half subtrahend pointer": (ok[0], [pb, pb + 1], [M - 8, 8], [F32, F16], 2),
            "a null minuend pointer": ([pa, None], *ok[1:]),
            "a misaligned minuend pointer": ([pa, pa + 2], *ok[1:]),
            "a host kind": (*ok[:3], [F32, ipls.HOST_F32], 2),
            "a negative length": (*ok[:2], [M, -1], [F32, F32], 2),
            "a negative count": (*ok[:4], -1),
        }
        for what, args in bad.items():
            assert update(agg, *args) == INVAL, what
            assert _same(_state(agg), after_ok), f"{what} changed the state"
            assert send(agg, *args) == INVAL, what
        assert update(agg, ok[0], [pb, pb + 2], *ok[2:]) == INVAL
        msg = agg._lib.ipls_agg_last_error(None).decode()
        assert "subtrahend segment 1" in msg, msg
        assert update(agg, [pa, pa + 2], *ok[1:]) == INVAL
        msg = agg._lib.ipls_agg_last_error(None).decode()
        assert "minuend segment 1" in msg, msg
        # a list that overruns a partition; a partition that does not exist; a null owned list
        assert update(agg, [pa, pa], [pb, pb], [M - 3, 4], [F32, F32], 2) == RANGE
        assert send(agg, [pa, pa], [pb, pb], [M - 3, 4], [F32, F32], 2) == RANGE
        assert update(agg, *ok, own=(ctypes.c_int32 * 2)(0, P), n_own=2) == RANGE
        assert send(agg, *ok, parts=(ctypes.c_int32 * 2)(0, P), n_parts=2) == RANGE
        assert update(agg, *ok, own=None, n_own=2) == INVAL
        assert update(agg, *ok, n_own=-1) == INVAL
        assert _same(_state(agg), after_ok), "a refused call changed the state"
        agg.sync()
        assert (out == S.SENTINEL).all(), "a refused send wrote text"
        assert send(agg, *ok) > 0                                     # ... and the same tables do send


# ---- no reads outside either list ----
@DEVICES
@pytest.mark.parametrize("name", ("aligned", "residues-f64", "residues-f32", "residues-half", "residues-bf16"))
def test_views_flush_against_the_end_of_their_allocation(ipls, O, T, devices, name):
    """Every view of both lists ends where its allocation ends: results as ever."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    A, B = D.build(np.random.default_rng(77), name, c, T)
    diff, keep = _difference(ipls, A, B, flush=True)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        agg.UpdateGradient(diff, range(P))
        want = D.expected_update(O, S.U.zeros(O, M, P), A, B, c, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"{name} AGG[{p}]")
        parts = [8, 0, 4]
        _assert_texts(agg.SendGradients(diff, parts, 2), D.expected_texts(O, A, B, c, parts, 2, b""),
                      [agg.lengths[p] for p in parts], b"", name)
    del keep


# ---- the Python surface ----
def test_two_flat_tensors_are_a_one_segment_difference(ipls, O, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    A, B = D.build(np.random.default_rng(12), "whole-f32", c, T)
    (_, a), (_, b) = _upload(A)[0], _upload(B)[0]
    d = ipls.Difference(a, b)
    assert (d.n, d.n_segs) == (M, 1)
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        agg.UpdateGradient(d, range(P))
        want = D.expected_update(O, S.U.zeros(O, M, P), A, B, c, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"AGG[{p}]")
        for call in (lambda: agg.InitializeWeights(d), lambda: agg.GetPartitions(out=d), lambda: agg.Update(d, 0),
                     lambda: agg.OrganizeGradients(d)):
            with pytest.raises((TypeError, ValueError)):
                call()
