"""K trainers' tensor lists folded by one call on the GPU: UpdateGradient over
ipls.PeerUpdates (ipls_agg_update_gradient_segs_peers; k_update_segs_peers), on
one shard and on two shards of one GPU.  Expected values come from numpy and
the oracle alone (seg_peers_cases.py: the twins' expectation applied once per
peer, in peer order); the same K calls through the existing Segments /
Difference route on a second handle are a second check, never the first.  A
NaN is compared as a NaN only.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal
import seg_cases as S
import seg_peers_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -2
P = S.P
TARGETS = (0, 1, 2, 4)   # AGG, REP, W, FUT
DEVICES = pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
CHUNK = pytest.mark.parametrize("ci", range(3), ids=("c9", "cT+9", "c2T+25"))
PEERS = pytest.mark.parametrize("ki", range(len(C.KS)), ids=[f"K{k}" for k in C.KS])
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
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
        agg.UpdateGradient([a], [0])
        twin = agg.last_launch()
        agg.UpdateGradient(ipls.PeerUpdates([[a], [a]]), [0])
        li = agg.last_launch()
        assert agg.read(0).tolist() == [3.0] * 8 + [3.0]
    assert twin["kernel"] == ipls.KERNEL_UPDATE_SEGS and li["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS, (twin, li)
    assert (li["block"], li["vectors"]) == (twin["block"], twin["vectors"])
    return li["block"] * li["vectors"]


def _upload(lists):
    """[[view tensor per segment] per list]: every backing array of every list
    starts on a 128-B line of its own in ONE device buffer (one copy), the view
    r elements into it, the rest of the backing array junk around it."""
    at, total = [], 0
    for segs in lists:
        for s in segs:
            at.append(total)
            total += -(-(s.backing.nbytes + 1) // 128) * 128
    host = np.full(max(total, 128), S.SENTINEL, dtype=np.uint8)
    k = 0
    for segs in lists:
        for s in segs:
            host[at[k]:at[k] + s.backing.nbytes] = np.ascontiguousarray(s.backing).view(np.uint8)
            k += 1
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 128 == 0
    out, k = [], 0
    for segs in lists:
        views = []
        for s in segs:
            v = buf[at[k]:at[k] + s.backing.nbytes].view(TORCH_DTYPE[s.fmt])[s.r:s.r + s.n]
            assert v.is_contiguous() and (not s.n or v.data_ptr() == buf.data_ptr() + at[k] + s.r * S.esize(s.fmt))
            views.append(v)
            k += 1
        out.append(views)
    return out, buf


def _upload_flush(segs):
    """Every view in an allocation of its own that ends with the view's last element."""
    out = []
    for s in segs:
        raw = np.ascontiguousarray(s.backing[:s.r + s.n]).view(np.uint8)
        b = torch.from_numpy(raw.copy()).cuda()
        v = b.view(TORCH_DTYPE[s.fmt])[s.r:s.r + s.n]
        assert not v.numel() or v.data_ptr() + v.numel() * v.element_size() == b.data_ptr() + b.numel()
        out.append((b, v))
    torch.cuda.synchronize()
    return out


def _peer_updates(ipls, rec, peers):
    """(the PeerUpdates, the K twin operands of the parent route, what keeps the memory)."""
    views, buf = _upload(([rec] if rec is not None else []) + list(peers))
    r = views[0] if rec is not None else None
    t = views[1:] if rec is not None else views
    twins = [ipls.Segments.from_tensors(x) if r is None else ipls.Difference(r, x) for x in t]
    return ipls.PeerUpdates(t, received=r), twins, buf


def _set_agg(agg, acc):
    """AGG := acc, from a reset handle (0.0 + x is x)."""
    agg.reset()
    for p in range(P):
        agg.Update(acc[p], p)


def _preload(agg, rng):
    for p in range(P):
        L = agg.lengths[p]
        agg.Update(rng.standard_normal(L), p, from_clients=False)
        agg.cache_partition(p, rng.standard_normal(L))
        agg.Update(rng.standard_normal(L), p, from_future=True)
        agg.Update(rng.standard_normal(L), p)


def _state(agg):
    return [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in TARGETS]


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


# ---- every layout, every K ----
@DEVICES
@CHUNK
@PEERS
def test_update_every_layout(ipls, O, T, devices, ci, ki):
    c, K = S.chunks(T)[ci], C.KS[ki]
    M = S.model_size(c)
    mine = _last_shard_parts(ipls, devices, range(P))
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg, \
            ipls.Aggregator(model_size=M, n_partitions=P) as ref:
        for li_, name in enumerate(C.LAYOUTS):
            rng = np.random.default_rng(3000 * ci + 10 * li_ + ki)
            rec, peers = C.build(rng, name, c, T, K, (li_ + ki) % 2 == 1)
            pu, twins, keep = _peer_updates(ipls, rec, peers)
            assert (pu.n, pu.n_segs, pu.n_peers) == (S.total(peers[0]), len(peers[0]), K)
            # into logical zeros, then into accumulators that make every triple's order count
            for start, acc in ((ipls.START_ZERO, None), (ipls.START_ACCUM, C.start_acc(rng, O, name, c, T))):
                what = f"{name} c={c} K={K} received={rec is not None} start={start}"
                if acc is None:
                    agg.reset(), ref.reset()
                    acc = S.U.zeros(O, M, P)
                else:
                    _set_agg(agg, acc), _set_agg(ref, acc)
                agg.UpdateGradient(pu, range(P))
                info = agg.last_launch()
                want = C.expected(O, acc, rec, peers, c, range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), want[p], f"{what} AGG[{p}]")
                assert info["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS and info["start"] == start, (what, info)
                assert info["block"] * info["vectors"] == T
                assert info["grid"] == S.n_update_items(O, c, T, mine), (what, info)
                assert info["seqf"] == int(_has_whole(peers[0], c, T, mine)), (what, info)
                # second check: the K calls this one replaces, through the existing route
                for tw in twins:
                    ref.UpdateGradient(tw, range(P))
                for p in range(P):
                    assert_bits_equal(agg.read(p), ref.read(p), f"{what} against the K calls, AGG[{p}]")
            del keep


@DEVICES
@CHUNK
@pytest.mark.parametrize("owned", ([1, 3], [8], [], [4, 4], [4, 1, 4, 0, 4]), ids=("1-3", "8", "none", "4-4", "4-1-4-0-4"))
def test_update_owned_subsets(ipls, O, T, devices, ci, owned):
    """Into preloaded accumulators; a repeated partition gets each peer's value that often in a row; one launch;
    nothing else changes."""
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg, \
            ipls.Aggregator(model_size=M, n_partitions=P) as ref:
        for li_, (name, K) in enumerate((("tiny", 3), ("residues-f32", 5), ("whole-bf16", 2), ("whole-half", 3))):
            rng = np.random.default_rng(60 + ci)
            rec, peers = C.build(rng, name, c, T, K, li_ % 2 == 0)
            pu, twins, keep = _peer_updates(ipls, rec, peers)
            agg.reset()
            _preload(agg, rng)
            before = _state(agg)
            acc = [b.view(np.float64).copy() for b in before[::4]]
            _set_agg(ref, acc)
            agg.UpdateGradient(pu, owned)
            info = agg.last_launch()   # of the last shard the call touched
            want = C.expected(O, acc, rec, peers, c, owned)
            for tw in twins:
                ref.UpdateGradient(tw, owned)
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{name} owned={owned} AGG[{p}]")
                assert_bits_equal(agg.read(p), ref.read(p), f"{name} owned={owned} against the K calls, AGG[{p}]")
            if owned:
                mine = _last_shard_parts(ipls, devices, sorted(set(owned)))
                assert info["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS
                assert info["grid"] == S.n_update_items(O, c, T, mine), "repeats are no launches and no blocks"
            now = _state(agg)
            for k, (a, b) in enumerate(zip(now, before)):
                if k % 4 or k // 4 not in owned:
                    assert np.array_equal(a, b), f"{name} owned={owned}: target {TARGETS[k % 4]} of {k // 4} changed"
            del keep


@DEVICES
def test_update_no_values(ipls, O, T, devices):
    """n_segs == 0 is the vector of no values, K times: the count slots count K."""
    c = S.chunks(T)[1]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _preload(agg, np.random.default_rng(1))
        acc = [agg.read(p).copy() for p in range(P)]
        for rec in (None, []):
            agg.UpdateGradient(ipls.PeerUpdates([[], [], []], received=rec), range(P))
            for _ in range(3):
                acc = S.U.expected(O, acc, np.zeros(0), 0, M, P, range(P))
            for p in range(P):
                assert_bits_equal(agg.read(p), acc[p], f"no values, AGG[{p}]")
            assert agg.last_launch()["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS


@DEVICES
def test_one_peer_is_the_twin_by_its_own_kernel(ipls, O, T, devices):
    c = S.chunks(T)[2]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg, \
            ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as twin:
        for li_, name in enumerate(("aligned", "residues-f64", "whole-f32", "short-b")):
            rng = np.random.default_rng(300 + li_)
            rec, peers = C.build(rng, name, c, T, 1, li_ % 2 == 0)
            pu, twins, keep = _peer_updates(ipls, rec, peers)
            for _ in range(2):   # into logical zeros, then into the result
                agg.UpdateGradient(pu, range(P))
                twin.UpdateGradient(twins[0], range(P))
                a, b = agg.last_launch(), twin.last_launch()
                assert a["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS, a
                assert b["kernel"] == (ipls.KERNEL_UPDATE_SEGS if rec is None else ipls.KERNEL_UPDATE_SEGS_DIFF), b
                assert {k: v for k, v in a.items() if k != "kernel"} == {k: v for k, v in b.items() if k != "kernel"}
                for p in range(P):
                    assert_bits_equal(agg.read(p), twin.read(p), f"{name} AGG[{p}]")
            del keep


@DEVICES
def test_queued_arrivals_fold_first(ipls, O, T, devices):
    """An arrival queued before the call is folded before anything of the call, as by a single UpdateGradient."""
    c = S.chunks(T)[1]
    M = S.model_size(c)
    rng = np.random.default_rng(9)
    rec, peers = C.build(rng, "whole-f32", c, T, 3, True)
    pu, _, keep = _peer_updates(ipls, rec, peers)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        acc = C.start_acc(rng, O, "whole-f32", c, T)
        _set_agg(agg, acc)
        for p in (2, 7):
            arrival = rng.standard_normal(agg.lengths[p]) * 2.0 ** 60   # folded later, it would round differently
            bucket = torch.from_numpy(arrival.copy()).cuda()
            torch.cuda.synchronize()
            ticket = agg.UpdateAsync(ipls.DeviceBuffer.from_tensor(bucket), p)
            acc[p] = acc[p] + arrival
            agg.UpdateGradient(pu, [p])
            agg.Wait(ticket)
            acc = C.expected(O, acc, rec, peers, c, [p])
            assert_bits_equal(agg.read(p), acc[p], f"AGG[{p}]")


# ---- aliasing ----
@DEVICES
def test_lists_may_alias(ipls, O, T, devices):
    """Every peer and the received model one and the same list: x - x K times; the peers one list: K folds of it."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    for name in ("tiny", "whole-f32", "residues-half"):
        segs = S.build(np.random.default_rng(8), S.shape(name, c, T), c, T)    # with the formats' edge values
        (x,), keep = _upload([segs])
        wide = S.concat(segs)
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            agg.UpdateGradient(ipls.PeerUpdates([x, x, x], received=x), range(P))
            for p in range(P):
                got = agg.read(p)
                w = wide[p * c:min((p + 1) * c, M)]
                bad = ~np.isfinite(w)
                assert np.isnan(got[:w.size][bad]).all(), f"{name} AGG[{p}]: inf - inf and NaN - NaN are NaN"
                rest = got[:w.size][~bad]
                assert not rest.any() and not np.signbit(rest).any(), f"{name} AGG[{p}]: x - x is +0.0"
                assert got[w.size] == 3.0 and not got[w.size + 1:].any(), f"{name} AGG[{p}]: count slot and tail"
            agg.reset()
            agg.UpdateGradient(ipls.PeerUpdates([x, x, x]), range(P))
            want = C.expected(O, S.U.zeros(O, M, P), None, [segs] * 3, c, range(P))
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{name} AGG[{p}]")
        del keep


# ---- refusals ----
def _arr(t, vals):
    return (t * max(len(vals), 1))(*vals) if vals is not None else None


@DEVICES
def test_refusals_leave_every_target(ipls, O, T, devices):
    c = S.chunks(T)[0]
    M = S.model_size(c)
    gm = torch.ones(M + 8, dtype=torch.float32, device="cuda")
    gt = [torch.full((M + 8,), v, dtype=torch.float32, device="cuda") for v in (0.25, 0.5)]
    torch.cuda.synchronize()
    owned = (ctypes.c_int32 * P)(*range(P))
    F32, F16 = ipls.DEV_F32, ipls.DEV_F16
    pm, (p0, p1) = gm.data_ptr(), (t.data_ptr() for t in gt)
    tail = 4 * (M - 8)

    def update(agg, m_ptrs, t_ptrs, K, ns, kinds, k, own=owned, n_own=P):
        return agg._lib.ipls_agg_update_gradient_segs_peers(
            agg._h, _arr(ctypes.c_void_p, m_ptrs), _arr(ctypes.c_void_p, t_ptrs), K, _arr(ctypes.c_int64, ns),
            _arr(ctypes.c_int32, kinds), k, own, n_own)

    ok = ([pm, pm + tail], [p0, p0 + tail, p1, p1 + tail], 2, [M - 8, 8], [F32, F32], 2)
    bad = {
        "no peers": (*ok[:2], 0, *ok[3:]),
        "a negative number of peers": (*ok[:2], -1, *ok[3:]),
        "too many peers": (*ok[:2], ipls.SEG_PEERS_MAX + 1, *ok[3:]),
        "a null peer table": (ok[0], None, *ok[2:]),
        "a null peer pointer": (ok[0], [p0, p0 + tail, p1, None], *ok[2:]),
        "a misaligned peer pointer": (ok[0], [p0, p0 + tail, p1, p1 + 2], *ok[2:]),
        "a misaligned half peer pointer": (ok[0], [p0, p0 + tail, p1, p1 + 1], 2, [M - 8, 8], [F32, F16], 2),
        "a null minuend pointer": ([pm, None], *ok[1:]),
        "a misaligned minuend pointer": ([pm, pm + 2], *ok[1:]),
        "a host kind": (*ok[:4], [F32, ipls.HOST_F32], 2),
        "a negative length": (*ok[:3], [M, -1], [F32, F32], 2),
        "a negative count": (*ok[:5], -1),
        "null lengths": (*ok[:3], None, [F32, F32], 2),
    }
    ranged = {
        "a list that overruns a partition": (([pm, pm], [p0, p0, p1, p1], 2, [M - 3, 4], [F32, F32], 2), {}),
        "a partition that does not exist": (ok, dict(own=(ctypes.c_int32 * 2)(0, P), n_own=2)),
    }

    def refuse_all(agg):
        for what, args in bad.items():
            assert update(agg, *args) == INVAL, what
        for what, (args, kw) in ranged.items():
            assert update(agg, *args, **kw) == RANGE, what
        assert update(agg, *ok, own=None, n_own=2) == INVAL
        assert update(agg, *ok, n_own=-1) == INVAL
        for args, name in ((bad["a misaligned peer pointer"], "peer 1 segment 1"),
                           (bad["a null peer pointer"], "peer 1 segment 1"),
                           (bad["a misaligned minuend pointer"], "minuend segment 1")):
            assert update(agg, *args) == INVAL
            msg = agg._lib.ipls_agg_last_error(None).decode()
            assert name in msg, msg
        # the order of the checks: geometry, owned, then the lists (minuend before the peers)
        assert update(agg, [pm, None], [p0, p0, p1, None], 2, [M - 3, 4], [F32, F32], 2) == RANGE
        assert update(agg, [pm, None], ok[1], *ok[2:], own=(ctypes.c_int32 * 2)(0, P), n_own=2) == RANGE
        assert update(agg, [pm, None], [p0, p0 + tail, p1, None], *ok[2:]) == INVAL
        assert "minuend" in agg._lib.ipls_agg_last_error(None).decode()

    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        # a fresh handle: refused calls leave the accumulators logically zero
        refuse_all(agg)
        assert update(agg, *ok) == 0
        assert agg.last_launch()["start"] == ipls.START_ZERO
        acc = S.U.zeros(O, M, P)
        for v in (0.75, 0.5):
            acc = S.U.expected(O, acc, np.full(M, v), M, M, P, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), acc[p], f"AGG[{p}]")
        # preloaded targets and a queued arrival: nothing moves, and the arrival is still queued afterwards
        agg.reset()
        _preload(agg, np.random.default_rng(3))
        before = _state(agg)
        L = agg.lengths[1]
        first, second = np.random.default_rng(4).standard_normal((2, L))
        bucket = torch.from_numpy(first.copy()).cuda()
        torch.cuda.synchronize()
        ticket = agg.UpdateAsync(ipls.DeviceBuffer.from_tensor(bucket), 1)
        refuse_all(agg)
        bucket.copy_(torch.from_numpy(second))
        torch.cuda.synchronize()
        agg.Wait(ticket)
        after = _state(agg)
        want1 = before[4].view(np.float64) + second
        assert_bits_equal(after[4].view(np.float64), want1, "the queued arrival was folded by a refused call")
        for k, (a, b) in enumerate(zip(after, before)):
            assert k == 4 or np.array_equal(a, b), f"a refused call changed target {TARGETS[k % 4]} of {k // 4}"
        assert update(agg, None, ok[1], *ok[2:]) == 0                  # ... and the same tables do fold, minuend or none
        assert not _same(_state(agg), after)


# ---- no reads outside any list ----
@DEVICES
@pytest.mark.parametrize("name", ("aligned", "residues-f64", "residues-f32", "residues-half", "residues-bf16"))
def test_views_flush_against_the_end_of_their_allocation(ipls, O, T, devices, name):
    """Every view of every list ends where its allocation ends: results as ever."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    for with_received in (False, True):
        rec, peers = C.build(np.random.default_rng(77), name, c, T, 3, with_received)
        ups = [_upload_flush(segs) for segs in ([rec] if with_received else []) + peers]
        lists = [[v for _, v in u] for u in ups]
        pu = ipls.PeerUpdates(lists[1:], received=lists[0]) if with_received else ipls.PeerUpdates(lists)
        with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
            agg.UpdateGradient(pu, range(P))
            want = C.expected(O, S.U.zeros(O, M, P), rec, peers, c, range(P))
            for p in range(P):
                assert_bits_equal(agg.read(p), want[p], f"{name} received={with_received} AGG[{p}]")
        del ups


# ---- the Python surface ----
def test_only_update_gradient_takes_peer_updates(ipls, O, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    rec, peers = C.build(np.random.default_rng(12), "whole-f32", c, T, 2, True)
    (r, a, b), keep = _upload([rec] + peers)
    pu = ipls.PeerUpdates([a[0], b[0]], received=r[0])           # single tensors are one-segment lists
    assert (pu.n, pu.n_segs, pu.n_peers) == (M, 1, 2)
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        agg.UpdateGradient(pu, range(P))
        want = C.expected(O, S.U.zeros(O, M, P), rec, peers, c, range(P))
        for p in range(P):
            assert_bits_equal(agg.read(p), want[p], f"AGG[{p}]")
        for call in (lambda: agg.InitializeWeights(pu), lambda: agg.GetPartitions(out=pu), lambda: agg.Update(pu, 0),
                     lambda: agg.OrganizeGradients(pu), lambda: agg.SendGradients(pu, [0], 1)):
            with pytest.raises((TypeError, ValueError)):
                call()
