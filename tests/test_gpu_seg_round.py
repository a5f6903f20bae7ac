"""The many-trainers round over tensor lists in one launch on the GPU:
Aggregator.round_peers (ipls_agg_round_segs_peers; k_round_segs_peers), on one
shard and on two shards of one GPU, plain and secure.  Expected values come
from the oracle alone (seg_round_cases.expected: the peer-list fold, the
oracle's aggregate_partition, the copy-list divide, all from the inputs as they
were before the call); the three existing calls on a second handle from the
same starts are a second check, never the first.  In place the outputs ARE the
inputs; every byte of the one buffer all lists lie in is compared, the junk
around the views included.  A NaN is compared as a NaN only.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal
import seg_cases as S
import seg_round_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -2
P = S.P
AGG, REP, W = 0, 1, 2
DEVICES = pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
CHUNK = pytest.mark.parametrize("ci", range(3), ids=("c9", "cT+9", "c2T+25"))
SECURE = pytest.mark.parametrize("secure", (False, True), ids=("plain", "secure"))
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
    r = torch.full((8,), 3.0, dtype=torch.float32, device="cuda")
    a = torch.ones(8, dtype=torch.float32, device="cuda")
    b = torch.full((8,), 2.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
        agg.UpdateGradient(ipls.PeerUpdates([[a]]), [0])
        twin = agg.last_launch()
        agg.reset()
        out = agg.round_peers(ipls.PeerUpdates([[a], [b]], received=[r]), [0])
        li = agg.last_launch()
        agg.sync()
        assert isinstance(out, ipls.ModelCopies) and out.n_lists == 3
        assert agg.read(0, W).tolist() == [3.0] * 8 + [2.0]          # (3 - 1) + (3 - 2), two trainers
        assert r.tolist() == a.tolist() == b.tolist() == [1.5] * 8
    assert twin["kernel"] == ipls.KERNEL_UPDATE_SEGS_PEERS and li["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS == 20, li
    assert (li["block"], li["vectors"]) == (twin["block"], twin["vectors"])
    assert li["block"] * li["vectors"] == S.TILE_DEFAULT
    return li["block"] * li["vectors"]


# ---- memory ----
def _layout(backings):
    at, total = [], 0
    for row in backings:
        for b in row:
            at.append(total)
            total += -(-(b.nbytes + 1) // 128) * 128
    return at, max(total, 128)


def _upload(backings, specs):
    """[[view tensor per segment] per list], the ONE device buffer they lie in, the host bytes it was made from and
    the backing arrays' offsets: every backing array starts on a 128-B line of its own, the view r elements in."""
    at, total = _layout(backings)
    host = np.full(total, S.SENTINEL, dtype=np.uint8)
    k = 0
    for row in backings:
        for b in row:
            host[at[k]:at[k] + b.nbytes] = np.ascontiguousarray(b).view(np.uint8)
            k += 1
    buf = torch.from_numpy(host.copy()).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 128 == 0
    out, k = [], 0
    for row, sp in zip(backings, specs):
        views = []
        for b, (fmt, n, r) in zip(row, sp):
            v = buf[at[k]:at[k] + b.nbytes].view(TORCH_DTYPE[fmt])[r:r + n]
            assert v.is_contiguous() and (not n or v.data_ptr() == buf.data_ptr() + at[k] + r * S.esize(fmt))
            views.append(v)
            k += 1
        out.append(views)
    return out, buf, host, at


def _upload_inputs(case):
    lists = case.inputs()
    return _upload([[s.backing for s in segs] for segs in lists], [[(s.fmt, s.n, s.r) for s in segs] for segs in lists])


def _peer_updates(ipls, case, views):
    return ipls.PeerUpdates(views[1:], received=views[0]) if case.rec is not None else ipls.PeerUpdates(views)


def _check_image(host, at, specs, mem, what):
    """Every backing array of every list: the views' elements bit-exact (a NaN against a NaN apart), every other
    byte of the buffer exactly as expected."""
    want = np.full(host.size, S.SENTINEL, dtype=np.uint8)
    k = 0
    for li, sp in enumerate(specs):
        for i, (fmt, n, r) in enumerate(sp):
            m = mem[li][i]
            esz = S.esize(fmt)
            a = at[k] + r * esz
            mine = host[a:a + n * esz].view(S.bits_dtype(fmt))
            exp = m[r * esz:(r + n) * esz].view(S.bits_dtype(fmt))
            nan = S.is_nan(mine, fmt) & S.is_nan(exp, fmt)
            bad = np.flatnonzero(mine[~nan] != exp[~nan])
            assert bad.size == 0, f"{what}: list {li}, segment {i} ({fmt}), first at {bad[:4]} of {n}"
            want[at[k]:at[k] + m.size] = m
            want[a:a + n * esz] = host[a:a + n * esz]
            k += 1
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes outside the views differ, first at {bad[:4]}"


# ---- the handle's state ----
def _put(ipls, agg, p, target, x, keep):
    """target[p] := x, bit for bit (a -0.0 stays -0.0)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).copy()).cuda()
    torch.cuda.synchronize()
    keep.append(t)
    agg.reduce_batch(p, [[ipls.DeviceBuffer.from_tensor(t)]], start_mode=ipls.START_FIRST, target=target)


def _set_state(ipls, agg, case):
    keep = []
    agg.reset()
    for p in range(P):
        agg.cache_partition(p, case.w0[p])
        if case.agg0 is not None:
            _put(ipls, agg, p, AGG, case.agg0[p], keep)
        if case.rep0[p] is not None:
            _put(ipls, agg, p, REP, case.rep0[p], keep)
    agg.sync()


def _three_calls(ref, pu, owned, out):
    ref.UpdateGradient(pu, owned)
    for p in dict.fromkeys(owned):
        ref.AggregatePartition(p)
    ref.GetPartitions(out=out)


def _check_state(agg, case, Wexp, what):
    for p in range(P):
        assert_bits_equal(agg.read(p, W), Wexp[p], f"{what} W[{p}]")
    for p in range(P):
        a, r = agg.read(p, AGG), agg.read(p, REP)
        if p in case.owned:   # left in place, flagged logically zero
            assert not a.any() and not np.signbit(a).any() and not r.any() and not np.signbit(r).any(), (what, p)
        else:
            assert_bits_equal(a, case.agg0[p] if case.agg0 is not None else np.zeros(a.size), f"{what} AGG[{p}]")
            assert_bits_equal(r, case.rep0[p] if case.rep0[p] is not None else np.zeros(r.size), f"{what} REP[{p}]")


def _last_shard_parts(ipls, devices):
    if devices is None:
        return list(range(P))
    owner = ipls.shard_plan(P, len(devices))
    return [p for p in range(P) if owner[p] == max(owner)]


# ---- the main case: in place ----
@DEVICES
@CHUNK
@SECURE
def test_round_in_place_every_layout(ipls, O, T, devices, ci, secure):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    mine = _last_shard_parts(ipls, devices)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg, \
            ipls.Aggregator(model_size=M, n_partitions=P, secure=secure) as ref:
        for li, name in enumerate(C.layouts(c, T)):
            for rot in range(2):
                K = C.KS[(li + rot + ci) % 4]
                own = list(C.OWNED)[(li + 2 * rot + int(secure)) % 4]
                start = C.STARTS[(li + 3 * rot + ci + 2 * int(secure)) % 4]
                case = C.build(O, 900 + 100 * ci + 10 * li + rot, name, c, T, K, C.OWNED[own], start,
                               (li + rot) % 3 != 1, secure=secure)
                what = f"{name} c={c} K={K} owned={own} start={start} received={case.rec is not None}"
                Wexp, mem = C.expected_image(O, case)
                views, buf, host0, at = _upload_inputs(case)
                pu = _peer_updates(ipls, case, views)
                _set_state(ipls, agg, case)
                out = agg.round_peers(pu, case.owned)
                info = agg.last_launch()
                agg.sync()
                assert isinstance(out, ipls.ModelCopies) and out.n_lists == len(views)
                assert info["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS and info["block"] * info["vectors"] == T, info
                assert info["grid"] == S.n_update_items(O, c, T, mine), (what, info)   # every partition, owned or not
                host = buf.cpu().numpy()
                _check_image(host, at, case.list_specs(), mem, what)
                _check_state(agg, case, Wexp, what)
                # second check: the three existing calls on a second handle from the same starts
                views2, buf2, _, at2 = _upload_inputs(case)
                pu2 = _peer_updates(ipls, case, views2)
                _set_state(ipls, ref, case)
                _three_calls(ref, pu2, case.owned, pu2.outputs())
                ref.sync()
                assert at2 == at and np.array_equal(buf2.cpu().numpy(), host), f"{what}: the three calls' bytes differ"
                for p in range(P):
                    assert np.array_equal(agg.read(p, W).view(np.uint64), ref.read(p, W).view(np.uint64)), (what, p)
                del views, views2, pu, pu2, out


# ---- separate outputs ----
@DEVICES
@CHUNK
@SECURE
def test_separate_outputs_leave_the_inputs(ipls, O, T, devices, ci, secure):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        for li, name in enumerate(C.layouts(c, T)):
            K = C.KS[(li + ci + 1) % 4]
            n_lists = C.n_lists_of(K)[(li + ci) % 3]
            own = list(C.OWNED)[(li + ci) % 4]
            case = C.build(O, 40 + 10 * ci + li, name, c, T, K, C.OWNED[own], C.STARTS[(li + 1) % 4], li % 2 == 0,
                           secure=secure, n_lists=n_lists)
            what = f"{name} c={c} K={K} n_lists={n_lists} owned={own} start={case.start}"
            Wexp, mem = C.expected_image(O, case)
            views, buf, host0, _ = _upload_inputs(case)
            oviews, obuf, _, oat = _upload(C.blank(case), case.out_specs)
            _set_state(ipls, agg, case)
            mc = ipls.ModelCopies(oviews)
            assert agg.round_peers(_peer_updates(ipls, case, views), case.owned, out=mc) is mc
            assert agg.last_launch()["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS
            agg.sync()
            assert np.array_equal(buf.cpu().numpy(), host0), f"{what}: an input list was written"
            _check_image(obuf.cpu().numpy(), oat, case.out_specs, mem, what)
            _check_state(agg, case, Wexp, what)
            del views, oviews, mc


# ---- two rounds back to back ----
@DEVICES
@SECURE
def test_two_rounds_back_to_back(ipls, O, T, devices, secure):
    """The second round's received model and trainers are the first round's output: every update is x - x, the
    accumulators start from logical zeros again and the count is K * mult again."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        for name, K, own in (("aligned", 3, "all"), ("residues-bf16", 2, "twice"), ("tiny", 5, "subset")):
            case = C.build(O, 5, name, c, T, K, C.OWNED[own], "both", True, secure=secure)
            views, buf, _, at = _upload_inputs(case)
            pu = _peer_updates(ipls, case, views)
            _set_state(ipls, agg, case)
            agg.round_peers(pu, case.owned)
            agg.round_peers(pu, case.owned)
            assert agg.last_launch()["start"] == ipls.START_ZERO
            agg.sync()
            W2 = C.second_round(O, case)
            for p in range(P):
                assert_bits_equal(agg.read(p, W), W2[p], f"{name} second round W[{p}]")
            for p in set(case.owned):
                w = agg.read(p, W)
                assert w[-1] == float(K * case.owned.count(p)), "the count starts again"
                fin = np.isfinite(w[:-1])
                assert not w[:-1][fin].any(), "x - x folded over logical zeros is +0.0"
            stale = C.second_round(O, case, stale_flag=True)
            assert not C.same_w_nan(W2, stale)


# ---- queued arrivals ----
@DEVICES
@SECURE
def test_queued_arrivals_fold_first(ipls, O, T, devices, secure):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    case = C.build(O, 9, "whole-f32", c, T, 3, C.OWNED["all"], "agg", True, secure=secure)
    views, buf, _, at = _upload_inputs(case)
    pu = _peer_updates(ipls, case, views)
    rng = np.random.default_rng(10)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        _set_state(ipls, agg, case)
        tickets, keep = [], []
        for p in (2, 7):
            arrival = rng.standard_normal(agg.lengths[p]) * 2.0 ** 60    # folded later, it would round differently
            arrival[-1] = 2.0
            bucket = torch.from_numpy(arrival.copy()).cuda()
            keep.append(bucket)
            torch.cuda.synchronize()
            tickets.append(agg.UpdateAsync(ipls.DeviceBuffer.from_tensor(bucket), p))
            case.agg0[p] = case.agg0[p] + arrival
        Wexp, mem = C.expected_image(O, case)
        agg.round_peers(pu, case.owned)
        for t in tickets:
            agg.Wait(t)
        agg.sync()
        _check_image(buf.cpu().numpy(), at, case.list_specs(), mem, "queued arrivals")
        for p in range(P):
            assert_bits_equal(agg.read(p, W), Wexp[p], f"W[{p}]")


# ---- one peer, one list ----
@DEVICES
@SECURE
def test_one_peer_one_list_against_the_twins(ipls, O, T, devices, secure):
    c = S.chunks(T)[2]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg, \
            ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as twin:
        for li, name in enumerate(("aligned", "residues-f64", "whole-half", "tiny")):
            case = C.build(O, 70 + li, name, c, T, 1, C.OWNED["all"], C.STARTS[li], li % 2 == 0, secure=secure,
                           n_lists=1)
            Wexp, mem = C.expected_image(O, case)
            views, buf, host0, _ = _upload_inputs(case)
            (oa,), obuf_a, _, oat = _upload(C.blank(case), case.out_specs)
            (ob,), obuf_b, _, _ = _upload(C.blank(case), case.out_specs)
            pu = _peer_updates(ipls, case, views)
            _set_state(ipls, agg, case)
            _set_state(ipls, twin, case)
            agg.round_peers(pu, case.owned, out=ipls.ModelCopies([oa]))
            assert agg.last_launch()["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS
            _three_calls(twin, pu, case.owned, ipls.ModelCopies([ob]))
            assert twin.last_launch()["kernel"] == ipls.KERNEL_DIVIDE_SEGS_COPIES
            agg.sync(), twin.sync()
            ha = obuf_a.cpu().numpy()
            assert np.array_equal(ha, obuf_b.cpu().numpy()), name
            _check_image(ha, oat, case.out_specs, mem, f"{name} one peer, one list")
            for p in range(P):
                assert np.array_equal(agg.read(p, W).view(np.uint64), twin.read(p, W).view(np.uint64)), (name, p)


# ---- refusals ----
def _arr(t, vals):
    return (t * max(len(vals), 1))(*vals) if vals is not None else None


@DEVICES
@SECURE
def test_refusals_leave_everything(ipls, O, T, devices, secure):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    K = 2
    case = C.build(O, 3, "aligned", c, T, K, C.OWNED["all"], "both", True, secure=secure)
    spec = case.spec
    k = len(spec)
    views, buf, host0, at = _upload_inputs(case)
    ptrs = [[int(v.data_ptr()) if v.numel() else None for v in row] for row in views]
    m_ptrs, t_ptrs, o_ptrs = ptrs[0], ptrs[1] + ptrs[2], ptrs[0] + ptrs[1] + ptrs[2]
    ns = [s[1] for s in spec]
    kinds = [S.KIND[s[0]] for s in spec]
    live = [i for i, s in enumerate(spec) if s[1]]
    wide = next(i for i in live if spec[i][0] in ("f64", "f32"))
    owned = list(range(P))
    short = S.shape("short-a", c, T)

    def call(agg, m=m_ptrs, t=t_ptrs, n_peers=K, o=o_ptrs, n_lists=K + 1, ns=ns, kinds=kinds, n_segs=k, own=owned,
             n_own=None):
        return agg._lib.ipls_agg_round_segs_peers(
            agg._h, _arr(ctypes.c_void_p, m), _arr(ctypes.c_void_p, t), n_peers, _arr(ctypes.c_void_p, o), n_lists,
            _arr(ctypes.c_int64, ns), _arr(ctypes.c_int32, kinds), n_segs, _arr(ctypes.c_int32, own),
            len(own) if n_own is None and own is not None else (n_own or 0))

    def edit(lst, i, v):
        out = list(lst)
        out[i] = v if not callable(v) else v(out[i])
        return out

    def refuse_all(agg):
        msg = lambda: agg._lib.ipls_agg_last_error(None).decode()   # noqa: E731
        for what, kw in {
                "no peers": dict(n_peers=0), "too many peers": dict(n_peers=ipls.SEG_PEERS_MAX + 1),
                "no lists": dict(n_lists=0), "too many lists": dict(n_lists=ipls.SEG_COPIES_MAX + 1),
                "a null peer table": dict(t=None), "a null output table": dict(o=None),
                "a null owned list": dict(own=None, n_own=2), "a negative owned count": dict(n_own=-1),
                "a host kind": dict(kinds=edit(kinds, wide, ipls.HOST_F32)),
                "a negative length": dict(ns=edit(ns, wide, -1)),
                "a null minuend pointer": dict(m=edit(m_ptrs, wide, None)),
                "a misaligned peer pointer": dict(t=edit(t_ptrs, k + wide, lambda x: x + 2)),
                "a null output pointer": dict(o=edit(o_ptrs, 2 * k + wide, None)),
                "a misaligned output pointer": dict(o=edit(o_ptrs, k + wide, lambda x: x + 2))}.items():
            assert call(agg, **kw) == INVAL, what
        assert call(agg, own=[0, P]) == RANGE
        # a short list (the model does not fit) and a long one (it overruns a partition)
        sn = [s[1] for s in short]
        sk = [S.KIND[s[0]] for s in short]
        some = [int(buf.data_ptr())] * len(short)
        assert sum(sn) < M and call(agg, m=some, t=some * K, o=some * (K + 1), ns=sn, kinds=sk, n_segs=len(short)) == RANGE
        assert "model size" in msg()
        assert call(agg, ns=edit(ns, live[-1], lambda x: x + c)) == RANGE
        assert "overruns" in msg()
        # the order: n_peers / n_lists, geometry, owned, the minuend, the peers, the size, the lists
        assert call(agg, t=edit(t_ptrs, k + wide, lambda x: x + 2), o=edit(o_ptrs, wide, None)) == INVAL
        assert f"segment {wide}" in msg() and "peer 1" in msg(), msg()
        assert call(agg, m=edit(m_ptrs, wide, None), t=edit(t_ptrs, wide, None)) == INVAL
        assert "minuend" in msg(), msg()
        assert call(agg, o=edit(o_ptrs, 2 * k + wide, lambda x: x + 2)) == INVAL
        assert f"segment {wide}" in msg() and "list 2" in msg() and "aligned" in msg(), msg()
        assert call(agg, own=[0, P], m=edit(m_ptrs, wide, None)) == RANGE
        assert call(agg, n_peers=0, own=[0, P]) == INVAL

    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        # a fresh handle: refused calls leave the accumulators logically zero
        refuse_all(agg)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), host0), "a refused call wrote to a list"
        # preloaded targets and a queued arrival: nothing moves, and the arrival is still queued afterwards
        _set_state(ipls, agg, case)
        before = [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in (AGG, REP, W)]
        L = agg.lengths[1]
        first, second = np.random.default_rng(4).standard_normal((2, L))
        bucket = torch.from_numpy(first.copy()).cuda()
        torch.cuda.synchronize()
        ticket = agg.UpdateAsync(ipls.DeviceBuffer.from_tensor(bucket), 1)
        refuse_all(agg)
        bucket.copy_(torch.from_numpy(second))
        torch.cuda.synchronize()
        agg.Wait(ticket)
        after = [agg.read(p, t).view(np.uint64).copy() for p in range(P) for t in (AGG, REP, W)]
        assert_bits_equal(after[3].view(np.float64), before[3].view(np.float64) + second,
                          "the queued arrival was folded by a refused call")
        for i, (a, b) in enumerate(zip(after, before)):
            assert i == 3 or np.array_equal(a, b), f"a refused call changed target {i % 3} of partition {i // 3}"
        assert np.array_equal(buf.cpu().numpy(), host0), "a refused call wrote to a list"
        # ... and the same tables do run
        assert call(agg) == 0
        assert agg.last_launch()["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS
        agg.sync()
        case.agg0[1] = case.agg0[1] + second
        Wexp, mem = C.expected_image(O, case)
        _check_image(buf.cpu().numpy(), at, case.list_specs(), mem, "after the refusals")
        for p in range(P):
            assert_bits_equal(agg.read(p, W), Wexp[p], f"after the refusals W[{p}]")
    # a fresh handle after refusals only: the flags are still logically zero
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        refuse_all(agg)
        assert call(agg) == 0 and agg.last_launch()["start"] == ipls.START_ZERO


# ---- no access outside any list ----
@DEVICES
@pytest.mark.parametrize("name", ("aligned", "residues-f64", "residues-f32", "residues-half", "residues-bf16"))
@SECURE
def test_views_flush_against_the_end_of_their_allocation(ipls, O, T, devices, name, secure):
    """Every view of every list ends where its allocation ends: results as ever, in place."""
    c = S.chunks(T)[2]
    M = S.model_size(c)
    case = C.build(O, 77, name, c, T, 3, C.OWNED["subset"], "rep", True, secure=secure)
    Wexp, mem = C.expected_image(O, case)
    ups = []
    for segs in case.inputs():
        row = []
        for s in segs:
            raw = np.ascontiguousarray(s.backing[:s.r + s.n]).view(np.uint8)
            b = torch.from_numpy(raw.copy()).cuda()
            v = b.view(TORCH_DTYPE[s.fmt])[s.r:s.r + s.n]
            assert not s.n or v.data_ptr() + s.n * S.esize(s.fmt) == b.data_ptr() + b.numel()
            row.append((b, v))
        ups.append(row)
    torch.cuda.synchronize()
    lists = [[v for _, v in row] for row in ups]
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        _set_state(ipls, agg, case)
        agg.round_peers(ipls.PeerUpdates(lists[1:], received=lists[0]), case.owned)
        agg.sync()
        for p in range(P):
            assert_bits_equal(agg.read(p, W), Wexp[p], f"{name} W[{p}]")
    for li, (segs, row) in enumerate(zip(case.inputs(), ups)):
        for i, (s, (b, _)) in enumerate(zip(segs, row)):
            got = b.cpu().numpy()
            exp = mem[li][i][:got.size]
            esz = S.esize(s.fmt)
            a, e = got[s.r * esz:].view(S.bits_dtype(s.fmt)), exp[s.r * esz:].view(S.bits_dtype(s.fmt))
            nan = S.is_nan(a, s.fmt) & S.is_nan(e, s.fmt)
            assert np.array_equal(a[~nan], e[~nan]), f"{name}: list {li}, segment {i}"
            assert np.array_equal(got[:s.r * esz], exp[:s.r * esz]), f"{name}: bytes before list {li}'s segment {i}"


# ---- the Python surface ----
def test_value_and_type_errors(ipls, O, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    f = lambda n=M, d=torch.float32: torch.zeros(n, dtype=d, device="cuda")   # noqa: E731
    r, a, b = f(), f(), f()
    torch.cuda.synchronize()
    pu = ipls.PeerUpdates([a, b], received=r)
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        for p in range(P):
            agg.cache_partition(p, np.full(agg.lengths[p], 2.0))
        before = [agg.read(p, W).copy() for p in range(P)]
        for bad in (ipls.ModelCopies([f(M - 1)]), ipls.ModelCopies([[f(M - 1), f(1)]]),
                    ipls.ModelCopies([f(M, torch.float16)])):
            with pytest.raises(ValueError):
                agg.round_peers(pu, range(P), out=bad)
        for bad in (ipls.Segments.from_tensors([a]), [a], a, None, ipls.Difference(r, a), ipls.ModelCopies([a])):
            with pytest.raises(TypeError):
                agg.round_peers(bad, range(P))
        for bad in (ipls.Segments.from_tensors([a]), [a], pu, ipls.DeviceBuffer.from_tensor(a)):
            with pytest.raises(TypeError):
                agg.round_peers(pu, range(P), out=bad)
        for p in range(P):
            assert np.array_equal(agg.read(p, W), before[p])
        # n_owned == 0 is the divide into the lists alone
        out = agg.round_peers(pu, [])
        li = agg.last_launch()
        assert li["kernel"] == ipls.KERNEL_ROUND_SEGS_PEERS and li["start"] == 0, li   # nothing starts: as the divide twins
        agg.sync()
        assert out.n_lists == 3 and r.tolist() == a.tolist() == b.tolist() == [1.0] * M
