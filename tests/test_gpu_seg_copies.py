"""GetPartitions into K trainers' tensor lists in one launch on the GPU:
GetPartitions(out=ipls.ModelCopies) (ipls_agg_get_partitions_segs_copies;
k_divide_segs_copies), on one shard and on two shards of one GPU, plain and
secure.  Expected values come from the oracle alone (get_partitions, then the
format's narrowing -- seg_copies_cases.expected); GetPartitions(out=Segments)
of every list on the same handle is a second check, never the first.  Every
list lies in backing arrays of its own that are SENTINEL before the call, and
every byte outside the views' elements below the model size must still be
SENTINEL after it.  Layouts, planted values and expectations are
seg_copies_cases.py's.
"""
import ctypes
import functools

import numpy as np
import pytest

import seg_cases as S
import seg_copies_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -2
P = S.P
DEVICES = pytest.mark.parametrize("devices", (None, [0, 0]), ids=("one-shard", "two-shards"))
CHUNK = pytest.mark.parametrize("ci", range(3), ids=("c9", "cT+9", "c2T+25"))
SECURE = pytest.mark.parametrize("secure", (False, True), ids=("plain", "secure"))
LISTS = pytest.mark.parametrize("n_lists", C.NS, ids=[f"n{k}" for k in C.NS])
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
    """The segment kernels' tile, block x vectors, from one launch's record; the twin's tile."""
    a = torch.zeros(8, dtype=torch.float32, device="cuda")
    b = torch.zeros(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=8, n_partitions=1) as agg:
        agg.cache_partition(0, np.array([2.0] * 8 + [4.0]))
        agg.GetPartitions(out=ipls.Segments.from_tensors([a]))
        twin = agg.last_launch()
        agg.GetPartitions(out=ipls.ModelCopies([[a], [b]]))
        li = agg.last_launch()
        agg.sync()
        assert a.tolist() == b.tolist() == [0.5] * 8
    assert twin["kernel"] == ipls.KERNEL_DIVIDE_SEGS and li["kernel"] == ipls.KERNEL_DIVIDE_SEGS_COPIES == 19, (twin, li)
    assert (li["block"], li["vectors"]) == (twin["block"], twin["vectors"])
    assert li["block"] * li["vectors"] == S.TILE_DEFAULT
    return li["block"] * li["vectors"]


@functools.lru_cache(maxsize=None)
def _case(name, ci, T, secure):
    """(W, planted, expected bits per segment): computed once per case, shared and never changed."""
    from oracle import oracle as o
    c = S.chunks(T)[ci]
    w, where = C.weights(np.random.default_rng(70 + 10 * ci + S.LAYOUTS.index(name)), o, name, c, T)
    want = C.expected(o, w, C.out_spec(name, c, T), S.model_size(c), secure)
    for x in w + want:
        x.setflags(write=False)
    return w, where, want


def _upload(specs):
    """[[view tensor per segment] per list] and the one device buffer they lie in: every backing array of every
    list starts on a 128-B line of its own, the view r elements into it, every byte SENTINEL."""
    at, total = [], 0
    for sp in specs:
        for fmt, n, r in sp:
            at.append(total)
            total += -(-((r + n + S.PAD) * S.esize(fmt) + 1) // 128) * 128
    buf = torch.full((max(total, 128),), S.SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    out, k = [], 0
    for sp in specs:
        views = []
        for fmt, n, r in sp:
            nb = (r + n + S.PAD) * S.esize(fmt)
            v = buf[at[k]:at[k] + nb].view(TORCH_DTYPE[fmt])[r:r + n]
            assert v.is_contiguous() and (not n or v.data_ptr() == buf.data_ptr() + at[k] + r * S.esize(fmt))
            views.append(v)
            k += 1
        out.append(views)
    torch.cuda.synchronize()
    return out, buf, at


def _check_image(host, at, specs, want, what):
    """Every list's every segment bit-exact (NaN against NaN apart), every other byte of the buffer SENTINEL."""
    rest = host.copy()
    k = 0
    for li, sp in enumerate(specs):
        for i, (fmt, n, r) in enumerate(sp):
            esz = S.esize(fmt)
            m = want[i].size
            a = at[k] + r * esz
            mine = host[a:a + m * esz].view(S.bits_dtype(fmt))
            nan = S.is_nan(mine, fmt) & S.is_nan(want[i], fmt)
            bad = np.flatnonzero(mine[~nan] != want[i][~nan])
            assert bad.size == 0, f"{what}: list {li}, segment {i} ({fmt}), first at {bad[:4]} of {m}"
            rest[a:a + m * esz] = S.SENTINEL
            k += 1
    bad = np.flatnonzero(rest != S.SENTINEL)
    assert bad.size == 0, f"{what}: {bad.size} bytes outside the views were written, first at {bad[:4]}"


def _load(agg, w):
    for p in range(P):
        agg.cache_partition(p, w[p])


# ---- every layout ----
@DEVICES
@CHUNK
@SECURE
@LISTS
def test_every_layout(ipls, O, T, devices, ci, secure, n_lists):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        for name in C.layouts(c):
            w, where, want = _case(name, ci, T, secure)
            _load(agg, w)
            spec = C.out_spec(name, c, T)
            specs = [C.list_spec(spec, k) for k in range(n_lists)]
            views, buf, at = _upload(specs)
            mc = ipls.ModelCopies(views)
            assert (mc.n, mc.n_segs, mc.n_lists) == (sum(s[1] for s in spec), len(spec), n_lists)
            assert agg.GetPartitions(out=mc) is mc
            info = agg.last_launch()
            agg.sync()
            assert info["kernel"] == ipls.KERNEL_DIVIDE_SEGS_COPIES and info["block"] * info["vectors"] == T, info
            if devices is None:   # one launch whatever n_lists: the twin's items over list 0
                assert info["grid"] == S.n_divide_items(spec, M, T), (name, info)
            host = buf.cpu().numpy()
            _check_image(host, at, specs, want, f"{name} c={c} n_lists={n_lists}")
            # the planted NaNs are NaNs in every list (the comparison above skipped exactly those)
            st = np.concatenate([[0], np.cumsum([s[1] for s in spec])])
            for f, q in where.items():
                if q == "nan":
                    i = int(np.searchsorted(st, f, side="right")) - 1
                    for li, sp in enumerate(specs):
                        fmt, n, r = sp[i]
                        a = at[li * len(spec) + i] + (r + f - int(st[i])) * S.esize(fmt)
                        assert S.is_nan(host[a:a + S.esize(fmt)].view(S.bits_dtype(fmt)), fmt)[0], (name, f, li)
            # second check: the twin on every list alone, same handle, into a second buffer
            views2, buf2, at2 = _upload(specs)
            for v in views2:
                agg.GetPartitions(out=ipls.Segments.from_tensors(v))
            assert agg.last_launch()["kernel"] == ipls.KERNEL_DIVIDE_SEGS
            agg.sync()
            assert at2 == at and np.array_equal(buf2.cpu().numpy(), host), f"{name}: the twin's bytes differ"
            del views, views2, mc


# ---- one list ----
@DEVICES
@SECURE
def test_one_list_is_the_twin_by_its_own_kernel(ipls, O, T, devices, secure):
    c = S.chunks(T)[2]
    M = S.model_size(c)
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices, secure=secure) as agg:
        for name in ("residues-bf16", "tiny", "aligned"):
            w, _, want = _case(name, 2, T, secure)
            _load(agg, w)
            specs = [C.out_spec(name, c, T)]
            (a,), buf_a, at = _upload(specs)
            (b,), buf_b, _ = _upload(specs)
            agg.GetPartitions(out=ipls.ModelCopies([a]))
            assert agg.last_launch()["kernel"] == ipls.KERNEL_DIVIDE_SEGS_COPIES
            agg.GetPartitions(out=ipls.Segments.from_tensors(b))
            assert agg.last_launch()["kernel"] == ipls.KERNEL_DIVIDE_SEGS
            agg.sync()
            ha, hb = buf_a.cpu().numpy(), buf_b.cpu().numpy()
            assert np.array_equal(ha, hb), name
            _check_image(ha, at, specs, want, f"{name} one list")


# ---- PeerUpdates.outputs() ----
@DEVICES
@pytest.mark.parametrize("with_received", (False, True), ids=("plain", "received"))
def test_peer_updates_outputs(ipls, O, T, devices, with_received):
    """The round's way out: received (when there is one) and every trained list get the model."""
    ci, name, K = 1, "aligned", 3
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    w, _, want = _case(name, ci, T, False)
    spec = C.out_spec(name, c, T)
    n = K + (1 if with_received else 0)
    specs = [C.list_spec(spec, k) for k in range(n)]
    views, buf, at = _upload(specs)
    pu = ipls.PeerUpdates(views[1:], received=views[0]) if with_received else ipls.PeerUpdates(views)
    out = pu.outputs()
    assert isinstance(out, ipls.ModelCopies) and out.n_lists == n and out.n_segs == pu.n_segs and out.n == pu.n
    assert [x.tensors for x in out.lists] == [tuple(v) for v in views]
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _load(agg, w)
        with pytest.raises(TypeError):
            agg.GetPartitions(out=pu)
        agg.sync()
        assert (buf.cpu().numpy() == S.SENTINEL).all()
        agg.GetPartitions(out=out)
        agg.sync()
    _check_image(buf.cpu().numpy(), at, specs, want, f"outputs() received={with_received}")


# ---- no stores outside any list ----
@DEVICES
@pytest.mark.parametrize("name", ("aligned", "residues-f64", "residues-f32", "residues-half", "residues-bf16"))
def test_views_flush_against_the_end_of_their_allocation(ipls, O, T, devices, name):
    """Every view of every list ends where its allocation ends: results as ever."""
    ci = 2
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    w, _, want = _case(name, ci, T, False)
    spec = C.out_spec(name, c, T)
    specs = [C.list_spec(spec, k) for k in range(3)]
    ups = []
    for sp in specs:
        row = []
        for fmt, n, r in sp:
            b = torch.full(((r + n) * S.esize(fmt),), S.SENTINEL, dtype=torch.uint8, device="cuda")
            v = b.view(TORCH_DTYPE[fmt])[r:r + n]
            assert not n or v.data_ptr() + n * S.esize(fmt) == b.data_ptr() + b.numel()
            row.append((b, v))
        ups.append(row)
    torch.cuda.synchronize()
    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _load(agg, w)
        agg.GetPartitions(out=ipls.ModelCopies([[v for _, v in row] for row in ups]))
        agg.sync()
    for li, (sp, row) in enumerate(zip(specs, ups)):
        for i, ((fmt, n, r), (b, _)) in enumerate(zip(sp, row)):
            got = b.cpu().numpy().view(S.bits_dtype(fmt))
            m = want[i].size
            mine = got[r:r + m]
            nan = S.is_nan(mine, fmt) & S.is_nan(want[i], fmt)
            assert np.array_equal(mine[~nan], want[i][~nan]), f"{name}: list {li}, segment {i}"
            junk = np.concatenate([got[:r], got[r + m:]]).view(np.uint8)
            assert (junk == S.SENTINEL).all(), f"{name}: bytes around list {li}'s segment {i} were written"


# ---- refusals ----
@DEVICES
def test_refusals_leave_every_list(ipls, O, T, devices):
    ci, name, K = 1, "aligned", 3
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    w, _, want = _case(name, ci, T, False)
    spec = C.out_spec(name, c, T)
    specs = [C.list_spec(spec, k) for k in range(K)]
    views, buf, at = _upload(specs)
    k = len(spec)
    ptrs = [int(v.data_ptr()) if v.numel() else None for row in views for v in row]
    ns = [s[1] for s in spec]
    kinds = [S.KIND[s[0]] for s in spec]
    live = [i for i, s in enumerate(spec) if s[1]]

    def call(agg, ptrs, n_lists, ns, kinds, n_segs):
        a = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
        b = (ctypes.c_int64 * max(len(ns), 1))(*ns)
        d = (ctypes.c_int32 * max(len(kinds), 1))(*kinds)
        return agg._lib.ipls_agg_get_partitions_segs_copies(agg._h, a, n_lists, b, d, n_segs)

    def untouched(what):
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == S.SENTINEL).all(), f"{what} wrote to a list"

    with ipls.Aggregator(model_size=M, n_partitions=P, devices=devices) as agg:
        _load(agg, w)
        # a short list and an empty list: the model does not fit
        first = live[0]
        short = list(ns)
        last_model = max(i for i in live if i < k - 3)
        short[last_model] -= 1
        short[k - 3:] = [0, 0, 0]
        assert sum(short) == M - 1
        assert call(agg, ptrs, K, short, kinds, k) == RANGE
        untouched("a short list")
        assert call(agg, ptrs, K, [], [], 0) == RANGE
        untouched("an empty list")
        with pytest.raises(ipls.IplsError) as e:
            agg.GetPartitions(out=ipls.ModelCopies([[], []]))
        assert e.value.code == RANGE
        # a misaligned pointer in list 2: named by segment and list
        seg = next(i for i in live if spec[i][0] != "half" and spec[i][0] != "bf16")
        bad = list(ptrs)
        bad[2 * k + seg] += 2
        assert call(agg, bad, K, ns, kinds, k) == INVAL
        msg = agg._lib.ipls_agg_last_error(None).decode()
        assert f"segment {seg}" in msg and "list 2" in msg and "aligned" in msg, msg
        untouched("a misaligned pointer in list 2")
        bad = list(ptrs)
        bad[1 * k + first] = None
        assert call(agg, bad, K, ns, kinds, k) == INVAL
        msg = agg._lib.ipls_agg_last_error(None).decode()
        assert f"segment {first}" in msg and "list 1" in msg and "null" in msg, msg
        untouched("a NULL pointer")
        assert call(agg, ptrs, 0, ns, kinds, k) == INVAL
        untouched("n_lists 0")
        assert call(agg, ptrs + [None] * (k * (1026 - K)), 1026, ns, kinds, k) == INVAL
        untouched("n_lists 1026")
        assert call(agg, None, K, ns, kinds, k) == INVAL
        untouched("a NULL table")
        # the pointer of an empty segment is not looked at, and the table itself is fine
        ok = list(ptrs)
        for i, s in enumerate(spec):
            if not s[1]:
                for li in range(K):
                    ok[li * k + i] = 3
        assert call(agg, ok, K, ns, kinds, k) == 0
        agg.sync()
    _check_image(buf.cpu().numpy(), at, specs, want, "after the refusals")


# ---- the Python surface ----
def test_only_get_partitions_takes_model_copies(ipls, O, T):
    c = S.chunks(T)[1]
    M = S.model_size(c)
    a = torch.zeros(M, dtype=torch.float32, device="cuda")
    b = torch.zeros(M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mc = ipls.ModelCopies([a, b])            # single tensors are one-segment lists
    assert (mc.n, mc.n_segs, mc.n_lists) == (M, 1, 2)
    with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
        for call in (lambda: agg.InitializeWeights(mc), lambda: agg.UpdateGradient(mc, range(P)),
                     lambda: agg.Update(mc, 0), lambda: agg.OrganizeGradients(mc), lambda: agg.SendGradients(mc, [0], 1),
                     lambda: agg.GetPartitions(out=ipls.PeerUpdates([a, b]))):
            with pytest.raises(TypeError):
                call()
        w, _, _ = _case("whole-f32", 1, T, False)
        _load(agg, w)
        agg.GetPartitions(out=mc)
        agg.sync()
        flat = agg.GetPartitions(dtype=np.float32)
    for t in (a, b):
        got = t.cpu().numpy()
        nan = np.isnan(got) & np.isnan(flat)
        assert np.array_equal(got.view(np.uint32)[~nan], flat.view(np.uint32)[~nan])
