"""The peer-list call without a GPU: the shared cases (seg_peers_cases.py)
cover what they claim to cover, the planted triples do what they are planted
for, numpy models of the mistakes a peer-list kernel can make each change an
expected bit of the accumulators, the header and the binding declare the call
and its kernel id, a NULL handle is refused, and ipls.PeerUpdates refuses
mismatched lists before any library call.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import seg_cases as S
import seg_peers_cases as C

torch = pytest.importorskip("torch")

CALL = "ipls_agg_update_gradient_segs_peers"
T = S.TILE_DEFAULT


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def _bits(parts):
    return [np.ascontiguousarray(p).view(np.uint64) for p in parts]


def _differ(a, b):
    """Some element differs in its bits, NaNs compared as NaN only."""
    for x, y in zip(_bits(a), _bits(b)):
        xf, yf = x.view(np.float64), y.view(np.float64)
        nan = np.isnan(xf) & np.isnan(yf)
        if not np.array_equal(x[~nan], y[~nan]):
            return True
    return False


# ---- the cases ----
def test_layouts_cover_their_cases():
    whole, spans = C.check_coverage(T)
    assert {f for f, mixed in whole if mixed} == set(C.FMTS)
    for G in C.GROUPS:   # a peer on both sides of every group seam
        assert any(k > G for k in C.KS) and any(k <= G for k in C.KS), G
    for c in S.chunks(T):
        for name in C.LAYOUTS:
            spec = S.shape(name, c, T)
            assert C.peer_spec(spec, 0) == spec
            for k in C.KS:
                ps = C.peer_spec(spec, k)
                assert [(f, n) for f, n, _ in ps] == [(f, n) for f, n, _ in spec]
                assert all(0 <= r < S.residues(f) for f, _, r in ps)


@pytest.mark.parametrize("fmt", C.FMTS)
def test_triples_depend_on_the_order(fmt):
    a, (x, y, z) = C.TRIPLE_START[fmt], C.TRIPLE[fmt]
    want = ((a + x) + y) + z
    assert want != ((a + z) + y) + x, "reverse order"
    if fmt != "half":
        assert ((0.0 + x) + y) + z != ((0.0 + z) + y) + x, "reverse order, from zero"
    assert want != a + ((x + y) + z), "summed first"
    assert want != ((a + y) + x) + z and want != ((a + x) + z) + y, "neighbours exchanged"
    for v in (x, y, z, -x, -y, -z):
        C.D.enc([v], fmt)   # exact in the format (asserted there)


@pytest.mark.parametrize("with_received", (False, True), ids=("plain", "received"))
def test_every_peer_is_a_list_of_its_own(with_received):
    """Own backing arrays, own residues, junk around the views, the triples where they belong."""
    c = S.chunks(T)[1]
    for name in ("whole-f32", "residues-half", "aligned"):
        rec, peers = C.build(np.random.default_rng(5), name, c, T, 5, with_received)
        spec = S.shape(name, c, T)
        assert (rec is None) == (not with_received)
        for k, segs in enumerate(peers):
            assert [(s.fmt, s.n, s.r) for s in segs] == C.peer_spec(spec, k)
            assert all(s.backing.size == s.r + s.n + S.PAD for s in segs)
        assert len({id(s.backing) for segs in peers for s in segs}) == 5 * len(spec)
        vecs = [C.peer_vector(rec, segs) for segs in peers]
        st = S.starts(peers[0])
        for t, f in enumerate(C.triple_positions(spec, c, T)):
            fmt = spec[int(np.searchsorted(st, f, side="right")) - 1][0]
            j = t % 3
            got = [v[f] for v in vecs]
            want = [0.0] * j + list(C.TRIPLE[fmt]) + [0.0] * (2 - j)
            assert got == want and not any(np.signbit(g) for g, w in zip(got, want) if w == 0.0), (name, f, got)


@pytest.mark.parametrize("ci", range(3))
def test_numpy_fold_is_the_oracles(O, ci):
    """The model the mistakes are written in gives the expectation when no mistake is made."""
    c = S.chunks(T)[ci]
    for li, name in enumerate(("tiny", "short-a", "whole-bf16", "residues-f64")):
        for owned in (range(S.P), [4, 1, 4]):
            rng = np.random.default_rng(10 * ci + li)
            rec, peers = C.build(rng, name, c, T, 3, li % 2 == 0)
            acc = C.start_acc(rng, O, name, c, T)
            want = C.expected(O, acc, rec, peers, c, owned)
            got = C.fold_peers(acc, [C.peer_vector(rec, s) for s in peers], c, list(owned))
            assert not _differ(want, got), (name, c)
            # a partition listed twice: each peer's value twice in a row before the next peer's
            rows = acc
            for segs in peers:
                for q in owned:
                    rows = C.fold_vec(rows, C.peer_vector(rec, segs), c, [q])
            assert not _differ(want, rows), (name, c)


@pytest.mark.parametrize("ci", range(3))
def test_inputs_distinguish_the_mistakes(O, ci):
    c = S.chunks(T)[ci]
    seen = set()
    for li, name in enumerate(C.LAYOUTS):
        for ki, K in enumerate(C.KS):
            with_received = (li + ki) % 2 == 1
            rng = np.random.default_rng(1000 * ci + 10 * li + ki)
            rec, peers = C.build(rng, name, c, T, K, with_received)
            for zero_start in (True, False):
                for owned in (list(range(S.P)), [1, 4, 4])[:2 if K <= 3 else 1]:
                    M = S.model_size(c)
                    acc = S.U.zeros(O, M, S.P) if zero_start else C.start_acc(rng, O, name, c, T)
                    want = C.fold_peers(acc, [C.peer_vector(rec, s) for s in peers], c, owned)
                    for what, got in C.mistakes(acc, rec, peers, c, T, owned, zero_start).items():
                        if _differ(want, got):
                            seen.add((what, name, K, zero_start))
                        elif what[0] in "347" or (what[0] == "5" and name.startswith("whole")):   # always visible
                            raise AssertionError(f"{name} c={c} K={K}: '{what}' goes unseen")
    kinds = {w for w, *_ in seen}
    assert {w[0] for w in kinds} == set("123456789"), sorted(kinds)
    for G in C.GROUPS:
        assert f"9 peers {G - 1} and {G} exchanged" in kinds
    # the order of the peers shows in whole tiles of every format: from zero for the formats that hold 2^53,
    # over the planted start for halves
    for fmt in C.FMTS:
        for what in ("1 peers folded in reverse order", "2 peers summed first, one add", "9 peers 1 and 2 exchanged",
                     "9 peers 3 and 4 exchanged", "9 peers 7 and 8 exchanged", "9 peers 15 and 16 exchanged"):
            zero = fmt != "half" and what[0] != "2"   # a sum made first shows over a non-zero accumulator only
            assert any(w == what and n == f"whole-{fmt}" and z == zero for w, n, _, z in seen), (fmt, what)
        assert any(w[0] == "6" and n == f"whole-{fmt}" for w, n, _, _ in seen), fmt


# ---- the binding ----
def test_header_declares_the_call_and_the_kernel():
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b%s\s*\(" % CALL, code)
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", text))
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(IPLS_KERNEL_\w+)\s*=\s*(\d+)", code))
    assert ids.get("IPLS_KERNEL_UPDATE_SEGS_PEERS") == 18
    older = [v for k, v in defs.items() if k.startswith("IPLS_KERNEL_")]
    assert len(set(older) | set(ids.values())) == len(older) + len(ids), "a kernel id is used twice"
    assert defs["IPLS_AGG_ABI_VERSION"] == 4 and defs["IPLS_SEG_PEERS_MAX"] == 1024
    for word in ("per-peer minuends", "pairs of different kinds", "host", "send twin", "mirrors", "cache of plans"):
        assert word in " ".join(text.split()).replace("* ", ""), word


def test_binding_has_the_signature():
    import ipls
    from ipls import _native as N
    L = ipls.lib()
    assert CALL in N.SIGNATURES and hasattr(L, CALL)
    assert N.SIGNATURES[CALL][0] is ctypes.c_int and len(N.SIGNATURES[CALL][1]) == 9
    assert N.KERNEL_UPDATE_SEGS_PEERS == ipls.KERNEL_UPDATE_SEGS_PEERS == 18
    assert N.SEG_PEERS_MAX == ipls.SEG_PEERS_MAX == 1024
    assert ctypes.sizeof(N.LaunchInfo) == 48 and N.ABI_VERSION == 4 and L.ipls_agg_abi_version() == 4


def test_null_handle_is_refused():
    import ipls
    assert ipls.lib().ipls_agg_update_gradient_segs_peers(None, None, None, 1, None, None, 0, None, 0) < 0


class _FakeCuda:
    """Stands in for a CUDA tensor where there is no GPU: Segments and PeerUpdates look at these attributes only."""
    is_cuda = True

    def __init__(self, t):
        self._t = t
        self.dtype = t.dtype

    def is_contiguous(self):
        return self._t.is_contiguous()

    def numel(self):
        return self._t.numel()

    def data_ptr(self):
        return self._t.data_ptr()


def test_peer_updates_refuses_before_any_library_call(monkeypatch):
    import ipls
    from ipls import _native as N

    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(N, "lib", no_lib)
    f = lambda n, d=torch.float32: _FakeCuda(torch.zeros(n, dtype=d))   # noqa: E731
    with pytest.raises(ValueError, match="peers"):
        ipls.PeerUpdates([])
    with pytest.raises(ValueError, match="peers"):
        ipls.PeerUpdates([[f(1)]] * 1025)
    with pytest.raises(ValueError, match="peer 2 has 1 tensors.*2"):
        ipls.PeerUpdates([[f(3), f(4)], [f(3), f(4)], [f(3)]])
    with pytest.raises(ValueError, match="peer 1, tensor 1.*5 elements.*4"):
        ipls.PeerUpdates([[f(3), f(4)], [f(3), f(5)]])
    with pytest.raises(ValueError, match="peer 1, tensor 0.*dtype"):
        ipls.PeerUpdates([[f(3), f(4)], [f(3, torch.float16), f(4)]])
    with pytest.raises(ValueError, match="received has 1 tensors"):
        ipls.PeerUpdates([[f(3), f(4)]], received=[f(3)])
    with pytest.raises(ValueError, match="received, tensor 1.*dtype"):
        ipls.PeerUpdates([[f(3), f(4)]], received=[f(3), f(4, torch.bfloat16)])
    with pytest.raises(ValueError, match="CUDA"):
        ipls.PeerUpdates([[f(3)], [torch.zeros(3)]])
    with pytest.raises(ValueError, match="contiguous"):
        ipls.PeerUpdates([[f(16)], [_FakeCuda(torch.zeros(4, 4).t())]])
    # what it accepts: lists, Segments, single tensors, lists of no tensors; every tensor is kept
    dts = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
    lists = [[f(3, d) for d in dts] + [f(0)] for _ in range(3)]
    rec = [f(3, d) for d in dts] + [f(0)]
    for received in (None, rec, ipls.Segments.from_tensors(rec)):
        pu = ipls.PeerUpdates([lists[0], tuple(lists[1]), ipls.Segments.from_tensors(lists[2])], received=received)
        assert (pu.n, pu.n_segs, pu.n_peers) == (12, 5, 3)
        m_ptrs, t_ptrs, K, ns, kinds, k = pu.tables
        assert (K, k) == (3, 5) and list(ns)[:5] == [3, 3, 3, 3, 0] and list(kinds)[:5] == [3, 11, 13, 15, 11]
        for p in range(3):   # peer-major
            assert [t_ptrs[5 * p + s] for s in range(4)] == [t.data_ptr() for t in lists[p][:4]]
            assert t_ptrs[5 * p + 4] is None
            assert pu.peers[p].tensors == tuple(lists[p])
        if received is None:
            assert m_ptrs is None and pu.received is None
        else:
            assert [m_ptrs[s] for s in range(4)] == [t.data_ptr() for t in rec[:4]] and pu.received.tensors == tuple(rec)
    one = ipls.PeerUpdates([lists[0][1], lists[1][1]], received=rec[1])   # single tensors: one-segment lists
    assert (one.n, one.n_segs, one.n_peers) == (3, 1, 2)
    none = ipls.PeerUpdates([[], []])
    assert (none.n, none.n_segs, none.n_peers) == (0, 0, 2)
    same = ipls.PeerUpdates([lists[0], lists[0]], received=lists[0])      # aliasing is allowed
    assert list(same.tables[1])[:4] == list(same.tables[1])[5:9] == list(same.tables[0])[:4]


def test_other_calls_refuse_peer_updates():
    """Only UpdateGradient takes a PeerUpdates: the generic operand path refuses it."""
    import ipls
    from ipls import aggregator as G
    pu = ipls.PeerUpdates([[]])
    with pytest.raises(TypeError):
        G._operand(pu, f32=True)
    assert G._segments(pu) is None and not isinstance(pu, (ipls.Segments, ipls.Difference))
