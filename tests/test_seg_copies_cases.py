"""The output-copy-list call without a GPU: the shared cases
(seg_copies_cases.py) cover what they claim to cover, every planted quotient
has the property it is planted for, the expectation holds NaNs at the planted
NaN positions only, numpy models of the mistakes such a kernel can make each
change an expected bit or a guard byte in some list, the header and the
binding declare the call and its kernel id, a NULL handle is refused, and
ipls.ModelCopies refuses mismatched lists before any library call.
"""
import ctypes
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import seg_cases as S
import seg_copies_cases as C

torch = pytest.importorskip("torch")

CALL = "ipls_agg_get_partitions_segs_copies"
T = S.TILE_DEFAULT


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


# ---- the cases ----
def test_layouts_cover_their_cases():
    whole, spans, seam = C.check_coverage(T)
    assert {f for f, mixed in whole if mixed} == set(C.FMTS) and {2, 3} <= spans and seam
    for c in S.chunks(T):
        assert C.layouts(c), c
        for name in C.layouts(c):
            spec = C.out_spec(name, c, T)
            assert spec[-3:] == C.EXTRA and sum(s[1] for s in spec[:-3]) >= S.model_size(c)
            assert C.list_spec(spec, 0) == spec
            for k in range(max(C.NS)):
                ls = C.list_spec(spec, k)
                assert [(f, n) for f, n, _ in ls] == [(f, n) for f, n, _ in spec]
                assert all(0 <= r < S.residues(f) for f, _, r in ls)
    # the items are the twin's count of them
    for c in S.chunks(T):
        for name in C.layouts(c):
            spec = C.out_spec(name, c, T)
            assert len(C.items(spec, S.model_size(c), T)) == S.n_divide_items(spec, S.model_size(c), T), (name, c)


def test_planted_quotients_have_their_properties():
    q = C.PLANTED
    counts = [float(p + 2) for p in range(S.P) if p != C.ZERO_COUNT]
    for name, v in q.items():
        if name == "nan":
            assert all(np.isnan(v * cnt) and np.isnan((v * cnt) / cnt) for cnt in counts)
            continue
        for cnt in counts:   # the product is exact in double, so the IEEE quotient is q itself
            assert Fraction(v * cnt) == Fraction(v) * Fraction(cnt), (name, cnt)
            assert np.array_equal(np.array([(v * cnt) / cnt]).view(np.uint64), np.array([v]).view(np.uint64)), (name, cnt)
    one = {"f32": 0x3F800000, "half": 0x3C00, "bf16": 0x3F80}
    assert np.signbit(q["negative zero"]) and q["negative zero"] == 0.0
    for fmt in C.FMTS:
        top = {"f64": 63, "f32": 31}.get(fmt, 15)
        assert int(S.narrow([q["negative zero"]], fmt)[0]) == 1 << top, fmt
    # exactly halfway between two floats: to even
    t = Fraction(q["f32 tie"])
    assert t - 1 == Fraction(1, 2 ** 24) and int(S.narrow([q["f32 tie"]], "f32")[0]) == one["f32"]
    # above the 16-bit tie, so ONE rounding goes up; its float is the tie, so the second rounding goes to even
    for name, fmt, ulp in (("bf16 double rounding", "bf16", Fraction(1, 2 ** 7)), ("half double rounding", "half",
                                                                                   Fraction(1, 2 ** 10))):
        x = Fraction(q[name])
        assert 1 + ulp / 2 < x < 1 + ulp
        assert Fraction(float(np.float32(q[name]))) == 1 + ulp / 2
        assert int(S.narrow([q[name]], fmt)[0]) == one[fmt]
        assert int(C.direct16([q[name]], fmt)[0]) == one[fmt] + 1
    assert np.isinf(S.widen(S.narrow([q["half overflow"]], "half"), "half"))[0]
    assert np.isfinite(np.float32(q["half overflow"])) and S.widen(S.narrow([q["half overflow"]], "bf16"), "bf16")[0] > 0
    sub = np.float32(q["f32 subnormal"])
    assert 0 < float(sub) < float(np.finfo(np.float32).tiny) and Fraction(float(sub)) == Fraction(q["f32 subnormal"])


def test_direct_rounding_model_is_one_rounding():
    """direct16 on floats is the two-step rule (a float rounds to itself first)."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096)).astype(np.float32).astype(np.float64)
    for fmt in ("half", "bf16"):
        assert np.array_equal(C.direct16(x, fmt), S.narrow(x, fmt)), fmt


@pytest.mark.parametrize("ci", range(3))
@pytest.mark.parametrize("secure", (False, True), ids=("plain", "secure"))
def test_expectation_holds_nans_at_the_planted_positions_only(O, ci, secure):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for li, name in enumerate(C.layouts(c)):
        w, where = C.weights(np.random.default_rng(100 * ci + li), O, name, c, T)
        assert set(where.values()) == set(C.PLANTED) or len(where) < len(C.PLANTED), name
        spec = C.out_spec(name, c, T)
        want = C.expected(O, w, spec, M, secure)
        assert [x.size for x in want[-3:]] == [0, 0, 0]
        at = 0
        for i, (fmt, n, _) in enumerate(spec):
            nan = {at + int(e) for e in np.flatnonzero(S.is_nan(want[i], fmt))}
            planted = {f for f, what in where.items() if what == "nan" and at <= f < at + want[i].size}
            assert nan == planted, (name, i)
            at += n
        if not secure:   # the quotient is q itself, in the doubles
            model = O.get_partitions(w, False)
            for f, what in where.items():
                q = C.PLANTED[what]
                assert (np.isnan(model[f]) and np.isnan(q)) or np.array([model[f]]).view(np.uint64)[0] == \
                    np.array([q]).view(np.uint64)[0], (name, f, what)


@pytest.mark.parametrize("ci", range(3))
def test_image_is_the_expectation(O, ci):
    """The model the mistakes are written in leaves the expectation when no mistake is made, and SENTINEL around."""
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    for li, name in enumerate(C.layouts(c)):
        for secure in (False, True):
            w, _ = C.weights(np.random.default_rng(7 * ci + li), O, name, c, T)
            spec = C.out_spec(name, c, T)
            want = C.expected(O, w, spec, M, secure)
            mem = C.image(O, w, name, c, T, 3, secure)
            for k in range(3):
                for i, (fmt, n, r) in enumerate(C.list_spec(spec, k)):
                    got = mem[k][i].view(S.bits_dtype(fmt))
                    m = want[i].size
                    assert got[r:r + m].tobytes() == want[i].tobytes(), (name, k, i)
                    junk = np.concatenate([got[:r], got[r + m:]]).view(np.uint8)
                    assert (junk == S.SENTINEL).all(), (name, k, i)


@pytest.mark.parametrize("ci", range(3))
def test_inputs_distinguish_the_mistakes(O, ci):
    c = S.chunks(T)[ci]
    seen = set()
    for li, name in enumerate(C.layouts(c)):
        w, _ = C.weights(np.random.default_rng(1000 * ci + li), O, name, c, T)
        for n_lists in C.NS:
            for secure in (False, True):
                # the mistakes about lists with every number of lists, those about the value with two lists
                which = (() if secure else C.MISTAKES[:6]) + (C.MISTAKES[6:] if n_lists == 2 else ())
                if not which:
                    continue
                want = C.image(O, w, name, c, T, n_lists, secure)
                for what in which:
                    got = C.image(O, w, name, c, T, n_lists, secure, what)
                    if got is None:
                        continue
                    if not C.same(want, got):
                        seen.add((what, name, n_lists, secure))
                    elif what.split()[0] in ("3", "6", "8", "10"):   # always visible
                        raise AssertionError(f"{name} c={c} n_lists={n_lists}: '{what}' goes unseen")
    kinds = {w for w, *_ in seen}
    want_kinds = set(C.MISTAKES) if ci else set(C.MISTAKES) - {C.MISTAKES[4]}   # c = 9 has no whole tile
    assert want_kinds <= kinds, sorted(want_kinds - kinds)
    for what in C.MISTAKES[:5]:   # the mistakes about lists show with every number of lists that has the premise
        if what in kinds:
            assert {n for w, _, n, _ in seen if w == what} >= set(C.NS) - {1}, what
    if ci:   # in whole tiles of every format
        for fmt in C.FMTS:
            assert any(w == C.MISTAKES[4] and n == f"whole-{fmt}" for w, n, _, _ in seen), fmt


# ---- the binding ----
def test_header_declares_the_call_and_the_kernel():
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b%s\s*\(" % CALL, code)
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", text))
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(IPLS_KERNEL_\w+)\s*=\s*(\d+)", code))
    assert ids.get("IPLS_KERNEL_DIVIDE_SEGS_COPIES") == 19 and ids.get("IPLS_KERNEL_UPDATE_SEGS_PEERS") == 18
    older = [v for k, v in defs.items() if k.startswith("IPLS_KERNEL_")]
    assert len(set(older) | set(ids.values())) == len(older) + len(ids), "a kernel id is used twice"
    assert defs["IPLS_AGG_ABI_VERSION"] == 4 and defs["IPLS_SEG_COPIES_MAX"] == 1025
    assert defs["IPLS_SEG_COPIES_MAX"] == defs["IPLS_SEG_PEERS_MAX"] + 1
    flat = " ".join(text.split()).replace("* ", "")
    for word in ("OUTPUT COPY LIST", "list-major", "given list k alone", "all or nothing", "\"list k\"",
                 "lists of different kinds", "host lists", "mirrors", "cache of plans"):
        assert word in flat, word


def test_exports_map_makes_the_call_global():
    text = (ROOT / "ipls-java-api_amd" / "csrc" / "exports.map").read_text()
    assert re.search(r"global:\s*ipls_\*;", text) and re.search(r"local:\s*\*;", text)
    import ipls
    assert hasattr(ipls.lib(), CALL)


def test_binding_has_the_signature():
    import ipls
    from ipls import _native as N
    L = ipls.lib()
    assert CALL in N.SIGNATURES and hasattr(L, CALL)
    assert N.SIGNATURES[CALL][0] is ctypes.c_int and len(N.SIGNATURES[CALL][1]) == 6
    assert N.KERNEL_DIVIDE_SEGS_COPIES == ipls.KERNEL_DIVIDE_SEGS_COPIES == 19
    assert N.SEG_COPIES_MAX == ipls.SEG_COPIES_MAX == 1025
    assert ipls.ModelCopies is ipls.aggregator.ModelCopies
    assert ctypes.sizeof(N.LaunchInfo) == 48 and N.ABI_VERSION == 4 and L.ipls_agg_abi_version() == 4


def test_null_handle_is_refused():
    import ipls
    assert ipls.lib().ipls_agg_get_partitions_segs_copies(None, None, 1, None, None, 0) < 0


class _FakeCuda:
    """Stands in for a CUDA tensor where there is no GPU: Segments and ModelCopies look at these attributes only."""
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


def test_model_copies_refuses_before_any_library_call(monkeypatch):
    import ipls
    from ipls import _native as N

    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(N, "lib", no_lib)
    f = lambda n, d=torch.float32: _FakeCuda(torch.zeros(n, dtype=d))   # noqa: E731
    with pytest.raises(ValueError, match="lists"):
        ipls.ModelCopies([])
    with pytest.raises(ValueError, match="lists"):
        ipls.ModelCopies([[f(1)]] * 1026)
    assert ipls.ModelCopies([[f(1)]] * 1025).n_lists == 1025
    with pytest.raises(ValueError, match="list 2 has 1 tensors.*2"):
        ipls.ModelCopies([[f(3), f(4)], [f(3), f(4)], [f(3)]])
    with pytest.raises(ValueError, match="list 1, tensor 1.*5 elements.*4"):
        ipls.ModelCopies([[f(3), f(4)], [f(3), f(5)]])
    with pytest.raises(ValueError, match="list 1, tensor 0.*dtype"):
        ipls.ModelCopies([[f(3), f(4)], [f(3, torch.float16), f(4)]])
    with pytest.raises(ValueError, match="CUDA"):
        ipls.ModelCopies([[f(3)], [torch.zeros(3)]])
    with pytest.raises(ValueError, match="contiguous"):
        ipls.ModelCopies([[f(16)], [_FakeCuda(torch.zeros(4, 4).t())]])
    # what it accepts: lists, Segments, single tensors, lists of no tensors; every tensor is kept
    dts = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
    lists = [[f(3, d) for d in dts] + [f(0)] for _ in range(3)]
    mc = ipls.ModelCopies([lists[0], tuple(lists[1]), ipls.Segments.from_tensors(lists[2])])
    assert (mc.n, mc.n_segs, mc.n_lists) == (12, 5, 3)
    o_ptrs, K, ns, kinds, k = mc.tables
    assert (K, k) == (3, 5) and list(ns)[:5] == [3, 3, 3, 3, 0] and list(kinds)[:5] == [3, 11, 13, 15, 11]
    for p in range(3):   # list-major
        assert [o_ptrs[5 * p + s] for s in range(4)] == [t.data_ptr() for t in lists[p][:4]]
        assert o_ptrs[5 * p + 4] is None
        assert mc.lists[p].tensors == tuple(lists[p])
    one = ipls.ModelCopies([lists[0][1], lists[1][1]])   # single tensors: one-segment lists
    assert (one.n, one.n_segs, one.n_lists) == (3, 1, 2)
    none = ipls.ModelCopies([[], []])
    assert (none.n, none.n_segs, none.n_lists) == (0, 0, 2)
    # PeerUpdates.outputs(): received first (when there is one), then the trained lists
    rec = [f(3, d) for d in dts] + [f(0)]
    out = ipls.PeerUpdates(lists, received=rec).outputs()
    assert isinstance(out, ipls.ModelCopies) and out.n_lists == 4
    assert [c.tensors for c in out.lists] == [tuple(rec)] + [tuple(x) for x in lists]
    out = ipls.PeerUpdates(lists).outputs()
    assert out.n_lists == 3 and [c.tensors for c in out.lists] == [tuple(x) for x in lists]


def test_other_calls_refuse_model_copies():
    """Only GetPartitions(out=) takes a ModelCopies: the generic operand path refuses it."""
    import ipls
    from ipls import aggregator as G
    mc = ipls.ModelCopies([[]])
    with pytest.raises(TypeError, match="ModelCopies"):
        G._operand(mc, f32=True)
    assert G._segments(mc) is None and not isinstance(mc, (ipls.Segments, ipls.Difference, ipls.PeerUpdates))
