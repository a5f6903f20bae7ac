"""The difference-list calls without a GPU: the shared cases
(seg_diff_cases.py) cover what they claim to cover, their planted pairs do what
they are planted for, numpy models of the mistakes a difference kernel can make
each change an expected bit of the accumulators and of the texts, the header
and the binding declare the two calls and their kernel ids, a NULL handle is
refused, and ipls.Difference refuses mismatched lists before any library call.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import seg_cases as S
import seg_diff_cases as D

torch = pytest.importorskip("torch")

CALLS = ("ipls_agg_update_gradient_segs_diff", "ipls_agg_send_gradients_segs_diff")
KERNELS = {"IPLS_KERNEL_UPDATE_SEGS_DIFF": 16, "IPLS_KERNEL_ENCODE_SEGS_DIFF": 17}
T = S.TILE_DEFAULT
TORCH_DTYPE = {"half": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


# ---- the cases ----
def test_layouts_cover_their_cases():
    whole, spans = D.check_coverage(T)
    assert len(whole) == 4 * len(D.FMTS)
    for c in S.chunks(T):
        for name in D.LAYOUTS:
            spec = S.shape(name, c, T)
            b = D.shape_b(name, spec)
            assert [(f, n) for f, n, _ in spec] == [(f, n) for f, n, _ in b]
            assert all(0 <= r < S.residues(f) for f, _, r in b)


@pytest.mark.parametrize("fmt", D.FMTS)
def test_planted_pairs_do_what_they_are_planted_for(fmt):
    pr = D.pairs(fmt)
    one = lambda k: D.sub_bits(np.array([pr[k][0]]), np.array([pr[k][1]]), fmt)   # noqa: E731
    val = lambda k: S.widen(one(k), fmt)[0]                                        # noqa: E731
    exact = lambda k: S.widen(np.array([pr[k][0]]), fmt)[0] - S.widen(np.array([pr[k][1]]), fmt)[0]   # noqa: E731
    m, e = D.MANT[fmt], D.EMIN[fmt]
    assert val("tie") == 1.0 and (fmt == "f64" or exact("tie") == 1.0 - 2.0 ** -(m + 1))   # half-way, to even
    assert val("inexact") == 1.0 - 2.0 ** -m and (fmt == "f64" or exact("inexact") != val("inexact"))
    assert val("subnormal") == 2.0 ** (e - 1) and 0 < val("subnormal") < 2.0 ** e
    assert val("overflow") == np.inf
    assert val("equal") == 0.0 and not np.signbit(val("equal"))
    assert val("negzero") == 0.0 and np.signbit(val("negzero"))
    assert np.isnan(val("infinf")) and np.isnan(val("nan"))


@pytest.mark.parametrize("fmt", ("half", "bf16"))
def test_numpy_difference_is_torch_sub(fmt):
    """The expectation's rule for the 16-bit formats is what torch.sub gives on the CPU, bit for bit (NaNs aside)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 16, 1 << 16).astype(np.uint16)
    b = rng.integers(0, 1 << 16, 1 << 16).astype(np.uint16)
    pr = D.pairs(fmt)
    for i, k in enumerate(D.PAIR_KINDS):
        a[i], b[i] = pr[k]
    want = D.sub_bits(a, b, fmt)
    ta = torch.from_numpy(a.view(np.int16)).view(TORCH_DTYPE[fmt])
    tb = torch.from_numpy(b.view(np.int16)).view(TORCH_DTYPE[fmt])
    got = torch.sub(ta, tb).view(torch.int16).numpy().view(np.uint16)
    nan = S.is_nan(want, fmt) & S.is_nan(got, fmt)
    assert np.array_equal(want[~nan], got[~nan])


def _bits(parts):
    return [np.ascontiguousarray(p).view(np.uint64) for p in parts]


def _differ(a, b):
    """Some element differs in its bits, NaNs compared as NaN only."""
    for x, y in zip(a, b):
        xf, yf = x.view(np.float64), y.view(np.float64)
        nan = np.isnan(xf) & np.isnan(yf)
        if not np.array_equal(x[~nan], y[~nan]):
            return True
    return False


@pytest.mark.parametrize("ci", range(3))
def test_inputs_distinguish_the_mistakes(O, ci):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    # accumulators of -0.0: the sum is then the value itself, sign of zero included
    base = [np.full(O.partition_len(M, S.P, p), -0.0) for p in range(S.P)]
    seen = set()
    for li, name in enumerate(D.LAYOUTS):
        A, B = D.build(np.random.default_rng(100 * ci + li), name, c, T)
        n = S.total(A)
        want_acc = _bits(D.expected_update(O, base, A, B, c, range(S.P)))
        want_txt = D.expected_texts(O, A, B, c, range(S.P), 5, b"Qm")
        true = S.concat(D.difference(A, B))
        here = set()
        for what, vec in D.mistake_vectors(A, B, c).items():
            assert vec.size == n, what
            nan = np.isnan(vec) & np.isnan(true)
            if np.array_equal(vec.view(np.uint64)[~nan], true.view(np.uint64)[~nan]):
                continue   # this layout has nothing the mistake would change
            got_acc = _bits(S.U.expected(O, base, vec, n, M, S.P, range(S.P)))
            assert _differ(want_acc, got_acc), f"{name} c={c}: '{what}' goes unseen in the accumulators"
            g = O.organize_gradients(vec, M, S.P)
            got_txt = [O.java_b64url_encode(O.frame_encode(g[p], p, 5, 3, b"Qm")) for p in range(S.P)]
            assert got_txt != want_txt, f"{name} c={c}: '{what}' goes unseen in the texts"
            here.add(what)
        assert "operands exchanged" in here, name
        assert "subtraction after widening" in here or all(a.fmt == "f64" for a in A if a.n), name
        seen |= here
    assert len(seen) == D.MISTAKES, seen


# ---- the binding ----
def test_header_declares_the_calls_and_kernels():
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", text))
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(IPLS_KERNEL_\w+)\s*=\s*(\d+)", code))
    for name, v in KERNELS.items():
        assert ids.get(name) == v, name
    older = [v for k, v in defs.items() if k.startswith("IPLS_KERNEL_")]
    assert len(set(older) | set(ids.values())) == len(older) + len(ids), "a kernel id is used twice"
    assert defs["IPLS_AGG_ABI_VERSION"] == 4
    assert "Model.java:413" in text


def test_binding_has_the_signatures():
    import ipls
    from ipls import _native as N
    L = ipls.lib()
    for name in CALLS:
        assert name in N.SIGNATURES and hasattr(L, name), name
    assert N.SIGNATURES[CALLS[0]][0] is ctypes.c_int and len(N.SIGNATURES[CALLS[0]][1]) == 8
    assert N.SIGNATURES[CALLS[1]][0] is ctypes.c_int64 and len(N.SIGNATURES[CALLS[1]][1]) == 17
    assert (N.KERNEL_UPDATE_SEGS_DIFF, N.KERNEL_ENCODE_SEGS_DIFF) == (16, 17)
    assert (ipls.KERNEL_UPDATE_SEGS_DIFF, ipls.KERNEL_ENCODE_SEGS_DIFF) == (16, 17)
    assert ctypes.sizeof(N.LaunchInfo) == 48 and N.ABI_VERSION == 4 and L.ipls_agg_abi_version() == 4
    assert ipls.Difference is not None


def test_null_handle_is_refused():
    import ipls
    L = ipls.lib()
    assert L.ipls_agg_update_gradient_segs_diff(None, None, None, None, None, 0, None, 0) < 0
    assert L.ipls_agg_send_gradients_segs_diff(None, None, None, None, None, 0, None, 0, 0, 3, None, 0, None, 0, 7,
                                               None, None) < 0


class _FakeCuda:
    """Stands in for a CUDA tensor where there is no GPU: Segments and Difference look at these attributes only."""
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


def test_difference_refuses_before_any_library_call(monkeypatch):
    import ipls
    from ipls import _native as N

    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(N, "lib", no_lib)
    f = lambda n, d=torch.float32: _FakeCuda(torch.zeros(n, dtype=d))   # noqa: E731
    with pytest.raises(ValueError, match="2 tensors.*1"):
        ipls.Difference([f(3), f(4)], [f(3)])
    with pytest.raises(ValueError, match="tensor 1.*4 elements.*5"):
        ipls.Difference([f(3), f(4)], [f(3), f(5)])
    with pytest.raises(ValueError, match="tensor 1.*dtype"):
        ipls.Difference([f(3), f(4)], [f(3), f(4, torch.float16)])
    with pytest.raises(ValueError, match="CUDA"):
        ipls.Difference([f(3)], [torch.zeros(3)])
    with pytest.raises(ValueError, match="contiguous"):
        ipls.Difference([_FakeCuda(torch.zeros(4, 4).t())], [f(16)])
    # what it accepts: lists, Segments, a mix of both, single tensors (a one-segment difference), nothing at all
    a = [f(3, d) for d in (torch.float64, torch.float32, torch.float16, torch.bfloat16)] + [f(0)]
    b = [f(3, d) for d in (torch.float64, torch.float32, torch.float16, torch.bfloat16)] + [f(0)]
    for x, y in ((a, b), (ipls.Segments.from_tensors(a), tuple(b)), (a, ipls.Segments.from_tensors(b))):
        d = ipls.Difference(x, y)
        assert (d.n, d.n_segs) == (12, 5)
        a_ptrs, b_ptrs, ns, kinds, k = d.tables
        assert k == 5 and list(ns)[:5] == [3, 3, 3, 3, 0] and list(kinds)[:5] == [3, 11, 13, 15, 11]
        assert [a_ptrs[i] for i in range(4)] == [t.data_ptr() for t in a[:4]] and a_ptrs[4] is None
        assert [b_ptrs[i] for i in range(4)] == [t.data_ptr() for t in b[:4]] and b_ptrs[4] is None
        assert d.minuend.tensors == tuple(a) and d.subtrahend.tensors == tuple(b)   # both lists are kept alive
    one = ipls.Difference(a[1], b[1])
    assert (one.n, one.n_segs) == (3, 1)
    same = ipls.Difference(a, a)
    assert list(same.tables[0])[:4] == list(same.tables[1])[:4]
    assert (ipls.Difference([], []).n, ipls.Difference([], []).n_segs) == (0, 0)


def test_other_calls_refuse_a_difference():
    """Only UpdateGradient and SendGradients take a Difference: the generic operand path refuses it."""
    import ipls
    from ipls import aggregator as G
    d = ipls.Difference([], [])
    with pytest.raises((TypeError, ValueError)):
        G._operand(d, f32=True)
    assert G._segments(d) is None and not isinstance(d, ipls.Segments)
