"""The many-trainers round without a GPU: the shared cases (seg_round_cases.py)
cover what they claim to cover, the numpy model of the call agrees with the
oracle's expectation bit for bit, the expectation holds NaNs at the planted
positions only, the numpy models of the mistakes such a kernel can make each
change an expected bit of W, of an output or of a guard byte, the header and
the binding declare the call and its kernel id, a NULL handle is refused, and
Aggregator.round_peers refuses mismatched operands before any library call.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
import seg_cases as S
import seg_copies_cases as SC
import seg_peers_cases as PC
import seg_round_cases as C

torch = pytest.importorskip("torch")

CALL = "ipls_agg_round_segs_peers"
T = S.TILE_DEFAULT


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def _cases(O, ci):
    """A spread over the layouts, K, the owned forms, the starts and the output forms for one chunk."""
    c = S.chunks(T)[ci]
    out = []
    for li, name in enumerate(C.layouts(c, T)):
        K = C.KS[(li + ci) % len(C.KS)]
        own = list(C.OWNED)[(li + 2 * ci) % len(C.OWNED)]
        start = C.STARTS[(li + ci) % len(C.STARTS)]
        n_lists = None if li % 2 == 0 else C.n_lists_of(K)[(li // 2) % 3]
        out.append(C.build(O, 500 + 20 * ci + li, name, c, T, K, C.OWNED[own], start, li % 3 != 1,
                           secure=li % 4 == 3, n_lists=n_lists))
    return out


def _same_mem(a, b):
    return SC.same(a, b)


# ---- the cases ----
def test_layouts_cover_their_cases():
    tot = C.check_coverage(T)
    assert tot["whole"] == set(C.FMTS)
    for c in S.chunks(T):
        M = S.model_size(c)
        names = C.layouts(c, T)
        assert {"tiny", "aligned"} <= set(names) and not any(n.startswith("short") for n in names)
        for name in names:
            assert sum(s[1] for s in S.shape(name, c, T)) == M
        for name in ("short-a", "short-b", "short-c"):
            assert sum(s[1] for s in S.shape(name, c, T)) < M    # the refusal's layouts
    assert C.KS == (1, 2, 3, 5) and all(C.n_lists_of(K) == (1, K + 1, 3) for K in C.KS)
    assert sorted(set(C.OWNED["all"])) == list(range(C.P)) and 0 < len(set(C.OWNED["subset"])) < C.P
    assert len(set(C.OWNED["twice"])) == len(C.OWNED["twice"]) - 1 and C.OWNED["none"] == []
    assert SC.ZERO_COUNT not in C.OWNED["subset"], "a partition that is not owned has the count 0.0"


@pytest.mark.parametrize("ci", range(3))
def test_numpy_model_is_the_oracles(O, ci):
    """model() with no mistake is the expectation, bit for bit: W and every byte of every list."""
    for case in _cases(O, ci):
        W, mem = C.expected_image(O, case)
        got = C.model(case)
        what = (case.name, case.c, case.K, case.owned, case.start)
        assert C.same_w_nan(got[0], W), what
        # NaN payloads may differ between numpy's adds and the oracle's; compare where the expectation has no NaN
        for la, lb, sp in zip(got[1], mem, case.list_specs()):
            for x, y, (fmt, n, r) in zip(la, lb, sp):
                a, b = x.view(S.bits_dtype(fmt)), y.view(S.bits_dtype(fmt))
                nan = S.is_nan(a, fmt) & S.is_nan(b, fmt)
                assert np.array_equal(a[~nan], b[~nan]), what


@pytest.mark.parametrize("ci", range(3))
def test_nans_stand_at_the_planted_positions_only(O, ci):
    for case in _cases(O, ci):
        W, bits = C.expected(O, case)
        spec, c, M = case.spec, case.c, case.M
        allowed = set(S.plant_positions(spec, c, T, M)) | set(SC.plant_positions(spec, c, T, M))
        at = 0
        for (fmt, n, r), b in zip(spec, bits):
            for e in np.flatnonzero(S.is_nan(b, fmt)):
                assert at + int(e) in allowed, (case.name, case.c, at + int(e))
            at += n
        # the planted quotients and the -0.0 sums are where they were put
        flat = np.concatenate([w[:-1] for w in W])[:M]
        for f, q in case.planted.items():
            p = f // c
            if q == "rep order":
                assert flat[f] == PC.BIG + case.K * case.owned.count(p), (case.name, f)
            elif q == "negzero sum":
                if case.rep0[p] is None:
                    assert flat[f] == 0.0 and not np.signbit(flat[f]), (case.name, f)
                else:
                    assert flat[f] == 0.0 and np.signbit(flat[f]), (case.name, f)
            elif q == "nan":
                assert np.isnan(flat[f])
            elif W[p][-1] != 0.0:
                assert flat[f] / W[p][-1] == SC.PLANTED[q] or q == "negative zero", (case.name, f, q)


def test_negzero_sum_becomes_positive_zero(O):
    c = S.chunks(T)[1]
    case = C.build(O, 1, "aligned", c, T, 3, C.OWNED["all"], "agg", True)
    hits = [f for f, q in case.planted.items() if q == "negzero sum"]
    assert len(hits) >= 8
    W, bits = C.expected(O, case)
    skipped = C.model(case, C.MISTAKES[5])[0]
    for f in hits:
        assert W[f // c][f % c] == 0.0 and not np.signbit(W[f // c][f % c])
        assert np.signbit(skipped[f // c][f % c])


# ---- the mistakes ----
@pytest.mark.parametrize("ci", range(3))
def test_every_mistake_changes_an_expected_bit(O, ci):
    seen = set()
    for case in _cases(O, ci) + [
            C.build(O, 7, "aligned", S.chunks(T)[ci], T, 3, C.OWNED["twice"], "both", True),
            C.build(O, 8, "tiny", S.chunks(T)[ci], T, 2, C.OWNED["subset"], "both", True),
            C.build(O, 9, "residues-f32", S.chunks(T)[ci], T, 5, C.OWNED["all"], "agg", False, n_lists=3)]:
        W, mem = C.expected_image(O, case)
        what = (case.name, case.c, case.K, case.owned, case.start)
        assert C.no_tail(O, case), what   # mistake 8 has no tail to write: the count slot is all of it
        for m in C.MISTAKES:
            if m == C.MISTAKES[7]:
                if case.agg0 is None or not case.owned:
                    continue
                good, bad = C.second_round(O, case), C.second_round(O, case, stale_flag=True)
                assert not C.same_w_nan(good, bad), (m, what)
            elif m == C.MISTAKES[10]:
                w = C.overwritten_received(O, case)
                if w is None:
                    continue
                assert not C.same_w_nan(w, W), (m, what)
            else:
                got = C.model(case, m)
                if got is None:
                    continue
                assert not (C.same_w_nan(got[0], W) and _same_mem(got[1], mem)), (m, what)
            seen.add(m)
    assert seen == set(C.MISTAKES), set(C.MISTAKES) - seen


# ---- the binding ----
def test_header_declares_the_call_and_the_kernel():
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b%s\s*\(" % CALL, code)
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", text))
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(IPLS_KERNEL_\w+)\s*=\s*(\d+)", code))
    ids.update({k: v for k, v in defs.items() if k.startswith("IPLS_KERNEL_")})
    assert ids.get("IPLS_KERNEL_ROUND_SEGS_PEERS") == 20
    assert ids["IPLS_KERNEL_UPDATE_SEGS_PEERS"] == 18 and ids["IPLS_KERNEL_DIVIDE_SEGS_COPIES"] == 19
    assert len(set(ids.values())) == len(ids), "a kernel id is used twice"
    assert defs["IPLS_AGG_ABI_VERSION"] == 4
    flat = " ".join(text.split()).replace("* ", "")
    for word in ("ALIASING is part of the contract", "AGG is never stored", "-0.0 sum becomes +0.0", "W is read only",
                 "before the first launch on any shard", "per-list dtypes", "host lists", "a fused send", "mirrors"):
        assert word in flat, word


def test_binding_has_the_signature():
    import ipls
    from ipls import _native as N
    L = ipls.lib()
    assert CALL in N.SIGNATURES and hasattr(L, CALL)
    assert N.SIGNATURES[CALL][0] is ctypes.c_int and len(N.SIGNATURES[CALL][1]) == 11
    assert N.KERNEL_ROUND_SEGS_PEERS == ipls.KERNEL_ROUND_SEGS_PEERS == 20
    assert N.ABI_VERSION == 4 and L.ipls_agg_abi_version() == 4
    assert callable(ipls.Aggregator.round_peers)


def test_null_handle_is_refused():
    import ipls
    assert ipls.lib().ipls_agg_round_segs_peers(None, None, None, 1, None, 1, None, None, 0, None, 0) < 0


class _FakeCuda:
    """Stands in for a CUDA tensor where there is no GPU: the list classes look at these attributes only."""
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


def test_round_peers_refuses_before_any_library_call():
    import ipls

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")

    agg = object.__new__(ipls.Aggregator)
    agg._lib, agg._h = NoLib(), None
    f = lambda n, d=torch.float32: _FakeCuda(torch.zeros(n, dtype=d))   # noqa: E731
    pu = ipls.PeerUpdates([[f(3), f(4)], [f(3), f(4)]], received=[f(3), f(4)])
    with pytest.raises(ValueError, match="1 tensors per list.*2"):
        agg.round_peers(pu, [0], out=ipls.ModelCopies([[f(3)]]))
    with pytest.raises(ValueError, match="tensor 1.*5 elements.*4"):
        agg.round_peers(pu, [0], out=ipls.ModelCopies([[f(3), f(5)]]))
    with pytest.raises(ValueError, match="tensor 0.*dtype"):
        agg.round_peers(pu, [0], out=ipls.ModelCopies([[f(3, torch.float16), f(4)]]))
    for bad in (ipls.Segments.from_tensors([f(3), f(4)]), [f(3), f(4)], None, ipls.ModelCopies([[f(3), f(4)]])):
        with pytest.raises(TypeError, match="PeerUpdates"):
            agg.round_peers(bad, [0])
    for bad in (ipls.Segments.from_tensors([f(3), f(4)]), [[f(3), f(4)]], pu):
        with pytest.raises(TypeError, match="ModelCopies"):
            agg.round_peers(pu, [0], out=bad)
    with pytest.raises(AssertionError, match="ipls_agg_round_segs_peers"):   # what passes the checks reaches the call
        agg.round_peers(pu, [0])
