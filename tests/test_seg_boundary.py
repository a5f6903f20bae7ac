"""The trainer boundary over a list of tensors, without a GPU: the header and
the binding declare the three segment-list calls and their kernel ids, a NULL
handle is refused, Segments.from_tensors refuses what it must before any
library call, the host plan (csrc/seg_plan.hpp) passes its brute-force check
under the sanitizers, the shared layouts (seg_cases.py) cover what they claim
to cover, and the inputs distinguish the mistakes a segment-list kernel can
make: each mistake, modelled in numpy, changes the expected bits.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
import seg_cases as S

torch = pytest.importorskip("torch")

CALLS = ("ipls_agg_update_gradient_segs", "ipls_agg_send_gradients_segs", "ipls_agg_get_partitions_segs")
KERNELS = {"IPLS_KERNEL_UPDATE_SEGS": 13, "IPLS_KERNEL_DIVIDE_SEGS": 14, "IPLS_KERNEL_ENCODE_SEGS": 15}
T = S.TILE_DEFAULT


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def test_header_declares_the_calls_and_kernels():
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", text))
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(IPLS_KERNEL_\w+)\s*=\s*(\d+)", code))
    for name, v in KERNELS.items():
        assert ids.get(name) == v, name
    # additive: no id is used twice
    older = [v for k, v in defs.items() if k.startswith("IPLS_KERNEL_")]
    assert len(set(older) | set(ids.values())) == len(older) + len(ids)
    assert defs["IPLS_AGG_ABI_VERSION"] == 4


def test_binding_has_the_signatures():
    import ipls
    from ipls import _native as N
    L = ipls.lib()
    for name in CALLS:
        assert name in N.SIGNATURES and hasattr(L, name), name
    assert N.SIGNATURES[CALLS[1]][0] is ctypes.c_int64
    assert (N.KERNEL_UPDATE_SEGS, N.KERNEL_DIVIDE_SEGS, N.KERNEL_ENCODE_SEGS) == (13, 14, 15)
    assert (ipls.KERNEL_UPDATE_SEGS, ipls.KERNEL_DIVIDE_SEGS, ipls.KERNEL_ENCODE_SEGS) == (13, 14, 15)
    assert ctypes.sizeof(N.LaunchInfo) == 48
    assert ipls.Segments is not None


def test_null_handle_is_refused():
    import ipls
    L = ipls.lib()
    assert L.ipls_agg_update_gradient_segs(None, None, None, None, 0, None, 0) < 0
    assert L.ipls_agg_get_partitions_segs(None, None, None, None, 0) < 0
    assert L.ipls_agg_send_gradients_segs(None, None, None, None, 0, None, 0, 0, 3, None, 0, None, 0, 7, None, None) < 0


class _FakeCuda:
    """Stands in for a CUDA tensor where there is no GPU: from_tensors looks at these attributes only."""
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


def test_segments_refuses_before_any_library_call(monkeypatch):
    import ipls
    from ipls import _native as N

    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(N, "lib", no_lib)
    with pytest.raises(ValueError, match="CUDA"):
        ipls.Segments.from_tensors([torch.zeros(4)])
    with pytest.raises(ValueError, match="contiguous"):
        ipls.Segments.from_tensors([_FakeCuda(torch.zeros(4, 4).t())])
    with pytest.raises(ValueError, match="dtype"):
        ipls.Segments.from_tensors([_FakeCuda(torch.zeros(4, dtype=torch.int32))])
    # what it accepts: the four dtypes, an empty tensor, no tensor at all
    ok = [_FakeCuda(torch.zeros(3, dtype=d)) for d in (torch.float64, torch.float32, torch.float16, torch.bfloat16)]
    ok.append(_FakeCuda(torch.zeros(0)))
    s = ipls.Segments.from_tensors(ok)
    assert (s.n, s.n_segs, len(s.tensors)) == (12, 5, 5)
    ptrs, ns, kinds, k = s.tables
    assert k == 5 and list(ns)[:5] == [3, 3, 3, 3, 0] and list(kinds)[:5] == [3, 11, 13, 15, 11]
    assert ptrs[4] is None and ptrs[0] == ok[0].data_ptr()
    e = ipls.Segments.from_tensors([])
    assert (e.n, e.n_segs) == (0, 0)


def test_plan_under_the_sanitizers():
    """make seg_plan_test builds tests/cpp/test_seg_plan.cpp with -fsanitize=address,undefined; then the program
    is run on its own."""
    r = subprocess.run(["make", "-C", str(PKG), "seg_plan_test"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "test_seg_plan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"seg_plan: \d+ plans ok", r.stdout), r.stdout


def test_layouts_cover_their_cases():
    whole, flags = S.check_coverage(T)
    assert len(whole) == sum(S.residues(f) for f in S.FMTS)
    for c in S.chunks(T):
        M = S.model_size(c)
        for name in S.LAYOUTS:
            spec = S.shape(name, c, T)
            n = sum(s[1] for s in spec)
            assert n <= M and (n == M or name.startswith("short")), (name, c)
            assert all(0 <= r < S.residues(f) for f, _, r in spec)
        # neighbouring formats differ in `tiny`, and all four are used
        tiny = [s for s in S.shape("tiny", c, T) if s[1]]
        assert all(a[0] != b[0] for a, b in zip(tiny, tiny[1:])) and {s[0] for s in tiny} == set(S.FMTS)
        # the short lists end inside partition 6 or at partition 7's start
        ends = [sum(s[1] for s in S.shape(f"short-{k}", c, T)) for k in "abc"]
        assert 6 * c < ends[0] < ends[1] < ends[2] == 7 * c


def _bits(parts):
    return [np.ascontiguousarray(p).view(np.uint64) for p in parts]


@pytest.mark.parametrize("ci", range(3))
def test_inputs_distinguish_the_update_mistakes(O, ci):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    seen = set()
    for li, name in enumerate(S.LAYOUTS):
        segs = S.build(np.random.default_rng(100 * ci + li), S.shape(name, c, T), c, T)
        n = S.total(segs)
        want = _bits(S.expected_update(O, U_zeros(O, M), segs, c, range(S.P)))
        for what, vec in S.mistake_vectors(segs).items():
            got = _bits(S.U.expected(O, U_zeros(O, M), vec, n, M, S.P, range(S.P)))
            assert any(not np.array_equal(a, b) for a, b in zip(want, got)), f"{name} c={c}: '{what}' goes unseen"
            seen.add(what)
        bad = S.mistake_ncopy_per_segment(O, segs, c)
        if bad is not None:
            assert any(not np.array_equal(a, b) for a, b in zip(want, _bits(bad))), f"{name} c={c}: ncopy per segment"
            seen.add("ncopy")
        else:
            assert name.startswith("whole") or (name == "aligned" and c < T), name
    assert len(seen) == 5, seen


def U_zeros(O, M):
    return S.U.zeros(O, M, S.P)


@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("ci", range(3))
def test_inputs_distinguish_the_divide_mistakes(O, ci, secure):
    c = S.chunks(T)[ci]
    M = S.model_size(c)
    w = S.weights(np.random.default_rng(7 + ci), O, c)
    model = O.get_partitions(w, secure)
    seen = set()
    for name in S.LAYOUTS:
        spec = S.shape(name, c, T)
        if sum(s[1] for s in spec) < M:
            continue
        want = S.expected_outputs(model, spec, M)
        for what, bad in S.mistake_models(w, spec, c, T, secure).items():
            got = S.expected_outputs(bad, spec, M)
            assert any(not np.array_equal(a, b) for a, b in zip(want, got)), f"{name} c={c}: '{what}' goes unseen"
            seen.add(what)
    assert len(seen) == 2, seen
