"""The whole-gradient streamed update without a GPU: the C-ABI boundary of
ipls_agg_update_gradient_chunked (header, binding, refusals that need no
device), the sanitizer run of its host plan (csrc/flat_plan.hpp), and, on the
oracle alone, that the inputs of test_gpu_update_flat.py can tell a correct
kernel from the mistakes such a kernel makes.
"""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import update_flat_cases as C

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "ipls-java-api_amd"
P = C.P_SWEEP
T = {"f64": 2048, "be": 2048, "f32": 4096, "half": 4096, "bf16": 4096}   # 256 lanes x 2 or 4 elements x 4 groups


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o
    return o


def test_header_declares_the_call():
    h = (ROOT / "include" / "ipls_agg.h").read_text()
    m = re.search(r"int\s+ipls_agg_update_gradient_chunked\s*\(([^;]*)\)\s*;", h)
    assert m, "include/ipls_agg.h does not declare ipls_agg_update_gradient_chunked"
    args = " ".join(m.group(1).split())
    assert args == ("ipls_agg *h, int64_t n, int src_kind, const int32_t *owned, int n_owned, "
                    "int64_t chunk, ipls_chunk_source source, void *ctx")
    assert re.search(r"#define\s+IPLS_KERNEL_UPDATE_FLAT\s+11\b", h)
    assert re.search(r"#define\s+IPLS_AGG_ABI_VERSION\s+4\b", h), "the call is additive: the ABI stays 4"


def test_binding_has_the_signature():
    from ipls import _native as N
    import ipls
    assert N.KERNEL_UPDATE_FLAT == 11 and ipls.KERNEL_UPDATE_FLAT == 11
    res, args = N.SIGNATURES["ipls_agg_update_gradient_chunked"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                    ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ipls.Aggregator, "UpdateGradientChunked")


def test_null_handle_is_refused():
    from ipls import _native as N
    calls = []

    @N.CHUNK_SOURCE
    def cb(ctx, dst, off, cnt):
        calls.append(off)
        return 0
    own = (ctypes.c_int32 * 1)(0)
    assert N.lib().ipls_agg_update_gradient_chunked(None, 8, N.HOST_BE, own, 1, 4, cb, None) < 0
    assert calls == []


def test_unknown_dtype_before_any_library_call():
    import ipls

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name} before the dtype check")
    agg = object.__new__(ipls.Aggregator)
    agg._lib, agg._h = NoLibrary(), None
    for bad in (np.int32, np.float64, "fp8", object()):
        with pytest.raises(ValueError):
            agg.UpdateGradientChunked(8, lambda *a: True, [0], dtype=bad)
    agg._lib = None


def test_flat_plan_under_the_sanitizers():
    subprocess.run(["make", "-C", str(PKG), "flat_plan_test"], check=True, capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "test_flat_plan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"flat_plan ok: (\d+) plans", r.stdout)
    assert m, r.stdout
    # the whole range: P <= 6, every n, owned subset, split into 1 to 3 shards and call chunk 2 .. 12
    assert int(m.group(1)) > 28_000_000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


# ---- the witnesses, on the oracle alone ----
def test_serial_orders_are_distinct_in_every_partition(O):
    M = C.sweep_model_size(65)
    base, grads, table = C.serial_witness(O, M, P)
    assert len(table) == 24
    for p in range(P):
        assert len({table[o][p].tobytes() for o in table}) == 24, f"partition {p}"


def test_order_witness_differs(O):
    base, a, b = C.order_witness()
    M = C.sweep_model_size(41)
    for kind in ("f64", "be", "f32", "bf16"):   # binary16 cannot hold A; the GPU test streams big-endian doubles
        C.from_doubles(np.full(M, a), kind)     # asserts that the format holds A exactly
    start = [np.full(O.partition_len(M, P, p), base) for p in range(P)]
    ba = C.expected(O, [s + b for s in start], np.full(M, a), M, M, P, range(P))
    ab = [s + b for s in C.expected(O, start, np.full(M, a), M, M, P, range(P))]
    for p in range(P - 1):
        assert ba[p][0] != ab[p][0], f"partition {p}: the two orders give the same bits"


def _mistakes(O, wide, acc, M, n):
    """What AGG would hold after the kernel mistakes the tests must catch (a vector of n values)."""
    good = C.expected(O, acc, wide, n, M, P, range(P))
    out = {}
    for name, shift in (("source shifted by +1", 1), ("source shifted by -1", -1)):
        out[name] = C.expected(O, acc, np.roll(wide, -shift), n, M, P, range(P))
    c = M // P + 1
    off_slot, skipped, read_zero = [], [], []
    for p in range(P):
        L = len(acc[p])
        nc = max(0, min((p + 1) * c, n) - p * c)
        g = np.zeros(L)
        g[:nc] = wide[p * c:p * c + nc]
        g1 = g.copy()
        g1[nc + 1 if nc + 1 < L else nc - 1] = 1.0                  # the count slot one place off
        off_slot.append(acc[p] + g1)
        g[nc] = 1.0
        s = acc[p].copy()
        s[:nc + 1] = acc[p][:nc + 1] + g[:nc + 1]                   # the tail above the count slot skipped
        skipped.append(s)
        read_zero.append(np.full(L, 7.0) + g)                       # a logically-zero accumulator read (stale bytes)
    out["count slot one place off"] = off_slot
    out["tail skipped"] = skipped
    out["logically-zero accumulator read"] = read_zero
    return good, out


@pytest.mark.parametrize("kind", C.KINDS)
def test_sweep_inputs_distinguish_the_mistakes(O, kind):
    for c in C.sweep_chunks(T[kind])[:2]:
        M = C.sweep_model_size(c)
        rng = np.random.default_rng(c)
        raw, wide = C.vector(rng, M, kind, C.sweep_plant(M, P, T[kind]))
        assert raw.size == M * C.esize(kind)
        # the residue sweep: the whole vector into +0.0 accumulators (no partition has a tail above its
        # count slot there); the short-vector test: n inside partition 6, into -0.0 accumulators
        cases = ((M, C.zeros(O, M, P), False),
                 (6 * c + 5, [np.full(O.partition_len(M, P, p), -0.0) for p in range(P)], True))
        for n, acc, has_tail in cases:
            good, bad = _mistakes(O, wide, acc, M, n)
            for name, state in bad.items():
                if name == "tail skipped" and not has_tail:
                    continue
                diff = [p for p in range(P)
                        if not np.array_equal(np.asarray(state[p]).view(np.uint64), good[p].view(np.uint64))]
                assert diff, f"{kind} c={c} n={n}: '{name}' gives the correct bits"
