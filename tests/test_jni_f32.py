"""The float[] natives of NativeAggregator (accumulateFloats,
getPartitionsFloats, updateGradientFloats, loadModelFloats) through the fake
JVM of test_jni.py.  A "float[]" there is fj_new_ints over the float bit
patterns: 4-byte elements, length in elements.  Bits against the oracle fed
the widened floats; JVM.call asserts fj_violations() == 0 after every native
(no critical region across a library call).

The ring chunk is the 524,288 values test_jni.py pins (IPLS_JNI_RING_CHUNK,
set when that module is imported, before the shim reads it).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_bits_equal
from test_jni import JVM, L64, _open   # noqa: F401 -- importing it pins the ring chunk

AIOOBE = "java/lang/ArrayIndexOutOfBoundsException"
IAE = "java/lang/IllegalArgumentException"


@pytest.fixture(scope="module")
def jvm():
    import test_jni
    if test_jni._j is None:
        test_jni._j = JVM()
    return test_jni._j


@pytest.fixture
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu run without a visible GPU")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def _floats(jvm, a):
    """A Java float[] holding the float32 array a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return jvm.ints(a.view(np.int32))


def _f32(rng, n):
    x = rng.standard_normal(n).astype(np.float32)
    x.view(np.uint32)[rng.integers(0, n, size=8)] = [0, 0x80000000, 0x7f800000, 0xff800000, 1, 0x807fffff,
                                                      0x7f7fffff, 0x7fc00000]
    return x


def _read(h, p, target, L):
    """An accumulator of the shim's handle, through the C-ABI."""
    from ipls import _native as N
    out = np.empty(L)
    assert N.lib().ipls_agg_read(ctypes.c_void_p(h.value), p, target, out.ctypes.data, L, N.HOST_F64) == 0
    return out


def _model_f32(h, M):
    """ipls_agg_get_partitions(HOST_F32) on the shim's handle: what GetPartitions(dtype=np.float32) calls."""
    from ipls import _native as N
    out = np.empty(M, dtype=np.float32)
    assert N.lib().ipls_agg_get_partitions(ctypes.c_void_p(h.value), out.ctypes.data, M, N.HOST_F32) == 0
    return out


def test_null_arrays_behave_as_their_double_twins(jvm):
    """accumulate(null) and updateGradient(null, ..) are no-ops (Gradient ==
    null), getPartitions(null) and loadModel(null) IllegalArgumentException:
    the float natives do the same, before any library call."""
    h = L64(0)
    for name, twin, args in (("accumulateFloats", "accumulate", (h, 0, 0, None)),
                             ("updateGradientFloats", "updateGradient", (h, None, None)),
                             ("getPartitionsFloats", "getPartitions", (h, None)),
                             ("loadModelFloats", "loadModel", (h, None))):
        before = jvm.L.fj_library_calls()
        _, exc = jvm.call(name, *args)
        _, exc_twin = jvm.call(twin, *args)
        assert exc == exc_twin, name
        assert jvm.L.fj_library_calls() == before, f"{name}(null) reached the library"
    _, exc = jvm.call("accumulateFloats", h, 0, 0, None)
    assert exc is None
    _, exc = jvm.call("getPartitionsFloats", h, None)
    assert exc == IAE


def _single_partition_model(O, L):
    """A model size whose single partition has length L (count slot included)."""
    for M in range(L - 4, L + 1):
        if M > 0 and O.partition_len(M, 1, 0) == L:
            return M
    raise AssertionError(f"no one-partition model with L = {L}")


@pytest.mark.gpu
def test_accumulate_floats_pipelined(jvm, gpu, O):
    """A 1,200,001-value float bucket: three ring chunks, the last of 151,425."""
    L = 1200001
    assert L - 2 * 524288 == 151425
    M = _single_partition_model(O, L)
    h = _open(jvm, M, 1)
    rng = np.random.default_rng(1)
    acc = {0: np.zeros(L), 1: np.zeros(L)}
    for k in range(2):
        for t in (0, 1):     # AGG, REP; k = 1 folds into a live accumulator, from a longer array
            g = _f32(rng, L + (5 if k else 0))
            g[L - 1] = 1.0
            _, exc = jvm.call("accumulateFloats", h, 0, t, _floats(jvm, g))
            assert exc is None
            acc[t] = O.fold(acc[t], g[:L].astype(np.float64))
    for t in (0, 1):
        assert_bits_equal(_read(h, 0, t, L), acc[t], f"target {t}")
    # a short array: ArrayIndexOutOfBoundsException, the accumulators unchanged
    _, exc = jvm.call("accumulateFloats", h, 0, 0, _floats(jvm, np.ones(L - 1, dtype=np.float32)))
    assert exc == AIOOBE
    _, exc = jvm.call("accumulateFloats", h, 3, 0, _floats(jvm, np.ones(L, dtype=np.float32)))
    assert exc == AIOOBE
    for t in (0, 1):
        assert_bits_equal(_read(h, 0, t, L), acc[t], f"target {t} after the refusals")
    jvm.call("close", h)


@pytest.mark.gpu
@pytest.mark.parametrize("M", (1200001, 30011), ids=("pipelined", "single-copy"))
def test_get_partitions_floats(jvm, gpu, O, M):
    P = 2
    h = _open(jvm, M, P)
    rng = np.random.default_rng(2)
    g = _f32(rng, M)
    _, exc = jvm.call("updateGradientFloats", h, _floats(jvm, g), jvm.ints([0, 1]))
    assert exc is None
    _, exc = jvm.call("updateGradientFloats", h, _floats(jvm, g), jvm.ints([1]))   # count slot 2 on partition 1
    assert exc is None
    for p in range(P):
        _, exc = jvm.call("finalizePartition", h, p, None)
        assert exc is None
    parts = O.organize_gradients(g.astype(np.float64), M, P)
    w = [O.reduce([parts[0]], len(parts[0])) + 0.0, O.reduce([parts[1], parts[1]], len(parts[1])) + 0.0]
    with np.errstate(over="ignore", invalid="ignore"):
        want = O.get_partitions(w).astype(np.float32)
    arr = _floats(jvm, np.full(M + 3, 7.0, dtype=np.float32))
    _, exc = jvm.call("getPartitionsFloats", h, arr)
    assert exc is None
    got = jvm.data(arr, np.float32)
    assert_bits_equal(got[:M].astype(np.float64), want.astype(np.float64), "model vs the oracle narrowed once")
    ref = _model_f32(h, M)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got[:M]), nan)
    assert np.array_equal(got[:M].view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), "GetPartitions(dtype=float32)"
    assert (got[M:] == 7.0).all(), "elements past the model keep theirs"
    short = _floats(jvm, np.full(M - 1, 5.0, dtype=np.float32))
    _, exc = jvm.call("getPartitionsFloats", h, short)
    assert exc == AIOOBE
    assert (jvm.data(short, np.float32) == 5.0).all()
    jvm.call("close", h)


@pytest.mark.gpu
def test_update_gradient_and_load_model_floats(jvm, gpu, O):
    """ETHModel's geometry: 443,610 values in 3 partitions."""
    M, P = 443610, 3
    h = _open(jvm, M, P)
    rng = np.random.default_rng(3)
    f1, f2 = _f32(rng, M), _f32(rng, M)
    lens = [O.partition_len(M, P, p) for p in range(P)]
    og1 = O.organize_gradients(f1.astype(np.float64), M, P)
    og2 = O.organize_gradients(f2.astype(np.float64), M, P)
    _, exc = jvm.call("updateGradientFloats", h, _floats(jvm, f1), jvm.ints([0, 2]))
    assert exc is None
    _, exc = jvm.call("updateGradientFloats", h, _floats(jvm, f2), jvm.ints([0, 1, 2]))
    assert exc is None
    _, exc = jvm.call("updateGradientFloats", h, _floats(jvm, np.ones(M + 1, dtype=np.float32)), jvm.ints([1]))
    assert exc == AIOOBE
    for p in range(P):
        want = O.fold(O.fold(np.zeros(lens[p]), og1[p]), og2[p]) if p != 1 else O.fold(np.zeros(lens[p]), og2[p])
        assert_bits_equal(_read(h, p, 0, lens[p]), want, f"AGG[{p}]")
    _, exc = jvm.call("loadModelFloats", h, _floats(jvm, f1))
    assert exc is None
    for p in range(P):
        w = og1[p].copy()
        w[-1] = 0.0        # InitializeWeights leaves the count slot 0.0 (IPLS.java:1880-1901)
        assert_bits_equal(_read(h, p, 2, lens[p]), w, f"W[{p}]")
    jvm.call("close", h)
