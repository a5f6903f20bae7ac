"""saveModel / loadSavedModel of the JNI shim through the fake JVM of
tests/test_jni.py: IPLS.save_model's file (IPLS.java:1904-1911) out of one
handle, DownloadMapParameters plus the leaving-peer blend (IPLS.java:728-731,
Updater.java:65-69) into another, against the writer restated in
tests/saved_model_writer.py and the oracle's blend."""
import ctypes

import numpy as np
import pytest

import saved_model_writer as W
from conftest import assert_bits_equal
from oracle import javaser as J
from test_jni import L64, O, _open, gpu, jvm  # noqa: F401 -- fixtures and the fake JVM


def test_null_arguments_are_java_exceptions(jvm):   # noqa: F811
    r, exc = jvm.call("loadSavedModel", L64(0), None, None, 0, res=ctypes.c_int32)
    assert exc == "java/lang/IllegalArgumentException" and r == -1
    r, exc = jvm.call("saveModel", L64(0), jvm.ints([0]), res=ctypes.c_void_p)
    assert exc == "java/lang/IllegalArgumentException" and r is None
    r, exc = jvm.call("loadSavedModel", L64(0), jvm.bytes_(W.write_map({}, [])), None, 0, res=ctypes.c_int32)
    assert exc == "java/lang/IllegalArgumentException" and r == -1


@pytest.mark.gpu
def test_jni_save_and_load_round_trip(jvm, gpu, O):   # noqa: F811
    M, P = 30011, 3
    src, dst = _open(jvm, M, P), _open(jvm, M, P)
    lens = []
    for p in range(P):
        n, exc = jvm.call("partitionLen", src, p, res=ctypes.c_int64)
        assert exc is None
        lens.append(n)
    w = [W.edge_values(L, 40 + p) for p, L in enumerate(lens)]
    w0 = [np.linspace(-1.0, 2.0, L) for L in lens]
    for h, vals in ((src, w), (dst, w0)):
        for p in range(P):
            be = np.frombuffer(W.raw_be(vals[p]), dtype=np.uint8)
            buf, mem = jvm.direct(be.size)
            mem[:] = be
            _, exc = jvm.call("setWeightsDirect", h, p, buf, 0, L64(lens[p]))
            assert exc is None
    auth = [2, 0, 1]
    out, exc = jvm.call("saveModel", src, jvm.ints(auth), res=ctypes.c_void_p)
    assert exc is None
    file = jvm.data(ctypes.c_void_p(out), np.uint8).tobytes()
    assert file == W.write_map(dict(enumerate(w)), auth)
    # the peer taking partitions 2 and 0 over: the leaving-peer blend, partition 1 untouched
    n, exc = jvm.call("loadSavedModel", dst, jvm.bytes_(file), jvm.ints([2, 0]), 1, res=ctypes.c_int32)
    assert exc is None and n == 2
    want = [O.blend(w0[0], w[0], 0.6, 1 - 0.6), w0[1], O.blend(w0[2], w[2], 0.6, 1 - 0.6)]
    n, exc = jvm.call("loadSavedModel", dst, jvm.bytes_(file[:-1]), None, 0, res=ctypes.c_int32)
    assert exc == "java/nio/BufferUnderflowException" and n == -1
    n, exc = jvm.call("loadSavedModel", dst, jvm.bytes_(W.write_map({0: w[0]}, [0])), jvm.ints([0, 1]), 0,
                      res=ctypes.c_int32)
    assert exc == "java/lang/ArrayIndexOutOfBoundsException" and n == -1
    back, exc = jvm.call("saveModel", dst, jvm.ints([0, 1, 2]), res=ctypes.c_void_p)
    assert exc is None
    got = jvm.data(ctypes.c_void_p(back), np.uint8).tobytes()
    obj, end = J.read_object(got)
    items = obj["annotations"]["java.util.HashMap"][1:]
    assert end == len(got) and [k["fields"][("java.lang.Integer", "value")] for k in items[0::2]] == [0, 1, 2]
    for p in range(P):
        assert_bits_equal(items[2 * p + 1]["values"], want[p], f"partition {p}")
    # SET of every key
    n, exc = jvm.call("loadSavedModel", dst, jvm.bytes_(file), None, 0, res=ctypes.c_int32)
    assert exc is None and n == P
    again, exc = jvm.call("saveModel", dst, jvm.ints(auth), res=ctypes.c_void_p)
    assert exc is None and jvm.data(ctypes.c_void_p(again), np.uint8).tobytes() == file
    jvm.call("close", src)
    jvm.call("close", dst)
