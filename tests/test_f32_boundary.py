"""The float32 trainer boundary, host side (no GPU): the new operand kinds of
include/ipls_agg.h against ipls._native, DeviceBuffer's dtype, and the bucket
table's element-count and one-kind-per-call checks.

Model.java:423 widens a float INDArray into the doubles UpdateGradient takes;
Model.java:388-390 narrows GetPartitions' doubles back.  IPLS_DEV_F32 /
IPLS_HOST_F32 move both onto the device.
"""
import ctypes
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ipls():
    import ipls as m
    return m


def _header_define(name):
    text = (ROOT / "include" / "ipls_agg.h").read_text()
    m = re.search(rf"^#define\s+{name}\s+(-?\d+)", text, re.M)
    assert m, f"{name} is not defined in include/ipls_agg.h"
    return int(m.group(1))


def test_header_constants_match_native(ipls):
    from ipls import _native as N
    assert _header_define("IPLS_DEV_F32") == N.DEV_F32 == ipls.DEV_F32 == 11
    assert _header_define("IPLS_HOST_F32") == N.HOST_F32 == ipls.HOST_F32 == 12
    assert _header_define("IPLS_KERNEL_REDUCE_F32") == N.KERNEL_REDUCE_F32 == ipls.KERNEL_REDUCE_F32 == 5
    assert _header_define("IPLS_AGG_ABI_VERSION") == 4


def test_device_buffer_dtype(ipls):
    from ipls import _native as N
    b = ipls.DeviceBuffer(0x1000, 8, dtype="f32")
    assert b.kind == N.DEV_F32 and b.n == 8 and b.dtype == "f32"
    assert ipls.DeviceBuffer(0x1000, 8).kind == N.DEV_F64
    assert ipls.DeviceBuffer(0x1000, 8).dtype == "f64"
    assert ipls.DeviceBuffer(0x1000, 8, True).kind == N.DEV_BE
    with pytest.raises(ValueError):
        ipls.DeviceBuffer(0x1000, 8, big_endian=True, dtype="f32")
    with pytest.raises(ValueError):
        ipls.DeviceBuffer(0x1000, 8, dtype="f16")


def test_bucket_table_kind_and_lengths(ipls):
    from ipls import _native as N
    from ipls.aggregator import _bucket_table, _bucket_table_kind
    D = ipls.DeviceBuffer
    L = [7, 7]
    f32 = lambda n: D(0x1000, n, dtype="f32")     # noqa: E731
    f64 = lambda n: D(0x2000, n)                  # noqa: E731
    # exactly L_p elements is enough, one fewer is not: elements, not bytes / 8
    flat, k, kind = _bucket_table_kind([[f32(7), f32(7)], [f32(9), f32(7)]], L, 0)
    assert (flat, k, kind) == ([0x1000] * 4, 2, N.DEV_F32)
    assert _bucket_table([[f32(7), f32(7)], [f32(9), f32(7)]], L, 0) == ([0x1000] * 4, 2)
    with pytest.raises(ValueError):
        _bucket_table([[f32(7), f32(6)]], L, 0)
    # f64 rows keep today's kinds
    assert _bucket_table_kind([[f64(7)]], L, 0)[2] == N.DEV_F64
    assert _bucket_table_kind([[f64(7)]], L, 0, True)[2] == N.DEV_BE
    # a row (or a table) that mixes f32 and f64 buffers is refused
    with pytest.raises(ValueError):
        _bucket_table([[f32(7), f64(7)]], L, 0)
    with pytest.raises(ValueError):
        _bucket_table([[f32(7)], [f64(7)]], L, 0)
    # big_endian is a property of f64 buckets
    with pytest.raises(ValueError):
        _bucket_table_kind([[f32(7)]], L, 0, True)


def test_null_handle_with_f32_kinds(ipls):
    from ipls import _native as N
    lib = N.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    for kind in (N.DEV_F32, N.HOST_F32):
        assert lib.ipls_agg_update_gradient(None, p, 8, kind, None, 0) < 0
        assert lib.ipls_agg_load_model(None, p, 8, kind) < 0
        assert lib.ipls_agg_accumulate(None, 0, N.TGT_AGG, p, 8, kind) < 0
        assert lib.ipls_agg_get_partitions(None, p, 8, kind) < 0
        assert lib.ipls_agg_split(None, p, 8, kind, 0, p, N.HOST_F64) < 0
    arr = (ctypes.c_void_p * 1)(p)
    assert lib.ipls_agg_reduce_batch(None, 0, 1, arr, 1, N.DEV_F32, N.START_ZERO, N.TGT_AGG) < 0
    assert lib.ipls_agg_aggregate_round(None, 0, 1, arr, 1, N.DEV_F32, p, N.DEV_F32) < 0
