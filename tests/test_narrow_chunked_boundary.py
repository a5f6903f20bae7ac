"""The streamed trainer-format calls at the interface (no GPU):
ipls_agg_accumulate_chunked_narrow, ipls_agg_get_partitions_chunked_narrow and
the launch-record codes of k_fold1_narrow, header against binding; NULL
handles; dtype checks of the Python wrappers before any library call.
"""
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = (ROOT / "include" / "ipls_agg.h").read_text()


def _proto(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_prototypes_codes_and_abi_version():
    from ipls import _native as N
    acc = _proto("ipls_agg_accumulate_chunked_narrow")
    assert acc == ["ipls_agg *h", "int p", "int target", "int64_t n", "int src_kind", "int64_t chunk",
                   "ipls_chunk_source source", "void *ctx"]
    get = _proto("ipls_agg_get_partitions_chunked_narrow")
    assert get == ["ipls_agg *h", "int out_kind", "int64_t chunk", "IPLS_BYTE_SINK_FN *sink", "void *ctx"]
    vp, i, i64 = N._vp, N._i, N._i64
    assert N.SIGNATURES["ipls_agg_accumulate_chunked_narrow"] == (i, [vp, i, i, i64, i, i64, vp, vp])
    assert N.SIGNATURES["ipls_agg_get_partitions_chunked_narrow"] == (i, [vp, i, i64, vp, vp])
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+IPLS_(KERNEL_\w+)\s+(\d+)", HEADER)}
    assert defs["KERNEL_FOLD1_F32"] == 9 == N.KERNEL_FOLD1_F32
    assert defs["KERNEL_FOLD1_H16"] == 10 == N.KERNEL_FOLD1_H16
    assert len(set(defs.values())) == len(defs) >= 10, defs     # distinct from the other eight (and any later one)
    for name, v in defs.items():
        assert getattr(N, name) == v, name
    import ipls
    assert ipls.KERNEL_FOLD1_F32 == 9 and ipls.KERNEL_FOLD1_H16 == 10
    assert int(re.search(r"#define\s+IPLS_AGG_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 4 == N.ABI_VERSION
    assert N.lib().ipls_agg_abi_version() == 4


def test_null_handle_is_a_negative_code():
    from ipls import _native as N
    L = N.lib()

    @N.CHUNK_SOURCE
    def src(ctx, dst, off, n):
        raise AssertionError("the source must not run")

    @N.BYTE_SINK
    def sink(ctx, b, off, n):
        raise AssertionError("the sink must not run")
    assert L.ipls_agg_accumulate_chunked_narrow(None, 0, N.TGT_AGG, 8, N.HOST_F32, 2, src, None) < 0
    assert L.ipls_agg_get_partitions_chunked_narrow(None, N.HOST_F32, 2, sink, None) < 0


class _NoLib:
    """Stands where the bound library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the dtype check")


@pytest.mark.parametrize("dtype", (np.float64, np.int32, "f32", "float", "bfloat16", object))
def test_unknown_dtype_is_rejected_before_the_library(dtype):
    from ipls.aggregator import Aggregator
    agg = object.__new__(Aggregator)
    agg._lib = _NoLib()
    agg._h = None
    with pytest.raises(ValueError):
        agg.UpdateChunked(0, 8, lambda dst, off, cnt: True, dtype=dtype)
    with pytest.raises(ValueError):
        agg.GetPartitionsChunked(lambda ptr, off, cnt: True, dtype=dtype)


def test_wire_with_a_dtype_is_a_value_error():
    from ipls.aggregator import Aggregator
    agg = object.__new__(Aggregator)
    agg._lib = _NoLib()
    agg._h = None
    for dt in (np.float32, np.float16, "bf16"):
        with pytest.raises(ValueError):
            agg.GetPartitionsChunked(lambda ptr, off, cnt: True, wire=True, dtype=dt)
