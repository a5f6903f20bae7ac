"""The half-precision trainer boundary, host side (no GPU): the four operand
kinds and the kernel code of include/ipls_agg.h against ipls._native,
DeviceBuffer's two 16-bit dtypes, the bucket table's element-count and
one-dtype-per-call checks, and the narrowing reference the GPU tests use
(tests/h16_ref.py) against torch's CPU casts.

A trainer under autocast holds torch.float16 / torch.bfloat16 parameters and
gradients; IPLS_DEV_F16 / IPLS_HOST_F16 / IPLS_DEV_BF16 / IPLS_HOST_BF16 let
the library widen and narrow them on the device.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT

import h16_ref as R


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
    assert _header_define("IPLS_DEV_F16") == N.DEV_F16 == ipls.DEV_F16 == 13
    assert _header_define("IPLS_HOST_F16") == N.HOST_F16 == ipls.HOST_F16 == 14
    assert _header_define("IPLS_DEV_BF16") == N.DEV_BF16 == ipls.DEV_BF16 == 15
    assert _header_define("IPLS_HOST_BF16") == N.HOST_BF16 == ipls.HOST_BF16 == 16
    assert _header_define("IPLS_KERNEL_REDUCE_H16") == N.KERNEL_REDUCE_H16 == ipls.KERNEL_REDUCE_H16 == 6
    assert _header_define("IPLS_AGG_ABI_VERSION") == N.ABI_VERSION == 4


def test_device_buffer_dtype(ipls):
    from ipls import _native as N
    h = ipls.DeviceBuffer(0x1000, 8, dtype="half")
    b = ipls.DeviceBuffer(0x1002, 9, dtype="bf16")
    assert h.kind == N.DEV_F16 and h.n == 8 and h.dtype == "half"
    assert b.kind == N.DEV_BF16 and b.n == 9 and b.dtype == "bf16"
    assert ipls.DeviceBuffer(0x1000, 8, dtype="f32").kind == N.DEV_F32
    assert ipls.DeviceBuffer(0x1000, 8).kind == N.DEV_F64
    with pytest.raises(ValueError):
        ipls.DeviceBuffer(0x1000, 8, dtype="f16")      # the name stays invalid
    for dt in R.FORMATS:
        with pytest.raises(ValueError):
            ipls.DeviceBuffer(0x1000, 8, big_endian=True, dtype=dt)


@pytest.mark.parametrize("dt", R.FORMATS)
def test_bucket_table_kind_and_lengths(ipls, dt):
    from ipls import _native as N
    from ipls.aggregator import _bucket_table, _bucket_table_kind
    D = ipls.DeviceBuffer
    kind = {"half": N.DEV_F16, "bf16": N.DEV_BF16}[dt]
    other = "bf16" if dt == "half" else "half"
    L = [7, 7]
    h = lambda n: D(0x1000, n, dtype=dt)          # noqa: E731
    # exactly L_p elements is enough, one fewer is not: elements, not bytes / 8
    assert _bucket_table_kind([[h(7), h(7)], [h(9), h(7)]], L, 0) == ([0x1000] * 4, 2, kind)
    assert _bucket_table([[h(7), h(7)], [h(9), h(7)]], L, 0) == ([0x1000] * 4, 2)
    with pytest.raises(ValueError):
        _bucket_table_kind([[h(7), h(6)]], L, 0)
    # one dtype per table
    for o in (D(0x2000, 7), D(0x2000, 7, dtype="f32"), D(0x2000, 7, dtype=other)):
        with pytest.raises(ValueError):
            _bucket_table_kind([[h(7), o]], L, 0)
        with pytest.raises(ValueError):
            _bucket_table_kind([[h(7)], [o]], L, 0)
    # big_endian is a property of f64 buckets
    with pytest.raises(ValueError):
        _bucket_table_kind([[h(7)]], L, 0, True)


def test_null_handle_with_h16_kinds(ipls):
    from ipls import _native as N
    lib = N.lib()
    buf = (ctypes.c_uint16 * 8)()
    p = ctypes.addressof(buf)
    arr = (ctypes.c_void_p * 1)(p)
    t = ctypes.c_uint64()
    for kind in (N.DEV_F16, N.HOST_F16, N.DEV_BF16, N.HOST_BF16):
        assert lib.ipls_agg_update_gradient(None, p, 8, kind, None, 0) < 0
        assert lib.ipls_agg_load_model(None, p, 8, kind) < 0
        assert lib.ipls_agg_accumulate(None, 0, N.TGT_AGG, p, 8, kind) < 0
        assert lib.ipls_agg_accumulate_async(None, 0, N.TGT_AGG, p, 8, kind, ctypes.byref(t)) < 0
        assert lib.ipls_agg_get_partitions(None, p, 8, kind) < 0
        assert lib.ipls_agg_split(None, p, 8, kind, 0, p, N.HOST_F64) < 0
    for kind in (N.DEV_F16, N.DEV_BF16):
        assert lib.ipls_agg_reduce_batch(None, 0, 1, arr, 1, kind, N.START_ZERO, N.TGT_AGG) < 0
        assert lib.ipls_agg_reduce_batch_out(None, 0, 1, arr, 1, kind, N.START_ZERO, arr, N.DEV_F64) < 0
        assert lib.ipls_agg_aggregate_round(None, 0, 1, arr, 1, kind, p, kind) < 0


def test_out_dtype_names(ipls):
    from ipls.aggregator import _out_dtype
    assert _out_dtype(np.float64) == "f64" and _out_dtype(np.float32) == "f32"
    assert _out_dtype(np.float16) == "half" and _out_dtype("bf16") == "bf16"


def _edge_floats():
    """float32 inputs of the narrowing: exact ties to even and to odd, the
    overflow threshold, subnormal results, -0.0, infinities, a quiet NaN."""
    f = lambda x: np.float32(x)   # noqa: E731
    vals = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan,
            # half: ulp(1) = 2^-10; ties at 1 + 2^-11 (to even 1.0) and 1 + 3*2^-11 (to even 1 + 2^-9)
            1 + 2.0**-11, 1 + 3 * 2.0**-11, 1 + 2.0**-11 + 2.0**-23, 1 + 2.0**-11 - 2.0**-23,
            # bf16: ulp(1) = 2^-7; ties at 1 + 2^-8 and 1 + 3*2^-8
            1 + 2.0**-8, 1 + 3 * 2.0**-8, 1 + 2.0**-8 + 2.0**-23, 1 + 2.0**-8 - 2.0**-23,
            65504.0, 65519.0, 65520.0, 65536.0, -65520.0,            # half: largest finite, below / at the overflow tie
            3.3895314e38, 3.3961775e38, 3.4e38, -3.4e38,             # bf16: largest finite, around its overflow tie
            2.0**-14, 2.0**-15, 2.0**-24, 2.0**-25, 1.5 * 2.0**-25, 2.0**-26, -2.0**-24,   # half subnormals
            2.0**-126, 2.0**-127, 2.0**-133, 2.0**-134, 1.5 * 2.0**-134, 2.0**-140, 2.0**-149]   # bf16 subnormals
    return np.array([f(v) for v in vals], dtype=np.float32)


def test_bf16_rne_matches_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0xB16)
    bits = rng.integers(0, 2**32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([bits.view(np.float32), _edge_floats()])
    # signalling NaNs are outside the contract: quieten them
    u = x.view(np.uint32).copy()
    snan = ((u & 0x7FFFFFFF) > 0x7F800000) & ((u & 0x00400000) == 0)
    u[snan] |= 0x00400000
    x = u.view(np.float32)
    got = R.bf16_rne(x)
    ref = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = R.is_nan(ref, "bf16")
    assert np.array_equal(nan, R.is_nan(got, "bf16"))
    assert np.array_equal(got[~nan], ref[~nan])
    # and the pinned two-step value of the issue: (float)(1 + 2^-8 + 2^-30) = 1 + 2^-8, a tie -> 0x3f80
    assert R.bf16_rne(np.array([np.float32(1 + 2.0**-8 + 2.0**-30)]))[0] == 0x3F80


def test_half_narrow_matches_torch():
    torch = pytest.importorskip("torch")
    x = _edge_floats()
    got = R.narrow(x, "half")
    ref = torch.from_numpy(x.copy()).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    nan = R.is_nan(ref, "half")
    assert np.array_equal(nan, R.is_nan(got, "half"))
    assert np.array_equal(got[~nan], ref[~nan])
    assert R.narrow(np.array([np.float32(1 + 2.0**-11 + 2.0**-30)]), "half")[0] == 0x3C00


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_widen_is_exact(fmt):
    torch = pytest.importorskip("torch")
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    w = R.widen(bits, fmt)
    tdt = torch.float16 if fmt == "half" else torch.bfloat16
    ref = torch.from_numpy(bits.view(np.int16).copy()).view(tdt).double().numpy()
    nan = R.is_nan(bits, fmt)
    assert np.array_equal(np.isnan(w), nan) and np.array_equal(np.isnan(ref), nan)
    assert np.array_equal(w[~nan].view(np.uint64), ref[~nan].view(np.uint64))
    # narrowing the widened value gives the pattern back (no flush of subnormals)
    back = R.narrow(w.astype(np.float32), fmt)
    assert np.array_equal(back[~nan], bits[~nan])
