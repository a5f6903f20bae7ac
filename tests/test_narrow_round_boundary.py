"""The fused round over trainer-format buckets, host side (no GPU): the two
launch-record codes of include/ipls_agg.h against ipls._native, and the ABI
number, which the fused kernel leaves alone (no prototype changed).
"""
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
    assert _header_define("IPLS_KERNEL_ROUND_F32") == N.KERNEL_ROUND_F32 == ipls.KERNEL_ROUND_F32 == 7
    assert _header_define("IPLS_KERNEL_ROUND_H16") == N.KERNEL_ROUND_H16 == ipls.KERNEL_ROUND_H16 == 8
    assert _header_define("IPLS_AGG_ABI_VERSION") == N.ABI_VERSION == 4


def test_kernel_codes_are_distinct(ipls):
    codes = [ipls.KERNEL_REDUCE, ipls.KERNEL_ROUND, ipls.KERNEL_FOLD1, ipls.KERNEL_REDUCE_SCALAR,
             ipls.KERNEL_REDUCE_F32, ipls.KERNEL_REDUCE_H16, ipls.KERNEL_ROUND_F32, ipls.KERNEL_ROUND_H16]
    assert len(set(codes)) == len(codes)
