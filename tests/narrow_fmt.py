"""Helpers shared by the k_fold1_narrow / narrow chunked tests: the three
trainer formats ("f32", "half", "bf16") as numpy bit patterns (uint32 for
floats, uint16 for the 16-bit formats), their exact widening, device and host
operands, and buckets with the special values planted.
"""
import numpy as np

import h16_ref as R

FMTS = ("f32", "half", "bf16")
# +-0, +-inf, smallest subnormal, largest subnormal (negative), largest finite, a quiet NaN
EDGE_BITS = {
    "f32": np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7f7fffff, 0x7fc00000],
                    dtype=np.uint32),
    "half": np.array([0x0000, 0x8000, 0x7c00, 0xfc00, 0x0001, 0x83ff, 0x7bff, 0x7e00], dtype=np.uint16),
    "bf16": np.array([0x0000, 0x8000, 0x7f80, 0xff80, 0x0001, 0x807f, 0x7f7f, 0x7fc0], dtype=np.uint16),
}
ONE = {"f32": 0x3f800000, "half": 0x3c00, "bf16": 0x3f80}
NEG_ZERO = {"f32": 0x80000000, "half": 0x8000, "bf16": 0x8000}


def esize(fmt):
    return 4 if fmt == "f32" else 2


def bits_dtype(fmt):
    return np.uint32 if fmt == "f32" else np.uint16


def np_dtype(fmt):
    """What UpdateChunked / GetPartitionsChunked / GetPartitions take as dtype=."""
    return {"f32": np.float32, "half": np.float16, "bf16": "bf16"}[fmt]


def widen(bits, fmt):
    """The exact doubles of the bit patterns (include/ipls_agg.h's widening rule)."""
    if fmt == "f32":
        with np.errstate(invalid="ignore"):
            return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)
    return R.widen(bits, fmt)


def from_f32(x, fmt):
    """Bit patterns of a float32 array narrowed to the format."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.view(np.uint32).copy() if fmt == "f32" else R.narrow(x, fmt)


def bucket(rng, L, fmt, plant=()):
    """One bucket of L elements as bit patterns: normals, the edge values at the
    positions `plant` that lie below the count slot, 1.0 in the count slot."""
    x = from_f32(rng.standard_normal(L).astype(np.float32), fmt)
    e = EDGE_BITS[fmt]
    for i, pos in enumerate(p for p in plant if 0 <= p < L - 1):
        x[pos] = e[i % e.size]
    x[L - 1] = ONE[fmt]
    return x


def dev(ipls, torch, bits, fmt, off=0):
    """(keepalive, DeviceBuffer) of the bucket in device memory, its base a
    16-B boundary plus `off` elements."""
    s = esize(fmt)
    raw = np.ascontiguousarray(bits).view(np.uint8)
    t = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[off * s:off * s + raw.size] = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    return t, ipls.DeviceBuffer(t.data_ptr() + off * s, int(bits.size), dtype=fmt)


def host(torch, bits, fmt):
    """A host operand of the HOST_F32 / HOST_F16 / HOST_BF16 kind."""
    bits = np.ascontiguousarray(bits)
    if fmt == "f32":
        return bits.view(np.float32)
    if fmt == "half":
        return bits.view(np.float16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def fold_kernel(ipls, fmt):
    return ipls.KERNEL_FOLD1_F32 if fmt == "f32" else ipls.KERNEL_FOLD1_H16


def reduce_kernel(ipls, fmt):
    return ipls.KERNEL_REDUCE_F32 if fmt == "f32" else ipls.KERNEL_REDUCE_H16
