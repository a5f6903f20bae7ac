"""Host references of the half-precision trainer boundary, shared by
test_h16_boundary.py (which checks them against torch's CPU casts) and
test_gpu_h16.py (which checks the kernels against them).

A 16-bit array is carried as numpy uint16 bit patterns for both formats:
numpy has float16 but no bfloat16.
"""
import numpy as np

FORMATS = ("half", "bf16")


def widen(bits, fmt):
    """The exact doubles of 16-bit patterns: f16 -> f32 -> f64, or
    (bits << 16) taken as an f32 -> f64 (include/ipls_agg.h)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):   # a NaN among the patterns is not an error
        if fmt == "half":
            return bits.view(np.float16).astype(np.float32).astype(np.float64)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_rne(f32):
    """float32 -> bfloat16 bit patterns, round to nearest even on the upper 16
    bits: u + 0x7fff + ((u >> 16) & 1), NaNs kept NaN (quiet bit set) instead
    of being carried into the exponent."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x0040).astype(np.uint16), r)


def narrow(f32, fmt):
    """The second rounding of the two-step rule: a float32 array to the 16-bit
    format's bit patterns (what the trainer's own narrowing gives)."""
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    if fmt == "half":
        with np.errstate(over="ignore"):
            return f32.astype(np.float16).view(np.uint16)
    return bf16_rne(f32)


def is_nan(bits, fmt):
    bits = np.asarray(bits, dtype=np.uint16)
    if fmt == "half":
        return (bits & 0x7FFF) > 0x7C00
    return (bits & 0x7FFF) > 0x7F80


def one(fmt):
    return 0x3C00 if fmt == "half" else 0x3F80


def edge_bits(fmt):
    """+-0, smallest / largest subnormal, smallest normal, largest finite,
    +-inf, a quiet NaN, 1.0, and a pair that cancels (x, -x)."""
    if fmt == "half":
        e = [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0x3C00, 0x3555, 0xB555,
             0x8001, 0xFBFF]
    else:
        e = [0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x7F7F, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0x3EAB, 0xBEAB,
             0x8001, 0xFF7F]
    return np.array(e, dtype=np.uint16)
