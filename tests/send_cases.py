"""Cases and a plain model of k_b64url_encode_flat's decomposition (SendGradients).

Shared by tests/test_send_cases.py (CPU: the cases reach what they claim and
tell a wrong kernel from the right one) and tests/test_gpu_send.py (GPU:
Aggregator.SendGradients against the oracle, byte for byte).  numpy and the
standard library only (codec_cases.py, which it takes the encoder's shape
from, is the same): importable without a GPU, the library or the oracle;
oracle_text takes the oracle as its first argument `O` (oracle.oracle).

Geometry of the kernel under test (ipls_kernels.hpp; test_send_cases.py reads
the header and compares).  The frame of partition p of a handle (M, P) is
[14 header bytes][L_p x f64 BE][origin]; with lo = p * chunk and ncopy = the
values of the flat vector of n values that fall into the partition, payload
value i is flat[lo + i] widened (i < ncopy), 1.0 (i == ncopy, the count slot)
or +0.0 (ncopy < i < L_p).  Lane g owns frame bytes [24g, 24g + 24) = 32
chars and spans payload values 3g - 2 .. 3g + 1; it is FAST when g >= 1 and
3g + 2 <= ncopy (all four values are copied ones: four element loads at
lo + 3g - 2), else SLOW (byte by byte: the header, the window that holds the
count slot, the zero tail, the origin).  Waves, rows and blocks are the
publish encoder's (codec_cases.py).

model_text restates which lane produces which char and what a wrong kernel
would put there instead.  It starts from the source's bits and the standard
library's base64; it never checks the library.
"""
import base64
import struct
import zlib

import numpy as np

import codec_cases as C

GROUP, GROUP_CHARS, WAVE_GROUPS, BLOCK = C.GROUP, C.GROUP_CHARS, C.WAVE_GROUPS, C.BLOCK
FILL, GUARD = C.FILL, C.GUARD
ENC_CENTRES = C.ENC_CENTRES                      # 24, 48, 768, 1536, 2304, 6144, 12288 frame bytes

FMTS = ("f64", "be", "f32", "f16", "bf16")       # x host / device = the ten source kinds
ESIZE = {"f64": 8, "be": 8, "f32": 4, "f16": 2, "bf16": 2}
BITS = {"f64": np.uint64, "be": np.uint64, "f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
ONE_F64 = 0x3FF0000000000000
NEG_ZERO_F64 = 0x8000000000000000
PAD = 8                                          # junk elements kept before and after every source vector

# -0.0, +0.0, the smallest subnormal, the largest finite value, +-inf, a quiet NaN (doubles: and one with a payload)
SPECIALS = {
    "f64": (0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000,
            0xFFF0000000000000, 0x7FF8000000000000, 0x7FF80000DEADBEEF),
    "f32": (0x80000000, 0x00000000, 0x00000001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000),
    "f16": (0x8000, 0x0000, 0x0001, 0x7BFF, 0x7C00, 0xFC00, 0x7E00),
    "bf16": (0x8000, 0x0000, 0x0001, 0x7F7F, 0x7F80, 0xFF80, 0x7FC0),
}
SPECIALS["be"] = SPECIALS["f64"]
EXP_MASK = {"f64": (0x7FF, 52), "be": (0x7FF, 52), "f32": (0xFF, 23), "f16": (0x1F, 10), "bf16": (0xFF, 7)}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------
# handle geometry (IPLS.java:1019-1028)
# --------------------------------------------------------------------------
def chunk(M, P):
    return M // P + 1


def lengths(M, P):
    return C.model_lengths(M, P)


def ncopy_of(M, P, n, p):
    """Values of a flat vector of n values that OrganizeGradients copies into partition p."""
    lo = p * chunk(M, P)
    return max(0, min(lo + chunk(M, P), n) - lo)


def lane_fast(g, ncopy):
    return g >= 1 and 3 * g + 2 <= ncopy


def fast_lanes(L, ncopy, o):
    return [g for g in range(C.n_groups(C.frame_len(L, o))) if lane_fast(g, ncopy)]


def slow_chars(L, ncopy, o):
    """Mask over the padded text: True where a slow lane produced the char."""
    T = C.text_len(C.frame_len(L, o))
    slow = np.ones(T, dtype=bool)
    for g in fast_lanes(L, ncopy, o):
        slow[GROUP_CHARS * g:GROUP_CHARS * (g + 1)] = False
    return slow


def model_for(L):
    """(M, P, p): a handle whose partition p has L doubles (the count slot among them)."""
    if L >= 3:
        return 2 * L - 3, 2, 0           # chunk L - 1: lengths [L, L - 1]
    return (1, 2, 1) if L == 1 else (1, 2, 0)   # lengths [2, 1]


def model_with_last(t):
    """(M, P): the smallest handle whose last partition has t doubles and whose others, which are always
    longer, have at most 6 (7 beside a last one of 6)."""
    for P in range(2, 12):
        for M in range(1, 80):
            ls = lengths(M, P)
            if ls[-1] == t and min(ls) >= 1 and max(ls) <= max(6, t + 1):
                return M, P
    raise AssertionError(t)


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
class Case:
    """One call: handle (M, P), a flat vector of n values, the listed
    partitions, the iteration, pid and origin length."""

    def __init__(self, name, M, P, n, parts, o):
        self.name, self.M, self.P, self.n, self.parts, self.o = name, M, P, n, tuple(parts), o
        r = _rng("send-header", name)
        self.iteration = int(r.integers(-2 ** 31, 2 ** 31))
        self.pid = int(r.integers(-2 ** 15, 2 ** 15))
        self.origin = r.integers(0, 256, size=o, dtype=np.uint8).tobytes()
        self.lengths = lengths(M, P)
        self.chunk = chunk(M, P)

    def __repr__(self):
        return self.name

    def lo(self, p):
        return p * self.chunk

    def ncopy(self, p):
        return ncopy_of(self.M, self.P, self.n, p)

    def frame_len(self, p):
        return C.frame_len(self.lengths[p], self.o)

    def fast(self, p):
        return fast_lanes(self.lengths[p], self.ncopy(p), self.o)


EDGE_ORIGINS = (0, 1, 2, 46)          # the issue's origins: F = c - 2, c - 1, c and c -+ 4 (46 = 6 mod 8)
EDGE_ORIGINS_ABOVE = (3, 4, 5)        # c is 2 mod 8 past the header, so only these reach c + 1 .. c + 3
COUNT_LANES = (1, WAVE_GROUPS - 1, BLOCK - 1)   # the second lane, a wave's last lane, a block's last lane
COUNT_MODEL = (1599, 2)               # chunk 800: partitions of 801 and 800 doubles
RESIDUE_MODEL = (583, 8)              # chunk 73 = 1 mod 8: lo = 73 p takes every residue mod 8
SHORT_MODEL, SHORT_N = (399, 4), 230  # chunk 100: partition 2 keeps 30 values, partition 3 none
LAST_MODEL = (396, 4)                 # chunk 100, a last partition of 97 doubles


def residue_cases():
    M, P = RESIDUE_MODEL
    return [Case("residues", M, P, M, range(P), 13)]


def edge_cases():
    """Frame lengths within 3 of every lane, half-row, wave and block edge
    (and 4 away with the 46-byte origin), the other partition of the handle
    listed behind the one under test."""
    out = []
    for c in ENC_CENTRES:
        for F in range(c - 4, c + 5):
            for o in EDGE_ORIGINS + EDGE_ORIGINS_ABOVE:
                if (F - 14 - o) % 8 or F - 14 - o < 8 or (abs(F - c) == 4) != (o == 46):
                    continue
                L = (F - 14 - o) // 8
                M, P, p = model_for(L)
                out.append(Case(f"edge-{c}{F - c:+d}-o{o}", M, P, M, (p, 1 - p), o))
    return out


def count_slot_cases():
    """ncopy at each of the four values 3g - 2 .. 3g + 1 of lane g's window
    (ncopy mod 3 = 1, 2, 0, 1), in partition 1 of the handle, whose first
    value lies at flat offset 800; partition 0 is listed too and is whole."""
    M, P = COUNT_MODEL
    out = []
    for g in COUNT_LANES:
        for k in (3 * g - 2, 3 * g - 1, 3 * g, 3 * g + 1):
            out.append(Case(f"count-g{g}-ncopy{k}", M, P, chunk(M, P) + k, (1, 0), 5))
    return out


def short_cases():
    M, P = SHORT_MODEL
    return [Case("short", M, P, SHORT_N, (3, 2, 0), 46), Case("short-first-only", M, P, 7, (0, 1), 0)]


def last_cases():
    M, P = LAST_MODEL
    return [Case("last-shorter", M, P, M, (3, 1), 2)]


def tiny_cases():
    """Last partitions of 1 .. 6 doubles beside partitions of at most 6.  In
    those of up to 5 no lane is fast (ncopy <= 4); one of 6 has ncopy = 5 and
    lane 1 alone is fast."""
    out = []
    for t in range(1, 7):
        M, P = model_with_last(t)
        out.append(Case(f"tiny-{t}", M, P, M, (P - 1, 0), (0, 1, 2, 46)[t % 4]))
    return out


def all_tiny_case():
    """Every listed partition has ncopy <= 4: no fast lane anywhere in the launch."""
    return next(c for c in tiny_cases() if all(c.ncopy(p) <= 4 for p in c.parts))


def all_cases():
    return residue_cases() + edge_cases() + count_slot_cases() + short_cases() + last_cases() + tiny_cases()


# --------------------------------------------------------------------------
# source vectors
# --------------------------------------------------------------------------
def source_bits(case, fmt):
    """PAD + n + PAD bit patterns of the format: finite random values (junk in
    the pads, which the call must never read into a text) with the specials
    planted in every listed partition that has copied values: -0.0 first,
    last and in the middle, the others spread over it."""
    dt = BITS[fmt]
    n = case.n
    r = _rng("send-source", case.name, fmt)
    v = r.integers(0, np.iinfo(dt).max, size=n + 2 * PAD, dtype=dt, endpoint=True)
    mask, shift = EXP_MASK[fmt]
    inf = (v >> dt(shift)) & dt(mask) == dt(mask)
    v[inf] ^= dt(1 << shift)                      # finite
    sp = SPECIALS[fmt]
    for p in case.parts:
        nc, lo = case.ncopy(p), PAD + case.lo(p)
        if nc == 0:
            continue
        if nc < 2 * len(sp):
            for j in range(nc):
                v[lo + j] = sp[(p + j) % len(sp)] if j % 2 == 0 or nc < 4 else v[lo + j]
            v[lo + nc - 1] = sp[0]
            continue
        for j, s in enumerate(sp):
            v[lo + j * nc // len(sp) + (p % 3 if j else 0)] = s
        v[lo + nc // 2] = sp[0]
        v[lo + nc - 1] = sp[0]
    return v


def source_bytes(bits, fmt):
    """The bytes of the padded source as the kind stores them."""
    return bits.astype(">u8").tobytes() if fmt == "be" else bits.tobytes()


def widen_bits(bits, fmt):
    """The doubles of the patterns, as 64-bit patterns (include/ipls_agg.h's widening rule), by numpy."""
    if fmt in ("f64", "be"):
        return np.ascontiguousarray(bits, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        if fmt == "f32":
            w = np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)
        elif fmt == "f16":
            w = np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)
        else:
            w = (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32) \
                .astype(np.float64)
    return w.view(np.uint64)


# --------------------------------------------------------------------------
# the decomposition and its wrong variants
# --------------------------------------------------------------------------
VARIANTS = ("count-missing", "count-at-end", "neg-zero-lost", "read-early", "read-late", "header-swapped",
            "tail-from-neighbour")
LANES = ("all", "fast", "slow")


def payload(case, p, wide, variant=None):
    """The L_p payload patterns of partition p from the widened padded source
    `wide`, as the kernel's value rule gives them or as a wrong variant would."""
    L, nc, lo = case.lengths[p], case.ncopy(p), PAD + case.lo(p)
    shift = {"read-early": -1, "read-late": 1}.get(variant, 0)
    v = np.zeros(L, dtype=np.uint64)
    v[:nc] = wide[lo + shift:lo + shift + nc]
    if variant == "neg-zero-lost":
        v[v == np.uint64(NEG_ZERO_F64)] = 0
    if variant == "tail-from-neighbour":
        hi = max(nc + 1, min(L, wide.size - lo))     # what the memory behind the vector holds, as far as it is known
        v[nc + 1:hi] = wide[lo + nc + 1:lo + hi]
    if variant == "count-at-end":
        v[L - 1] = ONE_F64
    elif variant != "count-missing":
        v[nc] = ONE_F64
    return v


def frame(case, p, wide, variant=None):
    a, b = (case.iteration, p) if variant == "header-swapped" else (p, case.iteration)
    head = struct.pack(">hiii", case.pid, case.lengths[p], a, b)
    return head + payload(case, p, wide, variant).astype(">u8").tobytes() + case.origin


def model_text(case, p, wide, variant=None, lanes="all"):
    """The text of partition p as the decomposition writes it: the chars of
    the lanes named by `lanes` come from the wrong variant's frame, every
    other char from the right one."""
    right = base64.urlsafe_b64encode(frame(case, p, wide))
    if variant is None:
        return right
    wrong = base64.urlsafe_b64encode(frame(case, p, wide, variant))
    if lanes == "all":
        return wrong
    slow = slow_chars(case.lengths[p], case.ncopy(p), case.o)
    take = slow if lanes == "slow" else ~slow
    out = np.frombuffer(right, dtype=np.uint8).copy()
    out[take] = np.frombuffer(wrong, dtype=np.uint8)[take]
    return out.tobytes()


def oracle_text(O, case, fmt, p):
    """What the call must produce, from the oracle (`O` = oracle.oracle) and
    nothing of ours: its OrganizeGradients, frame and Base64 restatements over
    the source converted to float64 by numpy (big-endian bytes through
    be_decode)."""
    bits = source_bits(case, fmt)[PAD:PAD + case.n]
    if fmt == "be":
        flat = O.be_decode(bits.astype(">u8").tobytes())
    else:
        flat = widen_bits(bits, fmt).view(np.float64)
    part = O.organize_gradients(flat, case.M, case.P)[p]
    return O.java_b64url_encode(O.frame_encode(part, p, case.iteration, case.pid, case.origin))


def null_text(case, p):
    """Marshall_Packet(null, ...): n = 0, the header and the origin."""
    return base64.urlsafe_b64encode(struct.pack(">hiii", case.pid, 0, p, case.iteration) + case.origin)


def batch_layout(lens):
    return C.batch_layout(lens)
