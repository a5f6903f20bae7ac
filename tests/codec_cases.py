"""Cases and a plain model of the pubsub codec kernels' decomposition.

Shared by tests/test_codec_cases.py (CPU: the cases reach what they claim and
tell a wrong kernel from a right one) and tests/test_gpu_codec_seams.py (GPU:
k_b64url_encode_frame, k_b64url_encode_frames and k_b64url_decode against the
oracle, byte for byte).  numpy and the standard library only: importable
without a GPU, the library or the oracle.  Functions that need the oracle
take it as their first argument `O` (oracle.oracle).

Geometry of the kernels under test (ipls_kernels.hpp; test_codec_cases.py
parses the header and compares):
  encoder  lane g owns frame bytes [24g, 24g + 24) = 32 chars; a wave's 64
           groups (1536 frame bytes, 2048 chars) leave as two rows of 1024
           chars (768 frame bytes each); a block of kBlock lanes covers 6144
           frame bytes.  A lane is FAST when g >= 1, 24g + 24 <= 14 + 8n and
           the source is not null; every other lane is SLOW (enc_lane_fast).
  decoder  a lane owns 4 units of 4 chars (16 chars, 12 bytes); a block covers
           4096 chars = 3072 decoded bytes.  With units = dc / 4 whole units
           and tail = dc % 4 data chars after them, lane l takes the VECTOR
           path when 4l + 4 <= units; the lane with 4l <= units < 4l + 4 runs
           the SCALAR loop over the whole units it has left and then the TAIL
           (dec_paths).

The model_* functions restate which lane, path and store slot produces or
consumes each byte, and the wrong variants a kernel could run instead.  They
start from the right text or the right bytes (the standard library's
base64, or the oracle's decoder) and move, drop or replace what the variant
would: they do not map symbols themselves and never check the library.
"""
import base64
import zlib

import numpy as np

ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
INVALID_BYTES = tuple(b for b in range(256) if b not in ALPHABET)   # 192 values, '=' among them

BLOCK = 256              # kBlock, ipls_kernels.hpp:37
GROUP = 24               # frame bytes per encoder lane (b0 = 24 * g)
GROUP_CHARS = 32         # their chars
WAVE_GROUPS = 64         # groups per wave: one LDS row of 128 16-B slots (128 * wv)
ROW_CHARS = 1024         # chars per stored row (1024 * h)
ENC_HALF = 768           # frame bytes per row
ENC_WAVE = 1536          # frame bytes per wave
ENC_BLOCK = 6144         # frame bytes per block
DEC_UNITS = 4            # 4-char units per decoder lane
DEC_LANE_CHARS = 16
DEC_BLOCK_CHARS = 4096   # chars per decoder block
DEC_BLOCK_BYTES = 3072   # decoded bytes per decoder block

FILL = 0xAB              # what a device text output holds before the call
GUARD = 64               # bytes of FILL kept on each side of a device text


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------
# the status rule of the ingest (tests/test_gpu_parity.py::_ingest_expected)
# --------------------------------------------------------------------------
def ingest_expected(O, m, layers, P, lengths, part=None):
    """Status the ingest must report for one text, from the oracle's Java
    restatement: -6 IllegalArgument/BufferUnderflow, 1 null gradient, -2 out
    of range (GET_GRADIENTS, MyIPFSClass.java:1437-1459), 0 folded."""
    try:
        fr = O.pubsub_decode(m) if layers == 2 else O.java_b64url_decode(m)
        pid, nn, a, b, gg, origin = O.frame_decode(fr)
    except ValueError:
        return -6, None
    if gg is None:
        return 1, None
    p = a if part is None else part
    if not 0 <= p < P or nn < lengths[p]:
        return -2, None
    return 0, (p, gg)


# --------------------------------------------------------------------------
# frame and text geometry
# --------------------------------------------------------------------------
def frame_len(n, o):
    return 14 + 8 * n + o


def text_len(F):
    """Chars of Base64.getUrlEncoder's padded text of F bytes."""
    return 4 * ((F + 2) // 3)


def data_chars(F):
    """Chars of the text without its '=' padding."""
    return 4 * (F // 3) + (0, 2, 3)[F % 3]


def n_groups(F):
    return (F + GROUP - 1) // GROUP


def enc_lane_fast(g, n, src_null):
    """The kernel's condition for the 8-B-load, funnel-shift, LDS-table path."""
    return g >= 1 and GROUP * g + GROUP <= 14 + 8 * n and not src_null


def enc_slow_chars(n, o, src_null):
    """Mask over the padded text: True where a slow lane produced the char."""
    F = frame_len(n, o)
    T = text_len(F)
    slow = np.zeros(T, dtype=bool)
    for g in range(n_groups(F)):
        if not enc_lane_fast(g, n, src_null):
            slow[GROUP_CHARS * g:GROUP_CHARS * (g + 1)] = True
    return slow


def boundary_group_from_end(n, o):
    """0 when the payload/origin boundary (frame byte 14 + 8n) lies in the last group, 1 in the second-last ..."""
    F = frame_len(n, o)
    return n_groups(F) - 1 - (14 + 8 * n) // GROUP


# --------------------------------------------------------------------------
# encoder cases
# --------------------------------------------------------------------------
ENC_CENTRES = (24, 48, ENC_HALF, ENC_WAVE, ENC_WAVE + ENC_HALF, ENC_BLOCK, 2 * ENC_BLOCK)
ENC_SMALL_N = (1, 2, 3, 4, 5, 6)
ENC_SMALL_O = (0, 1, 2, 10, 24, 25)


def encoder_pairs():
    """Sorted (n, o): every frame length F = 14 + 8n + o within 3 of a lane,
    half-row, wave and block edge, each with the origins ((F - 14) mod 8) +
    8k, k in (0, 3, 6), that leave n >= 1; and the texts of n = 1 .. 6 in
    which no lane, or only lane 1, is fast."""
    pairs = set()
    for c in ENC_CENTRES:
        for F in range(c - 3, c + 4):
            for k in (0, 3, 6):
                o = (F - 14) % 8 + 8 * k
                if F - 14 - o >= 8:
                    pairs.add(((F - 14 - o) // 8, o))
    for n in ENC_SMALL_N:
        for o in ENC_SMALL_O:
            pairs.add((n, o))
    return sorted(pairs)


def encoder_ns():
    return sorted({n for n, _ in encoder_pairs()})


def origins_of(n):
    return [o for m, o in encoder_pairs() if m == n]


_SPECIAL_BITS = (0x7FF80000DEADBEEF,   # quiet NaN with a payload
                 0x7FF0000000000001,   # signalling NaN
                 0xFFF4000000C0FFEE,   # negative signalling NaN with a payload
                 0x7FF0000000000000, 0xFFF0000000000000,   # +-inf
                 0x8000000000000000, 0x0000000000000000,   # -0.0, +0.0
                 0x0000000000000001, 0x800FFFFFFFFFFFFF,   # smallest and (negative) largest subnormal
                 0x000FEDCBA9876543)                        # a subnormal with a busy mantissa


def enc_values(n, p):
    """n arbitrary 64-bit patterns for partition p of the handle of n doubles
    (putDouble keeps raw bits): seeded random words with NaN payloads,
    infinities, both zeros and subnormals planted over them."""
    v = _rng("enc-values", n, p).integers(0, 2 ** 64, size=n, dtype=np.uint64)
    k = len(_SPECIAL_BITS)
    if n < 2 * k:
        v[p % n] = _SPECIAL_BITS[(n + p) % k]
        return v
    step = n // k
    for j, s in enumerate(_SPECIAL_BITS):
        v[j * step + p % step] = s
    return v


def enc_header(n, o):
    """(a, [b of partitions 0, 1, 2], pid) of the case: any int32 / int16."""
    r = _rng("enc-header", n, o)
    a = int(r.integers(-2 ** 31, 2 ** 31))
    bs = [int(x) for x in r.integers(-2 ** 31, 2 ** 31, size=3)]
    return a, bs, int(r.integers(-2 ** 15, 2 ** 15))


def enc_origin(n, o):
    return _rng("enc-origin", n, o).integers(0, 256, size=o, dtype=np.uint8).tobytes()


def frame_bytes(O, bits, a, b, pid, origin):
    """The Marshall_Packet frame of the planted patterns: the oracle's header,
    the patterns as big-endian words (never a value read back), the origin."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    head = O.frame_encode(np.zeros(bits.size), a, b, pid, b"")[:14]
    return head + bits.astype(">u8").tobytes() + bytes(origin)


def batch_layout(lens):
    """(offsets, end) of publish_partials' texts: each starts on a 64-B boundary."""
    offs, pos = [], 0
    for n in lens:
        pos = (pos + 63) // 64 * 64
        offs.append(pos)
        pos += n
    return offs, pos


# model geometry, Aggregator(M, P, devices=[0, 0]) (IPLS.java:1019-1028 restated in model_lengths): with M = P q + r
# the last partition has q + r - P + 2 doubles, so a last partition of fewer than 5 needs about as many partitions as
# the common length.  M = 190 * 191: 189 partitions of 193 = 192 + 1 doubles and a last one of 3.
ENC_MODEL = (36290, 190)
ENC_MODEL_BATCH = (189, 0, 94, 95, 188)    # the short one first, both sides of the shard boundary (p // 95)


def model_lengths(M, P):
    c = M // P + 1
    return [M - i * c + 1 if (i + 1) * c > M else c + 1 for i in range(P)]


# --------------------------------------------------------------------------
# the encoder's decomposition and its wrong variants
# --------------------------------------------------------------------------
ENC_VARIANTS = ("fast-limit+group", "funnel-8", "funnel-24", "row1-at-row0", "partial-dropped", "partial-whole",
                "pad-early")
ENC_UNOBSERVABLE = ("fast-limit-group",)   # the slow path computes any lane: one fast lane fewer writes the same text


def _b64(data):
    return base64.urlsafe_b64encode(bytes(data))


def model_encode(frame, n, src_null, variant=None, after=b""):
    """The device buffer [GUARD x FILL][text][GUARD x FILL] after the call,
    as the kernel's decomposition writes it -- or as a wrong variant would.
    `after`: what the accumulator's memory holds behind the payload (read only
    by the variant that takes one lane too many for a fast one)."""
    frame = bytes(frame)
    F = len(frame)
    T = text_len(F)
    text = bytearray(_b64(frame))
    G = n_groups(F)
    if variant in ("funnel-8", "funnel-24"):
        d = -1 if variant == "funnel-8" else 1           # the window starts 1 or 3 bytes into the doubles, not 2
        for g in range(G):
            if enc_lane_fast(g, n, src_null):
                text[GROUP_CHARS * g:GROUP_CHARS * (g + 1)] = _b64(frame[GROUP * g + d:GROUP * g + d + GROUP])
    elif variant == "fast-limit+group":
        g = next((g for g in range(1, G) if GROUP * g + GROUP > 14 + 8 * n), None)
        if g is not None and not src_null:
            mem = frame[14:14 + 8 * n] + bytes(after) + bytes(64)
            w = _b64(mem[GROUP * g - 14:GROUP * g - 14 + GROUP])
            lo = GROUP_CHARS * g
            text[lo:min(T, lo + GROUP_CHARS)] = w[:min(T, lo + GROUP_CHARS) - lo]
    elif variant == "fast-limit-group":
        pass                                             # the lane goes the slow way and writes the same chars
    elif variant == "pad-early" and F % 3:
        text[T - 1 - (3 - F % 3):] = b"=" * (1 + 3 - F % 3)
    buf = bytearray([FILL]) * (GUARD + T + GUARD)
    buf[GUARD:GUARD + T] = text
    if variant == "row1-at-row0":
        wave_chars = 2 * ROW_CHARS
        for wb in range(0, T, wave_chars):
            row1 = text[wb + ROW_CHARS:min(T, wb + wave_chars)]
            if row1:
                buf[GUARD + wb:GUARD + wb + len(row1)] = row1
                buf[GUARD + wb + ROW_CHARS:GUARD + wb + ROW_CHARS + len(row1)] = bytes([FILL]) * len(row1)
    elif variant == "partial-dropped" and T % 16:
        buf[GUARD + T - T % 16:GUARD + T] = bytes([FILL]) * (T % 16)
    elif variant == "partial-whole" and T % 16:
        buf[GUARD + T:GUARD + T + 16 - T % 16] = bytes(16 - T % 16)   # the staged row is zero past the text
    return bytes(buf)


# --------------------------------------------------------------------------
# decoder cases
# --------------------------------------------------------------------------
# 9: without an origin the outer layer's (units mod 4, tail) has period 9 in L, and (2, 2) needs L = 0 mod 9
DEC_LS = (2, 3, 4, 5, 6, 7, 9, 382, 383, 384, 385, 386, 766, 767, 768, 769, 770, 1536)
DEC_ORIGINS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 46)


def dec_paths(dc):
    """(units, tail, vector lanes, first scalar unit): the decomposition of a text of dc data chars."""
    units, tail = dc // 4, dc % 4
    vec = units // DEC_UNITS
    return units, tail, vec, DEC_UNITS * vec


def dec_char_path(dc, i):
    """'vector', 'scalar' or 'tail' for data char i, with its position in the unit."""
    units, tail, vec, s0 = dec_paths(dc)
    u = i // 4
    return ("tail" if u >= units else "vector" if u < s0 else "scalar"), i % 4


def dec_payload(L, *key):
    """L random 64-bit patterns whose exponent field is not 0x7FF (finite: +0.0 + x is x, -0.0 gives +0.0)."""
    v = _rng("dec-payload", L, *key).integers(0, 2 ** 64, size=L, dtype=np.uint64)
    inf = (v >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF)
    v[inf] &= np.uint64(0xBFFFFFFFFFFFFFFF)
    if L >= 4:
        v[1], v[2] = np.uint64(0x8000000000000000), np.uint64(1)     # -0.0 and the smallest subnormal
    return v


def folded_bits(bits):
    """Bits of +0.0 + x for every planted pattern."""
    x = np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64)
    return (0.0 + x).view(np.uint64)


def dec_header(L, o):
    r = _rng("dec-header", L, o)
    return int(r.integers(-2 ** 31, 2 ** 31)), int(r.integers(-2 ** 31, 2 ** 31)), 3


def dec_origin(L, o):
    return _rng("dec-origin", L, o).integers(0, 256, size=o, dtype=np.uint8).tobytes()


def strip(t):
    return bytes(t).rstrip(b"=")


def sweep_messages(O, L, layers):
    """[(text, planted bits, o, (inner data chars, outer data chars or None))]
    of one handle: frames of n = L doubles with every origin of DEC_ORIGINS,
    one layer padded and unpadded, two layers in the four pairings."""
    out = []
    for o in DEC_ORIGINS:
        a, b, pid = dec_header(L, o)
        forms = (0, 1) if layers == 1 else (0, 1, 2, 3)
        for form in forms:
            bits = dec_payload(L, o, layers, form)
            inner = O.java_b64url_encode(frame_bytes(O, bits, a, b, pid, dec_origin(L, o)))
            if form & 1:
                inner = strip(inner)
            if layers == 1:
                out.append((inner, bits, o, (len(strip(inner)), None)))
                continue
            outer = O.java_b64url_encode(inner)
            if form & 2:
                outer = strip(outer)
            out.append((outer, bits, o, (len(strip(inner)), len(strip(outer)))))
    return out


# alphabet cases: L = 4 (15 units: 3 vector lanes, 3 scalar units, a tail of 2) and L = 6 (20 units: 5 vector
# lanes, no scalar unit, a tail of 3 done by a lane of its own), one layer, no origin, 256 messages each
ALPHA_LS = (4, 6)
ALPHA_MSGS = 256


def alphabet_messages(O, L):
    """[(text, planted bits)]: message i ends in the frame bytes that make the
    tail's chars run over the alphabet (the count slot's low bytes are free)."""
    out = []
    for i in range(ALPHA_MSGS):
        bits = dec_payload(L, "alpha", i)
        if L % 3 == 1:      # tail 2: one byte, char 0 = i >> 2
            low = i
            bits[-1] = (bits[-1] & np.uint64(0xFFFFFFFFFFFFFF00)) | np.uint64(low)
        else:               # tail 3: two bytes, char 0 = i >> 2, char 1 = (i & 3) << 4 | (i >> 2) & 15
            low = (i << 8) | (((i >> 2) & 15) << 4) | ((i >> 4) & 15)
            bits[-1] = (bits[-1] & np.uint64(0xFFFFFFFFFFFF0000)) | np.uint64(low)
        text = O.java_b64url_encode(frame_bytes(O, bits, i, -i, 3, b""))
        out.append((text if i % 2 else strip(text), bits))
    return out


def discarded_bits_messages(O):
    """[(text, planted bits, layers)]: texts whose last data char of a two- or
    three-char tail carries non-zero bits that Java's decoder ignores, with
    every value of the ignored bits.  Frame layer, sent as one layer and
    wrapped in a second: frames of 4 and 6 doubles without an origin (tails of
    2 and 3), so that the tail's bytes lie in the last payload double and can
    be read back.  Outer layer: the texts of 4, 5 and 6 doubles, padded and
    not, wherever the outer text has a tail."""
    out = []

    def bump(text, k):
        """The unpadded text with k or'ed into its last char's symbol value."""
        t = bytearray(strip(text))
        t[-1] = ALPHABET[ALPHABET.index(bytes([t[-1]])) | k]
        return bytes(t)

    for Lf in (4, 6):
        free = 4 if data_chars(frame_len(Lf, 0)) % 4 == 2 else 2
        for k in range(1, 1 << free):
            for layers in (1, 2):
                bits = dec_payload(Lf, "discard", k, layers)
                inner = O.java_b64url_encode(frame_bytes(O, bits, k, 7, 3, b""))
                pad = inner[len(strip(inner)):]
                inner = bump(inner, k) + (pad if k % 2 else b"")
                out.append((inner if layers == 1 else O.java_b64url_encode(inner), bits, layers))
    # outer layer: an inner text of 3m + 1 and 3m + 2 bytes
    for Lf in (4, 5, 6):
        for padded in (False, True):
            bits = dec_payload(Lf, "discard-outer", padded)
            inner = O.java_b64url_encode(frame_bytes(O, bits, 1, 2, 3, b""))
            inner = inner if padded else strip(inner)
            outer = O.java_b64url_encode(inner)
            tail = len(strip(outer)) % 4
            if tail == 0:
                continue
            for k in range(1, 1 << (4 if tail == 2 else 2)):
                out.append((bump(outer, k) + (outer[len(strip(outer)):] if k % 2 else b""), bits, 2))
    return out


# --------------------------------------------------------------------------
# every invalid byte, by layer and position class
# --------------------------------------------------------------------------
INVALID_L = 5
# frames of n = 5 doubles: o = 4 / 5 give 19 whole units (4 vector lanes, 3 scalar units) and a tail of 2 / 3;
# o = 7 / 8 give 20 whole units (5 vector lanes; the tail's lane has no whole unit) and a tail of 2 / 3
INVALID_ORIGINS = (4, 5, 7, 8)


def position_classes(dc, T):
    """{class: char index} in a text of dc data chars and T chars in all."""
    units, tail, vec, s0 = dec_paths(dc)
    cls = {}
    if vec >= 2:
        cls["vector-first"] = DEC_LANE_CHARS * (vec - 1)
        cls["vector-last"] = DEC_LANE_CHARS * (vec - 1) - 1
    if units > s0:
        cls["scalar"] = 4 * s0 + 1 + 4 * ((units - s0) // 2)
    for j in range(tail):
        cls[f"tail-{j}"] = 4 * units + j
    cls["char-27"], cls["char-28"] = 27, 28
    cls["end-9"], cls["end-8"] = T - 9, T - 8
    return cls


def invalid_class_names():
    return ("vector-first", "vector-last", "scalar", "tail-0", "tail-1", "tail-2", "char-27", "char-28", "end-9",
            "end-8")


def invalid_batches(O):
    """{(layer, class): [(text, planted bits, bad)]}: per batch one message
    per invalid byte value carrying it at that class's position of that layer
    ('outer': in the text as sent; 'inner': in the inner text, then encoded
    again), a valid message after every third.  `bad` is None for the valid
    ones, else (byte, frame origin length, data chars of the layer, index)."""
    batches = {}
    for layer in ("outer", "inner"):
        for cname in invalid_class_names():
            msgs, k = [], 0
            for j, byte in enumerate(INVALID_BYTES):
                # the frames that have this class, in turn
                have = []
                for o in INVALID_ORIGINS:
                    F = frame_len(INVALID_L, o)
                    inner_T = text_len(F)
                    dc, T = (data_chars(F), inner_T) if layer == "inner" else (data_chars(inner_T), text_len(inner_T))
                    if cname in position_classes(dc, T):
                        have.append((o, dc, T))
                o, dc, T = have[j % len(have)]
                bits = dec_payload(INVALID_L, layer, cname, byte)
                inner = bytearray(O.java_b64url_encode(frame_bytes(O, bits, j, byte, 3, dec_origin(INVALID_L, o))))
                pos = position_classes(dc, T)[cname]
                if layer == "inner":
                    inner[pos] = byte
                    text = O.java_b64url_encode(bytes(inner))
                else:
                    t = bytearray(O.java_b64url_encode(bytes(inner)))
                    t[pos] = byte
                    text = bytes(t)
                msgs.append((text, bits, (byte, o, dc, pos)))
                k += 1
                if k % 3 == 0:
                    vb = dec_payload(INVALID_L, layer, cname, "valid", k)
                    vo = INVALID_ORIGINS[(k // 3) % len(INVALID_ORIGINS)]
                    msgs.append((O.pubsub_message(frame_bytes(O, vb, k, 1, 3, dec_origin(INVALID_L, vo))), vb, None))
            batches[(layer, cname)] = msgs
    return batches


# --------------------------------------------------------------------------
# the decoder's decomposition and its wrong variants
# --------------------------------------------------------------------------
# (test, admitted code point): each of the five range tests one code point wider at either end
WIDENED = {"A-Z-low": ord("A") - 1, "A-Z-high": ord("Z") + 1, "a-z-low": ord("a") - 1, "a-z-high": ord("z") + 1,
           "0-9-low": ord("0") - 1, "0-9-high": ord("9") + 1, "minus-low": ord("-") - 1, "minus-high": ord("-") + 1,
           "underscore-low": ord("_") - 1, "underscore-high": ord("_") + 1}
DEC_VARIANTS = ("tail-no-lane", "tail-wrong-unit") + tuple(WIDENED)


def host_checked(layers, layer, dc, i):
    """True when the host pre-check (pubsub_host.cpp) maps data char i of
    `layer` through its own alphabet test: of the text as sent, the units
    that hold the first 14 frame bytes (one layer) or the first 20 inner chars
    (two layers) and, with two layers, the units of the last 4 decoded bytes;
    of the inner text, the units of the first 14 frame bytes."""
    u = i // 4
    if layer == "inner":
        return 3 * u < 14
    if layers == 1:
        return 3 * u < 14
    n = 3 * (dc // 4) + (0, 0, 1, 2)[dc % 4]
    return 3 * u < 20 or 3 * u + 3 > n - min(4, n)


def model_decode_bytes(right, dc, variant=None):
    """(bytes, known): the decoder's output for a valid text of dc data chars
    whose right decoding is `right`, as the decomposition writes it or as a
    wrong variant would; known[i] False where the variant leaves byte i to
    whatever the scratch held."""
    right = bytearray(right)
    known = np.ones(len(right), dtype=bool)
    units, tail, vec, s0 = dec_paths(dc)
    if tail:
        nb = tail - 1
        if variant == "tail-no-lane" and units % DEC_UNITS == 0:
            known[3 * units:3 * units + nb] = False
        elif variant == "tail-wrong-unit" and units >= 1:
            right[3 * units:3 * units + nb] = right[3 * (units - 1):3 * (units - 1) + nb]
    return bytes(right), known


def model_status(right, layers, layer, byte, dc, i, variant=None):
    """The status of a message whose only invalid char is `byte` at data char
    i of `layer` (right status `right`) under a wrong variant.  A widened
    range test is widened in the kernel and in the host pre-check alike (they
    restate the same five tests); the tail variants are the kernel's alone, so
    a char that the host also maps keeps its status."""
    if right != -6 or i >= dc:
        return right
    if variant in WIDENED:
        return 0 if byte == WIDENED[variant] else right
    if host_checked(layers, layer, dc, i):
        return right
    path, _ = dec_char_path(dc, i)
    units = dc // 4
    if path == "tail" and variant == "tail-no-lane" and units % DEC_UNITS == 0:
        return 0
    if path == "tail" and variant == "tail-wrong-unit":
        return 0
    return right
