"""The cases of tests/test_gpu_codec_seams.py reach what they claim (CPU, numpy and the oracle only).

The kernel shape that tests/codec_cases.py restates is the header's; the
encoder list has the frame lengths, boundary phases, paddings and text
residues it is meant to have, and its slow lanes show the whole alphabet; the
decoder lists cover every (whole units mod 4, tail) that a frame can reach,
and every symbol on every path; and every wrong variant of the decomposition
model changes a compared byte, a guard byte or a status in at least one case.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import codec_cases as C

HPP = Path(__file__).resolve().parent.parent / "ipls-java-api_amd" / "csrc" / "ipls_kernels.hpp"


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o
    return o


def test_constants_match_the_header():
    src = HPP.read_text()
    block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    group = int(re.search(r"const int64_t b0 = (\d+) \* g;", src).group(1))
    row16 = int(re.search(r"u4w\* ws = stage \+ (\d+) \* wv;", src).group(1))          # 16-B slots per wave row
    m = re.search(r"const int64_t o = wbase \+ (\d+) \* h \+ (\d+) \* lane;", src)
    half_chars, slot = int(m.group(1)), int(m.group(2))
    assert re.search(r"g >= 1 && b0 \+ 24 <= 14 \+ 8 \* f\.n && src\)", src)
    assert re.search(r"const int64_t wbase = 32 \* gw;", src) and re.search(r"gw = g0 \+ 64 \* wv;", src)
    dec_units = int(re.search(r"\(int64_t\)blockIdx\.x \* kBlock \+ threadIdx\.x\) \* (\d+);", src).group(1))
    assert re.search(r"if \(u0 \+ 4 <= d\.units\)", src) and re.search(r"if \(d\.tail && u0 \+ 4 > d\.units\)", src)
    assert (block, group, row16, half_chars, slot, dec_units) == (256, 24, 128, 1024, 16, 4)
    assert (C.BLOCK, C.GROUP, C.GROUP_CHARS, C.DEC_UNITS) == (block, group, group * 4 // 3, dec_units)
    assert C.WAVE_GROUPS == row16 * slot // C.GROUP_CHARS == 64 and C.ROW_CHARS == half_chars
    assert C.ENC_WAVE == C.WAVE_GROUPS * group == 1536
    assert C.ENC_HALF == half_chars * 3 // 4 == 768
    assert C.ENC_BLOCK == block * group == 6144
    assert C.DEC_LANE_CHARS == 4 * dec_units == 16
    assert C.DEC_BLOCK_CHARS == block * 4 * dec_units == 4096
    assert C.DEC_BLOCK_BYTES == block * 3 * dec_units == 3072
    assert len(C.ALPHABET) == 64 and len(C.INVALID_BYTES) == 192 and ord("=") in C.INVALID_BYTES


# ---------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------
def test_encoder_list():
    pairs = C.encoder_pairs()
    ns = C.encoder_ns()
    assert (len(pairs), len(ns), max(ns), sum(n for n, _ in pairs)) == (152, 36, 1534, 60088)
    lengths = {C.frame_len(n, o) for n, o in pairs}
    for c in (24, 48, 768, 1536, 2304, 6144, 12288):
        assert {F for F in range(c - 3, c + 4) if F >= 22} <= lengths, c      # 22: one double, no origin
    # (payload-end phase, frame length mod 3): all nine with an origin.  Without one F = 14 + 8n is the phase
    # mod 24, so F mod 3 is the phase mod 3 and only three combinations exist: all three occur.
    with_o = {((14 + 8 * n) % 24, C.frame_len(n, o) % 3) for n, o in pairs if o}
    without = {((14 + 8 * n) % 24, C.frame_len(n, o) % 3) for n, o in pairs if not o}
    assert with_o == {(ph, r) for ph in (6, 14, 22) for r in (0, 1, 2)}
    assert without == {(6, 0), (14, 2), (22, 1)}
    assert {C.text_len(C.frame_len(n, o)) % 16 for n, o in pairs} == {0, 4, 8, 12}
    assert {0, 1, 2} <= {C.boundary_group_from_end(n, o) for n, o in pairs}
    # texts in which no lane is fast, only lane 1, and lanes on both sides of every edge
    fast = {(n, o): [g for g in range(C.n_groups(C.frame_len(n, o))) if C.enc_lane_fast(g, n, False)] for n, o in pairs}
    assert any(not f for f in fast.values()) and any(f == [1] for f in fast.values())
    assert max(len(f) for f in fast.values()) > C.BLOCK + 2 * C.WAVE_GROUPS   # fast lanes in the second block's waves
    for n in ns:
        assert len(C.origins_of(n)) >= 1


def test_encoder_model_geometry():
    lens = C.model_lengths(*C.ENC_MODEL)
    assert len(lens) == 190 and set(lens[:-1]) == {193} and 193 == 192 + 1 and 1 <= lens[-1] < 5
    assert sum(L - 1 for L in lens) == C.ENC_MODEL[0]
    owners = {p // 95 for p in C.ENC_MODEL_BATCH}
    assert owners == {0, 1} and C.ENC_MODEL_BATCH[0] == 189
    groups = [C.n_groups(C.frame_len(lens[p], 13)) for p in C.ENC_MODEL_BATCH]
    assert min(groups) == 3 and max(groups) > 64                       # three lanes against more than a wave


def test_encoder_values_and_symbols(O):
    """Raw patterns with every special among them; over the list the chars of
    slow lanes show all 64 symbols in each position of a unit, and the origin
    bytes run over 0 .. 255."""
    seen_special = set()
    origin_bytes = set()
    sym = [set() for _ in range(4)]
    for n in C.encoder_ns():
        vals = [np.zeros(n, dtype=np.uint64), C.enc_values(n, 1), C.enc_values(n, 2)]
        assert (vals[1] != vals[2]).any()
        for v in vals[1:]:
            seen_special |= set(int(x) for x in v) & set(C._SPECIAL_BITS)
        for o in C.origins_of(n):
            a, bs, pid = C.enc_header(n, o)
            origin = C.enc_origin(n, o)
            assert len(origin) == o
            origin_bytes |= set(origin)
            for p in range(3):
                frame = C.frame_bytes(O, vals[p], a, bs[p], pid, origin)
                assert len(frame) == C.frame_len(n, o)
                if not np.isnan(vals[p].view(np.float64)).any():
                    assert frame == O.frame_encode(vals[p].view(np.float64), a, bs[p], pid, origin)
                text = np.frombuffer(O.java_b64url_encode(frame), dtype=np.uint8)
                assert text.size == C.text_len(len(frame))
                slow = C.enc_slow_chars(n, o, p == 0)
                assert slow[:C.GROUP_CHARS].all() and (p != 0 or slow.all())
                idx = np.flatnonzero(slow & (text != ord("=")))
                for k in range(4):
                    sym[k] |= set(text[idx[idx % 4 == k]].tolist())
    assert seen_special == set(C._SPECIAL_BITS)
    assert origin_bytes == set(range(256))
    for k in range(4):
        assert sym[k] == set(C.ALPHABET), (k, len(sym[k]))


def _enc_cases(O):
    for n in C.encoder_ns():
        for o in C.origins_of(n):
            a, bs, pid = C.enc_header(n, o)
            for p in range(3):
                v = np.zeros(n, dtype=np.uint64) if p == 0 else C.enc_values(n, p)
                yield n, o, p, C.frame_bytes(O, v, a, bs[p], pid, C.enc_origin(n, o))


def test_encoder_variants_differ(O):
    """Every wrong decomposition changes a text or a guard byte of the list;
    the ones tied to a seam change it in every case that has the seam."""
    hit = {v: 0 for v in C.ENC_VARIANTS}
    for n, o, p, frame in _enc_cases(O):
        null = p == 0
        right = C.model_encode(frame, n, null)
        F, T = len(frame), C.text_len(len(frame))
        assert right[C.GUARD:C.GUARD + T] == O.java_b64url_encode(frame)
        assert set(right[:C.GUARD]) == set(right[C.GUARD + T:]) == {C.FILL}
        d = {v: C.model_encode(frame, n, null, v) != right for v in C.ENC_VARIANTS}
        for v in C.ENC_VARIANTS:
            hit[v] += d[v]
        n_fast = sum(C.enc_lane_fast(g, n, null) for g in range(C.n_groups(F)))
        if n_fast and n >= 16:
            assert d["funnel-8"] and d["funnel-24"], (n, o, p)
        assert d["row1-at-row0"] == (T > C.ROW_CHARS), (n, o, p)
        assert d["partial-dropped"] == d["partial-whole"] == (T % 16 != 0), (n, o, p)
        assert d["pad-early"] == (F % 3 != 0), (n, o, p)
        # one fast lane fewer: the slow path computes any lane, so the text is the same.  No input can show it.
        assert C.model_encode(frame, n, null, C.ENC_UNOBSERVABLE[0]) == right
    for v, k in hit.items():
        assert k, f"variant {v} never shows"
    assert hit["fast-limit+group"] >= 50


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
def _sweep(O):
    for L in C.DEC_LS:
        for layers in (1, 2):
            for text, bits, o, (dci, dco) in C.sweep_messages(O, L, layers):
                yield L, layers, text, bits, o, dci, dco


def test_decoder_sweep_coverage(O):
    """(whole units mod 4, tail) per layer.  Frame layer: with an origin all
    twelve occur; without one F = 14 + 8L ties the units mod 4 to L mod 3 (L =
    3m: 8m + 4 units and a tail of 3; 3m + 1: 8m + 7 and 2; 3m + 2: 8m + 10 and
    0), three combinations.  Outer layer: it encodes a base64 text, whose
    length is 4q, 4q + 2 or 4q + 3, never 4q + 1; that leaves nine of the
    twelve combinations whatever the frame (enumerated below over a whole
    period of 48 chars), and all nine occur with an origin and without."""
    cover = {(layer, bool(o)): set() for layer in ("frame", "outer") for o in (0, 1)}
    for L, layers, text, bits, o, dci, dco in _sweep(O):
        assert C.ingest_expected(O, text, layers, 1, [L], 0)[0] == 0
        assert dci == C.data_chars(C.frame_len(L, o))
        cover[("frame", bool(o))].add((dci // 4 % 4, dci % 4))
        if dco is not None:
            cover[("outer", bool(o))].add((dco // 4 % 4, dco % 4))
    twelve = {(u, t) for u in range(4) for t in (0, 2, 3)}
    reach = {(C.data_chars(n) // 4 % 4, C.data_chars(n) % 4) for n in range(20, 20 + 96) if n % 4 != 1}
    assert len(reach) == 9 and reach < twelve
    assert cover[("frame", True)] == twelve
    assert cover[("frame", False)] == {(0, 3), (3, 2), (2, 0)}
    assert cover[("outer", True)] == reach and cover[("outer", False)] == reach
    # the block edges of both layers lie inside the payload of the long cases
    assert C.data_chars(C.frame_len(1536, 0)) > 4 * C.DEC_BLOCK_CHARS
    assert C.data_chars(C.text_len(C.frame_len(1536, 0))) > 5 * C.DEC_BLOCK_CHARS
    assert 14 + 8 * 382 <= C.DEC_BLOCK_BYTES < 14 + 8 * 383


def test_decoder_alphabet_coverage(O):
    """Frame layer, no origin: every symbol in every unit position of the
    vector path, of the scalar loop and of the tail's chars before its last;
    in the tail's last char every value of the bits that count, and (from the
    discarded-bits cases, at each layer) every non-zero value of those that do not."""
    sym = {(path, k): set() for path in ("vector", "scalar", "tail") for k in range(4)}
    last = {2: set(), 3: set()}

    def take(inner):
        t = C.strip(inner)
        dc = len(t)
        for i, ch in enumerate(t):
            path, k = C.dec_char_path(dc, i)
            sym[(path, k)].add(ch)
        if dc % 4:
            last[dc % 4].add(C.ALPHABET.index(t[-1:]))

    for L, layers, text, bits, o, dci, dco in _sweep(O):
        if o == 0:
            take(text if layers == 1 else O.java_b64url_decode(text))
    for L in C.ALPHA_LS:
        msgs = C.alphabet_messages(O, L)
        assert len(msgs) == C.ALPHA_MSGS
        for text, bits in msgs:
            assert C.ingest_expected(O, text, 1, 1, [L], 0)[0] == 0
            take(text)
    full = set(C.ALPHABET)
    for path in ("vector", "scalar"):
        for k in range(4):
            assert sym[(path, k)] == full, (path, k, len(sym[(path, k)]))
    assert sym[("tail", 0)] == full and sym[("tail", 1)] == full
    assert {v >> 4 for v in last[2]} == set(range(4)) and {v >> 2 for v in last[3]} == set(range(16))
    # discarded bits: same bytes, status 0, every non-zero value of the ignored bits at each layer
    seen = {}
    for text, bits, layers in C.discarded_bits_messages(O):
        st, got = C.ingest_expected(O, text, layers, 1, [bits.size], 0)
        assert st == 0 and (np.asarray(got[1]).view(np.uint64)[:bits.size] == bits).all()
        outer = C.strip(text)
        inner = outer if layers == 1 else C.strip(O.java_b64url_decode(text))
        clean_inner = C.strip(O.java_b64url_encode(C.frame_bytes(O, bits, 0, 0, 3, b"")))
        for name, t, clean in (("inner", inner, clean_inner), ("outer", outer, None)):
            if name == "outer" and layers == 1:
                continue
            if len(t) % 4 == 0:
                continue
            free = 4 if len(t) % 4 == 2 else 2
            k = C.ALPHABET.index(t[-1:]) & ((1 << free) - 1)
            if k:
                seen.setdefault((name, layers, len(t) % 4), set()).add(k)
    assert seen[("inner", 1, 2)] == seen[("inner", 2, 2)] == seen[("outer", 2, 2)] == set(range(1, 16))
    assert seen[("inner", 1, 3)] == seen[("inner", 2, 3)] == seen[("outer", 2, 3)] == {1, 2, 3}


def test_invalid_batches(O):
    """Every invalid byte value in every position class of both layers, one
    per message; the classes sit on the paths their names say; a valid
    message follows every third bad one; '=' is the only byte Java ever
    accepts there, and it does at the end of a text alone."""
    batches = C.invalid_batches(O)
    assert set(batches) == {(layer, c) for layer in ("outer", "inner") for c in C.invalid_class_names()}
    P, lens = 256, [C.INVALID_L] * 256
    accepted = 0
    for (layer, cname), msgs in batches.items():
        assert len(msgs) == 192 + 64
        bad = [m for m in msgs if m[2] is not None]
        assert [m[2][0] for m in bad] == list(C.INVALID_BYTES)
        for i, (text, bits, info) in enumerate(msgs):
            st, got = C.ingest_expected(O, text, 2, P, lens, i)
            if info is None:
                assert i % 4 == 3 and st == 0
                assert (np.asarray(got[1]).view(np.uint64) == bits).all()
                continue
            byte, o, dc, pos = info
            if st == 0:
                accepted += 1
                assert byte == ord("=") and pos >= dc - 2, (layer, cname, pos, dc)
            else:
                assert st == -6
            if pos < dc:
                path, _ = C.dec_char_path(dc, pos)
                want = {"vector-first": "vector", "vector-last": "vector", "scalar": "scalar", "tail-0": "tail",
                        "tail-1": "tail", "tail-2": "tail"}.get(cname)
                assert want is None or path == want, (layer, cname, o, pos, dc)
                if cname == "vector-first":
                    assert pos % C.DEC_LANE_CHARS == 0
                if cname == "vector-last":
                    assert pos % C.DEC_LANE_CHARS == C.DEC_LANE_CHARS - 1
        # the tail classes see tails of both kinds of lane: one with whole units before it, one without
        if cname.startswith("tail") and layer == "inner":      # (the outer text's tail is read by the host as well)
            assert {m[2][2] // 4 % 4 == 0 for m in bad} == {True, False}, (layer, cname)
    assert accepted >= 1


def test_decoder_variants_differ(O):
    """A tail done by no lane, or taken from the wrong unit, changes a payload
    byte of a sweep case and a status of the invalid-byte list; every widened
    range test changes a status."""
    hit = {v: 0 for v in C.DEC_VARIANTS}
    for L, layers, text, bits, o, dci, dco in _sweep(O):
        if layers != 1:
            continue
        frame = O.java_b64url_decode(text)
        seen = 14 + 8 * L                       # what the fold consumes: the payload (the header is read by the host too)
        for v in ("tail-no-lane", "tail-wrong-unit"):
            got, known = C.model_decode_bytes(frame, dci, v)
            hit[v] += bool((~known[:seen]).any() or got[:seen] != frame[:seen])
        got, known = C.model_decode_bytes(frame, dci)
        assert got == frame and known.all()
    assert hit["tail-no-lane"] and hit["tail-wrong-unit"]
    status_hit = {v: 0 for v in C.DEC_VARIANTS}
    lens = [C.INVALID_L] * 256
    for (layer, cname), msgs in C.invalid_batches(O).items():
        for i, (text, bits, info) in enumerate(msgs):
            if info is None:
                continue
            byte, o, dc, pos = info
            right = C.ingest_expected(O, text, 2, 256, lens, i)[0]
            assert C.model_status(right, 2, layer, byte, dc, pos) == right
            for v in C.DEC_VARIANTS:
                status_hit[v] += C.model_status(right, 2, layer, byte, dc, pos, v) != right
    for v, k in status_hit.items():
        assert k, f"variant {v} changes no status"
    for v in C.WIDENED:
        assert status_hit[v] >= 20 - 2          # once per layer and class (bar a position that a text lacks)
    assert sorted(C.WIDENED.values()) == sorted(ord(c) for c in "@[`{/:,.^`")
