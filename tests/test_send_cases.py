"""The cases of tests/test_gpu_send.py reach what they claim (CPU, numpy and the oracle only).

The lane rule that tests/send_cases.py restates is the header's; the case
list has the flat-offset residues, frame lengths, count-slot positions, short
gradients and tiny partitions it is meant to have; every source carries the
planted values; the model's right text is the oracle's; and every wrong
kernel of the model changes a compared char in at least one case.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import codec_cases as C
import send_cases as S

HPP = Path(__file__).resolve().parent.parent / "ipls-java-api_amd" / "csrc" / "ipls_kernels.hpp"


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def cases():
    return S.all_cases()


def widened(case, fmt):
    return S.widen_bits(S.source_bits(case, fmt), fmt)


def test_lane_rule_matches_the_header():
    src = HPP.read_text()
    k = src[src.index("void k_b64url_encode_flat("):]
    assert re.search(r"g < groups && g >= 1 && 3 \* g \+ 2 <= ncopy\)", k)
    assert re.search(r"const T\* s = src \+ \(3 \* g - 2\);", k)
    assert re.search(r"const int64_t b = (\d+) \* g \+ 3 \* u;", k).group(1) == str(S.GROUP)
    assert re.search(r"i < ncopy \? flat_value_bits<S, BE_IN>\(src \+ i\) : i == ncopy \? 0x3FF0000000000000ull : 0ull", k)
    assert "window_chars(v0, v1, v2, v3, tab, c0, c1);" in k and "store_wave_text(ws, lane, c0, c1, j.out, gw, j.text_len);" in k
    # a lane's window: frame bytes [24g, 24g + 24) lie in payload values 3g - 2 .. 3g + 1
    for g in (1, 2, 63, 255):
        assert (S.GROUP * g - 14) // 8 == 3 * g - 2 and (S.GROUP * g + S.GROUP - 1 - 14) // 8 == 3 * g + 1
    assert S.lane_fast(1, 5) and not S.lane_fast(1, 4) and not S.lane_fast(0, 100)


def test_names_are_unique(cases):
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert all(0 <= p < c.P for p in c.parts) and c.lengths == S.lengths(c.M, c.P) and min(c.lengths) >= 1
        assert max(C.text_len(c.frame_len(p)) for p in c.parts) <= 16448      # the largest text is about 16 KiB


def test_residues():
    (c,) = S.residue_cases()
    assert c.P == 8 and c.chunk % 8 == 1 and c.parts == tuple(range(8))
    assert {c.lo(p) % 8 for p in c.parts} == set(range(8))
    for fmt in S.FMTS:                       # every 16-B residue an element of the format can have
        e = S.ESIZE[fmt]
        assert {c.lo(p) * e % 16 for p in c.parts} == set(range(0, 16, e))
    assert all(len(c.fast(p)) >= 20 for p in c.parts)


def test_edges():
    edges = S.edge_cases()
    got = {}
    for c in edges:
        p = c.parts[0]
        got.setdefault(c.frame_len(p), set()).add(c.o)
    assert S.ENC_CENTRES == (24, 48, 768, 1536, 2304, 6144, 12288)
    for centre in S.ENC_CENTRES:
        # every centre is 2 mod 8 past the 14 header bytes: origins 0, 1, 2 give c - 2, c - 1, c; 3, 4, 5 give
        # c + 1 .. c + 3; 46 (6 mod 8) gives c - 4 and c + 4 where a payload fits; c - 3 would need 7 mod 8
        assert [got.get(centre + d) for d in range(-2, 4)] == [{0}, {1}, {2}, {3}, {4}, {5}], centre
        assert centre - 3 not in got
        if centre >= 768:
            assert got[centre - 4] == {46} == got[centre + 4]
    assert {c.o for c in edges} == set(S.EDGE_ORIGINS + S.EDGE_ORIGINS_ABOVE)
    # whole partitions: the count slot is the last double, no zero tail, and the other partition rides along
    assert all(c.ncopy(c.parts[0]) == c.lengths[c.parts[0]] - 1 and len(c.parts) == 2 for c in edges)
    assert max(len(c.fast(c.parts[0])) for c in edges) > S.BLOCK + 2 * S.WAVE_GROUPS   # fast lanes in the second block


def test_count_slot_positions():
    cs = S.count_slot_cases()
    seen = set()
    for c in cs:
        p = c.parts[0]
        nc = c.ncopy(p)
        assert p == 1 and c.lo(p) == 800 and 0 < nc < c.lengths[p] - 1
        g = next(g for g in S.COUNT_LANES if 3 * g - 2 <= nc <= 3 * g + 1)
        assert not S.lane_fast(g, nc)                           # the window that holds ncopy is slow ...
        assert g == 1 or S.lane_fast(g - 1, nc) == (nc >= 3 * g - 1)   # ... and the lane before it fast once its four lie below
        seen.add((g, nc - (3 * g - 2), nc % 3))
        assert c.ncopy(0) == c.lengths[0] - 1                   # partition 0 is whole
    assert seen == {(g, k, (3 * g - 2 + k) % 3) for g in S.COUNT_LANES for k in range(4)}
    assert {m for _, _, m in seen} == {0, 1, 2}
    assert S.COUNT_LANES == (1, 63, 255)


def test_short_last_and_tiny():
    short = S.short_cases()[0]
    nc = {p: short.ncopy(p) for p in short.parts}
    assert nc[3] == 0 and 0 < nc[2] < short.lengths[2] - 1 and nc[0] == short.lengths[0] - 1
    assert (short.lengths[2] - 1 - nc[2]) // 3 >= 5               # a zero tail several lanes long
    assert short.n < short.M
    first = S.short_cases()[1]
    assert first.ncopy(0) == 7 and first.ncopy(1) == 0
    (last,) = S.last_cases()
    assert last.lengths[-1] < last.lengths[0] and last.parts[0] == last.P - 1 and last.n == last.M
    tiny = S.tiny_cases()
    assert [c.lengths[c.parts[0]] for c in tiny] == [1, 2, 3, 4, 5, 6]
    for c in tiny:
        for p in c.parts:
            assert c.lengths[p] <= 7
            assert c.fast(p) == ([] if c.lengths[p] <= 5 else [1])
    t = S.all_tiny_case()
    assert all(not t.fast(p) for p in t.parts)


def test_planted_values(cases):
    """Every special of every format lies among the copied values of some
    listed partition; -0.0 in a fast lane's values and in a slow lane's; the
    doubles carry a NaN with a payload; nothing else is a NaN or an infinity."""
    for fmt in S.FMTS:
        seen, neg_fast, neg_slow = set(), False, False
        for c in cases:
            bits = S.source_bits(c, fmt)
            assert bits.size == c.n + 2 * S.PAD and bits.dtype == S.BITS[fmt]
            for p in c.parts:
                nc, lo = c.ncopy(p), S.PAD + c.lo(p)
                vals = bits[lo:lo + nc]
                seen |= set(int(x) for x in vals) & set(S.SPECIALS[fmt])
                fast = c.fast(p)
                for i in np.flatnonzero(vals == S.SPECIALS[fmt][0]):
                    lanes = {(14 + 8 * int(i)) // S.GROUP, (14 + 8 * int(i) + 7) // S.GROUP}
                    neg_fast |= bool(lanes & set(fast))
                    neg_slow |= bool(lanes - set(fast))
        assert seen == set(S.SPECIALS[fmt]), fmt
        assert neg_fast and neg_slow, fmt
    assert 0x7FF80000DEADBEEF in S.SPECIALS["f64"] and S.SPECIALS["be"] is S.SPECIALS["f64"]
    assert S.widen_bits(np.array(S.SPECIALS["f32"], dtype=np.uint32), "f32")[0] == S.NEG_ZERO_F64
    assert S.widen_bits(np.array(S.SPECIALS["f16"], dtype=np.uint16), "f16")[2] == 0x3E70000000000000   # 2^-24
    assert S.widen_bits(np.array(S.SPECIALS["bf16"], dtype=np.uint16), "bf16")[3] == 0x47EFE00000000000


def test_model_is_the_oracle(O, cases):
    """The model's right text is the oracle's restatement over the numpy-widened source, for every case and format."""
    for c in cases:
        for fmt in S.FMTS:
            wide = widened(c, fmt)
            for p in c.parts:
                assert S.model_text(c, p, wide) == S.oracle_text(O, c, fmt, p), (c, fmt, p)
                assert len(S.model_text(c, p, wide)) == C.text_len(c.frame_len(p))
        for p in c.parts:
            fr = O.java_b64url_decode(S.null_text(c, p))
            assert O.frame_decode(fr) == (c.pid, 0, p, c.iteration, None, c.origin)


# where a wrong kernel can show: the header, the count slot and the zero tail are never in a fast lane
OBSERVABLE = {"count-missing": ("all", "slow"), "count-at-end": ("all", "slow"), "header-swapped": ("all", "slow"),
              "tail-from-neighbour": ("all", "slow"), "neg-zero-lost": S.LANES, "read-early": S.LANES,
              "read-late": S.LANES}


def test_wrong_kernels_are_told_apart(cases):
    assert set(OBSERVABLE) == set(S.VARIANTS)
    for fmt in S.FMTS:
        caught = {(v, ln): 0 for v in S.VARIANTS for ln in S.LANES}
        for c in cases:
            wide = widened(c, fmt)
            for p in c.parts:
                right = S.model_text(c, p, wide)
                for v in S.VARIANTS:
                    for ln in S.LANES:
                        caught[(v, ln)] += S.model_text(c, p, wide, v, ln) != right
        for v in S.VARIANTS:
            for ln in S.LANES:
                assert (caught[(v, ln)] > 0) == (ln in OBSERVABLE[v]), (fmt, v, ln, caught[(v, ln)])
