"""Inputs and expectations shared by the peer-list tests (test_gpu_seg_peers.py
on the GPU, test_seg_peers_cases.py on the CPU): K lists over one layout of
seg_cases.py, folded by one call in peer order, with or without the one shared
minuend list (the received model).  Every peer's views sit at their own
residues in their own backing arrays with junk around them; the twins' edge
patterns stand at the segment ends, tile seams and partition boundaries of
every list, and beside every seam stand TRIPLES across three consecutive peers
for which the order of the additions changes the bits of the double sum.

The expectation is the twins' alone, applied K times in order:
seg_cases.expected_update of peer k's list, or seg_diff_cases.expected_update
of (received, peer k's list).

The triples.  From a +0.0 accumulator ((2^53 + 1) - 2^53) is 0.0 while the
reverse order gives 1.0; 2^53 and 1 are exact in f64, f32 and bf16.  Summing the
three first and adding once shows only over a non-zero accumulator (0 + x is x):
start_acc() puts 0.75 under these triples, which the sum in order rounds away
and the sum made first keeps.  A half holds nothing above 65504 and nothing
below 2^-24, so three halves sum exactly in a double whatever the order: there
the sensitivity needs the accumulator, and start_acc() puts 2^67 (one ulp =
2^15) under the half triple (2^14, 2^15, 3 * 2^14): half an ulp (a tie, to
even), one ulp, one and a half; every reordering and the sum made first end
elsewhere.  With a minuend the triple value v is
planted as (+0.0) - (-v), exact in every format.
"""
import numpy as np

import seg_cases as S
import seg_diff_cases as D

FMTS = S.FMTS
P = S.P
LAYOUTS = S.LAYOUTS
KS = (1, 2, 3, 5, 9, 17)          # a peer on both sides of every group seam for any group of 2, 4, 8 or 16
GROUPS = (2, 4, 8, 16)
BIG = 2.0 ** 53
TRIPLE = {"f64": (BIG, 1.0, -BIG), "f32": (BIG, 1.0, -BIG), "bf16": (BIG, 1.0, -BIG),
          "half": (2.0 ** 14, 2.0 ** 15, 3 * 2.0 ** 14)}
TRIPLE_START = {"f64": 0.75, "f32": 0.75, "bf16": 0.75, "half": 2.0 ** 67}
MISTAKES = 9


def peer_spec(spec, k):
    """Peer k's residues: the layout's own moved by an amount that differs from
    peer to peer and from segment to segment (peer 0 keeps the layout's)."""
    return [(fmt, n, (r + k * (1 + i % 2)) % S.residues(fmt)) for i, (fmt, n, r) in enumerate(spec)]


def triple_positions(spec, c, T):
    """Flat positions beside every tile seam and partition boundary that hold
    no edge pattern, sorted: position number i carries a triple over peers
    j, j + 1, j + 2 with j = i mod (K - 2)."""
    M = S.model_size(c)
    n = sum(s[1] for s in spec)
    plant = S.plant_positions(spec, c, T, M)
    out = set()
    for b in S.boundaries(c, T, M):
        out.update(f for f in (b + 1, b - 2, b + 4, b - 4) if 0 <= f < n and f not in plant)
    return sorted(out)


def _locate(st, f):
    """(segment, element) of flat position f."""
    i = int(np.searchsorted(st, f, side="right")) - 1
    return i, int(f - st[i])


def build(rng, name, c, T, K, with_received):
    """(received Segs or None, [peer 0's Segs, .., peer K-1's]): normals, the
    twins' planted values, the triples, junk around every view."""
    spec = S.shape(name, c, T)
    M = S.model_size(c)
    st = np.concatenate([[0], np.cumsum([s[1] for s in spec])]).astype(np.int64)

    def backing(fmt, n, r):
        x = rng.standard_normal(r + n + S.PAD)
        return x.view(np.uint64).copy() if fmt == "f64" else S.F.from_f32(x.astype(np.float32), fmt)

    rec = [S.Seg(f, n, r, backing(f, n, r)) for f, n, r in D.shape_b(name, spec)] if with_received else None
    peers = [[S.Seg(f, n, r, backing(f, n, r)) for f, n, r in peer_spec(spec, k)] for k in range(K)]
    for kk, f in enumerate(sorted(S.plant_positions(spec, c, T, M))):
        if f >= st[-1]:
            continue
        i, e = _locate(st, f)
        fmt = spec[i][0]
        if with_received:
            pr = D.pairs(fmt)
            rec[i].backing[rec[i].r + e] = pr[D.PAIR_KINDS[kk % len(D.PAIR_KINDS)]][0]
            for k in range(K):
                peers[k][i].backing[peers[k][i].r + e] = pr[D.PAIR_KINDS[(kk + k) % len(D.PAIR_KINDS)]][1]
        else:
            eb = S.edge_bits(fmt)
            for k in range(K):
                peers[k][i].backing[peers[k][i].r + e] = eb[(kk + k) % eb.size]
    for t, f in enumerate(triple_positions(spec, c, T)):
        i, e = _locate(st, f)
        fmt = spec[i][0]
        j = t % (K - 2) if K >= 3 else None
        sign = -1.0 if with_received else 1.0
        if with_received:
            rec[i].backing[rec[i].r + e] = D.enc([0.0], fmt)[0]
        for k in range(K):
            v = TRIPLE[fmt][k - j] if j is not None and j <= k < j + 3 else 0.0
            peers[k][i].backing[peers[k][i].r + e] = D.enc([sign * v if v else 0.0], fmt)[0]
    return rec, peers


def start_acc(rng, O, name, c, T):
    """Non-zero accumulators: normals, and under every triple the start its format needs."""
    spec = S.shape(name, c, T)
    M = S.model_size(c)
    st = np.concatenate([[0], np.cumsum([s[1] for s in spec])]).astype(np.int64)
    acc = [rng.standard_normal(O.partition_len(M, P, p)) for p in range(P)]
    for f in triple_positions(spec, c, T):
        i, _ = _locate(st, f)
        acc[f // c][f % c] = TRIPLE_START[spec[i][0]]
    return acc


def peer_vector(rec, segs):
    """Peer's flat vector, widened: its list, or received minus its list."""
    return S.concat(segs if rec is None else D.difference(rec, segs))


def expected(O, acc, rec, peers, c, owned):
    """The twins' expectation applied once per peer, in peer order."""
    owned = list(owned)
    for segs in peers:
        acc = S.expected_update(O, acc, segs, c, owned) if rec is None else D.expected_update(O, acc, rec, segs, c, owned)
    return acc


# ---- coverage ----
def coverage(name, c, T, K):
    """({(fmt, peers at residue 0 and peers not?)} of the whole tiles, {segments a partial tile spans})."""
    spec = S.shape(name, c, T)
    specs = [peer_spec(spec, k) for k in range(K)]
    segs = [S.Seg(f, n, r) for f, n, r in spec]
    n = sum(s[1] for s in spec)
    whole, spans = set(), set()
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, n) - p * c)
        for lo in range(0, ncopy, T):
            hi = min(lo + T, ncopy)
            pcs = S.pieces_of(segs, p * c + lo, p * c + hi)
            if len(pcs) == 1 and hi - lo == T:
                i, e, _ = pcs[0]
                fmt = spec[i][0]
                al = {(specs[k][i][2] + e) % S.residues(fmt) == 0 for k in range(K)}
                whole.add((fmt, len(al) == 2))
            else:
                spans.add(len(pcs))
    return whole, spans


def check_coverage(T):
    """Whole tiles of every format whose peers lie at differing residues (some
    aligned, some not), partial tiles over two and over three segments, and
    triples beside the seams of every chunk (asserted)."""
    whole, spans = set(), set()
    for c in S.chunks(T):
        for name in LAYOUTS:
            w, s = coverage(name, c, T, max(KS))
            whole |= w
            spans |= s
            assert len(triple_positions(S.shape(name, c, T), c, T)) >= (0 if name == "tiny" else 8), (name, c)
    for fmt in FMTS:
        assert (fmt, True) in whole, f"no whole {fmt} tile with aligned and unaligned peers"
    assert 2 in spans and 3 in spans, spans
    return whole, spans


# ---- the mistakes, each as the accumulators a kernel making it would leave ----
def fold_vec(acc, vec, c, owned, count=1.0):
    """numpy's model of one fold of a flat vector: values, `count` at the count slot, +0.0 above it."""
    out = [a.copy() for a in acc]
    with np.errstate(over="ignore", invalid="ignore"):
        for p in owned:
            v = vec[p * c:(p + 1) * c]
            out[p][:v.size] += v
            out[p][v.size] += count
            out[p][v.size + 1:] += 0.0
    return out


def fold_peers(acc, vecs, c, owned, counts=None):
    for k, v in enumerate(vecs):
        acc = fold_vec(acc, v, c, owned, 1.0 if counts is None else counts[k])
    return acc


def first_pieces(segs, c, T):
    """Flat [lo, hi) of the first piece of every tile."""
    n = S.total(segs)
    st = S.starts(segs)
    out = []
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, n) - p * c)
        for lo in range(0, ncopy, T):
            pcs = S.pieces_of(segs, p * c + lo, p * c + min(lo + T, ncopy))
            i, e, k = pcs[0]
            out.append((int(st[i]) + e, int(st[i]) + e + k))
    return out


def mistakes(acc, rec, peers, c, T, owned, zero_start):
    """{mistake: accumulators}; only the mistakes whose premise the case has."""
    owned = list(owned)
    K = len(peers)
    vecs = [peer_vector(rec, segs) for segs in peers]
    uniq = list(dict.fromkeys(owned))
    out = {}
    if K >= 2:
        out["1 peers folded in reverse order"] = fold_peers(acc, vecs[::-1], c, owned)
        with np.errstate(over="ignore", invalid="ignore"):
            total = vecs[0].copy()
            for v in vecs[1:]:
                total = total + v
        if len(uniq) == len(owned):
            out["2 peers summed first, one add"] = fold_vec(acc, total, c, owned, float(K))
        out["3 count slot added once"] = fold_peers(acc, vecs, c, owned, [1.0] + [0.0] * (K - 1))
        if zero_start:
            out["4 zero flag applied at every peer"] = fold_vec([np.zeros_like(a) for a in acc], vecs[-1], c, uniq)
        shifted = []
        for k in range(K):
            v = vecs[k].copy()
            if k:
                for lo, hi in first_pieces(peers[0], c, T):
                    v[lo:hi] = vecs[k - 1][lo:hi]
            shifted.append(v)
        out["5 peer k's first piece of a tile from peer k-1"] = fold_peers(acc, shifted, c, owned)
        at0 = [[S.Seg(s.fmt, s.n, s0.r, s.backing) for s, s0 in zip(segs, peers[0])] for segs in peers]
        if any(s.r != s0.r and s.n for segs in peers for s, s0 in zip(segs, peers[0])):
            out["6 every peer read at peer 0's residue"] = fold_peers(acc, [peer_vector(rec, a) for a in at0], c, owned)
        if rec is not None and len(uniq) == len(owned):
            with np.errstate(over="ignore", invalid="ignore"):
                tsum = S.concat(peers[0])
                for segs in peers[1:]:
                    tsum = tsum + S.concat(segs)
                out["7 minuend subtracted after the sum"] = fold_vec(acc, K * S.concat(rec) - tsum, c, owned, float(K))
        if len(uniq) < len(owned):
            again = acc
            for t in range(max(owned.count(q) for q in uniq)):
                again = fold_peers(again, vecs, c, [q for q in uniq if owned.count(q) > t])
            out["8 repeats as all peers, then all peers again"] = again
        for G in GROUPS:
            if K > G:
                sw = list(vecs)
                sw[G - 1], sw[G] = sw[G], sw[G - 1]
                out[f"9 peers {G - 1} and {G} exchanged"] = fold_peers(acc, sw, c, owned)
    return out
