"""Inputs and expectations shared by the many-trainers-round tests
(test_gpu_seg_round.py on the GPU, test_seg_round_cases.py on the CPU): K
lists over one layout of seg_cases.py folded over the accumulators, W = that +
REP, and W divided into n_lists output lists -- the trainers' own arrays and
the received model (in place), or lists of their own in SENTINEL-filled backing
arrays -- by ONE call (ipls_agg_round_segs_peers; k_round_segs_peers).

Only the layouts whose n equals the model size serve (both twins' bounds
together leave nothing else); a `short` layout serves the refusal.  The peers'
values are seg_peers_cases.build's: the twins' edge patterns and difference
pairs at every segment end, tile seam and partition seam, and the order
triples beside them.  On top of them stand, at every third of those positions,
  QUOTIENTS  seg_copies_cases.PLANTED (the f32 tie, the two-step patterns for
             bf16 and half, 70000, 2^-140, a NaN, -0.0) as q * cnt in W of a
             partition that is not owned, and in AGG (all peers giving +0.0
             there) of an owned one whose AGG is planted, cnt its final count;
  NEGZERO    a sum that is exactly -0.0 (AGG -0.0, every peer's value -0.0)
             going into the finalize: with REP logically zero W and every
             output are +0.0.
The count slots are small integers, so every q * cnt is exact in double.

The expectation is the oracle's alone, from the inputs as they were before
the call: seg_peers_cases.expected, the oracle's aggregate_partition of every
owned partition, seg_copies_cases.expected.

model() is a numpy model of the state the call leaves (W, the lists' memory);
with a `mistake` it is what a kernel making that mistake would leave.
"""
from dataclasses import dataclass, field

import numpy as np

import seg_cases as S
import seg_copies_cases as SC
import seg_diff_cases as D
import seg_peers_cases as C

FMTS = S.FMTS
P = S.P
KS = (1, 2, 3, 5)                  # a peer on both sides of a G = 2 seam, and an odd tail
OWNED = {"all": list(range(P)), "subset": [1, 3, 6, 8], "twice": [0, 2, 5, 2, 7], "none": []}
STARTS = ("zero", "agg", "rep", "both")
REP_ON = (0, 3, 5, 6)              # the partitions whose REP is planted (starts "rep" and "both")
MISTAKES = ("1 divided by the count before REP is added", "2a the count with 1.0 added once",
            "2b the count with K additions, not K * mult", "3 W's stale count slot read instead of computed",
            "4 REP added before the peers", "5 the REP-zero form skips the + 0.0", "6 a not-owned partition folded",
            "7 an owned partition's AGG flag left non-zero", "8 the count slot written into a list",
            "9 list k at list 0's residue", "10 received overwritten before peer k >= 1 is read")


# Mistake 8 is "the count slot or the tail written into a list".  In every case this call accepts there is no tail:
# n equals the model size, so every partition has ncopy == L - 1 and its count slot is its last element (the engine
# refuses anything else; no_tail() asserts it of the cases).  The count slot written one element on is therefore the
# whole of that mistake; where it falls behind the last segment it lands in the guard bytes, which image() keeps.


def no_tail(O, case):
    """Every partition's values are its whole body: the count slot stands at ncopy == L - 1, nothing above it."""
    M, c = case.M, case.c
    return all(O.partition_len(M, P, p) - 1 == max(0, min((p + 1) * c, M) - p * c) for p in range(P))


def layouts(c, T=S.TILE_DEFAULT):
    """The layouts that hold exactly the model."""
    M = S.model_size(c)
    return tuple(name for name in S.LAYOUTS if sum(s[1] for s in S.shape(name, c, T)) == M)


def n_lists_of(K):
    return (1, K + 1, 3)


@dataclass
class Case:
    name: str
    c: int
    T: int
    K: int
    owned: list
    start: str
    secure: bool
    rec: list            # Segs of the received model, or None
    peers: list          # [Segs per peer]
    agg0: list           # per partition, or None: logically zero
    rep0: list           # per partition an array, or None: logically zero
    w0: list             # W before the call
    out_specs: list      # per output list [(fmt, n, r)]; None: in place ([received] + peers)
    planted: dict = field(default_factory=dict)   # flat position -> what stands there

    @property
    def M(self):
        return S.model_size(self.c)

    @property
    def spec(self):
        return S.shape(self.name, self.c, self.T)

    @property
    def in_place(self):
        return self.out_specs is None

    def inputs(self):
        return ([self.rec] if self.rec is not None else []) + list(self.peers)

    def list_specs(self):
        if self.in_place:
            return [[(s.fmt, s.n, s.r) for s in segs] for segs in self.inputs()]
        return self.out_specs

    def mult(self):
        return {p: self.owned.count(p) for p in dict.fromkeys(self.owned)}


def final_count(case, p):
    """An owned partition's count: small integers, exact."""
    a = 0.0 if case.agg0 is None else float(case.agg0[p][-1])
    r = 0.0 if case.rep0[p] is None else float(case.rep0[p][-1])
    return a + float(case.K * case.owned.count(p)) + r


def build(O, seed, name, c, T, K, owned, start, with_received, secure=False, n_lists=None):
    """n_lists None: in place."""
    rng = np.random.default_rng(seed)
    spec = S.shape(name, c, T)
    M = S.model_size(c)
    assert sum(s[1] for s in spec) == M, name
    owned = list(owned)
    rec, peers = C.build(rng, name, c, T, K, with_received)
    st = np.concatenate([[0], np.cumsum([s[1] for s in spec])]).astype(np.int64)
    lens = [O.partition_len(M, P, p) for p in range(P)]
    agg0 = None
    if start in ("agg", "both"):
        agg0 = C.start_acc(rng, O, name, c, T)
        for p in range(P):
            agg0[p][-1] = float(1 + p % 3)
    rep0 = [None] * P
    if start in ("rep", "both"):
        for p in REP_ON:
            rep0[p] = rng.standard_normal(lens[p])
            rep0[p][-1] = float(p % 4)
    w0, _ = SC.weights(rng, O, name, c, T) if name in SC.layouts(c) else (S.weights(rng, O, c), None)
    case = Case(name, c, T, K, owned, start, secure, rec, peers, agg0, rep0, w0,
                None if n_lists is None else [C.peer_spec(spec, k) for k in range(n_lists)])

    def put_all(f, rec_v, peer_v):
        i, e = C._locate(st, f)
        fmt = spec[i][0]
        if rec is not None:
            rec[i].backing[rec[i].r + e] = D.enc([rec_v], fmt)[0]
        for k in range(K):
            peers[k][i].backing[peers[k][i].r + e] = D.enc([peer_v], fmt)[0]

    names = list(SC.PLANTED)
    for t, f in enumerate(sorted(x for x in S.plant_positions(spec, c, T, M) if 0 <= x < M)):
        p, j = f // c, f % c
        if t % 3 == 0:
            q = names[(t // 3) % len(names)]
            if p not in owned:
                cnt = w0[p][-1]
                w0[p][j] = SC.PLANTED[q] if cnt == 0.0 else SC.PLANTED[q] * cnt
                case.planted[f] = q
            elif agg0 is not None:
                put_all(f, 0.0, 0.0)                       # every peer gives +0.0 here
                agg0[p][j] = SC.PLANTED[q] * final_count(case, p)
                if rep0[p] is not None:
                    rep0[p][j] = 0.0
                case.planted[f] = q
        elif t % 3 == 1 and p in owned and agg0 is not None:
            # -0.0 - (+0.0) = -0.0 with a received model, -0.0 itself without
            put_all(f, -0.0, 0.0 if rec is not None else -0.0)
            agg0[p][j] = -0.0
            if rep0[p] is not None:
                rep0[p][j] = -0.0
            case.planted[f] = "negzero sum"
    # the witness of REP's place in the order: every peer gives 1.0 under a REP of 2^53.  Added last, REP sees the
    # whole sum K * mult; added first, every 1.0 after it is half an ulp and rounds away (to even)
    for p in REP_ON:
        if rep0[p] is not None and p in owned and lens[p] > 2:
            put_all(p * c + 1, 1.0, 0.0 if rec is not None else 1.0)
            rep0[p][1] = C.BIG
            if agg0 is not None:
                agg0[p][1] = 0.0
            case.planted[p * c + 1] = "rep order"
    return case


# ---- the expectation: the oracle alone ----
def expected(O, case):
    """(W per partition, the bit patterns per segment that every list holds)."""
    acc0 = case.agg0 if case.agg0 is not None else S.U.zeros(O, case.M, P)
    acc = C.expected(O, acc0, case.rec, case.peers, case.c, case.owned)
    W = [w.copy() for w in case.w0]
    for p in sorted(set(case.owned)):
        rep = case.rep0[p] if case.rep0[p] is not None else np.zeros(acc[p].size)
        w, wa = np.empty(acc[p].size), np.empty(acc[p].size)
        with np.errstate(over="ignore", invalid="ignore"):
            O.aggregate_partition(acc[p].copy(), rep.copy(), w, wa)
        W[p] = w
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return W, SC.expected(O, W, case.spec, case.M, case.secure)


def blank(case):
    """The lists' memory before the call: [[backing bytes per segment] per list]."""
    if case.in_place:
        return [[np.ascontiguousarray(s.backing).view(np.uint8).copy() for s in segs] for segs in case.inputs()]
    return SC.blank(case.out_specs)


def image(case, bits, mem=None, at_residue_of=None):
    """mem with the segments' bits written at every list's views."""
    mem = blank(case) if mem is None else mem
    for k, sp in enumerate(case.list_specs()):
        for i, (fmt, n, r) in enumerate(sp):
            if at_residue_of is not None:
                r = case.list_specs()[at_residue_of][i][2]
            raw = np.ascontiguousarray(bits[i]).view(np.uint8)
            a = r * S.esize(fmt)
            m = max(0, min(raw.size, mem[k][i].size - a))
            mem[k][i][a:a + m] = raw[:m]
    return mem


def expected_image(O, case):
    W, bits = expected(O, case)
    return W, image(case, bits)


# ---- the numpy model, and the mistakes ----
def _fold(case, rec, peers, agg_start, mult, rep_first=False):
    vecs = [C.peer_vector(rec, segs) for segs in peers]
    out = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for p, m in mult.items():
            L = case.w0[p].size
            a = np.zeros(L) if agg_start is None else agg_start[p].copy()
            if rep_first and case.rep0[p] is not None:
                a = a + case.rep0[p]
            v1 = np.zeros(L)
            for v in vecs:
                v1[:L - 1] = v[p * case.c:p * case.c + L - 1]
                v1[L - 1] = 1.0
                for _ in range(m):
                    a = a + v1
            out[p] = a
    return out


def model(case, mistake=None, rec=None, agg_start="own"):
    """(W, the lists' memory) by numpy; None when the mistake's premise is not in the case."""
    K, c, M = case.K, case.c, case.M
    mult = case.mult()
    rec = case.rec if rec is None else rec
    agg_start = case.agg0 if isinstance(agg_start, str) else agg_start
    owned_rep = [p for p in mult if case.rep0[p] is not None]
    if mistake == MISTAKES[0] and not any(case.rep0[p][-1] != 0.0 for p in owned_rep):
        return None
    if mistake == MISTAKES[1] and not any(K * m > 1 for m in mult.values()):
        return None
    if mistake == MISTAKES[2] and not any(m > 1 for m in mult.values()):
        return None
    if mistake in (MISTAKES[3], MISTAKES[8]) and not mult:
        return None
    if mistake == MISTAKES[4] and not any(K * mult[p] >= 2 for p in owned_rep):
        return None       # one addition onto +0.0 commutes with REP's
    if mistake == MISTAKES[5] and not any(q == "negzero sum" and case.rep0[f // c] is None
                                          for f, q in case.planted.items()):
        return None
    if mistake == MISTAKES[6]:
        if len(mult) == P:
            return None
        mult = {p: mult.get(p, 1) for p in range(P)}
    if mistake == MISTAKES[9] and (case.in_place or len(case.out_specs) < 2):
        return None
    if mistake == MISTAKES[10] and not (case.in_place and case.rec is not None and K >= 2):
        return None
    sums = _fold(case, rec, case.peers, agg_start, mult, rep_first=mistake == MISTAKES[4])
    W = [w.copy() for w in case.w0]
    den = [w[-1] for w in W]
    with np.errstate(over="ignore", invalid="ignore"):
        for p, a in sums.items():
            rep = case.rep0[p]
            if mistake == MISTAKES[4]:
                W[p] = a
            elif rep is None:
                W[p] = a if mistake == MISTAKES[5] else a + 0.0
            else:
                W[p] = a + rep
            den[p] = W[p][-1]
            start = 0.0 if agg_start is None else agg_start[p][-1]
            r = 0.0 if rep is None else rep[-1]
            if mistake == MISTAKES[0]:
                den[p] = a[-1]
            elif mistake == MISTAKES[1]:
                den[p] = (start + 1.0) + r
            elif mistake == MISTAKES[2]:
                den[p] = (start + float(K)) + r
            elif mistake == MISTAKES[3]:
                den[p] = case.w0[p][-1]
    parts = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for p in range(P):
            d = 1e12 * den[p] if case.secure else den[p]
            parts.append(W[p][:-1] if den[p] == 0.0 else W[p][:-1] / d)
    flat = np.concatenate(parts)[:M]
    bits = S.expected_outputs(flat, case.spec, M)
    if mistake == MISTAKES[9]:
        return W, image(case, bits, at_residue_of=0)
    mem = image(case, bits)
    if mistake == MISTAKES[8]:
        # the count slot's quotient lands on the element after the partition's last: the next partition's first
        # value, or the guard bytes behind the last segment
        st = np.concatenate([[0], np.cumsum([s[1] for s in case.spec])]).astype(np.int64)
        live = [i for i, s in enumerate(case.spec) if s[1]]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for p in mult:
                f = p * c + W[p].size - 1
                i = live[-1] if f >= M else C._locate(st, f)[0]
                y = W[p][-1] if den[p] == 0.0 else W[p][-1] / (1e12 * den[p] if case.secure else den[p])
                for k, sp in enumerate(case.list_specs()):
                    fmt, n, r = sp[i]
                    raw = S.narrow(np.array([y]), fmt).view(np.uint8)
                    a = (r + f - int(st[i])) * S.esize(fmt)
                    mem[k][i][a:a + raw.size] = raw
    return W, mem


def overwritten_received(O, case):
    """Mistake 10: list 0 (the received model) holds the new model before peers 1 .. K-1 are read."""
    if not (case.in_place and case.rec is not None and case.K >= 2):
        return None
    _, bits = expected(O, case)
    new_rec = [S.Seg(s.fmt, s.n, s.r, s.backing.copy()) for s in case.rec]
    for s, b in zip(new_rec, bits):
        s.backing[s.r:s.r + s.n] = b
    vecs = [C.peer_vector(case.rec, case.peers[0])] + [C.peer_vector(new_rec, t) for t in case.peers[1:]]
    plain = [[S.Seg("f64", v.size, 0, v.view(np.uint64))] for v in vecs]
    twin = Case(case.name, case.c, case.T, case.K, case.owned, case.start, case.secure, None, plain, case.agg0,
                case.rep0, case.w0, None)
    W, _ = model(twin)
    return W


def second_round(O, case, stale_flag=False):
    """The W of a second round on the same handle, `received` and every trainer holding the first round's output:
    every update is x - x.  With the AGG flag left non-zero the second fold starts from the stale AGG."""
    _, bits = expected(O, case)
    segs = [S.Seg(s.fmt, s.n, 0, b) for s, b in zip(case.peers[0], bits)]
    nxt = Case(case.name, case.c, case.T, case.K, case.owned, "zero", case.secure, segs if case.rec is not None else None,
               [segs] * case.K, case.agg0 if stale_flag else None, [None] * P, expected(O, case)[0], None)
    return model(nxt)[0]


def same_w(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def same_w_nan(a, b):
    """Bit-equal, a NaN matching any NaN."""
    for x, y in zip(a, b):
        nan = np.isnan(x) & np.isnan(y)
        if not np.array_equal(x.view(np.uint64)[~nan], y.view(np.uint64)[~nan]):
            return False
    return True


# ---- coverage ----
def coverage(name, c, T, K, owned, n_lists):
    """Facts about what the blocks of one call see, from the shapes alone."""
    spec = S.shape(name, c, T)
    segs = [S.Seg(f, n, r) for f, n, r in spec]
    M = S.model_size(c)
    specs = [C.peer_spec(spec, k) for k in range(n_lists)]
    st = S.starts(segs)
    cov = dict(whole=set(), partial=set(), owned_tiles=set(), out_al=set(), seam_in_seg=False)
    for i, (fmt, n, r) in enumerate(spec):
        if any(st[i] < p * c < st[i + 1] for p in range(1, P)):
            cov["seam_in_seg"] = True
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, M) - p * c)
        for lo in range(0, ncopy + 1, T):
            hi = min(lo + T, ncopy)
            pcs = S.pieces_of(segs, p * c + lo, p * c + hi)
            whole = len(pcs) == 1 and hi - lo == T
            cov["owned_tiles"].add((p in owned, whole))
            for i, e, _ in pcs:
                fmt = spec[i][0]
                (cov["whole"] if whole else cov["partial"]).add(fmt)
                if whole:
                    for k in range(n_lists):
                        cov["out_al"].add((fmt, ((specs[k][i][2] + e) * S.esize(fmt)) % 16 == 0))
    return cov


def check_coverage(T):
    """Whole and partial tiles of every format, owned and not-owned tiles of both kinds, a partition seam inside a
    segment, and whole tiles stored to 16-B aligned and to misaligned lists in every format (asserted)."""
    tot = dict(whole=set(), partial=set(), owned_tiles=set(), out_al=set(), seam_in_seg=False)
    for c in S.chunks(T):
        assert layouts(c, T), c
        for name in layouts(c, T):
            cov = coverage(name, c, T, max(KS), OWNED["subset"], max(KS) + 1)
            for k, v in cov.items():
                tot[k] = (tot[k] or v) if isinstance(v, bool) else (tot[k] | v)
    assert tot["whole"] == set(FMTS) and tot["partial"] == set(FMTS), tot
    assert tot["owned_tiles"] == {(a, b) for a in (False, True) for b in (False, True)}, tot
    assert tot["out_al"] == {(f, a) for f in FMTS for a in (False, True)}, tot
    assert tot["seam_in_seg"]
    return tot
