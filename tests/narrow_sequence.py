"""Plan and model of the stateful random sequence over the trainer-format
(f32 / half / bf16) and saved-model calls.  No GPU and no library import:
tests/test_narrow_sequence.py inspects the plans on the oracle alone,
tests/test_gpu_stateful_narrow.py replays them against the library.

``plan(seed, lengths, offsets, steps)`` draws every step from the seed up
front.  ``Model`` holds the Java state as numpy doubles per partition (agg,
rep, fut, w) and returns what each step must produce.  Per accumulator it keeps
the *physical* contents (``val``: what the arena would still hold) and the
"logically +0.0" flag apart, so that "would a stale read be visible here?" has
an answer (``Model.events``), and so that deliberately wrong variants of the
model (``bugs``: the flag mistakes an entry point can make) can be replayed.

Targets are named "agg", "rep", "fut", "w"; start modes "zero", "accum",
"first"; formats "f64", "be" (big-endian double bytes), "f32", "half", "bf16";
operand forms "dev" (a DeviceBuffer ``off`` elements past a 16-B boundary),
"host" (numpy / CPU torch) and "pinned".
"""
import numpy as np

import h16_ref as R
import narrow_fmt as F
from oracle import oracle as O

NARROW = F.FMTS
ACC = ("agg", "rep", "fut")
TARGETS = ("agg", "rep", "fut", "w")
START = {"zero": O.START_ZERO, "accum": O.START_ACCUM, "first": O.START_FIRST}
N_GENERAL = {"f64": 8, "f32": 10, "half": 10, "bf16": 10}
# order witnesses: f64[WPOS[e]], a narrow bucket of ones, f64[WNEG[e]] give +0.0
# in this order and 1.0 with the two doubles folded first (2^53 + 1 == 2^53;
# 2^60 where the issue names it for f32 and bf16)
WPOS = {"half": 8, "f32": 10, "bf16": 10}
WNEG = {"half": 9, "f32": 11, "bf16": 11}
ONES = 10
TILE16 = 16384          # elements per tile of k_reduce_narrow over 16-bit buckets (the GPU test checks the launch record)
BLOCK16 = 1024
BUGS = {
    "a": "arrivals ignore the flag and add to the stale contents",
    "b": "arrivals do not clear the flag",
    "c": "the round reads REP although it is flagged",
    "d": "the round and AggregatePartition do not flag AGG / REP",
    "e": "SET leaves the flag set",
    "f": "save_* packs the stale contents",
    "g": "a zero start is a copy of the first bucket (keeps -0.0)",
    "h": "the queue folds each format's arrivals as a group",
    "i": "a refused call changes state",
}


def geometry(M, P):
    """(lengths, offsets) of the reference chunk rule, Aggregator(M, P)."""
    c = O.chunk_size(M, P)
    return [O.partition_len(M, P, i) for i in range(P)], [i * c for i in range(P)]


GEOMETRIES = {
    # chunk 5003: lengths 5004 x 3 + 5001, flat offsets 0, 11, 6, 1 mod 16
    "short": (20009, 4),
    # odd chunk T + 8 b + 5 for the 16-bit tile: one full tile, two vector steps, a scalar remainder of 2 and 1
    "tile": (2 * (TILE16 + 8 * BLOCK16 + 4) + 1, 2),
}


# The committed cases of tests/test_gpu_stateful_narrow.py: (seed, geometry, random steps after the prefix,
# coalescing group, devices, secure).  tests/test_narrow_sequence.py inspects the plan of each (seed, geometry, steps).
CASES = [(1, "short", 300, 1, None, False), (2, "short", 300, 4, None, False), (3, "short", 300, 32, None, False),
         (8, "short", 300, 4, [0, 0], False), (5, "short", 300, 32, [0, 0, 0], False), (6, "short", 300, 4, None, True),
         (7, "tile", 150, 32, None, False)]
CASE_IDS = ["group1", "group4", "group32", "two-shards", "three-shards", "secure", "one-narrow-tile"]


def narrow_out(q64, fmt):
    """The averages' rule: the f64 quotient rounded to float, then to the format."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        f = np.ascontiguousarray(q64, dtype=np.float64).astype(np.float32)
    return f.view(np.uint32).copy() if fmt == "f32" else R.narrow(f, fmt)


def is_nan_bits(bits, fmt):
    if fmt == "f32":
        return (np.asarray(bits, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000
    return R.is_nan(bits, fmt)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Pool:
    """The buckets and flat vectors of one (seed, geometry), as values only.
    ``f64[k]``: doubles (the "be" operands are their big-endian bytes);
    ``bits[fmt][k]``: bit patterns; every bucket is max(lengths) long and is
    used through its first L_p elements, with 1.0 in every partition's count
    slot.  Bucket 1 is bucket 0 with every sign flipped (they cancel to +0.0).
    The largest finite value of each narrow format is planted; the doubles
    carry 1e300 instead of DBL_MAX, so that no fold overflows to an infinity
    and no NaN (whose payload Java leaves open) reaches a saved file."""

    def __init__(self, seed, lengths, offsets):
        rng = np.random.default_rng([seed, 0x5EED])
        self.lengths, self.offsets = list(lengths), list(offsets)
        self.Lmax = Lm = max(lengths)
        self.M = max(o + L - 1 for o, L in zip(offsets, lengths))
        slots = sorted({L - 1 for L in lengths})
        self.f64 = []
        for k in range(N_GENERAL["f64"]):
            g = O.synth_bucket(Lm, 9, k) * (10.0 ** rng.integers(-3, 4))
            g[rng.integers(0, Lm, 40)] = -0.0
            g[rng.integers(0, Lm, 10)] = 5e-324
            g[rng.integers(0, Lm, 5)] = 1e300
            self.f64.append(g)
        self.f64[1] = -self.f64[0]
        for g in self.f64:
            g[slots] = 1.0
        self.f64 += [np.full(Lm, 2.0 ** 53), np.full(Lm, -2.0 ** 53), np.full(Lm, 2.0 ** 60), np.full(Lm, -2.0 ** 60)]
        self.bits, self.wide = {}, {}
        for fmt in NARROW:
            e = R.edge_bits(fmt) if fmt != "f32" else F.EDGE_BITS["f32"]
            fin = np.array([b for b in e if not is_nan_bits(b, fmt) and np.isfinite(F.widen(np.array([b], e.dtype), fmt)[0])],
                           dtype=e.dtype)
            bs = []
            for k in range(N_GENERAL[fmt]):
                x = F.bucket(rng, Lm, fmt)
                x[rng.integers(0, Lm, 40)] = F.NEG_ZERO[fmt]
                pos = rng.integers(0, Lm, 3 * fin.size)
                x[pos] = np.tile(fin, 3)
                bs.append(x)
            bs[1] = bs[0] ^ bs[0].dtype.type(F.NEG_ZERO[fmt])
            for x in bs:
                x[slots] = F.ONE[fmt]
            bs.append(np.full(Lm, F.ONE[fmt], dtype=F.bits_dtype(fmt)))
            self.bits[fmt] = bs
            self.wide[fmt] = [F.widen(x, fmt) for x in bs]
        # flat gradient / model vectors of M elements per narrow format, and doubles for the ArrayList<Double>
        self.flat = {fmt: [np.concatenate([self.bits[fmt][(3 * j + i) % N_GENERAL[fmt]][:L - 1] for i, L in enumerate(lengths)])
                           for j in range(3)] for fmt in NARROW}
        self.flat_wide = {fmt: [F.widen(x, fmt) for x in self.flat[fmt]] for fmt in NARROW}
        self.dlist = [np.concatenate([np.concatenate([self.f64[(j + i) % 8][:L - 1] for i, L in enumerate(lengths)]),
                                      [7.0, -7.0][:2 * j]]) for j in range(2)]
        assert all(x.size == self.M for fmt in NARROW for x in self.flat[fmt])

    def values(self, fmt, k, L):
        """The doubles a bucket stands for, its first L elements."""
        return (self.f64[k] if fmt in ("f64", "be") else self.wide[fmt][k])[:L]

    def file_arrays(self, held):
        """{p: doubles} of a load step's saved-model file: the arrays of odd
        partitions are as long as the longest partition (the first L_p count)."""
        return {q: self.values(f, k, self.Lmax if q & 1 else self.lengths[q]) for q, (f, k) in held.items()}


# --------------------------------------------------------------------------
# the plan
# --------------------------------------------------------------------------
def _forms(rng):
    f = ["dev", "devoff", "host", "pinned"][int(rng.integers(0, 4))]
    return {"form": "dev" if f == "devoff" else f, "off": int(rng.integers(1, 4)) if f == "devoff" else 0}


def _narrow(rng):
    return NARROW[int(rng.integers(0, 3))]


def _draw(rng, op, pool, fixed):
    """One complete step of class ``op``; ``fixed`` overrides single draws."""
    P, lengths = len(pool.lengths), pool.lengths
    s = {"op": op}
    p = s["p"] = fixed.get("p", int(rng.integers(0, P)))
    L = lengths[p]

    def pick(fmt):
        return int(rng.integers(0, N_GENERAL["f64" if fmt == "be" else fmt]))
    if op == "update":                                   # Update(narrow, p) into AGG, REP or FUTURE
        s.update(tgt=ACC[int(rng.integers(0, 3))], fmt=_narrow(rng), **_forms(rng))
        s["k"] = pick(s["fmt"])
    elif op == "update64":                               # state mover: Update(f64 | BE bytes)
        s.update(tgt=ACC[int(rng.integers(0, 3))], fmt=("f64", "be")[int(rng.integers(0, 2))], form="host", off=0)
        s["k"] = pick("f64")
    elif op == "queue":                                  # UpdateAsync / UpdateAsyncMany, then Wait
        s.update(tgt=ACC[int(rng.integers(0, 2))], many=bool(rng.integers(0, 2)))
        if fixed.get("witness", rng.integers(0, 3) == 0):
            e = fixed.get("fmt", _narrow(rng))
            s.update(witness=True, items=[("f64", WPOS[e], 0), (e, ONES, 0), ("f64", WNEG[e], 0)])
        else:
            items = []
            for _ in range(int(rng.integers(1, 6))):
                fmt = ("f64", "be", *NARROW)[int(rng.integers(0, 5))]
                items.append((fmt, pick(fmt), int(rng.integers(0, 4)) if fmt in NARROW and rng.integers(0, 3) == 0 else 0))
            s.update(witness=False, items=items)
    elif op == "batch":                                  # reduce_batch with narrow rows, one dtype per table
        n = s["n"] = fixed.get("n", int(rng.integers(1, P - p + 1)))
        fmt = s["fmt"] = _narrow(rng)
        kk = int(rng.integers(1, 4))
        s.update(rows=[[pick(fmt) for _ in range(kk)] for _ in range(n)], mode=("zero", "accum", "first")[int(rng.integers(0, 3))],
                 tgt=ACC[int(rng.integers(0, 2))], off=int(rng.integers(1, 4)) if rng.integers(0, 4) == 0 else 0)
    elif op == "chunked":                                # UpdateChunked(p, n, source, dtype=)
        s.update(tgt=ACC[int(rng.integers(0, 2))], fmt=_narrow(rng), chunk=2 * int(rng.integers(max(1, L // 4096), L // 2 + 2)),
                 stop_at=int(rng.integers(0, 4)) if rng.integers(0, 5) == 0 else -1)
        s["k"] = pick(s["fmt"])
    elif op == "round":                                  # aggregate_round: source format x average format
        n = s["n"] = fixed.get("n", int(rng.integers(1, P - p + 1)))
        kk = fixed.get("kk", int(rng.integers(0, 4)))
        src = s["src"] = fixed.get("src", ("f64", *NARROW, *NARROW)[int(rng.integers(0, 7))])
        s["rows"] = [[pick(src) for _ in range(kk)] for _ in range(n)]
        how = ("dtype", "out", "none")[int(rng.integers(0, 3))]
        s["avg"] = (how, ("f64", *NARROW, *NARROW)[int(rng.integers(0, 7))], int(rng.integers(0, 8)))
        # one bucket 1..3 elements off a 16-B boundary: the three-launch fallback
        s["misalign"] = int(rng.integers(1, 4)) if src in NARROW and kk and rng.integers(0, 5) == 0 else 0
    elif op == "get":                                    # GetPartitions(dtype= | out=), GetPartitionsChunked
        s.update(how=("dtype", "out", "chunked")[int(rng.integers(0, 3))], fmt=_narrow(rng), off=int(rng.integers(0, 8)),
                 chunk=2 * int(rng.integers(max(1, pool.M // 4096), pool.M // 2 + 2)))
    elif op in ("ugrad", "init", "organize"):            # narrow flat vectors
        s.update(fmt=_narrow(rng), j=int(rng.integers(0, 3)), **_forms(rng))
        s["off"] = min(s["off"], 1)
        if op == "ugrad":
            s["auth"] = sorted({int(x) for x in rng.integers(0, P, int(rng.integers(1, P + 1)))})
    elif op in ("save_model", "save_sink"):
        s.update(tgt=("w", "agg", "rep")[int(rng.integers(0, 3))],
                 auth=[int(x) for x in rng.permutation(P)[:int(rng.integers(0, P + 1))]],
                 chunk_bytes=int(rng.integers(64, 40000)))
    elif op in ("save_partition", "save_list", "publish"):
        s.update(tgt=("w", "agg", "rep")[int(rng.integers(0, 3))], a=int(rng.integers(0, 100)), b=int(rng.integers(1, 9)))
    elif op == "load":                                   # LoadSavedModel: SET / BLEND into WEIGHTS / AGG / REP
        keys = [int(x) for x in rng.permutation(P)]
        s["held"] = {}
        for q in keys:
            f = ("f64", *NARROW)[int(rng.integers(0, 4))]
            s["held"][q] = (f, pick(f))
        sub = list(dict.fromkeys([p] + keys[:int(rng.integers(0, P))]))[::-1]
        s.update(order=keys, parts=None if rng.integers(0, 3) == 0 else sub,
                 leaving=bool(rng.integers(0, 2)), tgt=("w", "agg", "rep")[int(rng.integers(0, 3))])
    elif op == "init_dlist":                             # InitializeWeights(dlist, java_list=True)
        s["j"] = int(rng.integers(0, 2))
    elif op == "reset":
        s["all"] = bool(rng.integers(0, 3) == 0)
    elif op == "promote":
        s["qs"] = sorted({int(x) for x in rng.integers(0, P, 2)})
    elif op == "cache":
        s.update(k=pick("f64"), n=int(rng.integers(1, L + 1)))
    elif op == "refuse":                                 # a narrow operand where the call takes doubles only
        s.update(which=("cache", "areplica", "leaving", "other", "mixed")[int(rng.integers(0, 5))], fmt=_narrow(rng))
        s["k"] = pick(s["fmt"])
        s["fmt2"] = [f for f in ("f64", *NARROW) if f != s["fmt"]][int(rng.integers(0, 3))]
        s["k2"] = pick(s["fmt2"])
    else:
        assert op in ("aggpart", "read"), op
    s.update(fixed)
    return s


# op classes of the vocabulary and their weights in the random part
OPS = [("update", 5), ("update64", 2), ("queue", 4), ("batch", 4), ("chunked", 2), ("round", 5), ("get", 2), ("ugrad", 2),
       ("init", 1), ("organize", 1), ("save_model", 1), ("save_partition", 1), ("save_sink", 1), ("save_list", 1), ("load", 3),
       ("init_dlist", 1), ("aggpart", 2), ("reset", 1), ("promote", 1), ("cache", 1), ("publish", 1), ("refuse", 2), ("read", 1)]


def prefix(P):
    """Scripted steps that make the coverage conditions hold whatever the seed
    (as production_prefix does for the f64 sequence's launch shapes); the draws
    they do not fix come from the seed."""
    st = []
    forms = [("dev", 0), ("dev", 1), ("host", 0), ("pinned", 0)]
    last = P - 1
    for j, (form, off) in enumerate(forms):              # every operand form into stale, then non-zero, accumulators
        fmt, i = NARROW[j % 3], j % P
        st += [dict(op="update64", p=i, tgt="agg", k=2 + j), dict(op="aggpart", p=i),
               dict(op="update", p=i, tgt="agg", form=form, off=off, fmt=fmt, k=3), dict(op="read", p=i),
               dict(op="update", p=i, tgt="agg", form=form, off=off, fmt=fmt, k=4), dict(op="read", p=i)]
    for fmt in NARROW:                                   # ACCUM over a range with some partitions flagged
        st += [dict(op="reset", p=1, all=False), dict(op="batch", p=0, n=min(3, P), fmt=fmt, mode="accum", tgt="agg", off=0)]
    for fmt in NARROW:                                   # the other two start modes of k_reduce_narrow, each element size
        st += [dict(op="batch", p=0, n=min(2, P), fmt=fmt, mode=m, tgt="agg", off=0) for m in ("zero", "first")]
    for fmt in NARROW:                                   # the fused round: kAccum, REP read; then REP flagged over stale sums
        st += [dict(op="update64", p=0, tgt="rep", k=5), dict(op="update64", p=0, tgt="agg", k=6),
               dict(op="round", p=0, n=1, kk=2, src=fmt, avg=("dtype", fmt, 0), misalign=0),
               dict(op="round", p=0, n=1, kk=1, src=fmt, avg=("out", fmt, 3), misalign=0)]
    st += [dict(op="update64", p=0, tgt="agg", k=6),     # the three fallbacks
           dict(op="round", p=0, n=2, kk=2, src="half", avg=("dtype", "f64", 0), misalign=0),
           dict(op="round", p=0, n=2, kk=2, src="f64", avg=("dtype", "bf16", 0), misalign=0),
           dict(op="round", p=0, n=2, kk=2, src="f32", avg=("dtype", "f32", 0), misalign=1),
           dict(op="round", p=0, n=2, kk=1, src="bf16", avg=("none", "f64", 0), misalign=0)]
    for fmt in NARROW:                                   # a queue whose order shows
        st += [dict(op="queue", p=2 % P, tgt="agg", witness=True, fmt=fmt), dict(op="read", p=2 % P), dict(op="reset", p=2 % P, all=False)]
    st += [dict(op="update64", p=last, tgt="agg", k=2), dict(op="update64", p=last, tgt="rep", k=3), dict(op="aggpart", p=last),
           dict(op="save_partition", p=last, tgt="agg"), dict(op="save_model", p=last, tgt="rep", auth=[last, 0]),
           dict(op="save_sink", p=last, tgt="agg", auth=[1, last]), dict(op="save_list", p=last, tgt="rep"),
           dict(op="publish", p=last, tgt="agg"),
           # SET and BLEND into flagged accumulators, each followed by an ACCUM arrival
           dict(op="load", p=last, tgt="agg", leaving=False, parts=[last]), dict(op="read", p=last),
           dict(op="update", p=last, tgt="agg"), dict(op="read", p=last),
           dict(op="load", p=last, tgt="rep", leaving=True, parts=[last]), dict(op="read", p=last),
           dict(op="batch", p=last, n=1, mode="accum", tgt="rep"), dict(op="read", p=last)]
    for op in ("init", "init_dlist"):                    # InitializeWeights over non-zero AGG, REP and FUTURE
        st += [dict(op="update64", p=1, tgt=t) for t in ACC] + [dict(op=op, p=1), dict(op="read", p=1)]
    st += [dict(op="chunked", p=0, tgt="agg", stop_at=-1), dict(op="chunked", p=0, tgt="agg", stop_at=0),
           dict(op="chunked", p=0, tgt="rep", stop_at=-1)]
    st += [dict(op="refuse", p=0, which=w) for w in ("cache", "areplica", "leaving", "other", "mixed")]
    st += [dict(op="get", how=h) for h in ("dtype", "out", "chunked")]
    st += [dict(op=o) for o in ("ugrad", "ugrad", "organize", "promote", "cache")]
    return st


def plan(seed, lengths, offsets, steps, *, with_prefix=True):
    """The list of step dicts of one (seed, geometry): the scripted prefix, then
    ``steps`` random steps.  Every 25th step reads the four targets of its
    partition (``check``), every 40th the whole model as doubles (``model``)."""
    pool = Pool(seed, lengths, offsets)
    rng = np.random.default_rng([seed, 0x91A7])
    P = len(lengths)
    names = [o for o, w in OPS for _ in range(w)]
    out = []
    script = prefix(P) if with_prefix else []
    for i in range(len(script) + steps):
        fixed = dict(script[i]) if i < len(script) else {}
        op = fixed.pop("op", None) or names[int(rng.integers(0, len(names)))]
        s = _draw(rng, op, pool, fixed)
        s["i"] = i
        s["check"] = i % 25 == 24
        s["model"] = i % 40 == 39
        out.append(s)
    return out


# --------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------
class Refused(Exception):
    """The step must raise IplsError with this code; state stays."""


class Model:
    def __init__(self, pool, *, secure=False, bugs=()):
        self.pool, self.secure, self.bugs = pool, secure, set(bugs)
        self.lengths, self.offsets, self.P = pool.lengths, pool.offsets, len(pool.lengths)
        self.val = {t: [np.zeros(L) for L in self.lengths] for t in TARGETS}      # physical contents
        self.flag = {t: [True] * self.P for t in ACC}                           # "logically +0.0"
        self.events = set()
        self.pending = {}           # (tgt, p) -> "set" / "blend": loaded into a flagged accumulator, no arrival yet

    # ---- state ----
    def logical(self, t, p):
        if t != "w" and self.flag[t][p]:
            return np.zeros(self.lengths[p])
        return self.val[t][p]

    def stale(self, t, p):
        """A flagged accumulator over contents that are not all +0.0."""
        return t != "w" and self.flag[t][p] and bool(_bits(self.val[t][p]).any())

    def nonzero(self, t, p):
        return (t == "w" or not self.flag[t][p]) and bool(_bits(self.val[t][p]).any())

    def _flag(self, t, p):
        self.flag[t][p] = True
        self.pending.pop((t, p), None)

    def _start(self, t, p):
        if "a" in self.bugs:
            return self.val[t][p]
        return self.logical(t, p)

    def _fold(self, t, p, bufs, mode="accum"):
        """One launch's worth of arrivals into (t, p)."""
        L = self.lengths[p]
        zero_start = mode == "zero" or (mode == "accum" and self.flag[t][p] and "a" not in self.bugs)
        if mode == "accum" and (t, p) in self.pending:
            self.events.add(("load_then_accum", self.pending.pop((t, p))))
        if "g" in self.bugs and zero_start:
            new = O.reduce(bufs, L, O.START_FIRST)
        elif mode == "accum":
            new = O.reduce(bufs, L, O.START_ACCUM, acc=self._start(t, p))
        else:
            new = O.reduce(bufs, L, START[mode])
        self.val[t][p] = new
        if "b" not in self.bugs:
            self.flag[t][p] = False

    def _arrival_event(self, t, p, form):
        if self.stale(t, p):
            self.events.add(("arrival", form, "stale"))
        elif self.nonzero(t, p):
            self.events.add(("arrival", form, "nonzero"))

    def _aggregate(self, p, a):
        """W = a + REP; AGG and REP end logically zero."""
        rep = self.val["rep"][p] if "c" in self.bugs else self.logical("rep", p)
        self.val["w"][p] = a + rep
        if "d" not in self.bugs:
            self._flag("agg", p)
            self._flag("rep", p)

    def _saved(self, t, p):
        if "f" in self.bugs:
            return self.val[t][p]
        if self.stale(t, p):
            self.events.add("save_flagged_stale")
        return self.logical(t, p)

    def state(self, parts=None):
        return [(f"{t}[{p}]", "f64", self.logical(t, p).copy()) for p in (range(self.P) if parts is None else parts)
                for t in TARGETS]

    # ---- one step: the list of (name, kind, value) it must produce ----
    def apply(self, s):
        out = self._apply(s)
        self.events.add(s["op"])
        if s.get("check"):
            out += self.state([s["p"]])
        if s.get("model"):
            out.append(("GetPartitions", "f64", O.get_partitions([self.val["w"][p] for p in range(self.P)], self.secure)))
        return out

    def _apply(self, s):
        op, p, pool = s["op"], s["p"], self.pool
        L = self.lengths[p]
        if op in ("update", "update64"):
            if op == "update":
                self._arrival_event(s["tgt"], p, "devoff" if s["off"] else s["form"])
            self._fold(s["tgt"], p, [pool.values(s["fmt"], s["k"], L)])
            return []
        if op == "queue":
            items = list(s["items"])
            if len({f for f, _, _ in items}) > 1 and s["witness"]:
                self.events.add("queue_mixed_witness")
            if "h" in self.bugs:
                order = list(dict.fromkeys(f for f, _, _ in items))
                items.sort(key=lambda it: order.index(it[0]))
            for f, k, _ in items:
                self._fold(s["tgt"], p, [pool.values(f, k, L)])
            return []
        if op == "batch":
            qs = range(p, p + s["n"])
            if s["mode"] == "accum" and len({self.flag[s["tgt"]][q] for q in qs}) == 2:
                self.events.add("batch_accum_mixed")
            self.events.add(("batch", s["mode"]))
            for q, row in zip(qs, s["rows"]):
                self._fold(s["tgt"], q, [pool.values(s["fmt"], k, self.lengths[q]) for k in row], s["mode"])
            return []
        if op == "chunked":
            ch = min(s["chunk"], L)
            if 0 <= s["stop_at"] < -(-L // ch):
                self.events.add("chunked_stopped")
                return [("code", "refused", "INVAL")]
            self._arrival_event(s["tgt"], p, "chunked")
            self._fold(s["tgt"], p, [pool.values(s["fmt"], s["k"], L)])
            return [("code", "refused", None)]
        if op == "round":
            how, afmt, _ = s["avg"]
            exp = []
            has = bool(s["rows"][0])
            fused = s["src"] in NARROW and has and not s["misalign"] and (how == "none" or afmt in NARROW)
            for q, row in zip(range(p, p + s["n"]), s["rows"]):
                if fused:                                # k_round_narrow
                    self.events.add("round_narrow")
                    if self.nonzero("rep", q):
                        self.events.add("round_rep_nonzero")
                    if self.stale("rep", q):
                        self.events.add("round_rep_flagged_stale")
                    if self.nonzero("agg", q):
                        self.events.add("round_agg_nonzero")
                elif has and s["misalign"]:
                    self.events.add(("round_fallback", "misalign"))
                elif has and s["src"] in NARROW:
                    self.events.add(("round_fallback", "narrow_to_f64"))
                elif has and how != "none" and afmt in NARROW:
                    self.events.add(("round_fallback", "f64_to_narrow"))
                if row:
                    self._fold("agg", q, [pool.values(s["src"], k, self.lengths[q]) for k in row])
                self._aggregate(q, self.logical("agg", q))
                exp.append(O.divide(self.val["w"][q], self.secure))
            if how == "none":
                return []
            avg = np.concatenate(exp)
            return [("averages", afmt, avg if afmt == "f64" else narrow_out(avg, afmt))]
        if op == "get":
            g = O.get_partitions([self.val["w"][q] for q in range(self.P)], self.secure)
            return [("model", s["fmt"], narrow_out(g, s["fmt"]))]
        if op in ("ugrad", "init", "organize"):
            og = O.organize_gradients(pool.flat_wide[s["fmt"]][s["j"]], pool.M, self.P)
            if op == "organize":
                return [(f"organize[{q}]", "f64", og[q]) for q in range(self.P)]
            if op == "ugrad":
                for q in s["auth"]:
                    self._arrival_event("agg", q, "flat")
                    self._fold("agg", q, [og[q]])
                return []
            return self._init(og, "init_narrow")
        if op == "init_dlist":
            og = O.organize_gradients(pool.dlist[s["j"]][:pool.M], pool.M, self.P)
            return self._init(og, "init_dlist")
        if op in ("save_model", "save_sink"):
            return [("file", "map", ({q: self._saved(s["tgt"], q).copy() for q in s["auth"]}, list(s["auth"])))]
        if op == "save_partition":
            return [("file", "darr", self._saved(s["tgt"], p).copy())]
        if op == "save_list":
            return [("file", "dlist", np.concatenate([self._saved(s["tgt"], q) for q in range(self.P)]))]
        if op == "publish":
            return [("text", "frame", (self._saved(s["tgt"], p).copy(), s["a"], s["b"]))]
        if op == "load":
            held, t = self.pool.file_arrays(s["held"]), s["tgt"]
            parts = list(s["order"]) if s["parts"] is None else s["parts"]
            for q in parts:
                Lq = self.lengths[q]
                was_flagged = t != "w" and self.flag[t][q]
                if s["leaving"]:
                    self.val[t][q] = O.blend(self.logical(t, q), held[q][:Lq], 0.6, 1 - 0.6)
                else:
                    self.val[t][q] = held[q][:Lq].copy()
                if t != "w" and (s["leaving"] or "e" not in self.bugs):
                    self.flag[t][q] = False
                if was_flagged:
                    self.pending[(t, q)] = "blend" if s["leaving"] else "set"
            return [("done", "int", len(set(parts)))]
        if op == "aggpart":
            self._aggregate(p, self.logical("agg", p))
            return []
        if op == "reset":
            for q in (range(self.P) if s["all"] else [p]):
                self._flag("agg", q)
                self._flag("rep", q)
            return []
        if op == "promote":
            for q in s["qs"]:                            # the arena blocks change places; FUTURE ends flagged
                self.val["agg"][q], self.val["fut"][q] = self.val["fut"][q], self.val["agg"][q]
                self.flag["agg"][q] = self.flag["fut"][q]
                self.flag["fut"][q] = True
                self.pending.pop(("agg", q), None)
            return []
        if op == "cache":
            w = self.val["w"][p].copy()
            w[:s["n"]] = pool.f64[s["k"]][:s["n"]]
            self.val["w"][p] = w
            return []
        if op == "refuse":
            if "i" in self.bugs:                         # the call goes through as if it took the operand
                g = pool.values(s["fmt"], s["k"], L)
                if s["which"] == "cache":
                    self.val["w"][p] = g.copy()
                elif s["which"] == "areplica":
                    self.val["w"][p] = O.blend(self.val["w"][p], g, 0.75, 1.0)
                elif s["which"] == "leaving":
                    self.val["w"][p] = O.blend(self.val["w"][p], g, 0.6, 1 - 0.6)
                elif s["which"] == "other":
                    self.val["rep"][p] = self.logical("rep", p) + g
                    self.flag["rep"][p] = False
                else:
                    self.val["agg"][p] = O.reduce([g, pool.values(s["fmt2"], s["k2"], L)], L, O.START_ZERO)
                    self.flag["agg"][p] = False
            self.events.add(("refuse", s["which"]))
            return [("code", "refused", "INVAL")] + self.state()
        assert op == "read", op
        return self.state([p])

    def _init(self, og, tag):
        if any(all(self.nonzero(t, q) for t in ACC) for q in range(self.P)):
            self.events.add((tag, "all_nonzero"))
        for q in range(self.P):
            w = og[q].copy()
            w[-1] = 0.0                                  # IPLS.java:1883-1895: the count slot is 0.0
            self.val["w"][q] = w
            for t in ACC:
                self._flag(t, q)
        return []

    def final(self):
        return self.state()


def same(a, b):
    """Whether two lists of step outputs agree in every compared value."""
    if len(a) != len(b):
        return False
    for (na, ka, va), (nb, kb, vb) in zip(a, b):
        if (na, ka) != (nb, kb):
            return False
        if ka == "map":
            if va[1] != vb[1] or any(not np.array_equal(_bits(va[0][q]), _bits(vb[0][q])) for q in va[0]):
                return False
        elif ka == "frame":
            if va[1:] != vb[1:] or not np.array_equal(_bits(va[0]), _bits(vb[0])):
                return False
        elif ka in ("f64", "darr", "dlist"):
            if not np.array_equal(_bits(va), _bits(vb)):
                return False
        elif ka in NARROW:
            if not np.array_equal(va, vb):
                return False
        elif va != vb:
            return False
    return True
