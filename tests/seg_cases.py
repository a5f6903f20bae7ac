"""Inputs and oracle-side expectations shared by the segment-list tests
(test_gpu_segs.py on the GPU, test_seg_boundary.py on the CPU): the layouts of
a flat vector as a list of arrays of mixed formats, each a view at an element
offset into its own backing array with junk around it, the planted edge
values, the expected state (the oracle alone: organize_gradients on the
widened concatenation, then fold; get_partitions, then the format's narrowing;
frame_encode under java_b64url_encode), numpy models of the mistakes a
segment-list kernel can make, and the coverage conditions the layouts must
meet -- asserted, so a layout cannot silently stop covering its case.
"""
from dataclasses import dataclass

import numpy as np

import h16_ref as R
import narrow_fmt as F
import update_flat_cases as U

FMTS = ("f64", "f32", "half", "bf16")
KIND = {"f64": 3, "f32": 11, "half": 13, "bf16": 15}       # IPLS_DEV_F64 / F32 / F16 / BF16
P = U.P_SWEEP
TILE_DEFAULT = 2048          # block x vectors of the segment kernels; the GPU tests read it from last_launch
LAYOUTS = ("whole-f64", "whole-f32", "whole-half", "whole-bf16", "residues-f64", "residues-f32", "residues-half",
           "residues-bf16", "tiny", "aligned", "short-a", "short-b", "short-c")
SENTINEL = 0xA5


def esize(fmt):
    return 8 if fmt == "f64" else F.esize(fmt)


def bits_dtype(fmt):
    return np.uint64 if fmt == "f64" else F.bits_dtype(fmt)


def edge_bits(fmt):
    return U.EDGE_F64 if fmt == "f64" else F.EDGE_BITS[fmt]


def widen(bits, fmt):
    return U.widen(bits, fmt)


def residues(fmt):
    return 16 // esize(fmt)


def chunks(T):
    return U.sweep_chunks(T)


def model_size(c):
    return U.sweep_model_size(c)


@dataclass
class Seg:
    """One segment: elements [r, r + n) of `backing` (bit patterns of the
    format); everything else in the backing array is junk."""
    fmt: str
    n: int
    r: int
    backing: np.ndarray = None

    @property
    def bits(self):
        return self.backing[self.r:self.r + self.n]

    @property
    def wide(self):
        return widen(self.bits, self.fmt)


PAD = 24   # junk elements after a view (and r before it)


def boundaries(c, T, M):
    """Every partition boundary and tile seam of the model, as flat indices in (0, M)."""
    out = set()
    for p in range(P):
        lo, hi = p * c, min((p + 1) * c, M)
        out.add(lo)
        out.update(range(lo + T, hi, T))
    return sorted(b for b in out if 0 < b < M)


def _cut(seams, n, fmt_of, res_of):
    """Segments between consecutive seams (a repeated seam gives an empty one) up to n."""
    out, at = [], 0
    for k, b in enumerate(list(seams) + [n]):
        b = min(b, n)
        if b < at:
            continue
        fmt = fmt_of(len(out))
        out.append((fmt, b - at, res_of(len(out)) % residues(fmt)))
        at = b
    return out


def shape(name, c, T):
    """The layout as [(fmt, n, r)]; the values come from build()."""
    M = model_size(c)
    kind, _, arg = name.partition("-")
    if kind == "whole":
        return [(arg, M, 0)]
    if kind == "residues":
        # a short head, then one segment of c values at every residue (each holds the second tile of a partition
        # when c > 2 T), then the rest
        k = residues(arg)
        out, left = [(arg, 5, 1 % k)], M - 5
        for i in range(k):
            out.append((arg, min(c, left), i))
            left -= out[-1][1]
        if left:
            out.append((arg, left, 0))
        return out
    if kind == "tiny":
        seams = []
        for b in boundaries(c, T, M):
            seams += [b - 2, b - 1, b, b, b + 1, b + 3]
        assert seams == sorted(seams)
        return _cut([s for s in seams if 0 < s < M], M, lambda i: FMTS[i % 4], lambda i: i + 1)
    if kind == "aligned":
        return _cut(boundaries(c, T, M), M, lambda i: FMTS[(i + 1) % 4], lambda i: 3 * i + 1)
    if kind == "short":
        end = {"a": 6 * c + max(1, min(T, c - 1) - 3), "b": 6 * c + min(T + 3, c - 1), "c": 7 * c}[arg]
        step = c // 2 + 1
        # a seam every `step` values, and an empty segment in the middle of a tile
        seams = sorted(list(range(step, end, step)) + [step + 2, step + 2])
        return _cut(seams, end, lambda i: FMTS[(i + 2) % 4], lambda i: i + 2)
    raise KeyError(name)


def plant_positions(spec, c, T, M):
    """Flat positions of the planted edge values: first and last element of
    every segment, both sides of every tile seam and partition boundary."""
    pos, at = set(), 0
    for _, n, _ in spec:
        if n:
            pos.update((at, at + n - 1))
        at += n
    for b in boundaries(c, T, M):
        pos.update((b - 1, b))
    return pos


def build(rng, spec, c, T):
    """Seg objects with values: normals, the format's edge bit patterns at the
    planted positions, junk (other normals) around every view."""
    M = model_size(c)
    plant = plant_positions(spec, c, T, M)
    out, at, k = [], 0, 0
    for fmt, n, r in spec:
        x = rng.standard_normal(r + n + PAD)
        backing = x.view(np.uint64).copy() if fmt == "f64" else F.from_f32(x.astype(np.float32), fmt)
        e = edge_bits(fmt)
        for i in range(n):
            if at + i in plant:
                backing[r + i] = e[k % e.size]
                k += 1
        out.append(Seg(fmt, n, r, backing))
        at += n
    return out


def total(segs):
    return sum(s.n for s in segs)


def concat(segs):
    """The flat vector the list stands for, widened."""
    return np.concatenate([s.wide for s in segs] + [np.zeros(0)])


def starts(segs):
    return np.concatenate([[0], np.cumsum([s.n for s in segs])]).astype(np.int64)


# ---- expectations: the oracle alone ----
def expected_update(O, acc, segs, c, owned):
    M = model_size(c)
    return U.expected(O, acc, concat(segs), total(segs), M, P, owned)


def expected_texts(O, segs, c, parts, iteration, origin, pid=3):
    M = model_size(c)
    g = O.organize_gradients(concat(segs), M, P)
    return [O.java_b64url_encode(O.frame_encode(g[p], p, iteration, pid, origin)) for p in parts]


def narrow(x, fmt):
    """Doubles to the format's bit patterns by the output rule: as they are,
    one rounding to float, or that float rounded again to the 16-bit format."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if fmt == "f64":
        return x.view(np.uint64).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
    return f.view(np.uint32).copy() if fmt == "f32" else R.narrow(f, fmt)


def is_nan(bits, fmt):
    if fmt == "f64":
        return np.isnan(np.asarray(bits, dtype=np.uint64).view(np.float64))
    if fmt == "f32":
        return np.isnan(np.asarray(bits, dtype=np.uint32).view(np.float32))
    return R.is_nan(bits, fmt)


def expected_outputs(model, spec, M):
    """Per output segment: (bit patterns of elements below M, how many)."""
    out, at = [], 0
    for fmt, n, _ in spec:
        k = max(0, min(at + n, M) - at)
        out.append(narrow(model[at:at + k], fmt))
        at += n
    return out


def weights(rng, O, c):
    """W per partition with a different count each, one of them 0.0."""
    M = model_size(c)
    w = []
    for p in range(P):
        L = O.partition_len(M, P, p)
        x = rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)
        x[L - 1] = 0.0 if p == 4 else float(p + 2)
        w.append(x)
    return w


# ---- the items a call makes (block count of its launch) ----
def n_update_items(O, c, T, parts):
    M = model_size(c)
    return sum(-(-O.partition_len(M, P, p) // T) for p in parts)


def n_divide_items(spec, M, T, addr_mod=lambda i: 0):
    """One item for the head up to the first 128-B line of each output segment, then tiles of T."""
    n_items, at = 0, 0
    for i, (fmt, n, r) in enumerate(spec):
        k = max(0, min(at + n, M) - at)
        at += n
        if not k:
            continue
        a = (addr_mod(i) + r * esize(fmt)) % 128
        head = min(((128 - a) % 128) // esize(fmt), k)
        n_items += (1 if head else 0) + -(-(k - head) // T)
    return n_items


# ---- what a tile sees (the coverage conditions) ----
def pieces_of(segs, lo, hi):
    """[(seg index, first element in it, count)] covering flat [lo, hi)."""
    st = starts(segs)
    out = []
    for i, s in enumerate(segs):
        a, b = max(lo, st[i]), min(hi, st[i + 1])
        if b > a:
            out.append((i, int(a - st[i]), int(b - a)))
    return out


def coverage(spec, c, T):
    """Facts about a layout, computed from its shape alone."""
    M = model_size(c)
    n = sum(s[1] for s in spec)
    st = np.concatenate([[0], np.cumsum([s[1] for s in spec])]).astype(np.int64)
    segs = [Seg(f, k, r) for f, k, r in spec]
    cov = dict(whole=set(), fmts3=False, empty_in_tile=False, part_seam_in_seg=False, part_seam_in_out_tile=False,
               seg_seam_on_tile_seam=False, first_tile_res=False, last_tile_res=False)
    tile_seams = set(boundaries(c, T, M))
    for i, (fmt, k, r) in enumerate(spec):
        if k and 0 < st[i] < n and int(st[i]) in tile_seams:
            cov["seg_seam_on_tile_seam"] = True
        if any(st[i] < p * c < st[i + 1] for p in range(1, P)):
            cov["part_seam_in_seg"] = True
        # output tiles: head to the first line, then tiles of T (backing arrays start on a line)
        a = (r * esize(fmt)) % 128
        head = min(((128 - a) % 128) // esize(fmt), k)
        e = 0
        while e < min(k, M - st[i]):
            hi = min(e + (head if e == 0 and head else T), k)
            if (st[i] + e) // c != (st[i] + hi - 1) // c:
                cov["part_seam_in_out_tile"] = True
            e = hi
    for p in range(P):
        ncopy = max(0, min((p + 1) * c, n) - p * c)
        for lo in range(0, ncopy, T):
            hi = min(lo + T, ncopy)
            pcs = pieces_of(segs, p * c + lo, p * c + hi)
            if len({spec[i][0] for i, _, _ in pcs}) >= 3:
                cov["fmts3"] = True
            if any(spec[i][1] == 0 and p * c + lo < st[i] < p * c + hi for i in range(len(spec))):
                cov["empty_in_tile"] = True
            i, e, k = pcs[0]
            fmt, sn, r = spec[i]
            res = (r + e) % residues(fmt)
            if len(pcs) == 1 and hi - lo == T:
                cov["whole"].add((fmt, res))
            if len(pcs) == 1 and res and e < T:
                cov["first_tile_res"] = True
            if len(pcs) == 1 and res and e + k + T > sn:
                cov["last_tile_res"] = True
    return cov


def check_coverage(T):
    """The union over the chunks and layouts covers every case (asserted)."""
    whole, flags = set(), {}
    for c in chunks(T):
        for name in LAYOUTS:
            cov = coverage(shape(name, c, T), c, T)
            whole |= cov.pop("whole")
            for k, v in cov.items():
                flags[k] = flags.get(k, False) or v
    for fmt in FMTS:
        for r in range(residues(fmt)):
            assert (fmt, r) in whole, f"no whole tile of {fmt} at residue {r}"
    for k, v in flags.items():
        assert v, f"no layout covers {k}"
    return whole, flags


# ---- the mistakes, modelled on the widened vector / on the model ----
def _reread(s, first, fmt=None):
    """n elements of s's backing array from element `first`, widened."""
    return widen(s.backing[first:first + s.n], fmt or s.fmt)


def mistake_vectors(segs):
    """{mistake: the flat vector a kernel making it would read} -- only the
    mistakes that apply to the layout."""
    live = [s for s in segs if s.n]
    out = {}
    if live:
        out["source offset off by one"] = np.concatenate([_reread(s, s.r + 1) for s in live])
    if any(s.r for s in live):
        out["residue ignored"] = np.concatenate([_reread(s, 0) for s in live])
    if any(a.fmt != b.fmt for a, b in zip(live, live[1:])):
        parts, prev = [], None
        for s in live:
            w = s.wide.copy()
            if prev is not None and prev.fmt != s.fmt:
                raw = s.backing[s.r:].view(np.uint8)[:8]
                w[0] = widen(raw[:esize(prev.fmt)].copy().view(bits_dtype(prev.fmt)), prev.fmt)[0]
            parts.append(w)
            prev = s
        out["previous format for the first element"] = np.concatenate(parts)
    if any(s.n == 0 for s in segs[:-1]):
        parts = []
        for s in segs:
            parts.append(s.wide if s.n else np.array([123.456]))
        out["an empty segment consumes an element"] = np.concatenate(parts)[:total(segs)]
    return out


def mistake_ncopy_per_segment(O, segs, c):
    """Expected AGG (from zeros) when a partition's ncopy ends with its first piece; None if no partition has two."""
    M = model_size(c)
    n = total(segs)
    g = O.organize_gradients(concat(segs), M, P)
    hit = False
    for p in range(P):
        pcs = pieces_of(segs, p * c, min((p + 1) * c, n))
        if len(pcs) >= 2:
            hit = True
            k = pcs[0][2]
            g[p] = g[p].copy()
            g[p][k:] = 0.0
            g[p][k] = 1.0
    return [g[p] + 0.0 for p in range(P)] if hit else None


def mistake_models(w, spec, c, T, secure):
    """{mistake: the flat model a divide making it would write} for an output layout."""
    M = model_size(c)
    den = [(1e12 * x[-1] if secure else x[-1]) for x in w]
    st = np.concatenate([[0], np.cumsum([s[1] for s in spec])]).astype(np.int64)

    def value(f, p_cnt, p_val=None, j=None):
        p_val = f // c if p_val is None else p_val
        j = f - (f // c) * c if j is None else j
        x = w[p_val][j]
        return x if w[p_cnt][-1] == 0.0 else x / den[p_cnt]

    local, neigh = np.zeros(M), np.zeros(M)
    local_hit = neigh_hit = False
    for i, (fmt, k, r) in enumerate(spec):
        a = (r * esize(fmt)) % 128
        head = min(((128 - a) % 128) // esize(fmt), k)
        e = 0
        while e < k and st[i] + e < M:
            hi = min(e + (head if e == 0 and head else T), k)
            p0 = int(st[i] + e) // c
            for x in range(e, hi):
                f = int(st[i] + x)
                if f >= M:
                    break
                neigh[f] = value(f, p0)
                neigh_hit = neigh_hit or p0 != f // c
                pl = min(x // c, P - 1)           # the partition of the segment-local index
                jl = min(x - (x // c) * c, len(w[pl]) - 2) if len(w[pl]) > 1 else 0
                local[f] = value(f, pl, pl, jl) if len(w[pl]) > 1 else 0.0
                local_hit = local_hit or pl != f // c
            e = hi
    out = {}
    if local_hit:
        out["partition from the segment-local index"] = local
    if neigh_hit:
        out["the neighbour's count across a partition seam"] = neigh
    return out
