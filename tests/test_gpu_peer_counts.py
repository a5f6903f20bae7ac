"""Peer-count sweep of the fold kernels: K up to 129 on every path, bit for bit.

Every fold kernel has code whose behaviour changes with the number of peers K:
groups of 8 loads in flight and their remainder loops (reduce_tiles' G = 8 and
kPB = 8, the narrow kernels' kPeersVec = 8 and kPB = 8), the next-peer
prefetch of the narrow full tile (guarded by j + 1 < k), the plain loop of
k_reduce_scalar, and the count pre-passes, which give one lane to each peer
and walk K in chunks of 64.  This file moves along K on each of them:

  kernel (shape)                                K reached here
  k_reduce, small shape (reduce_batch[_out])    1 2 7 8 9 16 17 33 64 65        (KFOLD)
  k_reduce_scalar (buckets at 8 mod 16)         KFOLD
  k_reduce_narrow f32 / half / bf16             KFOLD, aligned (map 3) and element by element
  k_round + k_round_counts, small shape         0 1 2 7 8 9 15 16 17 31 32 33 63 64 65 127 128 129   (KROUND)
  k_round_narrow + k_round_counts_narrow        KROUND (K = 0 names no format: the unfused steps, bits only)
  k_reduce / k_round, mid, half and big shape   8 17 65

The inputs are those of tests/peer_witness.py: witness columns in which the
exchange of any two adjacent peers turns 0.0 into 1.0, random columns that
show a dropped or a duplicated peer, and count slots whose count is 4.0 in
order and 3.0 with the peers around 8, 64, 128 or K - 1 exchanged
(tests/test_peer_witness.py proves with the oracle alone that every such
mistake changes the bits).  Halves have no witness columns: sums of up to 129
halves are exact in f64, so the order cannot be observed; their random
columns and counts still show drops and duplicates.  One block of witness and
random columns stands at the start of each code region of the length under
test -- full tile, vector step of the partial tile, element-by-element
remainder -- and the lengths are the smallest that have all three (T and the
lanes b come from the launch record).  The small shape of reduce_tiles holds
one vector per lane, so its 2b-element step is a full tile and its partial
tile has the remainder only: three full tiles (peers in groups of G = 8), then
150 elements by element (groups of kPB = 8).  The vector steps of the partial
tile (kPB = 8 again) exist in the wide shapes alone and run in case 6.  A partition's buckets are the pool
rotated by one block's worth of columns per partition, so peer 0 stays peer
0; the count slots are rewritten for every K.

Every case asserts the launch record, compares every element with the oracle
(O.reduce, O.aggregate_partition, O.get_partitions, then the narrowing rule
of h16_ref for narrow averages) and keeps caller-owned outputs between
sentinel guard bands.  The inputs hold no NaN: every comparison is plain
equality of bits.  One handle serves the K values of a case, ascending then
descending.
"""
import zlib

import numpy as np
import pytest

import narrow_fmt as NF
import peer_witness as PW

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KFOLD = (1, 2, 7, 8, 9, 16, 17, 33, 64, 65)
KROUND = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
KSECURE = (9, 64, 65, 129)
KBE = (8, 9, 65)
KCROSS = (9, 65)          # averages in the other two formats / big-endian reduce_batch_out
P = 4
GUARD = 40
NARROW = ("f32", "half", "bf16")
SENT = {"f64": 0x7FF45EA1A15EF47F, "f32": 0x55555555, "half": 0x5555, "bf16": 0x5555}
CARRIER = {"f64": torch.int64, "f32": torch.int32, "half": torch.int16, "bf16": torch.int16}
NPCARRIER = {"f64": np.int64, "f32": np.int32, "half": np.int16, "bf16": np.int16}
NPBITS = {"f64": np.uint64, "f32": np.uint32, "half": np.uint16, "bf16": np.uint16}


@pytest.fixture(scope="module")
def ipls():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu run without a visible GPU")
    import ipls as m
    return m


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def _esz(fmt):
    return 8 if fmt == "f64" else NF.esize(fmt)


def _updown(ks):
    return tuple(ks) + tuple(ks)[::-1]


def _same(got, want, fmt, what):
    g = np.ascontiguousarray(got).view(NPBITS[fmt]).ravel()
    w = np.ascontiguousarray(want).view(NPBITS[fmt]).ravel()
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g != w)
    assert not bad.size, f"{what}: {bad.size} of {g.size} differ; first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"


def _avg_bits(q64, fmt):
    """The averages' rule: doubles, or the quotient rounded to float and then to the 16-bit format."""
    if fmt == "f64":
        return np.ascontiguousarray(q64).view(np.uint64)
    with np.errstate(over="ignore", under="ignore"):
        return NF.from_f32(np.ascontiguousarray(q64).astype(np.float32), fmt)


# --------------------------------------------------------------------------
# tiles, from the launch record
# --------------------------------------------------------------------------
_TILE = {}


def _tile(ipls, fmt):
    """(T, b, elements per vector step of the partial tile) of the fold over buckets of the format."""
    key = _esz(fmt)
    if key not in _TILE:
        one = PW.to_bits(np.ones((2, 2, 9)), fmt)
        t = torch.from_numpy(np.zeros((4, 16), dtype=NPCARRIER[fmt])).cuda()
        t[:, :9] = torch.from_numpy(one.reshape(4, 9).view(NPCARRIER[fmt])).cuda()
        torch.cuda.synchronize()
        tab = [[_buf(ipls, t.data_ptr() + _esz(fmt) * 16 * (2 * q + j), 9, fmt) for j in range(2)] for q in range(2)]
        with ipls.Aggregator(n_partitions=2, bucket_len=9) as agg:
            agg.aggregate_round(0, tab, with_average=False)
            li = agg.last_launch()
        per = 2 if fmt == "f64" else 4                    # elements of a lane's vector
        assert li["kernel"] == _round_kernel(ipls, fmt), li
        _TILE[key] = (li["block"] * per * li["vectors"], li["block"], li["block"] * per)
    return _TILE[key]


def _buf(ipls, ptr, n, fmt, be=False):
    return ipls.DeviceBuffer(int(ptr), n, big_endian=be) if fmt == "f64" else ipls.DeviceBuffer(int(ptr), n, dtype=fmt)


def _round_kernel(ipls, fmt):
    return {"f64": ipls.KERNEL_ROUND, "f32": ipls.KERNEL_ROUND_F32}.get(fmt, ipls.KERNEL_ROUND_H16)


def _fold_kernel(ipls, fmt):
    return ipls.KERNEL_REDUCE if fmt == "f64" else NF.reduce_kernel(ipls, fmt)


# --------------------------------------------------------------------------
# the pools: generated once per module
# --------------------------------------------------------------------------
class Pool:
    """P x kmax buckets of one format and length on the device, in the
    placements a case asks for: "a" every bucket on a 16-B boundary, "o" off it
    (doubles: every bucket at 8 mod 16; narrow formats: bucket 0 of partition
    1 one element past a boundary), "abe" / "obe" the same as big-endian bytes."""

    def __init__(self, ipls, fmt, L, starts, seed, places, kmax):
        self.ipls, self.fmt, self.L, self.kmax, self.starts = ipls, fmt, L, kmax, starts
        rng = np.random.default_rng(seed)
        self.x = PW.layout(kmax, P, L, starts, rng, fmt)
        W = PW.n_witness(kmax, fmt)
        # what an ACCUM case starts from: +0.0 in the witness columns, two earlier arrivals counted in partition 0
        self.prior = PW.random_values(rng, (P, L), "f64")
        for s in starts:
            self.prior[:, s:s + W] = 0.0
        self.prior[:, L - 1] = 0.0
        self.prior[0, L - 1] = 2.0
        self.rep = PW.random_values(rng, (L,), "f64")
        self.rep[L - 1] = 0.0
        self.K = None
        self.cache = {}
        per16 = 16 // _esz(fmt)
        self.stride = (L + 1 + per16 - 1) // per16 * per16
        self.dev = {}
        rows = np.arange(P * kmax)
        for name in places:
            off = np.zeros(P * kmax, dtype=np.int64)
            if name.startswith("o"):
                if fmt == "f64":
                    off[:] = 1
                else:
                    off[kmax] = 1
            t = torch.zeros((P * kmax, self.stride), dtype=CARRIER[fmt], device="cuda")
            assert t.data_ptr() % 16 == 0
            src = torch.from_numpy(self._carrier(self.x.reshape(P * kmax, L), name)).cuda()
            for o in (0, 1):
                idx = torch.from_numpy(np.flatnonzero(off == o)).cuda()
                t[idx, o:o + L] = src[idx]
            self.dev[name] = (t, off, torch.from_numpy(rows).cuda(), torch.from_numpy(off + L - 1).cuda())
        pr = torch.zeros((P, self.stride8()), dtype=torch.int64, device="cuda")
        pr[:, :L] = torch.from_numpy(self.prior.view(np.int64)).cuda()
        self.dprior = pr
        torch.cuda.synchronize()

    def stride8(self):
        return (self.L + 2) // 2 * 2

    def _carrier(self, doubles, name):
        b = PW.to_bits(doubles, self.fmt)
        if self.fmt == "f64":
            b = b.view(np.uint64)
            if name.endswith("be"):
                b = b.byteswap()
        return np.ascontiguousarray(b).view(NPCARRIER[self.fmt])

    def set_k(self, K):
        """The count slots of K peers (peer_witness.count_slots), on the host and in every placement."""
        if K == self.K:
            return
        c = np.zeros((P, self.kmax))
        c[:, :K] = PW.count_slots(K, P, self.fmt)[0]
        self.x[:, :, self.L - 1] = c
        for name, (t, off, rows, cols) in self.dev.items():
            t[rows, cols] = torch.from_numpy(self._carrier(c.reshape(-1), name)).cuda()
        torch.cuda.synchronize()
        self.K = K

    def table(self, K, name):
        t, off, _, _ = self.dev[name]
        e, base = _esz(self.fmt), t.data_ptr()
        return [[_buf(self.ipls, base + e * ((q * self.kmax + j) * self.stride + off[q * self.kmax + j]), self.L,
                      self.fmt, name.endswith("be")) for j in range(K)] for q in range(P)]

    def prior_table(self):
        return [[self.ipls.DeviceBuffer(self.dprior.data_ptr() + 8 * q * self.stride8(), self.L)] for q in range(P)]

    # ---- the oracle, once per (K, start) ----
    def fold(self, O, K, start):
        """O.reduce of the first K buckets of every partition, in order."""
        assert K == self.K
        key = ("fold", K, start)
        if key not in self.cache:
            self.cache[key] = [O.reduce([self.x[q, j] for j in range(K)], self.L, start,
                                        self.prior[q] if start == O.START_ACCUM else None) for q in range(P)]
        return self.cache[key]

    def weights(self, O, K, accum, rep_on=1):
        """W of a round: the fold from AGG (the prior, or +0.0), then AGG + REP (REP on one partition)."""
        key = ("w", K, accum)
        if key not in self.cache:
            ws = []
            for q, a in enumerate(self.fold(O, K, O.START_ACCUM if accum else O.START_ZERO)):
                w, wa = np.zeros(self.L), np.zeros(self.L)
                O.aggregate_partition(a.copy(), self.rep.copy() if q == rep_on else np.zeros(self.L), w, wa)
                ws.append(w)
            self.cache[key] = ws
        return self.cache[key]


_POOLS = {}


def _pool(ipls, fmt, kind):
    """kind: "fold" (kmax 65), "round" (kmax 129), "scalar" (doubles, 300 elements)."""
    key = (fmt, kind)
    if key not in _POOLS:
        T, b, step = _tile(ipls, fmt)
        B = PW.block_width(129, fmt)
        rem = 150
        assert B <= rem < b                               # the remainder holds one block and stays a remainder
        if kind == "scalar":
            L, starts, places = 300, (0, 150), ("o", "obe")
        elif fmt == "f64":
            # two full tiles, 2b elements more (a third full tile here: T = 2b), 150 by element, the count slot
            L, starts = 2 * T + step + rem + 1, (0, T, 2 * T, 2 * T + step)
            places = ("a", "abe")
        else:
            # one full tile, one vector step of 4b elements, 150 by element, the count slot; (L - 1) mod 4 != 0
            L, starts = T + step + rem + 1, (0, T, T + step)
            places = ("a", "o") if kind == "fold" else ("a",)
            assert (L - 1) % 4 != 0
        kmax = 129 if kind == "round" else 65
        _POOLS[key] = Pool(ipls, fmt, L, starts, zlib.crc32(repr(key).encode()), places, kmax)
    return _POOLS[key]


class Out:
    """n caller-owned elements of a format on the device, `off` elements past a 16-B boundary, between sentinels."""

    def __init__(self, ipls, n, fmt, off, be=False):
        self.n, self.fmt, self.off = n, fmt, off
        per16 = 16 // _esz(fmt)
        self.lead = GUARD // per16 * per16 + off
        self.t = torch.full((self.lead + n + GUARD,), SENT[fmt], dtype=CARRIER[fmt], device="cuda")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + _esz(fmt) * self.lead
        self.buf = _buf(ipls, self.ptr, n, fmt, be)

    def fill(self, bits):
        self.t[self.lead:self.lead + self.n] = torch.from_numpy(np.ascontiguousarray(bits).view(NPCARRIER[self.fmt])).cuda()
        torch.cuda.synchronize()

    def bits(self):
        h = self.t.cpu().numpy().view(NPBITS[self.fmt])
        assert (h[:self.lead] == SENT[self.fmt]).all() and (h[self.lead + self.n:] == SENT[self.fmt]).all(), \
            "wrote outside the output"
        return h[self.lead:self.lead + self.n].copy()


def _record(li, what, **want):
    got = {f: li[f] for f in want}
    assert got == want, f"{what}: launch record {got} != {want}"


def _check_agg(agg, want, what):
    for q in range(P):
        _same(agg.read(q), want[q], "f64", f"{what}: AGG p={q}")


def _set_prior(ipls, agg, pool):
    """AGG[p] = the prior, exactly (a FIRST-started fold of one f64 device bucket)."""
    agg.reduce_batch(0, pool.prior_table(), start_mode=ipls.START_FIRST)


# --------------------------------------------------------------------------
# 1. k_reduce, small shape
# --------------------------------------------------------------------------
def test_reduce_small(ipls, O):
    """reduce_batch over KFOLD: native and big-endian input, ZERO, FIRST and
    ACCUM onto a prior fold; at K = 9 and 65 also reduce_batch_out into
    guarded big-endian destinations."""
    pool = _pool(ipls, "f64", "fold")
    T, b, step = _tile(ipls, "f64")
    L = pool.L
    tiles = -(-L // T)
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for K in _updown(KFOLD):
            pool.set_k(K)
            for start in (ipls.START_ZERO, ipls.START_FIRST, ipls.START_ACCUM):
                want = pool.fold(O, K, start)
                for be in (False, True):
                    what = f"k_reduce small K={K} start={start} be={be}"
                    if start == ipls.START_ACCUM:
                        _set_prior(ipls, agg, pool)
                    agg.reduce_batch(0, pool.table(K, "abe" if be else "a"), start_mode=start, big_endian=be)
                    _record(agg.last_launch(), what, kernel=ipls.KERNEL_REDUCE, shape=ipls.SHAPE_SMALL, block=b,
                            vectors=T // (2 * b), map=0, seqf=0, grid=tiles * P, be_in=int(be), be_out=0, start=start)
                    _check_agg(agg, want, what)
            if K in KCROSS:
                for be_in, start in ((False, ipls.START_ZERO), (True, ipls.START_FIRST), (False, ipls.START_ACCUM)):
                    what = f"reduce_batch_out K={K} start={start} be_in={be_in} -> big-endian"
                    outs = [Out(ipls, L, "f64", 0, be=True) for _ in range(P)]
                    if start == ipls.START_ACCUM:
                        for q, o in enumerate(outs):
                            o.fill(pool.prior[q].view(np.uint64).byteswap())
                    agg.reduce_batch_out(0, pool.table(K, "abe" if be_in else "a"), [o.buf for o in outs],
                                         start_mode=start, big_endian_in=be_in, big_endian_out=True)
                    _record(agg.last_launch(), what, kernel=ipls.KERNEL_REDUCE, shape=ipls.SHAPE_SMALL, block=b,
                            map=0, grid=tiles * P, be_in=int(be_in), be_out=1, start=start)
                    agg.sync()
                    for q, o in enumerate(outs):
                        _same(o.bits(), pool.fold(O, K, start)[q].view(np.uint64).byteswap(), "f64", f"{what} p={q}")


# --------------------------------------------------------------------------
# 2. k_reduce_scalar
# --------------------------------------------------------------------------
def test_reduce_scalar(ipls, O):
    """The same kind of buckets at 8 mod 16, 300 elements: ZERO and ACCUM, native and big-endian."""
    pool = _pool(ipls, "f64", "scalar")
    with ipls.Aggregator(n_partitions=P, bucket_len=pool.L) as agg:
        for K in _updown(KFOLD):
            pool.set_k(K)
            for start in (ipls.START_ZERO, ipls.START_ACCUM):
                want = pool.fold(O, K, start)
                for be in (False, True):
                    what = f"k_reduce_scalar K={K} start={start} be={be}"
                    if start == ipls.START_ACCUM:
                        _set_prior(ipls, agg, pool)
                    tab = pool.table(K, "obe" if be else "o")
                    assert all(d.ptr % 16 == 8 for row in tab for d in row)
                    agg.reduce_batch(0, tab, start_mode=start, big_endian=be)
                    _record(agg.last_launch(), what, kernel=ipls.KERNEL_REDUCE_SCALAR, block=256, vectors=1, map=0,
                            grid=P, be_in=int(be), be_out=0, start=start)
                    _check_agg(agg, want, what)


# --------------------------------------------------------------------------
# 3. k_round + k_round_counts, small shape
# --------------------------------------------------------------------------
def _round_case(ipls, O, agg, pool, K, accum, shift, secure, avg_fmt, place="a", be=False, fused=True):
    """One aggregate_round on a reset handle: REP on partition 1, AGG loaded
    by one Update per partition when accum; W in full (the count W[L - 1]
    included) and the averages in a guarded device buffer `shift` elements
    past a 16-B boundary."""
    fmt, L = pool.fmt, pool.L
    what = f"round {fmt}->{avg_fmt} K={K} accum={accum} shift={shift} secure={secure} be={be}"
    if accum:
        for q in range(P):
            agg.Update(pool.prior[q], q)
    agg.Update(pool.rep, 1, from_clients=False)
    ws = pool.weights(O, K, accum)
    out = Out(ipls, P * (L - 1), avg_fmt, shift)
    assert agg.aggregate_round(0, pool.table(K, place), big_endian=be, out=out.buf) is out.buf
    if fused:
        T, b, _ = _tile(ipls, fmt)
        extra = dict(shape=ipls.SHAPE_SMALL, seqf=0, map=0) if fmt == "f64" else dict(seqf=1, map=3)
        _record(agg.last_launch(), what, kernel=_round_kernel(ipls, fmt), block=b, grid=-(-L // T) * P, be_in=int(be),
                be_out=0, start=ipls.START_ACCUM if accum else ipls.START_ZERO, **extra)
    agg.sync()
    _same(out.bits(), _avg_bits(O.get_partitions(ws, secure), avg_fmt), avg_fmt, f"{what}: averages")
    for q in range(P):
        _same(agg.read(q, ipls.TGT_WEIGHTS), ws[q], "f64", f"{what}: W p={q}")
    return what


def _consumed(ipls, agg, what):
    """AGG and REP ended logically zero: a following round without buckets gives W = +0.0."""
    agg.aggregate_round(0, [[] for _ in range(P)], with_average=False)
    for q in range(P):
        assert not agg.read(q, ipls.TGT_WEIGHTS).view(np.uint64).any(), f"{what}: W p={q} of an empty round is not +0.0"


@pytest.mark.parametrize("secure", (False, True))
def test_round_small(ipls, O, secure):
    """aggregate_round over KROUND (secure: K = 9, 64, 65, 129): from ZERO and
    from ACCUM, the averages at a 16-B boundary and at 8 mod 16 (each start
    meets both on the way up and down), big-endian input at K = 8, 9, 65."""
    pool = _pool(ipls, "f64", "round")
    ks = KSECURE if secure else KROUND
    with ipls.Aggregator(n_partitions=P, bucket_len=pool.L, secure=secure) as agg:
        for n, K in enumerate(_updown(ks)):
            pool.set_k(K)
            down = n >= len(ks)
            for accum in (False, True):
                what = _round_case(ipls, O, agg, pool, K, accum, int(accum != down), secure, "f64")
            if K in KBE:
                what = _round_case(ipls, O, agg, pool, K, down, 1, secure, "f64", place="abe", be=True)
            _consumed(ipls, agg, what)


# --------------------------------------------------------------------------
# 4. k_reduce_narrow
# --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NARROW)
def test_reduce_narrow(ipls, O, fmt):
    """reduce_batch over KFOLD with every bucket aligned (seqf 1, map 3: the
    prefetching full tile, the vector step, the remainder) and with one bucket
    one element past a 16-B boundary (seqf 0: the whole grid element by
    element); ZERO, FIRST and ACCUM."""
    pool = _pool(ipls, fmt, "fold")
    T, b, _ = _tile(ipls, fmt)
    L = pool.L
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for K in _updown(KFOLD):
            pool.set_k(K)
            for start in (ipls.START_ZERO, ipls.START_FIRST, ipls.START_ACCUM):
                want = pool.fold(O, K, start)
                for place, seqf, mp in (("a", 1, 3), ("o", 0, 0)):
                    what = f"k_reduce_narrow {fmt} K={K} start={start} placement={place}"
                    if start == ipls.START_ACCUM:
                        _set_prior(ipls, agg, pool)
                    tab = pool.table(K, place)
                    assert (tab[1][0].ptr % 16 != 0) == (place == "o")
                    agg.reduce_batch(0, tab, start_mode=start)
                    _record(agg.last_launch(), what, kernel=_fold_kernel(ipls, fmt), block=b, vectors=T // (4 * b),
                            seqf=seqf, map=mp, grid=-(-L // T) * P, be_in=0, be_out=0, start=start)
                    _check_agg(agg, want, what)


# --------------------------------------------------------------------------
# 5. k_round_narrow + k_round_counts_narrow
# --------------------------------------------------------------------------
@pytest.mark.parametrize("secure", (False, True))
@pytest.mark.parametrize("src", NARROW)
def test_round_narrow(ipls, O, src, secure):
    """aggregate_round over KROUND (secure: K = 9, 64, 65, 129) with f32, half
    and bf16 buckets: averages in the source's format for every K, in the
    other two at K = 9 and 65; ZERO and ACCUM with REP on one partition;
    output offsets 0 and 3 elements.  K = 0 carries no bucket, so the call
    names no trainer format and runs the unfused steps: its bits are compared,
    its launch record is not the fused kernel's."""
    pool = _pool(ipls, src, "round")
    ks = KSECURE if secure else KROUND
    with ipls.Aggregator(n_partitions=P, bucket_len=pool.L, secure=secure) as agg:
        for n, K in enumerate(_updown(ks)):
            pool.set_k(K)
            down = n >= len(ks)
            for accum in (False, True):
                what = _round_case(ipls, O, agg, pool, K, accum, 3 * int(accum != down), secure, src, fused=K > 0)
            if K in KCROSS:
                for i, avg in enumerate(f for f in NARROW if f != src):
                    what = _round_case(ipls, O, agg, pool, K, bool(i) != down, 3 * i, secure, avg)
            _consumed(ipls, agg, what)


# --------------------------------------------------------------------------
# 6. the wide shapes (mid, half, big) at K = 8, 17, 65
# --------------------------------------------------------------------------
WIDE_K = (8, 17, 65)
WIDE_CLASSES = 5
WIDE_ENDS = (None, 7, 8, 16, 64)   # rotation class c: every count slot 1.0, or the witness of the exchange that ends here


def _wide_pool(L, starts, kmax=max(WIDE_K), C=WIDE_CLASSES):
    """kmax peers' buckets, the PRIOR and the REP bucket for test_gpu_wide_small's Rig,
    (C - 1) blocks wider than a partition: class c reads from column c * B on,
    so block c stands at each of `starts` for it, and its count slot is column
    L - 1 + c * B.  The exchanges that end at peers 7 and 16 are the last of 8
    and of 17 peers; cut to fewer peers a count witness is a finite sum."""
    B = PW.block_width(kmax)
    h = PW.random_values(np.random.default_rng(77), (kmax + 2, L + (C - 1) * B), "f64")
    for s in starts:
        for c in range(C):
            assert s + (c + 1) * B <= L - 1
            PW.plant_witness(h[:kmax], s + c * B)
            h[kmax, s + c * B:s + c * B + kmax - 2] = 0.0
    for c, end in enumerate(WIDE_ENDS):
        col = L - 1 + c * B
        h[:, col] = 0.0
        h[:kmax, col] = 1.0 if end is None else PW.count_column(kmax, end - 1)
    return h, B


@pytest.mark.parametrize("name", ["mid", "half", "big"])
def test_wide_shapes(ipls, O, name):
    """One reduce_batch per K going up and one aggregate_round per K coming
    down, in the partial-tile geometry of test_gpu_wide_small's
    test_matrix[partial]: 256 partitions (big: 1024, the 1.1 GB handle) of a
    whole tile and R_PART elements.  The bucket table of 65 peers passes the
    first 64 KiB of the handle's table slots and shrinks again in the same
    slots.  The oracle runs once per rotation class (Rig)."""
    import test_gpu_wide_small as WS
    Pw, L, rshape, fshape = WS._matrix_geometry(ipls, name, True)
    s1 = L - WS.R_PART                                   # the partial tile: vector steps, then (big) the remainder
    h, B = _wide_pool(L, (0, 8192, s1, s1 + 2048))
    Z = ipls.START_ZERO
    with WS.Rig(ipls, O, Pw, L, pool=h, classes=WIDE_CLASSES, shift=B) as rig:
        for K in WIDE_K:
            for c in range(WIDE_CLASSES):                # the inputs are what the docstring says
                a = O.reduce(rig.bufs(c, L, K), L, Z)
                assert not a[s1:s1 + K - 2].any() and not a[:K - 2].any()
                assert a[L - 1] == (K if WIDE_ENDS[c] is None else 4.0 if WIDE_ENDS[c] < K else a[L - 1])
            rig.reduce_handle(K, False, Z, rshape[Z], 3)
        for K in WIDE_K[::-1]:
            rig.round(K, False, False, 1, fshape[Z], 3)
