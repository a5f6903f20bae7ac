"""Seams and special values of the wide fold shapes, at the smallest sizes that reach them.

engine.hip launch_reduce_v runs reduce_tiles (ipls_kernels.hpp) in four
shapes, chosen by plan_reduce (reduce_plan.hpp).  tests/test_gpu_shapes.py and four tests of tests/test_gpu_parity.py
reach the three wide ones (mid = 256 lanes, half = 512, big = 1024) at
production sizes, with uniform buckets and mostly by checksum; the edge sweeps
of the suite all run the small shape, in which the PAIRS epilogue of the fused
round, the SEQ schedule, the G = 1 peer loop, map 2's padded grid, map 3 and
the partial tile at 512 and 1024 lanes are compiled out.  fill() and
use_half() count tiles over the whole batch, so a few hundred short
partitions take the wide shapes too: this file sweeps them there, bit for
bit, with special values on every seam.  (Division of labour: production
sizes and checksums in test_gpu_shapes.py, seams and special values here.)

Inputs.  One pool of KMAX distinct buckets per case (synth_bucket scaled by
10^-3 .. 10^3), as native doubles and as big-endian bytes.  Partition p folds
the pool rotated by p mod KMAX and cut to K, so different partitions fold in
different orders and the oracle (O.reduce, + REP, O.divide) runs once per
rotation class.  seam_positions() lists where the pool carries -0.0,
subnormals, +-1e300, 1e16 / -1e16 pairs that cancel in one order only, +inf
and one quiet NaN with a payload (never two different NaNs nor inf - inf in
one element: a single NaN operand propagates unchanged on the CPU and through
v_add_f64 alike, so those bits are compared raw as well).

tests/test_gpu_peer_counts.py drives the same Rig at K = 8, 17, 65 with a pool
of its own (65 buckets with witness columns, rotated by columns instead of by
peer: Rig's pool, classes and shift parameters).

Every case makes one launch, asserts the whole launch record
(check_record), and compares bits: caller-owned outputs in full on the device
between sentinel guard bands, handle targets by the checksum of every
partition and by full reads of the first 2 * KMAX partitions (every rotation
class at both parities of the averages), of the first of those with REP, and
of the last two.  After a round AGG and REP read as +0.0.  A case that lands
on another shape than written fails.  The last test checks that the records
seen are exactly the combinations plan_reduce can give for mid, half and
big (expected_combinations()).

What the geometry forbids, found while writing the cases:
  * big from ZERO / FIRST with a full tile needs 1024 whole 32768-double
    tiles (below that use_half() takes the batch): 33.5M doubles per target,
    a 1.1 GB handle.  It is the smallest that exists; every test that opens
    it says so.
  * mid never runs with one tile per partition (its tile count would equal
    big's, which comes first), so "r on top of one full tile" starts at r = 1
    there and the whole-tile case is two tiles.
  * the reference chunk rule (IPLS.java:1019-1028) shortens the last
    partition by at most P elements, so a last partition of 3 or 1 elements
    beside partitions of T + 1 needs P >= T - 2 partitions.  Those cases open
    a handle of T partitions (8.6 GB at the half tile) and run the launch on
    its last 256 or 128 partitions (a sub-range call).
  * fill() takes 256 tiles, or 410 and more: 300 partitions of a few
    elements do not fill and run the small shape (test_many_tiny_partitions
    keeps that case, asserts that record, and adds 500 partitions for the
    padded map-2 grid on the big shape).
  * one call folds the same number of buckets into every partition
    (aggregator._bucket_table_kind), so K = 0 cannot be given to one
    partition of a wide batch: K = 0 runs for a whole sub-range instead.
  * the averages of a round are one contiguous run (the flat model), so the
    guard bands of aggregate_round(out=) stand before and after the run, not
    between partitions; reduce_batch_out destinations have them around every
    partition.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KMAX = 9                  # distinct buckets in a pool (odd: 2 * KMAX consecutive partitions = every class x parity)
GUARD = 64                # sentinel elements on each side of a caller-owned output
# A signalling NaN whose bytes read the same in both byte orders.  No result
# can take it: sums and quotients give quiet NaNs, exact copies (K = 1 FIRST)
# copy pool values, and the pool's only NaN is quiet.
SENTINEL = 0x7FF45EA1A15EF47F
NAN_BITS = 0x7FF80000DEADBEEF
M64 = (1 << 64) - 1
PRIOR, REPB = 4, 5        # pool rotation of the bucket an ACCUM case starts from / of the REP bucket
R_PART = 3 * 1024 + 1     # partial tile of the matrix cases: vector steps and scalar trips at every lane count


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


# ---------------------------------------------------------------------------
# the combinations plan_reduce can give for the wide shapes, in one place
# ---------------------------------------------------------------------------
def variant(ipls, shape, be_in, start):
    """(lanes, 16-B vectors per lane, SEQ code) of a wide shape: half is 512 x
    16; big is 1024 x 16 (SEQF = 3 for big-endian input) and 1024 x 8 from
    ACCUM; mid is 256 x 16 for native doubles from ZERO / FIRST, else 256 x 8."""
    if shape == ipls.SHAPE_HALF:
        return 512, 16, 0
    if shape == ipls.SHAPE_BIG:
        return (1024, 8, 0) if start == ipls.START_ACCUM else (1024, 16, 3 if be_in else 0)
    if shape == ipls.SHAPE_SMALL:   # not a subject of this file: asserted where fill() sends a listed case there
        return 256, 1, 0
    assert shape == ipls.SHAPE_MID
    return (256, 8, 0) if (be_in or start == ipls.START_ACCUM) else (256, 16, 0)


def expected_combinations(ipls):
    """(kernel, shape, block, vectors, seqf, map, be_in, be_out, start): 78 of
    k_reduce and 22 of k_round.  Maps: 0 (whole tiles or a single partial
    tile), 3 (partial last tile beside full ones); big with big-endian input
    also 2 (at most 4096 tiles and no map 3).  The fused round writes native
    doubles, never starts FIRST, and takes the half shape only from ZERO."""
    out = set()
    for kernel in (ipls.KERNEL_REDUCE, ipls.KERNEL_ROUND):
        fin = kernel == ipls.KERNEL_ROUND
        for be_in in (0, 1):
            for be_out in ((0,) if fin else (0, 1)):
                for start in (ipls.START_ZERO, ipls.START_ACCUM) + (() if fin else (ipls.START_FIRST,)):
                    for shape in (ipls.SHAPE_HALF, ipls.SHAPE_BIG, ipls.SHAPE_MID):
                        if fin and shape == ipls.SHAPE_HALF and start == ipls.START_ACCUM:
                            continue
                        maps = (0, 3) + ((2,) if shape == ipls.SHAPE_BIG and be_in else ())
                        for m in maps:
                            out.add((kernel, shape) + variant(ipls, shape, be_in, start) + (m, be_in, be_out, start))
    return out


SEEN = set()


def check_record(ipls, li, kernel, shape, mapping, be_in, be_out, start, n_parts, max_len):
    """The whole launch record of the one launch under test."""
    block, vectors, seqf = variant(ipls, shape, be_in, start)
    tiles = -(-max_len // (2 * block * vectors)) * n_parts
    want = dict(kernel=kernel, shape=shape, block=block, vectors=vectors, seqf=seqf, map=mapping,
                be_in=int(be_in), be_out=int(be_out), start=start,
                grid=(tiles + 7) // 8 * 8 if mapping == 2 else tiles)
    got = {f: li[f] for f in want}
    assert got == want, f"launch record {got} != {want}"
    if shape != ipls.SHAPE_SMALL:
        SEEN.add((kernel, shape, block, vectors, seqf, mapping, int(be_in), int(be_out), start))


def whole_map(ipls, shape, be_in, tiles=0):
    """Map of a batch without map 3: XCD-chunked for big with big-endian input on at most 4096 tiles."""
    return 2 if (shape == ipls.SHAPE_BIG and be_in and tiles <= 4096) else 0


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def seam_positions(L):
    """Elements below the count slot where a wide path has a seam: 0, 1, 126 ..
    129 of a tile (wave and PAIRS piece boundaries), 2 * BS - 2 .. 2 * BS + 1
    (first vector step of the partial tile, second pair of pieces), the last
    four elements of a tile and the first two of the next, for every tile size
    in use, and L - 3, L - 2 before the count slot L - 1."""
    rel = [0, 1, 126, 127, 128, 129]
    for bs in (256, 512, 1024):
        rel += [2 * bs - 2, 2 * bs - 1, 2 * bs, 2 * bs + 1]
    pos = {L - 3, L - 2}
    for tile in (4096, 8192, 16384, 32768):   # mid x 8, mid x 16, half and big x 8, big x 16
        for base in range(0, L, tile):
            pos.update(base + r for r in rel)
            pos.update(base + tile + d for d in (-4, -3, -2, -1, 0, 1))
    return sorted(e for e in pos if 0 <= e < L - 1)


def make_pool(O, L, count=1.0, count_at=(), kmax=KMAX):
    """kmax buckets of L doubles; element L - 1 (and len - 1 for each shorter
    partition length in count_at) is the count slot."""
    h = np.stack([O.synth_bucket(L, 7, j) * 10.0 ** (j % 7 - 3) for j in range(kmax)])
    for n, e in enumerate(seam_positions(L)):
        kind = n % 8
        if kind in (0, 7):      # cancels in one order only: 1e16 + x - 1e16 != 1e16 - 1e16 + x
            h[0, e], h[1, e] = 1e16, -1e16
        elif kind == 1:         # -0.0 everywhere: FIRST keeps it, ZERO (+0.0 + -0.0) and + REP do not
            h[:, e] = -0.0
        elif kind == 2:         # subnormals only: flushing them to zero would show
            h[:, e] = 5e-324 * (np.arange(kmax) + 1)
        elif kind == 3:
            h[2, e], h[5, e] = 1e300, -1e300
        elif kind == 5:
            h[3, e] = np.inf
        elif kind == 6:
            h[4:5, e].view(np.uint64)[0] = NAN_BITS
    for n in (L,) + tuple(count_at):
        h[:, n - 1] = count
    return h


def dev_bits(a, be=False):
    """Host doubles -> int64 device tensor of their bits (byte-swapped: big-endian bytes)."""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return torch.from_numpy((u.byteswap() if be else u).view(np.int64)).to("cuda")


def same_bits(got, want, what):
    g = np.ascontiguousarray(got, dtype=np.float64).view(np.uint64)
    w = np.ascontiguousarray(want, dtype=np.float64).view(np.uint64)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g != w)
    assert not bad.size, f"{what}: {bad.size} elements differ; first at {bad[0]}: {g[bad[0]]:#018x} != {w[bad[0]]:#018x}"


def same_device(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).flatten().nonzero().flatten()
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} words differ; first at flat index {i} of {tuple(got.shape)}: "
                         f"{int(got.flatten()[i]) & M64:#018x} != {int(want.flatten()[i]) & M64:#018x}")


class Rig:
    """One handle, one pool, and the three launches under test.

    The pool is make_pool's `kmax` buckets, rotated by peer: partition p folds
    buckets p, p + 1, .. (mod kmax), so there are kmax rotation classes.  Or
    the caller gives `pool` (tests/test_gpu_peer_counts.py): its rows are the
    peers' buckets in order, then the bucket an ACCUM case starts from and the
    REP bucket, each `shift` * (classes - 1) columns wider than a partition;
    partition p then folds the same peers in the same order from column
    (p mod classes) * shift on -- a rotation by columns, under which peer 0
    stays peer 0."""

    def __init__(self, ipls, O, P=0, L=0, *, model=None, secure=False, count=1.0, count_at=(), kmax=KMAX,
                 pool=None, classes=0, shift=0):
        self.ipls, self.O, self.secure = ipls, O, secure
        if model:
            self.agg = ipls.Aggregator(model[0], model[1], secure=secure)
        else:
            self.agg = ipls.Aggregator(n_partitions=P, bucket_len=L, secure=secure)
        self.P, self.lens, self.offs = self.agg.n_partitions, self.agg.lengths, self.agg.offsets
        self.L = max(self.lens)
        if pool is None:
            self.h, self.kmax, self.C, self.shift = make_pool(O, self.L, count, count_at, kmax), kmax, kmax, 0
        else:
            assert shift > 0 and shift % 2 == 0 and pool.shape[1] == self.L + (classes - 1) * shift
            self.h, self.kmax, self.C, self.shift = pool, pool.shape[0] - 2, classes, shift
        width = self.h.shape[1]
        self.stride = (width + 63) // 32 * 32             # even: every bucket 16-B aligned
        host = np.zeros((self.h.shape[0], self.stride))
        host[:, :width] = self.h
        self.native, self.be = dev_bits(host), dev_bits(host, be=True)
        torch.cuda.synchronize()   # uploads ran on torch's stream; the handle's does not order after it

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.agg.close()
        self.native = self.be = None
        torch.cuda.empty_cache()

    def _src(self, c, i, first):
        """(pool row, first column) of bucket i of a partition of rotation class c."""
        if self.shift:
            return {0: i, PRIOR: self.kmax, REPB: self.kmax + 1}[first], c * self.shift
        return (c + first + i) % self.kmax, 0

    def rows(self, parts, K, be, first=0):
        """Bucket table: partition p folds pool buckets p + first, p + first + 1, .. (mod kmax), or with a
        caller's pool buckets 0, 1, .. from its class's column on (first: the PRIOR or the REP bucket alone)."""
        base = int((self.be if be else self.native).data_ptr())
        out = []
        for p in parts:
            src = [self._src(p % self.C, i, first) for i in range(K)]
            out.append([self.ipls.DeviceBuffer(base + 8 * (r * self.stride + col), self.lens[p], big_endian=be)
                        for r, col in src])
        return out

    def bufs(self, c, n, K, first=0):
        return [self.h[r][col:col + n] for r, col in (self._src(c, i, first) for i in range(K))]

    def full_reads(self, parts, extra=()):
        parts = list(parts)
        return sorted(set(parts[:2 * self.C] + parts[-2:] + list(extra)))

    # ---- k_reduce into caller buffers (reduce_batch_out), guard bands around every partition ----
    def reduce_out(self, K, be_in, be_out, start, shape, mapping, p_first=0, n=None):
        ipls, O, agg = self.ipls, self.O, self.agg
        n = self.P - p_first if n is None else n
        parts = list(range(p_first, p_first + n))
        L = self.lens[p_first]
        assert all(self.lens[p] == L for p in parts)
        stride = GUARD + (L + 1) // 2 * 2 + GUARD
        out = torch.full((n, stride), SENTINEL, dtype=torch.int64, device="cuda")
        want = out.clone()
        C = self.C                                        # rotation classes
        cls = torch.arange(p_first, p_first + n, device="cuda") % C
        prior = [None] * C
        if start == ipls.START_ACCUM:   # the destination holds a bucket, in the byte order it is written in
            prior = [self.bufs(c, L, 1, PRIOR)[0] for c in range(C)]
            out[:, GUARD:GUARD + L] = dev_bits(np.stack(prior), be_out)[cls]
        with np.errstate(all="ignore"):
            exp = np.stack([O.reduce(self.bufs(c, L, K), L, start, prior[c]) for c in range(C)])
        want[:, GUARD:GUARD + L] = dev_bits(exp, be_out)[cls]
        dsts = [ipls.DeviceBuffer(int(out.data_ptr()) + 8 * (q * stride + GUARD), L, big_endian=be_out)
                for q in range(n)]
        torch.cuda.synchronize()
        agg.reduce_batch_out(p_first, self.rows(parts, K, be_in), dsts, start_mode=start, big_endian_in=be_in,
                             big_endian_out=be_out)
        check_record(ipls, agg.last_launch(), ipls.KERNEL_REDUCE, shape, mapping, be_in, be_out, start, n, L)
        agg.sync()
        same_device(out, want, f"reduce_batch_out K={K} be_in={be_in} be_out={be_out} start={start} "
                               f"(rows of {stride}: {GUARD} guard + {L} + guard)")

    # ---- k_reduce into the handle's accumulators (reduce_batch) ----
    def reduce_handle(self, K, be_in, start, shape, mapping, p_first=0, n=None):
        ipls, O, agg = self.ipls, self.O, self.agg
        n = self.P - p_first if n is None else n
        parts = list(range(p_first, p_first + n))
        if start == ipls.START_ACCUM:   # ACCUM into logically zero targets would resolve to ZERO: copy a bucket in
            agg.reduce_batch(p_first, self.rows(parts, 1, False, first=PRIOR), start_mode=ipls.START_FIRST)
        agg.reduce_batch(p_first, self.rows(parts, K, be_in), start_mode=start, big_endian=be_in)
        check_record(ipls, agg.last_launch(), ipls.KERNEL_REDUCE, shape, mapping, be_in, False, start, n,
                     max(self.lens[p] for p in parts))
        exp = {}
        for p in parts:
            key = (p % self.C, self.lens[p])
            if key not in exp:
                c, Lq = key
                with np.errstate(all="ignore"):
                    acc = self.bufs(c, Lq, 1, PRIOR)[0] if start == ipls.START_ACCUM else None
                    e = O.reduce(self.bufs(c, Lq, K), Lq, start, acc)
                exp[key] = (e, O.checksum(e))
            assert agg.checksum(p) == exp[key][1], f"AGG[{p}] checksum, K={K} be_in={be_in} start={start}"
        for p in self.full_reads(parts):
            same_bits(agg.read(p), exp[(p % self.C, self.lens[p])][0], f"AGG[{p}] K={K} be_in={be_in} start={start}")

    # ---- k_round (aggregate_round): W to the handle, averages to a guarded device buffer ----
    def round(self, K, be_in, accum, shift, shape, mapping, p_first=0, n=None, with_average=True, rep=True):
        ipls, O, agg, C = self.ipls, self.O, self.agg, self.C
        n = self.P - p_first if n is None else n
        parts = list(range(p_first, p_first + n))
        lens = [self.lens[p] for p in parts]
        agg.reset()
        if accum:
            agg.reduce_batch(p_first, self.rows(parts, 1, False, first=PRIOR), start_mode=ipls.START_FIRST)
        ra, rb = (p_first + n // 4, p_first + n // 2 + 1) if rep else (0, 0)   # partitions with REP
        if rep:
            agg.reduce_batch(ra, self.rows(range(ra, rb), 1, False, first=REPB), start_mode=ipls.START_FIRST,
                             target=ipls.TGT_REP)
        n_avg = self.offs[parts[-1]] + lens[-1] - 1 - self.offs[p_first]
        buf = torch.full((2 * GUARD + n_avg + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        want = buf.clone()
        out = ipls.DeviceBuffer(int(buf.data_ptr()) + 8 * (GUARD + shift), n_avg) if with_average else None
        torch.cuda.synchronize()
        agg.aggregate_round(p_first, self.rows(parts, K, be_in), big_endian=be_in, with_average=with_average, out=out)
        start = ipls.START_ACCUM if accum else ipls.START_ZERO
        check_record(ipls, agg.last_launch(), ipls.KERNEL_ROUND, shape, mapping, be_in, False, start, n, max(lens))
        agg.sync()
        what = f"round K={K} be_in={be_in} accum={accum} shift={shift} secure={self.secure}"

        exp = {}

        def ref(p):
            return ref_key(p % C, self.lens[p], ra <= p < rb)

        def ref_key(c, Lq, has_rep):
            key = (c, Lq, has_rep)
            if key not in exp:
                with np.errstate(all="ignore"):
                    a = self.bufs(c, Lq, 1, PRIOR)[0] if accum else np.zeros(Lq)
                    a = O.reduce(self.bufs(c, Lq, K), Lq, O.START_ACCUM, acc=a)
                    r = self.bufs(c, Lq, 1, REPB)[0] if has_rep else np.zeros(Lq)
                    w = a + r
                    exp[key] = (w, O.checksum(w), O.divide(w, self.secure))
            return exp[key]

        if with_average:
            pos, L0 = GUARD + shift, lens[0]
            nu = sum(1 for x in lens if x == L0)
            assert lens[:nu] == [L0] * nu and all(self.offs[p] - self.offs[p_first] == (p - p_first) * (L0 - 1)
                                                   for p in parts)
            if L0 > 1:   # the uniform partitions: one gather per rotation class x REP on the device
                table = dev_bits(np.stack([ref_key(c, L0, r)[2] for r in (False, True) for c in range(C)]))
                p = torch.arange(p_first, p_first + nu, device="cuda")
                want[pos:pos + nu * (L0 - 1)] = table[p % C + C * ((p >= ra) & (p < rb))].flatten()
                pos += nu * (L0 - 1)
            for p in parts[nu:]:   # a ragged last partition
                a = ref(p)[2]
                want[pos:pos + a.size] = dev_bits(a)
                pos += a.size
            assert pos == GUARD + shift + n_avg
        same_device(buf, want, f"{what}: averages ({GUARD} guard + {n_avg} + guard)")
        for p in parts:
            assert agg.checksum(p, ipls.TGT_WEIGHTS) == ref(p)[1], f"{what}: W[{p}] checksum"
        full = self.full_reads(parts, extra=[q for q in range(ra, min(rb, ra + 2 * C))])
        for p in full:
            same_bits(agg.read(p, ipls.TGT_WEIGHTS), ref(p)[0], f"{what}: W[{p}]")
        for p in (parts[0], ra if rep else parts[0], parts[-1]):
            for tgt in (ipls.TGT_AGG, ipls.TGT_REP):
                assert not agg.read(p, tgt).view(np.uint64).any(), f"{what}: target {tgt} of {p} is not +0.0 after the round"


Z, F, A = 1, 2, 0   # START_ZERO, START_FIRST, START_ACCUM (asserted against the package below)


def test_constants(ipls, O):
    assert (ipls.START_ZERO, ipls.START_FIRST, ipls.START_ACCUM) == (Z, F, A) == (O.START_ZERO, O.START_FIRST,
                                                                                    O.START_ACCUM)
    assert len(expected_combinations(ipls)) == 100
    h = make_pool(O, 40000)
    assert h[4].view(np.uint64)[h[4] != h[4]].tolist() and set(h[4].view(np.uint64)[h[4] != h[4]]) == {NAN_BITS}
    assert np.isinf(h[3]).any() and np.signbit(h[:, seam_positions(40000)[1]]).all() and (h[:, -1] == 1.0).all()


# ---------------------------------------------------------------------------
# 1. lengths: r elements on top of one (and, for half and mid, two) full tiles
# ---------------------------------------------------------------------------
def _partitions_for(tiles_per_part):
    """A partition count whose tiles fill the chip (fill(): 256 tiles, or 410
    and more) while the next wider shape's do not."""
    return {2: 128, 3: 171}[tiles_per_part]


def _length_cases():
    cases = []
    for name, tile, bs, fulls in (("half", 16384, 512, (1, 2)), ("mid16", 8192, 256, (1, 2)),
                                  ("mid8", 4096, 256, (1, 2)), ("big16", 32768, 1024, (1,)),
                                  ("big8", 16384, 1024, (1,))):
        for nf in fulls:
            for r in (0, 1, 2, 2 * bs - 1, 2 * bs, 2 * bs + 1, 3 * bs + 1, tile - 1):
                if name.startswith("mid") and nf == 1 and r == 0:
                    continue   # one tile per partition never runs mid (module docstring)
                cases.append(pytest.param(name, tile, nf, r, id=f"{name}-{nf}x{tile}+{r}"))
    return cases


@pytest.mark.parametrize("name,tile,nf,r", _length_cases())
def test_lengths(ipls, O, name, tile, nf, r):
    """Whole tiles (r = 0), a one-element partial tile, vector steps only
    (2 * BS), vector steps plus one and two scalar trips (2 * BS + 1, 3 * BS +
    1), and a partial tile one element short of full, per shape: the batched
    fold into guarded caller buffers and the fused round with REP on part of
    the batch, averages at 0 and at 8 mod 16.  big16 opens the 1.1 GB (r = T -
    1: 2.1 GB) handle of 1024 partitions: the smallest batch whose ZERO-start
    fold takes the big shape with a full tile."""
    L = nf * tile + r
    partial = r != 0
    if name == "half":       # native doubles from ZERO, 512 lanes
        with Rig(ipls, O, 256 // nf, L) as rig:
            rig.reduce_out(3, False, False, Z, ipls.SHAPE_HALF, 3 if partial else 0)
            for shift in (0, 1):
                rig.round(3, False, False, shift, ipls.SHAPE_HALF, 3 if partial else 0)
    elif name in ("mid16", "mid8"):   # native doubles x 16, big-endian input x 8
        be = name == "mid8"
        with Rig(ipls, O, _partitions_for(-(-L // tile)), L) as rig:
            rig.reduce_out(3, be, be, Z, ipls.SHAPE_MID, 3 if partial else 0)
            for shift in (0, 1):
                rig.round(3, be, False, shift, ipls.SHAPE_MID, 3 if partial else 0)
    elif name == "big16":    # big-endian input: the SEQ schedule; ACCUM on the same batch: 1024 x 8
        with Rig(ipls, O, 1024, L) as rig:
            rig.reduce_out(3, True, True, Z, ipls.SHAPE_BIG, 3 if partial else 2)
            rig.reduce_out(2, False, False, A, ipls.SHAPE_BIG, 3 if L % 16384 else 0)
            for shift in (0, 1):
                rig.round(3, True, False, shift, ipls.SHAPE_BIG, 3 if partial else 2)
    else:                    # big8: the fused round on top of AGG (the batched ACCUM fold runs half here)
        with Rig(ipls, O, 256, L) as rig:
            for shift in (0, 1):
                rig.round(3, False, True, shift, ipls.SHAPE_BIG, 3 if partial else 0)
            rig.reduce_out(3, False, False, A, ipls.SHAPE_HALF, 3 if partial else 0)


# ---------------------------------------------------------------------------
# 2-4. K, byte orders, start modes, destinations, both kernels: per shape and map
# ---------------------------------------------------------------------------
def _matrix_geometry(ipls, name, partial):
    """(P, L, shape of k_reduce per start, shape of k_round per start)."""
    big, half, mid = ipls.SHAPE_BIG, ipls.SHAPE_HALF, ipls.SHAPE_MID
    r = R_PART if partial else 0
    if name == "big":
        return 1024, 32768 + r, {Z: big, F: big, A: big}, {Z: big, A: big}
    if name == "half":   # the fused round's ACCUM start has no half shape: big x 8 on the same batch
        return 256, 16384 + r, {Z: half, F: half, A: half}, {Z: half, A: big}
    return (171 if partial else 128), 16384 + r, {Z: mid, F: mid, A: mid}, {Z: mid, A: mid}


@pytest.mark.parametrize("partial", [False, True], ids=["whole", "partial"])
@pytest.mark.parametrize("name", ["big", "half", "mid"])
def test_matrix(ipls, O, name, partial):
    """k_reduce: {native, big-endian} in x {native, big-endian} out x {ZERO,
    FIRST, ACCUM} into guarded caller buffers, and every input order and
    start into the handle's accumulators (which hold native doubles); ACCUM
    with big-endian out starts from a big-endian destination.  k_round:
    {native, big-endian} in x {ZERO, ACCUM} x averages at 0 / 8 mod 16 (L - 1
    odd at the whole-tile lengths: both parities within one launch), REP on a
    quarter of the partitions, one round without averages, one with K = 0 over
    a sub-range.  K = 1, 2, 9 besides 3: K = 1 FIRST is an exact copy, K = 1
    ZERO turns -0.0 into +0.0, K = 9 crosses the partial tile's groups of 8
    peers.  "big" opens the 1.1 GB handle (module docstring)."""
    P, L, rshape, fshape = _matrix_geometry(ipls, name, partial)

    def m(shape, be_in, start, n=P):
        if partial:
            return 3
        block, vectors, _ = variant(ipls, shape, be_in, start)
        return whole_map(ipls, shape, be_in, -(-L // (2 * block * vectors)) * n)

    with Rig(ipls, O, P, L) as rig:
        for start in (Z, F, A):
            for be_in in (False, True):
                for be_out in (False, True):
                    rig.reduce_out(3, be_in, be_out, start, rshape[start], m(rshape[start], be_in, start))
                rig.reduce_handle(3, be_in, start, rshape[start], m(rshape[start], be_in, start))
        for K in (1, 2, 9):
            rig.reduce_out(K, False, False, Z, rshape[Z], m(rshape[Z], False, Z))
            rig.reduce_out(K, True, True, F, rshape[F], m(rshape[F], True, F))
            rig.reduce_handle(K, False, A, rshape[A], m(rshape[A], False, A))
        for accum in (False, True):
            start = A if accum else Z
            for be_in in (False, True):
                for shift in (0, 1):
                    rig.round(3, be_in, accum, shift, fshape[start], m(fshape[start], be_in, start))
        for K in (1, 2, 9):
            rig.round(K, K == 2, False, 1, fshape[Z], m(fshape[Z], K == 2, Z))
        rig.round(3, False, False, 0, fshape[Z], m(fshape[Z], False, Z), with_average=False)
        if name != "big":   # K = 0 over the last P - 3 partitions: W = AGG + REP, averages from it
            # (253 whole tiles of 1024 x 8 no longer fill: that one sub-range runs mid)
            shape = ipls.SHAPE_MID if (name == "half" and not partial) else fshape[A]
            rig.round(0, False, True, 1, shape, m(shape, False, A, P - 3), p_first=3)


@pytest.mark.parametrize("name", ["big", "half", "mid"])
@pytest.mark.parametrize("what", ["secure", "count0", "count-0"])
def test_round_divide_variants(ipls, O, name, what):
    """The secure divide (10^12 * count), a zero count slot and count slots
    that sum to -0.0 where REP holds one (+0.0 elsewhere): values pass
    through undivided.  Partial-tile geometry of test_matrix, ZERO and ACCUM
    start, averages at 8 mod 16 and at 0 mod 16.  "big" opens the 1.1 GB handle."""
    P, L, _, fshape = _matrix_geometry(ipls, name, True)
    count = {"secure": 1.0, "count0": 0.0, "count-0": -0.0}[what]
    with Rig(ipls, O, P, L, secure=what == "secure", count=count) as rig:
        rig.round(3, False, False, 1, fshape[Z], 3)
        rig.round(3, True, True, 1, fshape[A], 3)
        rig.round(2, True, False, 0, fshape[Z], 3)


def test_map2_padding_whole_tiles(ipls, O):
    """Map 2 on whole tiles with a tile count that is no multiple of 8 (the
    padding blocks map past the last tile and exit).  The fused round from
    ACCUM at 411 x 16384 (411 tiles of 1024 x 8, grid 416); the batched fold
    needs 1024 or more whole big tiles that the half shape would not fill
    better: 1279 x 32768 (grid 1280 at x 16, 2558 -> 2560 tiles at x 8), a 1.3 GB handle."""
    with Rig(ipls, O, 411, 16384) as rig:
        for shift in (0, 1):
            rig.round(3, True, True, shift, ipls.SHAPE_BIG, 2)
    with Rig(ipls, O, 1279, 32768) as rig:
        rig.reduce_out(2, True, True, Z, ipls.SHAPE_BIG, 2)
        rig.reduce_out(2, True, False, F, ipls.SHAPE_BIG, 2)
        rig.reduce_out(2, True, True, A, ipls.SHAPE_BIG, 2)
        rig.reduce_handle(2, True, Z, ipls.SHAPE_BIG, 2)
        rig.round(2, True, False, 1, ipls.SHAPE_BIG, 2)


# ---------------------------------------------------------------------------
# 5. ragged geometry: common length T + 1 (map 3), a shorter last partition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("last", [0, 3, 1], ids=["lastT", "last3", "last1"])
@pytest.mark.parametrize("name,tile,n", [("half", 16384, 256), ("mid", 8192, 128)])
def test_ragged(ipls, O, name, tile, n, last):
    """Aggregator(M, P) handles whose partitions are T + 1 long (one full
    tile and the count slot: map 3) while the last one is exactly T (its last
    tile is empty: the block returns), 3 elements, or 1 (the count slot only,
    no averages).  The chunk rule allows the two short ones only with P >= T -
    2 partitions, so those open a handle of T partitions (8.6 GB for half, 2.1
    GB for mid) and launch on its last n partitions; lastT launches on all n."""
    last = last or tile
    P = n if last == tile else tile
    M = (P - 1) * tile + last - 1
    assert [O.partition_len(M, P, i) for i in (0, P - 2, P - 1)] == [tile + 1, tile + 1, last]
    shape = ipls.SHAPE_HALF if name == "half" else ipls.SHAPE_MID
    with Rig(ipls, O, model=(M, P), count_at=(last,)) as rig:
        assert rig.lens == [O.partition_len(M, P, i) for i in range(P)]
        p0 = P - n
        for be in (False, True) if name == "half" else (False,):   # big-endian mid tiles are 4096: 3 per partition, no fill
            for start in (Z, F) + ((A,) if name == "half" else ()):
                rig.reduce_handle(3, be, start, shape, 3, p_first=p0, n=n)
            for shift in (0, 1):
                rig.round(3, be, False, shift, shape, 3, p_first=p0, n=n)
        rig.round(9, False, False, 1, shape, 3, p_first=p0, n=n, rep=False)


# ---------------------------------------------------------------------------
# 6. many tiny partitions: the big shape with no full tile at all
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("P,L", [(P, L) for P in (256, 500, 300) for L in (1, 2, 3, 5)] + [(4100, 3)])
def test_many_tiny_partitions(ipls, O, P, L):
    """Partitions of a few elements whose count alone fills the chip are
    dispatched to 1024-lane blocks that each run the scalar loop of the
    partial tile once: native doubles in partition order (map 0), big-endian
    input XCD-chunked (map 2; 500 tiles are padded to 504 blocks), and past
    4096 tiles in partition order again.  All three starts,
    both byte orders in and out, and the fused round with the averages at both
    alignments (L = 1: the count slot only, no averages).
    300 partitions do not fill by fill()'s rule (256 tiles, or 410 and more:
    two rounds of 256 CUs with at most a fifth idle), so that batch runs the
    small shape; its record is asserted as such and its bits
    are compared like the others'."""
    shape = ipls.SHAPE_SMALL if P == 300 else ipls.SHAPE_BIG
    with Rig(ipls, O, P, L) as rig:
        for be_in in (False, True):
            mp = whole_map(ipls, shape, be_in, P)
            for start in (Z, F, A):
                rig.reduce_handle(3, be_in, start, shape, mp)
                for be_out in (False, True):
                    rig.reduce_out(9 if be_out else 2, be_in, be_out, start, shape, mp)
            for accum in (False, True):
                for shift in (0, 1):
                    rig.round(3, be_in, accum, shift, shape, mp)


def test_every_combination_ran(ipls):
    """The launch records asserted above are exactly the combinations
    plan_reduce can give for the mid, half and big shapes (needs the
    whole file to have run)."""
    want = expected_combinations(ipls)
    assert SEEN == want, f"never launched: {sorted(want - SEEN)}; unexpected: {sorted(SEEN - want)}"
